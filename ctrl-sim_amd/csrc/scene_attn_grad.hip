// Training (e): the backward of a scene-encoder layer's first sublayer — key-padded self-attention over ONE source, then norm1,
//   Q | K | V = X Win^T + bin                                                      (in_proj_weight [768, 256])
//   O = concat_h softmax_{non-padded j}(Q_h K_h^T / sqrt(32)) V_h                  (8 heads x 32; every key of a context padded: O = 0)
//   S = X + O Wo^T + bo,  Y = LayerNorm(S; g, be)                                  (eps 1e-5)
// over contexts of L rows (torch.nn.TransformerEncoderLayer, post-LN, src_key_padding_mask), as an op: from X, key_pad, dY and the six
// fp32 master tensors to the six gradients and (optionally) dX.  Called by encoder_layer_grad.hip (X = the rows that enter the layer,
// dY = ffn_grad.hip's dU).
//
// This is self_attn_grad.hip's chunk-local pipeline under attn_grad.hip's mask: the keys are the chunk's own rows, so per chunk of whole
// contexts (<= 8192 rows where a context has no more)
//   1. Q | K | V [rows, 768] = X Win^T + bin         (one product, hg_gemm.h)
//   2. O and the statistics                           ag_fwd_kernel<AgPadMask>, Lq = Lk = L, pad offset by the chunk's first context
//   3. S = X + O Wo^T + bo                            (HG_EPI_RES)
//   4. dS = LayerNorm backward of dY; partials (dY xhat, dY, dS): dg, dbe, dbo
//   5. dWo (+)= dS^T O            6. dO = dS Wo, over S
//   7. delta and dQ -> dQKV[:, 0:256]                 ag_dq_kernel<AgPadMask>
//   8. dK | dV      -> dQKV[:, 256:768]               ag_dkv_kernel<AgPadMask>
//   9. dWin (+)= dQKV^T X  (one product)       10. dbin partials       11. dX = dS + dQKV Win  (one product with K = 768, HG_EPI_RES)
// Against the cross op called with Mem = X (attn_grad.hip, which keeps K | V and dK | dV of ALL contexts and leaves dX + dMem to the
// caller): two products and one elementwise pass fewer, and no [B L, 512] buffers.  The workspace is self_attn_grad.hip's carve: the
// buffers are the same.
//
// ARITHMETIC, RECOMPUTE and SUMS OVER ROWS are the sibling ops', as requirements: every product on the f32-input MFMA from the fp32
// masters; nothing of a forward is read but X and key_pad; slabs / fixed-order float64 sums (fg_reduce.h); no atomics: identical bits
// from run to run, whatever the workspace held.  A padded key and a key at or beyond L are excluded by index: their P is exactly 0, so
// their dK and dV are exactly 0; where such a row's dY is zero too, its dS, dO and dQ are zero and so is its dX.
#include "ag_pad_mask.h"
#include "../../include/ctrlsim.h"

namespace {

// the core's operands: everything is chunk-local, Q and K | V, dQ and dK | dV the thirds of one buffer's rows
AgOperands operands(char* ws, const SelfAttnGradWs& w, int L) {
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  const long nstat = (long)w.chunk_ctx * L * NHEAD;
  float *QKV = f(w.QKV), *dQKV = f(w.dQKV), *smax = f(w.stat);
  return AgOperands{QKV, QKV + DM, f(w.S), f(w.O), dQKV, dQKV + DM, smax, smax + nstat, smax + 2 * nstat,
                    3 * DM, 3 * DM, L, L};
}

}  // namespace

bool scene_attn_grad_dims_ok(int B, int L) {
  return B >= 1 && L >= 1 && L <= 0x7fffffffL / (3 * DM) && (long)B * L <= 0x7fffffffL / (3 * DM);
}

// Steps 1 and 2 for the contexts of the chunk from c0 on, into the op's chunk buffers.  The op's own chunk loop and
// encoder_layer_grad.hip's recompute of the sublayer's output call it.
int launch_scene_attn_chunk_fwd(const float* X, int ldx, const unsigned char* key_pad, const float* Win, const float* bin, int B, int L, int c0,
                                char* ws, const SelfAttnGradWs& w, hipStream_t st) {
  const int nc = B - c0 < w.chunk_ctx ? B - c0 : w.chunk_ctx;
  float* QKV = reinterpret_cast<float*>(ws + w.QKV);
  FG_CHK(hg_gemm_t<true, true, HG_EPI_PLAIN>(HgGemm{X + (long)c0 * L * ldx, ldx, 1, Win, 1, DM, QKV, 3 * DM, 0, bin, nc * L, 3 * DM, DM, DM, 0}, st));
  hipLaunchKernelGGL(ag_fwd_kernel<AgPadMask>, dim3((L + 127) / 128, NHEAD, nc), dim3(256), 0, st, operands(ws, w, L),
                     ag_pad_mask(key_pad, c0, L));
  return ctrlsim_launch_status();
}

int launch_scene_attn_block_grad(const float* X, int ldx, const unsigned char* key_pad, const float* dY, int lddy, const float* Win,
                                 const float* bin, const float* Wo, const float* bo, const float* gamma, const float* beta, int B, int L,
                                 char* ws, const SelfAttnGradWs& w, float* grads, float* dX, int lddx, hipStream_t st) {
  (void)beta;                                          // the backward of a LayerNorm does not read its bias
  if (!X || !dY || !Win || !bin || !Wo || !bo || !gamma || !ws || !grads || !scene_attn_grad_dims_ok(B, L) || ldx < DM || lddy < DM ||
      (dX && lddx < DM) || w.chunk_ctx < 1 || (reinterpret_cast<uintptr_t>(ws) & 15))
    return CTRLSIM_EINVAL;
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *dQKV = f(w.dQKV), *O = f(w.O), *S = f(w.S), *dS = f(w.dS), *slab = f(w.slab);
  float *pln = f(w.part_ln), *pcs = f(w.part_cs);
  const long wsz = (long)DM * DM;
  const AgGrads g = ag_grads(grads);
  const AgOperands a = operands(ws, w, L);
  const unsigned nadd = (unsigned)((wsz + 255) / 256);
  long nln = 0, ncs = 0;
  for (int c0 = 0; c0 < B; c0 += w.chunk_ctx) {
    const int nc = B - c0 < w.chunk_ctx ? B - c0 : w.chunk_ctx, nr = nc * L;
    const int acc = c0 > 0, nslab = (nr + FG_KS - 1) / FG_KS;
    const long r0 = (long)c0 * L;
    const float* Xc = X + r0 * ldx;
    const AgPadMask mask = ag_pad_mask(key_pad, c0, L);
    // 1. Q | K | V      2. O, statistics
    FG_CHK(launch_scene_attn_chunk_fwd(X, ldx, key_pad, Win, bin, B, L, c0, ws, w, st));
    // 3. S = X + O Wo^T + bo      4. dY -> dS, partials of dg, dbe, dbo      5. dWo (+)= dS^T O      6. dO = dS Wo, over S
    FG_CHK(ag_out_proj_bwd(Xc, ldx, dY + r0 * lddy, lddy, O, Wo, bo, gamma, S, dS, slab, g.Wo, nr, acc, pln, nln, st));
    // 7. delta, dQ      8. dK | dV
    hipLaunchKernelGGL(ag_dq_kernel<AgPadMask>, dim3((L + 127) / 128, NHEAD, nc), dim3(256), 0, st, a, mask);
    hipLaunchKernelGGL(ag_dkv_kernel<AgPadMask>, dim3((L + 63) / 64, NHEAD, nc), dim3(256), 0, st, a, mask);
    // 9. dWin (+)= dQKV^T X      10. dbin partials      11. dX = dS + dQKV Win
    FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{dQKV, 1, 3 * DM, Xc, ldx, 1, slab, DM, 3 * wsz, nullptr, 3 * DM, DM, nr, FG_KS, 0}, st));
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3(3 * nadd), dim3(256), 0, st, slab, nslab, 3 * wsz, g.Win, acc);
    const int ncb = (nr + FG_CS_ROWS - 1) / FG_CS_ROWS;
    hipLaunchKernelGGL(fg_colsum_kernel, dim3(3, ncb), dim3(256), 0, st, dQKV, 3L * DM, nr, 3 * DM, pcs + ncs * 3 * DM);
    ncs += ncb;
    if (dX)
      FG_CHK(hg_gemm_t<true, false, HG_EPI_RES>(HgGemm{dQKV, 3 * DM, 1, Win, DM, 1, dX + r0 * lddx, lddx, 0, nullptr, nr, DM, 3 * DM, 3 * DM, 0,
                                                       dS, DM}, st));
  }
  if (nln > w.nln || ncs > w.ncs) return CTRLSIM_EINVAL;
  ag_ln_reduce(pln, nln, g, st);
  hipLaunchKernelGGL(fg_colreduce_kernel, dim3(3 * DM / 16), dim3(256), 0, st, pcs, (int)ncs, 3L * DM, 3 * DM, g.bin);
  return ctrlsim_launch_status();
}

// ---- the op as a C ABI entry (include/ctrlsim.h)
extern "C" int64_t ctrlsim_scene_attn_block_grad_workspace_bytes(int B, int L) {
  if (!scene_attn_grad_dims_ok(B, L)) return CTRLSIM_EINVAL;
  return (int64_t)self_attn_grad_carve(0, B, L).bytes;
}
extern "C" int ctrlsim_scene_attn_block_grad_chunk_contexts(int B, int L) {
  if (!scene_attn_grad_dims_ok(B, L)) return CTRLSIM_EINVAL;
  return ag_chunk_contexts(B, L);
}
extern "C" int ctrlsim_scene_attn_block_grad(const float* X, int ldx, const uint8_t* key_pad, const float* dY, int lddy,
                                             const float* in_proj_weight, const float* in_proj_bias, const float* out_proj_weight,
                                             const float* out_proj_bias, const float* gamma, const float* beta, int B, int L,
                                             void* workspace, float* grads, float* dX, int lddx, hipStream_t stream) {
  if (!scene_attn_grad_dims_ok(B, L) || !beta || !workspace) return CTRLSIM_EINVAL;
  return launch_scene_attn_block_grad(X, ldx, key_pad, dY, lddy, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, gamma, beta, B,
                                      L, static_cast<char*>(workspace), self_attn_grad_carve(0, B, L), grads, dX, lddx, stream);
}
