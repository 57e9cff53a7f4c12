// Training, second stage (b): the backward of the post-LN attention sublayer with a key-padding mask,
//   Q = X Wq^T + bq,  K = Mem Wk^T + bk,  V = Mem Wv^T + bv                      (in_proj_weight [768, 256] = Wq; Wk; Wv)
//   O = concat_h softmax_keys(Q_h K_h^T / sqrt(32), padded keys = -inf) V_h      (8 heads x 32; every key of a context padded: O = 0)
//   S = X + O Wo^T + bo,  Y = LayerNorm(S; g, be)                                (eps 1e-5)
// as an op: from X, Mem, key_pad, dY and the six fp32 master tensors to the six gradients and (optionally) dX and dMem.  Called today by
// ctrlsim_forward_loss_grad_cross for the last decoder layer's cross-attention (X = norm1 output, Mem = the scene encoder's output,
// dY = ffn_grad.hip's dU); with X = Mem it is the scene encoder's self-attention sublayer.
//
// ARITHMETIC as ffn_grad.hip: every product on the f32-input MFMA (v_mfma_f32_32x32x2_f32) from the fp32 masters, the same under either
// operand split of the forward; edges are zero-filled or excluded by index, so any B, Lq, Lk >= 1 work.
//
// RECOMPUTE, DO NOT KEEP.  Nothing of the forward is read but X, Mem and key_pad.  K | V [B Lk, 512] are computed once.  The query rows are
// walked in chunks of whole contexts (attn_grad_carve: <= 8192 rows where a context has no more), per chunk
//   1. Q  = X Wq^T + bq                              (hg_gemm.h)
//   2. O and the rows' softmax statistics (max, log2 of the sum; log2 domain)     ag_fwd_kernel
//   3. S  = X + O Wo^T + bo                          (HG_EPI_RES)
//   4. dS = LayerNorm backward of dY; block partials (dY xhat, dY, dS): dg, dbe, dbo     (fg_reduce.h)
//   5. dWo (+)= dS^T O            6. dO = dS Wo, over S
//   7. delta = sum_keys P o dP and dQ = sum_keys dSc K / sqrt(32), P = exp2(s - max - log2sum), dP = dO V^T, dSc = P o (dP - delta)   ag_dq_kernel
//   8. dK = sum_queries dSc^T Q / sqrt(32), dV = sum_queries P^T dO of the chunk's contexts     ag_dkv_kernel
//   9. dWq (+)= dQ^T X           10. dbq partials          11. dX = dS + dQ Wq   (HG_EPI_RES)
// and behind the chunks dWk | dWv = (dK | dV)^T Mem, dbk | dbv, dMem = dK Wk + dV Wv.  The softmax of 7 and 8 is normalised from the
// statistics of 2, recomputed here; the bk slice of the bias gradient is computed like the others (it is zero in exact arithmetic).
//
// THE ATTENTION CORE is ag_tile.h's (ag_fwd_kernel, ag_dq_kernel, ag_dkv_kernel: one wave = a 32 x 32 tile of scores, a key tile has one
// owner) under AgPadMask (ag_pad_mask.h): every tile of a context is visited, a padded key and a key at or beyond Lk are excluded by index —
// their P is exactly 0, so their dK, dV and dMem rows are exactly 0.
//
// SUMS OVER ROWS as ffn_grad.hip (fg_reduce.h): slabs of 1024 rows added in slab order in float64, chunks in stream order; column sums
// through partials and one fixed-order float64 reduction.  Identical bits from run to run, whatever the workspace held.
#include "ag_pad_mask.h"
#include "../../include/ctrlsim.h"

#define AG_KVROWS 8192           // memory rows per pass of dWk | dWv

namespace {

// the core's operands for the contexts from c0 on: Q, O, dO, dQ and the statistics are chunk-local, K | V, dK | dV and key_pad are not
AgOperands operands(char* ws, const AttnGradWs& w, int c0, int Lq, int Lk) {
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  const long nstat = (long)w.chunk_ctx * Lq * NHEAD, k0 = (long)c0 * Lk * (2 * DM);
  float *KV = f(w.KV) + k0, *dKV = f(w.dKV) + k0, *smax = f(w.stat);
  return AgOperands{f(w.Q), KV, f(w.S), f(w.O), f(w.dQ), dKV, smax, smax + nstat, smax + 2 * nstat, DM, 2 * DM, Lq, Lk};
}

}  // namespace

bool attn_grad_dims_ok(int B, int Lq, int Lk) {
  return B >= 1 && Lq >= 1 && Lk >= 1 && (long)B * Lq <= 0x7fffffffL / DM && (long)B * Lk <= 0x7fffffffL / (2 * DM);
}

// Workspace behind `base`: K | V and dK | dV of all contexts [B Lk, 512], the chunk buffers Q, O, S (then dO), dS, dQ [chunk rows, 256] and
// the three statistics [chunk rows, 8], the product slabs of one chunk / one pass over the memory rows, and the column-sum partials
AttnGradWs attn_grad_carve(size_t base, int B, int Lq, int Lk) {
  AttnGradWs w;
  size_t off = fg_up(base);
  auto take = [&](size_t n) { const size_t o = off; off += fg_up(n); return o; };
  const int cc = w.chunk_ctx = ag_chunk_contexts(B, Lq);
  const long crows = (long)cc * Lq, rows = (long)B * Lq, rowsk = (long)B * Lk, nchunks = (B + cc - 1) / cc;
  const long kvr = rowsk < AG_KVROWS ? rowsk : AG_KVROWS;
  const long nslab_q = (crows + FG_KS - 1) / FG_KS, nslab_k = 2 * ((kvr + FG_KS - 1) / FG_KS);
  w.nln = (rows + FG_LN_ROWS - 1) / FG_LN_ROWS + nchunks;
  w.ncq = (rows + FG_CS_ROWS - 1) / FG_CS_ROWS + nchunks;
  w.nck = (rowsk + FG_CS_ROWS - 1) / FG_CS_ROWS + (rowsk + AG_KVROWS - 1) / AG_KVROWS;
  w.KV = take((size_t)rowsk * 2 * DM * sizeof(float));
  w.dKV = take((size_t)rowsk * 2 * DM * sizeof(float));
  w.Q = take((size_t)crows * DM * sizeof(float));
  w.O = take((size_t)crows * DM * sizeof(float));
  w.S = take((size_t)crows * DM * sizeof(float));
  w.dS = take((size_t)crows * DM * sizeof(float));
  w.dQ = take((size_t)crows * DM * sizeof(float));
  w.stat = take((size_t)crows * NHEAD * 3 * sizeof(float));
  w.slab = take((size_t)(nslab_q > nslab_k ? nslab_q : nslab_k) * DM * DM * sizeof(float));
  w.part_ln = take((size_t)w.nln * 3 * DM * sizeof(float));
  w.part_cq = take((size_t)w.ncq * DM * sizeof(float));
  w.part_ck = take((size_t)w.nck * 2 * DM * sizeof(float));
  w.bytes = off;
  return w;
}

// Steps 1 and 2 for the contexts of the chunk from c0 on, into the op's chunk buffers: Q = X Wq^T + bq, then O and the statistics; the first
// chunk projects K | V = Mem (Wk; Wv)^T + (bk; bv) of ALL contexts before.  The op's own chunk loop and decoder_layer_grad.hip's recompute
// of the sublayer's output call it.
int launch_attn_chunk_fwd(const float* X, int ldx, const float* Mem, int ldm, const unsigned char* key_pad, const float* Win, const float* bin,
                          int B, int Lq, int Lk, int c0, char* ws, const AttnGradWs& w, hipStream_t st) {
  const int nc = B - c0 < w.chunk_ctx ? B - c0 : w.chunk_ctx;
  float *KV = reinterpret_cast<float*>(ws + w.KV), *Q = reinterpret_cast<float*>(ws + w.Q);
  if (c0 == 0)
    FG_CHK(hg_gemm_t<true, true, HG_EPI_PLAIN>(HgGemm{Mem, ldm, 1, Win + (long)DM * DM, 1, DM, KV, 2 * DM, 0, bin + DM, B * Lk, 2 * DM, DM, DM, 0}, st));
  FG_CHK(hg_gemm_t<true, true, HG_EPI_PLAIN>(HgGemm{X + (long)c0 * Lq * ldx, ldx, 1, Win, 1, DM, Q, DM, 0, bin, nc * Lq, DM, DM, DM, 0}, st));
  hipLaunchKernelGGL(ag_fwd_kernel<AgPadMask>, dim3((Lq + 127) / 128, NHEAD, nc), dim3(256), 0, st,
                     operands(ws, w, c0, Lq, Lk), ag_pad_mask(key_pad, c0, Lk));
  return ctrlsim_launch_status();
}

int launch_attn_block_grad(const float* X, int ldx, const float* Mem, int ldm, const unsigned char* key_pad, const float* dY, int lddy,
                           const float* Win, const float* bin, const float* Wo, const float* bo, const float* gamma, const float* beta,
                           int B, int Lq, int Lk, char* ws, const AttnGradWs& w, float* grads, float* dX, int lddx, float* dMem, int lddm,
                           int accumulate_dmem, hipStream_t st) {
  (void)beta;                                          // the backward of a LayerNorm does not read its bias
  if (!X || !Mem || !dY || !Win || !bin || !Wo || !bo || !gamma || !ws || !grads || !attn_grad_dims_ok(B, Lq, Lk) || ldx < DM || ldm < DM ||
      lddy < DM || (dX && lddx < DM) || (dMem && lddm < DM) || w.chunk_ctx < 1 || (reinterpret_cast<uintptr_t>(ws) & 15))
    return CTRLSIM_EINVAL;
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *dKV = f(w.dKV), *O = f(w.O), *S = f(w.S), *dS = f(w.dS), *dQ = f(w.dQ), *slab = f(w.slab);
  float *pln = f(w.part_ln), *pcq = f(w.part_cq), *pck = f(w.part_ck);
  const long wsz = (long)DM * DM;
  const AgGrads g = ag_grads(grads);
  const int rowsk = B * Lk;
  const unsigned nadd = (unsigned)((wsz + 255) / 256);
  long nln = 0, ncq = 0, nck = 0;
  for (int c0 = 0; c0 < B; c0 += w.chunk_ctx) {
    const int nc = B - c0 < w.chunk_ctx ? B - c0 : w.chunk_ctx, nr = nc * Lq;
    const int acc = c0 > 0, nslab = (nr + FG_KS - 1) / FG_KS;
    const long r0 = (long)c0 * Lq;
    const float* Xc = X + r0 * ldx;
    // (K | V before the first chunk)      1. Q      2. O, statistics
    FG_CHK(launch_attn_chunk_fwd(X, ldx, Mem, ldm, key_pad, Win, bin, B, Lq, Lk, c0, ws, w, st));
    // 3. S = X + O Wo^T + bo      4. dY -> dS, partials of dg, dbe, dbo      5. dWo (+)= dS^T O      6. dO = dS Wo, over S
    FG_CHK(ag_out_proj_bwd(Xc, ldx, dY + r0 * lddy, lddy, O, Wo, bo, gamma, S, dS, slab, g.Wo, nr, acc, pln, nln, st));
    // 7. delta, dQ      8. dK | dV of these contexts
    const AgOperands a = operands(ws, w, c0, Lq, Lk);
    hipLaunchKernelGGL(ag_dq_kernel<AgPadMask>, dim3((Lq + 127) / 128, NHEAD, nc), dim3(256), 0, st, a, ag_pad_mask(key_pad, c0, Lk));
    hipLaunchKernelGGL(ag_dkv_kernel<AgPadMask>, dim3((Lk + 63) / 64, NHEAD, nc), dim3(256), 0, st, a, ag_pad_mask(key_pad, c0, Lk));
    // 9. dWq (+)= dQ^T X      10. dbq partials      11. dX = dS + dQ Wq
    FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{dQ, 1, DM, Xc, ldx, 1, slab, DM, wsz, nullptr, DM, DM, nr, FG_KS, 0}, st));
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3(nadd), dim3(256), 0, st, slab, nslab, wsz, g.Win, acc);
    const int ncb = (nr + FG_CS_ROWS - 1) / FG_CS_ROWS;
    hipLaunchKernelGGL(fg_colsum_kernel, dim3(1, ncb), dim3(256), 0, st, dQ, (long)DM, nr, DM, pcq + ncq * DM);
    ncq += ncb;
    if (dX)
      FG_CHK(hg_gemm_t<true, false, HG_EPI_RES>(HgGemm{dQ, DM, 1, Win, DM, 1, dX + r0 * lddx, lddx, 0, nullptr, nr, DM, DM, DM, 0, dS, DM}, st));
  }
  // dWk | dWv (+)= (dK | dV)^T Mem and the partials of dbk | dbv, a pass of memory rows at a time
  for (int k0 = 0; k0 < rowsk; k0 += AG_KVROWS) {
    const int nk = rowsk - k0 < AG_KVROWS ? rowsk - k0 : AG_KVROWS, nslab = (nk + FG_KS - 1) / FG_KS;
    const float* dKVc = dKV + (long)k0 * 2 * DM;
    FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{dKVc, 1, 2 * DM, Mem + (long)k0 * ldm, ldm, 1, slab, DM, 2 * wsz, nullptr, 2 * DM, DM,
                                                         nk, FG_KS, 0}, st));
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3(2 * nadd), dim3(256), 0, st, slab, nslab, 2 * wsz, g.Win + wsz, k0 > 0);
    const int ncb = (nk + FG_CS_ROWS - 1) / FG_CS_ROWS;
    hipLaunchKernelGGL(fg_colsum_kernel, dim3(2, ncb), dim3(256), 0, st, dKVc, 2L * DM, nk, 2 * DM, pck + nck * 2 * DM);
    nck += ncb;
  }
  // dMem (+)= dK Wk + dV Wv: each element has one owner, which with accumulate_dmem adds its sum to what dMem holds (a padded key's
  // row adds an exact +0)
  if (dMem)
    FG_CHK(hg_gemm_t<true, false, HG_EPI_PLAIN>(HgGemm{dKV, 2 * DM, 1, Win + wsz, DM, 1, dMem, lddm, 0, nullptr, rowsk, DM, 2 * DM, 2 * DM,
                                                       accumulate_dmem ? 1 : 0}, st));
  if (nln > w.nln || ncq > w.ncq || nck > w.nck) return CTRLSIM_EINVAL;
  ag_ln_reduce(pln, nln, g, st);
  hipLaunchKernelGGL(fg_colreduce_kernel, dim3(DM / 16), dim3(256), 0, st, pcq, (int)ncq, (long)DM, DM, g.bin);
  hipLaunchKernelGGL(fg_colreduce_kernel, dim3(2 * DM / 16), dim3(256), 0, st, pck, (int)nck, 2L * DM, 2 * DM, g.bin + DM);
  return ctrlsim_launch_status();
}

// ---- the op as a C ABI entry (include/ctrlsim.h)
extern "C" int64_t ctrlsim_attn_block_grad_workspace_bytes(int B, int Lq, int Lk) {
  if (!attn_grad_dims_ok(B, Lq, Lk)) return CTRLSIM_EINVAL;
  return (int64_t)attn_grad_carve(0, B, Lq, Lk).bytes;
}
extern "C" int ctrlsim_attn_block_grad_chunk_contexts(int B, int Lq, int Lk) {
  if (B < 1 || Lq < 1 || Lk < 1) return CTRLSIM_EINVAL;     // (the chunk size of any positive shape, also of one the op refuses)
  return ag_chunk_contexts(B, Lq);
}
extern "C" int ctrlsim_attn_block_grad(const float* X, int ldx, const float* Mem, int ldm, const uint8_t* key_pad, const float* dY, int lddy,
                                       const float* in_proj_weight, const float* in_proj_bias, const float* out_proj_weight,
                                       const float* out_proj_bias, const float* gamma, const float* beta, int B, int Lq, int Lk,
                                       void* workspace, float* grads, float* dX, int lddx, float* dMem, int lddm, hipStream_t stream) {
  if (!attn_grad_dims_ok(B, Lq, Lk) || !beta || !workspace) return CTRLSIM_EINVAL;
  return launch_attn_block_grad(X, ldx, Mem, ldm, key_pad, dY, lddy, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, gamma, beta,
                                B, Lq, Lk, static_cast<char*>(workspace), attn_grad_carve(0, B, Lq, Lk), grads, dX, lddx, dMem, lddm, 0, stream);
}
