// Training (c): the backward of a decoder layer's first sublayer — self-attention under the structured multi-agent causal mask, then norm1,
//   Q | K | V = X Win^T + bin                                                      (in_proj_weight [768, 256])
//   O = concat_h softmax_{visible j}(Q_h K_h^T / sqrt(32)) V_h                     (8 heads x 32)
//   S = X + O Wo^T + bo,  Y = LayerNorm(S; g, be)                                  (eps 1e-5)
// over contexts of L = 3 T A token rows, token i = (t, a, k) = (i / 3A, (i / 3) % A, i % 3), as an op: from X, dY and the six fp32 master
// tensors to the six gradients and (optionally) dX.  Called by ctrlsim_forward_loss_grad_layer for the last decoder layer (X = the rows that
// enter the layer, dY = attn_grad.hip's dX1).
//
// THE MASK (oracle/model_oracle.py:causal_mask_closed_form; no key-padding mask, as the reference's decoder layer):
//   mode 0   visible(i, j) <=> t_j < t_i  or  (t_j == t_i and ((a_j == a_i and k_j <= k_i) or k_j == 0))
//   mode 1   (attend_own_return_action) the t_j < t_i term holds only where a_j == a_i or k_j == 0
// The state tokens (k = 0) of LATER agents of the same timestep are visible although j > i: the mask is not lower-triangular.  Token 0 is
// visible to every row and every row sees itself.  Masked pairs are excluded BY INDEX (sa_visible): their P is exactly 0 — nothing is
// excluded by adding a large negative number to a score.
//
// ARITHMETIC, RECOMPUTE and SUMS OVER ROWS are attn_grad.hip's, as requirements: every product on the f32-input MFMA from the fp32
// masters; nothing of the forward is read but X; query rows in chunks of whole contexts of at most 8192 rows; the backward's softmax is
// normalised from statistics recomputed here; delta = sum_keys P o dP from the very P and dP the second key pass takes dSc from; one owner
// per dK | dV tile; slabs / fixed-order float64 sums (fg_reduce.h); no atomics: identical bits from run to run, whatever the workspace held.
// The keys are the chunk's own rows, so everything is chunk-local, per chunk
//   1. Q | K | V [rows, 768] = X Win^T + bin         (one product, hg_gemm.h)
//   2. O and the statistics                           ag_fwd_kernel<SaCausalMask>
//   3. S = X + O Wo^T + bo                            (HG_EPI_RES)
//   4. dS = LayerNorm backward of dY; partials (dY xhat, dY, dS): dg, dbe, dbo
//   5. dWo (+)= dS^T O            6. dO = dS Wo, over S
//   7. delta and dQ -> dQKV[:, 0:256]                 ag_dq_kernel<SaCausalMask>
//   8. dK | dV      -> dQKV[:, 256:768]               ag_dkv_kernel<SaCausalMask>
//   9. dWin (+)= dQKV^T X  (one product)       10. dbin partials       11. dX = dS + dQKV Win  (one product with K = 768, HG_EPI_RES)
// hg_gemm.h serves all of them without a new epilogue.
//
// THE ATTENTION CORE is ag_tile.h's (ag_fwd_kernel, ag_dq_kernel, ag_dkv_kernel: one wave = a 32 x 32 tile of scores) under
// SaCausalMask below, which puts the mask's structure on top.  With A3 = 3A keys per timestep, a wave's 32 queries span the timesteps
// t_lo .. t_hi, and a 32-key tile [j0, j0 + 32) is
//   skipped    where j0 >= (t_hi + 1) A3: wholly beyond the last visible key — about half of the score matrix is never computed; the
//              workgroup's tile loops end at its last query's band (ag_fwd, ag_dq) or begin at its first key's (ag_dkv);
//   unmasked   in mode 0 where j0 + 31 < t_lo A3: wholly below the first timestep row of the wave's queries, every pair visible;
//   masked     otherwise: the closed form per pair, from the pair's (t, a, k) — the tile's 64 keys' (ag_fwd, ag_dq) or 64 queries'
//              (ag_dkv) triples are computed once per tile into LDS, the lane's own once per kernel.
// Mode 1 evaluates the closed form in EVERY visited tile (below the band visibility depends on the agent pair: no tile of 32 keys is
// wholly visible once A >= 2); its work is the same MFMA count as mode 0's, the mask costs VALU only.  The query blocks of ag_fwd and
// ag_dq are walked from the last to the first: the longest key ranges start first.
#include "ag_tile.h"
#include "../../include/ctrlsim.h"

namespace {

// (tq, aq, kq): the query's triple; tj and akj = 4 a_j + k_j: the key's.  A key at or beyond L has t_j >= T: never visible.
__device__ __forceinline__ bool sa_visible(int mode, int tq, int aq, int kq, int tj, int akj) {
  const int kj = akj & 3;
  const bool same = (akj >> 2) == aq, state = kj == 0;
  return tj < tq ? (mode == 0 || same || state) : (tj == tq && ((same && kj <= kq) || state));
}

// The multi-agent causal mask as ag_tile.h's policy.  L = the context's rows (Lq = Lk).  t, a, k / ak: the lane's own token — the query
// clamped to the context, or the key as it is (a key at or beyond L has t >= T: visible to no query); t0: the first timestep of the
// wave's keys.
struct SaCausalMask {
  int A, mode;
  int A3, t, a, k, ak, t0;
  static constexpr bool REVERSE = true;
  struct Tile { int t[64], ak[64]; };                  // the 64 staged tokens: timestep and 4 a + k
  using KeyTile = Tile;
  using QueryTile = Tile;
  __device__ void set_query(int, int qrow, int) { A3 = 3 * A; t = qrow / A3; a = (qrow / 3) % A; k = qrow % 3; }
  __device__ void set_key(int, int j0, int key, int) { A3 = 3 * A; t = key / A3; ak = (((key / 3) % A) << 2) | (key % 3); t0 = j0 / A3; }
  __device__ int key_end(int q, int L, int) const { return min(L, (min(q, L - 1) / A3 + 1) * A3); }
  __device__ int first_query(int kb) const { return (((kb / A3) * A3) / 64) * 64; }   // (a multiple of 64: even / odd blocks keep their waves)
  __device__ bool beyond(int q, int L) const { return t0 > min(q, L - 1) / A3; }
  __device__ int band(int q) const { return mode == 0 ? (q / A3) * A3 : AG_NO_BAND; }
  __device__ void stage(Tile& tl, int i0, int tid) const {
    if (tid < 64) {
      const int i = i0 + tid;
      tl.t[tid] = i / A3;
      tl.ak[tid] = (((i / 3) % A) << 2) | (i % 3);
    }
  }
  __device__ void stage_keys(Tile& tl, int k0, int, int tid) const { stage(tl, k0, tid); }
  __device__ void stage_queries(Tile& tl, int q0, int tid) const { stage(tl, q0, tid); }
  __device__ float score(const Tile& tl, float s, int jj) const {
    return key_visible(tl, jj) ? s : -__builtin_inff();   // selected by index, nothing added to a score
  }
  __device__ bool key_visible(const Tile& tl, int jj) const { return sa_visible(mode, t, a, k, tl.t[jj], tl.ak[jj]); }
  __device__ bool query_visible(const Tile& tl, int q) const { return sa_visible(mode, tl.t[q], tl.ak[q] >> 2, tl.ak[q] & 3, t, ak); }
};

// the core's operands: everything is chunk-local, Q and K | V, dQ and dK | dV the thirds of one buffer's rows
AgOperands operands(char* ws, const SelfAttnGradWs& w, int L) {
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  const long nstat = (long)w.chunk_ctx * L * NHEAD;
  float *QKV = f(w.QKV), *dQKV = f(w.dQKV), *smax = f(w.stat);
  return AgOperands{QKV, QKV + DM, f(w.S), f(w.O), dQKV, dQKV + DM, smax, smax + nstat, smax + 2 * nstat,
                    3 * DM, 3 * DM, L, L};
}

}  // namespace

bool self_attn_grad_dims_ok(int B, int T, int A) {
  return B >= 1 && T >= 1 && A >= 1 && 3L * T * A <= 0x7fffffffL / (3 * DM) && (long)B * 3 * T * A <= 0x7fffffffL / (3 * DM);
}

// Workspace behind `base`: the chunk buffers Q | K | V and dQ | dK | dV [chunk rows, 768], O, S (then dO), dS [chunk rows, 256], the three
// statistics [chunk rows, 8], the product slabs of one chunk, and the column-sum partials
SelfAttnGradWs self_attn_grad_carve(size_t base, int B, int L) {
  SelfAttnGradWs w;
  size_t off = fg_up(base);
  auto take = [&](size_t n) { const size_t o = off; off += fg_up(n); return o; };
  const int cc = w.chunk_ctx = ag_chunk_contexts(B, L);
  const long crows = (long)cc * L, rows = (long)B * L, nchunks = (B + cc - 1) / cc;
  const long nslab = (crows + FG_KS - 1) / FG_KS;
  w.nln = (rows + FG_LN_ROWS - 1) / FG_LN_ROWS + nchunks;
  w.ncs = (rows + FG_CS_ROWS - 1) / FG_CS_ROWS + nchunks;
  w.QKV = take((size_t)crows * 3 * DM * sizeof(float));
  w.dQKV = take((size_t)crows * 3 * DM * sizeof(float));
  w.O = take((size_t)crows * DM * sizeof(float));
  w.S = take((size_t)crows * DM * sizeof(float));
  w.dS = take((size_t)crows * DM * sizeof(float));
  w.stat = take((size_t)crows * NHEAD * 3 * sizeof(float));
  w.slab = take((size_t)nslab * 3 * DM * DM * sizeof(float));
  w.part_ln = take((size_t)w.nln * 3 * DM * sizeof(float));
  w.part_cs = take((size_t)w.ncs * 3 * DM * sizeof(float));
  w.bytes = off;
  return w;
}

// Steps 1 and 2 for the contexts of the chunk from c0 on, into the op's chunk buffers: Q | K | V = X Win^T + bin, then O and the statistics.
// The op's own chunk loop and decoder_layer_grad.hip's recompute of the sublayer's output call it.
int launch_self_attn_chunk_fwd(const float* X, int ldx, const float* Win, const float* bin, int B, int L, int A, int mask_mode, int c0, char* ws,
                               const SelfAttnGradWs& w, hipStream_t st) {
  const int nc = B - c0 < w.chunk_ctx ? B - c0 : w.chunk_ctx;
  float* QKV = reinterpret_cast<float*>(ws + w.QKV);
  FG_CHK(hg_gemm_t<true, true, HG_EPI_PLAIN>(HgGemm{X + (long)c0 * L * ldx, ldx, 1, Win, 1, DM, QKV, 3 * DM, 0, bin, nc * L, 3 * DM, DM, DM, 0}, st));
  hipLaunchKernelGGL(ag_fwd_kernel<SaCausalMask>, dim3((L + 127) / 128, NHEAD, nc), dim3(256), 0, st, operands(ws, w, L),
                     SaCausalMask{A, mask_mode});
  return ctrlsim_launch_status();
}

int launch_self_attn_block_grad(const float* X, int ldx, const float* dY, int lddy, const float* Win, const float* bin, const float* Wo,
                                const float* bo, const float* gamma, const float* beta, int B, int T, int A, int mask_mode, char* ws,
                                const SelfAttnGradWs& w, float* grads, float* dX, int lddx, hipStream_t st) {
  (void)beta;                                          // the backward of a LayerNorm does not read its bias
  if (!X || !dY || !Win || !bin || !Wo || !bo || !gamma || !ws || !grads || !self_attn_grad_dims_ok(B, T, A) ||
      (mask_mode != 0 && mask_mode != 1) || ldx < DM || lddy < DM || (dX && lddx < DM) || w.chunk_ctx < 1 ||
      (reinterpret_cast<uintptr_t>(ws) & 15))
    return CTRLSIM_EINVAL;
  const int L = 3 * T * A;
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *dQKV = f(w.dQKV), *O = f(w.O), *S = f(w.S), *dS = f(w.dS), *slab = f(w.slab);
  float *pln = f(w.part_ln), *pcs = f(w.part_cs);
  const long wsz = (long)DM * DM;
  const AgGrads g = ag_grads(grads);
  const AgOperands a = operands(ws, w, L);
  const SaCausalMask mask{A, mask_mode};
  const unsigned nadd = (unsigned)((wsz + 255) / 256);
  long nln = 0, ncs = 0;
  for (int c0 = 0; c0 < B; c0 += w.chunk_ctx) {
    const int nc = B - c0 < w.chunk_ctx ? B - c0 : w.chunk_ctx, nr = nc * L;
    const int acc = c0 > 0, nslab = (nr + FG_KS - 1) / FG_KS;
    const long r0 = (long)c0 * L;
    const float* Xc = X + r0 * ldx;
    // 1. Q | K | V      2. O, statistics
    FG_CHK(launch_self_attn_chunk_fwd(X, ldx, Win, bin, B, L, A, mask_mode, c0, ws, w, st));
    // 3. S = X + O Wo^T + bo      4. dY -> dS, partials of dg, dbe, dbo      5. dWo (+)= dS^T O      6. dO = dS Wo, over S
    FG_CHK(ag_out_proj_bwd(Xc, ldx, dY + r0 * lddy, lddy, O, Wo, bo, gamma, S, dS, slab, g.Wo, nr, acc, pln, nln, st));
    // 7. delta, dQ      8. dK | dV
    hipLaunchKernelGGL(ag_dq_kernel<SaCausalMask>, dim3((L + 127) / 128, NHEAD, nc), dim3(256), 0, st, a, mask);
    hipLaunchKernelGGL(ag_dkv_kernel<SaCausalMask>, dim3((L + 63) / 64, NHEAD, nc), dim3(256), 0, st, a, mask);
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
extern "C" int64_t ctrlsim_self_attn_block_grad_workspace_bytes(int B, int T, int A) {
  if (!self_attn_grad_dims_ok(B, T, A)) return CTRLSIM_EINVAL;
  return (int64_t)self_attn_grad_carve(0, B, 3 * T * A).bytes;
}
extern "C" int ctrlsim_self_attn_block_grad_chunk_contexts(int B, int T, int A) {
  if (!self_attn_grad_dims_ok(B, T, A)) return CTRLSIM_EINVAL;
  return ag_chunk_contexts(B, 3 * T * A);
}
extern "C" int ctrlsim_self_attn_block_grad(const float* X, int ldx, const float* dY, int lddy, const float* in_proj_weight,
                                            const float* in_proj_bias, const float* out_proj_weight, const float* out_proj_bias,
                                            const float* gamma, const float* beta, int B, int T, int A, int mask_mode, void* workspace,
                                            float* grads, float* dX, int lddx, hipStream_t stream) {
  if (!self_attn_grad_dims_ok(B, T, A) || !beta || !workspace) return CTRLSIM_EINVAL;
  return launch_self_attn_block_grad(X, ldx, dY, lddy, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, gamma, beta, B, T, A,
                                     mask_mode, static_cast<char*>(workspace), self_attn_grad_carve(0, B, 3 * T * A), grads, dX, lddx, stream);
}
