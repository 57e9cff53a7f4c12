// Training, second stage (a): the backward of the post-LN feed-forward block every transformer layer ends in,
//   Hp = U W1^T + b1,  H = relu(Hp),  S = U + H W2^T + b2,  Y = LayerNorm(S; g, be)        (width 256, hidden width F, eps 1e-5, relu'(0) = 0)
// as an op: from U, dY and the six fp32 master tensors to dW1, db1, dW2, db2, dg, dbe and (optionally) dU.  The dual of the forward's
// ffn_block (forward.hip), called once per layer by whatever differentiates a layer; today by ctrlsim_forward_loss_grad_ffn for the
// last decoder layer, where head_grad.hip's dX arrives.
//
// ARITHMETIC as head_grad.hip: every product on the f32-input MFMA (v_mfma_f32_32x32x2_f32, hg_gemm.h) from the fp32 masters, the same
// under either operand split of the forward; edges are zero-filled by index, so any F >= 1 and any row count work.
//
// RECOMPUTE, DO NOT KEEP.  Nothing of the forward is stored but U.  The rows are walked in chunks (ffn_grad_carve: <= 8192 rows, fewer
// where F > 1024, so that the H chunk [chunk, F] is <= 32 MB and stays L2 / MALL resident between its writers and readers); per chunk
//   1. H  = relu(U W1^T + b1)                                 (epilogue HG_EPI_RELU)
//   2. S  = U + H W2^T + b2                                   (HG_EPI_RES)
//   3. dS = LayerNorm backward of dY, mean / rstd recomputed from S, one row per wave; block partials (dY xhat, dY, dS): dg, dbe, db2.
//      dS goes to a chunk buffer of its own, not over dY: dY is the caller's (ctrlsim_forward_loss_grad_ffn returns it as dX).
//   4. dW2 (+)= dS^T H       5. dHp = (dS W2) * [H > 0] written over H (HG_EPI_MASK: a thread reads and overwrites its own element)
//   6. db1 partials          7. dW1 (+)= dHp^T U              8. dU = dS + dHp W1   (HG_EPI_RES)
//
// SUMS OVER ROWS (no float atomics: identical bits from run to run, whatever the workspace held).  Inside a chunk the row sum is the K
// dimension of products 4 and 7; K is cut into slabs of FG_KS = 1024 rows (<= 8 per chunk, a fixed number for a given shape) to fill
// the chip, and fg_slab_add_kernel adds the slabs in slab order in float64 and then — from the second chunk on — onto the gradient
// buffer (beta = 1): across chunks the stream order is the summation order.  The column sums keep the partials of ALL chunks (7 MB at
// 147 456 rows) and are added once at the end by fg_colreduce_kernel: 16 columns x 16 row groups per workgroup, every thread four
// independent float64 sums in a fixed order, then a fixed LDS tree — not one workgroup walking the partials in sequence.
#include "fg_reduce.h"
#include "../../include/ctrlsim.h"

// Workspace behind `base`: the H chunk [chunk_rows, ldh], the S and dS chunks [chunk_rows, 256], the product slabs of one chunk and the
// column-sum partials of all rows
FfnGradWs ffn_grad_carve(size_t base, long rows, int F) {
  FfnGradWs w;
  size_t off = fg_up(base);
  auto take = [&](size_t n) { const size_t o = off; off += fg_up(n); return o; };
  long cap = (8192L * 1024) / F / FG_KS * FG_KS;       // H chunk <= 32 MB, whole slabs
  cap = cap < FG_KS ? FG_KS : cap > 8192 ? 8192 : cap;
  w.chunk_rows = (int)(rows < cap ? rows : cap);
  w.ldh = (F + 3) & ~3;
  const long nchunks = (rows + w.chunk_rows - 1) / w.chunk_rows;
  const long nslab = (w.chunk_rows + FG_KS - 1) / FG_KS;
  w.nln = (rows + FG_LN_ROWS - 1) / FG_LN_ROWS + nchunks;
  w.ncs = (rows + FG_CS_ROWS - 1) / FG_CS_ROWS + nchunks;
  w.H = take((size_t)w.chunk_rows * w.ldh * sizeof(float));
  w.S = take((size_t)w.chunk_rows * DM * sizeof(float));
  w.dS = take((size_t)w.chunk_rows * DM * sizeof(float));
  w.slab = take((size_t)nslab * F * DM * sizeof(float));
  w.part_ln = take((size_t)w.nln * 3 * DM * sizeof(float));
  w.part_cs = take((size_t)w.ncs * F * sizeof(float));
  w.bytes = off;
  return w;
}

int launch_ffn_block_grad(const float* U, int ldu, const float* dY, int lddy, const float* W1, const float* b1, const float* W2,
                          const float* b2, const float* gamma, const float* beta, long rows, int F, char* ws, const FfnGradWs& w,
                          float* grads, float* dU, int lddu, hipStream_t st) {
  (void)beta;                                          // the backward of a LayerNorm does not read its bias
  if (!U || !dY || !W1 || !b1 || !W2 || !b2 || !gamma || !ws || !grads || rows < 1 || rows > 0x7fffffffL / DM || F < 1 ||
      ldu < DM || lddy < DM || (dU && lddu < DM) || w.chunk_rows < 1 || (reinterpret_cast<uintptr_t>(ws) & 15))
    return CTRLSIM_EINVAL;
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *H = f(w.H), *S = f(w.S), *dS = f(w.dS), *slab = f(w.slab), *pln = f(w.part_ln), *pcs = f(w.part_cs);
  float *gW1 = grads, *gb1 = gW1 + (long)F * DM, *gW2 = gb1 + F, *gb2 = gW2 + (long)DM * F, *gg = gb2 + DM, *gbe = gg + DM;
  const long ldh = w.ldh, wsz = (long)F * DM;
  int nln = 0, ncs = 0;
  for (long r0 = 0; r0 < rows; r0 += w.chunk_rows) {
    const int nr = (int)(rows - r0 < w.chunk_rows ? rows - r0 : w.chunk_rows);
    const int acc = r0 > 0, nslab = (nr + FG_KS - 1) / FG_KS;
    const float* Uc = U + r0 * ldu;
    const float* dYc = dY + r0 * lddy;
    // 1. H = relu(U W1^T + b1)      2. S = U + H W2^T + b2
    FG_CHK(hg_gemm_t<true, true, HG_EPI_RELU>(HgGemm{Uc, ldu, 1, W1, 1, DM, H, ldh, 0, b1, nr, F, DM, DM, 0}, st));
    FG_CHK(hg_gemm_t<true, true, HG_EPI_RES>(HgGemm{H, ldh, 1, W2, 1, F, S, DM, 0, b2, nr, DM, F, F, 0, Uc, ldu}, st));
    // 3. dY -> dS, partials of dg, dbe, db2
    const int nb = (nr + FG_LN_ROWS - 1) / FG_LN_ROWS;
    hipLaunchKernelGGL(fg_ln_bwd_kernel, dim3(nb), dim3(256), 0, st, S, gamma, dYc, (long)lddy, dS, nr, pln + (long)nln * 3 * DM);
    nln += nb;
    // 4. dW2 (+)= dS^T H: slabs over blocks of FG_KS rows, added in slab order
    FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{dS, 1, DM, H, ldh, 1, slab, F, wsz, nullptr, DM, F, nr, FG_KS, 0}, st));
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3((unsigned)((wsz + 255) / 256)), dim3(256), 0, st, slab, nslab, wsz, gW2, acc);
    // 5. dHp = (dS W2) * [H > 0], over H
    FG_CHK(hg_gemm_t<true, false, HG_EPI_MASK>(HgGemm{dS, DM, 1, W2, F, 1, H, ldh, 0, nullptr, nr, F, DM, DM, 0}, st));
    // 6. db1 partials
    const int ncb = (nr + FG_CS_ROWS - 1) / FG_CS_ROWS;
    hipLaunchKernelGGL(fg_colsum_kernel, dim3((F + 255) / 256, ncb), dim3(256), 0, st, H, ldh, nr, F, pcs + (long)ncs * F);
    ncs += ncb;
    // 7. dW1 (+)= dHp^T U
    FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{H, 1, ldh, Uc, ldu, 1, slab, DM, wsz, nullptr, F, DM, nr, FG_KS, 0}, st));
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3((unsigned)((wsz + 255) / 256)), dim3(256), 0, st, slab, nslab, wsz, gW1, acc);
    // 8. dU = dS + dHp W1
    if (dU)
      FG_CHK(hg_gemm_t<true, false, HG_EPI_RES>(HgGemm{H, ldh, 1, W1, DM, 1, dU + r0 * lddu, lddu, 0, nullptr, nr, DM, F, F, 0, dS, DM}, st));
  }
  if (nln > w.nln || ncs > w.ncs) return CTRLSIM_EINVAL;
  float* const col3[3] = {gg, gbe, gb2};               // the LayerNorm backward's partial rows are [3][256]: (dY xhat, dY, dS)
  for (int q = 0; q < 3; ++q)
    hipLaunchKernelGGL(fg_colreduce_kernel, dim3(DM / 16), dim3(256), 0, st, pln + q * DM, nln, 3L * DM, DM, col3[q]);
  hipLaunchKernelGGL(fg_colreduce_kernel, dim3((F + 15) / 16), dim3(256), 0, st, pcs, ncs, (long)F, F, gb1);
  return ctrlsim_launch_status();
}

// ---- the op as a C ABI entry (include/ctrlsim.h)
extern "C" int64_t ctrlsim_ffn_block_grad_workspace_bytes(int rows, int F) {
  if (rows < 1 || F < 1) return CTRLSIM_EINVAL;
  return (int64_t)ffn_grad_carve(0, rows, F).bytes;
}
extern "C" int ctrlsim_ffn_block_grad_chunk_rows(int rows, int F) {
  if (rows < 1 || F < 1) return CTRLSIM_EINVAL;
  return ffn_grad_carve(0, rows, F).chunk_rows;
}
extern "C" int ctrlsim_ffn_block_grad(const float* U, int ldu, const float* dY, int lddy, const float* W1, const float* b1, const float* W2,
                                      const float* b2, const float* gamma, const float* beta, int rows, int F, void* workspace, float* grads,
                                      float* dU, int lddu, hipStream_t stream) {
  if (rows < 1 || F < 1 || !beta || !workspace) return CTRLSIM_EINVAL;
  return launch_ffn_block_grad(U, ldu, dY, lddy, W1, b1, W2, b2, gamma, beta, rows, F, static_cast<char*>(workspace),
                               ffn_grad_carve(0, rows, F), grads, dU, lddu, stream);
}
