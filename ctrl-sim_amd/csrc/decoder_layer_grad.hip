// Training (d): the backward of one whole decoder layer from the rows that enter it,
//   X1 = LayerNorm(X0 + SelfAttn(X0) Wo^T + bo; norm1)           (self_attn_grad.hip's forward: the multi-agent causal mask)
//   U  = LayerNorm(X1 + CrossAttn(X1, Mem) Wo^T + bo; norm2)     (attn_grad.hip's forward: the key-padding mask)
//   Y  = LayerNorm(U + relu(U W1^T + b1) W2^T + b2; norm3)       (ffn_grad.hip's forward)
// as an op: from X0, Mem, key_pad, dY and the layer's 18 fp32 master tensors to the 18 gradients and (optionally) dX0 and dMem.  The
// decoder's forward keeps nothing of a layer but the rows that enter it; this op RECOMPUTES X1 and U from them, then runs the three
// backward ops from the layer's output back: ffn (U, dY -> dU), cross-attention (X1, Mem, dU -> dX1, dMem), self-attention (X0, dX1 ->
// dX0).  The gradient is that of the layer function evaluated this way on X0 as given — the contract the three ops state for their own
// inputs.  The ops recompute their sublayer's inside (Q, K, V, statistics, O, S) once more from X0 / X1 / U: the double computation is
// the price of calling them unchanged.
//
// THE RECOMPUTE, per chunk of whole contexts (the ops' chunks: <= 8192 rows where a context has no more), in the ops' own arithmetic
// (f32-input MFMA from the fp32 masters) and their own workspace carves, which the backward then overwrites:
//   self:   Q | K | V = X0 Win^T + bin;  O           (launch_self_attn_chunk_fwd);  X1 = LayerNorm(X0 + O Wo^T + bo)    dl_proj_ln_kernel
//   cross:  K | V of Mem once;  Q = X1 Wq^T + bq;  O  (launch_attn_chunk_fwd);       U  = LayerNorm(X1 + O Wo^T + bo)
// — steps 1 and 2 of the ops' own chunk loops, by the ops' own launchers (ag_tile.h's ag_fwd_kernel under either mask).
// dl_proj_ln_kernel: the out-projection, the residual and the LayerNorm in one kernel — a workgroup owns 32 whole rows, a wave 64 of
// their 256 columns in two accumulator tiles; the rows never leave the registers between the product and the norm, the row sums are
// shuffles within a wave and one fixed-order add of the four waves' partials.  No atomics anywhere; nothing is read but the arguments;
// every workspace element that is read has been written by this call: identical bits from run to run, whatever the workspace held.
#include "ag_tile.h"
#include "../../include/ctrlsim.h"

namespace {

// Y = LayerNorm(R + O Wo^T + bo; gamma, beta) for 32 rows per workgroup.  O [rows, 256] dense; R / Y with leading dimensions.
__global__ __launch_bounds__(256) void dl_proj_ln_kernel(const float* __restrict__ O, const float* __restrict__ Wo, const float* __restrict__ bo,
                                                         const float* __restrict__ R, long ldr, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ Y, long ldy, int rows) {
  __shared__ __attribute__((aligned(16))) float As[16 * HG_LS];
  __shared__ __attribute__((aligned(16))) float Bs[4][16 * HG_LS];
  __shared__ float red[2][4][32];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, l31 = lane & 31, half = lane >> 5;
  const int m0 = blockIdx.x * 32;
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
  float va[4], vb[4][4];
  auto gload = [&](int k0) {
    if (t < 128) hg_load_kc(O, DM, m0, rows, k0, DM, t, va);          // 32 rows x 16 k; rows at or beyond `rows` read as zero
#pragma unroll
    for (int j = 0; j < 4; ++j) hg_load_kc(Wo, DM, 64 * j, DM, k0, DM, t, vb[j]);
  };
  gload(0);
  for (int k0 = 0; k0 < DM; k0 += 16) {
    if (t < 128) hg_store_kc(As, t, va);
#pragma unroll
    for (int j = 0; j < 4; ++j) hg_store_kc(Bs[j], t, vb[j]);
    __syncthreads();
    if (k0 + 16 < DM) gload(k0 + 16);                  // the next tile's loads are in flight during the products
    const float* as = As + half * HG_LS + l31;
    const float* bs = Bs[wave] + half * HG_LS + l31;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const float a = as[2 * s * HG_LS];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bs[2 * s * HG_LS], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bs[2 * s * HG_LS + 32], acc1, 0, 0, 0);
    }
    __syncthreads();
  }
  // S = acc + bo + R: register r is row mfma_row(r, half) of the block, columns n0 and n0 + 32 of it
  const int n0 = 64 * wave + l31;
  const float b0 = bo[n0], b1 = bo[n0 + 32];
  float v0[16], v1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + mfma_row(r, half);
    const float* rp = R + (long)(m < rows ? m : rows - 1) * ldr + n0;
    v0[r] = (acc0[r] + b0) + rp[0];
    v1[r] = (acc1[r] + b1) + rp[32];
  }
  // the rows' means, then their variances: 32 lanes of a half-wave by shuffles, the four waves' partials in wave order
  float mean[16], rstd[16];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s;
      if (pass == 0) s = v0[r] + v1[r];
      else { v0[r] -= mean[r]; v1[r] -= mean[r]; s = v0[r] * v0[r] + v1[r] * v1[r]; }
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
      if (l31 == 0) red[pass][wave][mfma_row(r, half)] = s;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = mfma_row(r, half);
      const float s = ((red[pass][0][q] + red[pass][1][q]) + (red[pass][2][q] + red[pass][3][q])) * (1.0f / DM);
      if (pass == 0) mean[r] = s; else rstd[r] = 1.0f / sqrtf(s + 1e-5f);
    }
  }
  const float g0 = gamma[n0], g1 = gamma[n0 + 32], e0 = beta[n0], e1 = beta[n0 + 32];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + mfma_row(r, half);
    if (m < rows) {
      float* yp = Y + (long)m * ldy + n0;
      yp[0] = (v0[r] * rstd[r]) * g0 + e0;
      yp[32] = (v1[r] * rstd[r]) * g1 + e1;
    }
  }
}

int copy_out(float* dst, const float* src, size_t rows, hipStream_t st) {
  if (dst && hipMemcpyAsync(dst, src, rows * DM * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) return CTRLSIM_ELAUNCH;
  return CTRLSIM_OK;
}

}  // namespace

// dl_proj_ln_kernel for `rows` rows (launchers.h: encoder_layer_grad.hip's recompute calls it too)
int launch_proj_ln(const float* O, const float* Wo, const float* bo, const float* R, long ldr, const float* gamma, const float* beta, float* Y,
                   long ldy, int rows, hipStream_t st) {
  hipLaunchKernelGGL(dl_proj_ln_kernel, dim3((rows + 31) / 32), dim3(256), 0, st, O, Wo, bo, R, ldr, gamma, beta, Y, ldy, rows);
  return ctrlsim_launch_status();
}

// what the two attention ops accept, for contexts of 3 T A rows
bool decoder_layer_grad_dims_ok(int B, int T, int A, int Lk, int F) {
  return F >= 1 && Lk >= 1 && self_attn_grad_dims_ok(B, T, A) && attn_grad_dims_ok(B, 3 * T * A, Lk);
}

// Workspace behind `base`: X1, U and the two gradients between the ops (dU, dX1) [B 3TA, 256], then the three ops' carves on top of
// each other — they run one after the other, and the recompute uses the attention ops' own chunk buffers before their backward does.
DecLayerGradWs decoder_layer_grad_carve(size_t base, int B, int T, int A, int Lk, int F) {
  DecLayerGradWs w;
  const int L = 3 * T * A;
  const size_t n = fg_up((size_t)B * L * DM * sizeof(float));
  w.X1 = fg_up(base); w.U = w.X1 + n; w.dU = w.U + n; w.dX1 = w.dU + n;
  const size_t ops = w.dX1 + n;
  w.f = ffn_grad_carve(ops, (long)B * L, F);
  w.a = attn_grad_carve(ops, B, L, Lk);
  w.s = self_attn_grad_carve(ops, B, L);
  w.bytes = w.f.bytes > w.a.bytes ? w.f.bytes : w.a.bytes;
  if (w.s.bytes > w.bytes) w.bytes = w.s.bytes;
  return w;
}

int launch_decoder_layer_grad(const float* X0, int ldx, const float* Mem, int ldm, const unsigned char* key_pad, const float* dY, int lddy,
                              const float* const* tn, int B, int T, int A, int Lk, int F, int mask_mode, char* ws, const DecLayerGradWs& w,
                              float* grads, float* dX0, int lddx0, float* dMem, int lddm, int accumulate_dmem, float* x1_out, float* u_out,
                              hipStream_t st) {
  if (!X0 || !Mem || !dY || !tn || !ws || !grads || !decoder_layer_grad_dims_ok(B, T, A, Lk, F) || (mask_mode != 0 && mask_mode != 1) ||
      ldx < DM || ldm < DM || lddy < DM || (dX0 && lddx0 < DM) || (dMem && lddm < DM) || (reinterpret_cast<uintptr_t>(ws) & 15))
    return CTRLSIM_EINVAL;
  for (int i = 0; i < 18; ++i)
    if (!tn[i]) return CTRLSIM_EINVAL;
  const float* const* fw = tn;          // linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm3.weight, norm3.bias
  const float* const* cw = tn + 6;      // multihead_attn: in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias; norm2.weight, .bias
  const float* const* sw = tn + 12;     // self_attn: the same; norm1.weight, norm1.bias
  const int L = 3 * T * A;
  const long rows = (long)B * L;
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *X1 = f(w.X1), *U = f(w.U), *dU = f(w.dU), *dX1 = f(w.dX1);
  // ---- X1: the self-attention sublayer's output, through the self-attention op's chunk buffers
  for (int c0 = 0; c0 < B; c0 += w.s.chunk_ctx) {
    const int nc = B - c0 < w.s.chunk_ctx ? B - c0 : w.s.chunk_ctx;
    const long r0 = (long)c0 * L;
    FG_CHK(launch_self_attn_chunk_fwd(X0, ldx, sw[0], sw[1], B, L, A, mask_mode, c0, ws, w.s, st));
    FG_CHK(launch_proj_ln(f(w.s.O), sw[2], sw[3], X0 + r0 * ldx, ldx, sw[4], sw[5], X1 + r0 * DM, DM, nc * L, st));
  }
  // ---- U: the cross-attention sublayer's output, through the cross-attention op's buffers
  for (int c0 = 0; c0 < B; c0 += w.a.chunk_ctx) {
    const int nc = B - c0 < w.a.chunk_ctx ? B - c0 : w.a.chunk_ctx;
    const long r0 = (long)c0 * L;
    FG_CHK(launch_attn_chunk_fwd(X1, DM, Mem, ldm, key_pad, cw[0], cw[1], B, L, Lk, c0, ws, w.a, st));
    FG_CHK(launch_proj_ln(f(w.a.O), cw[2], cw[3], X1 + r0 * DM, DM, cw[4], cw[5], U + r0 * DM, DM, nc * L, st));
  }
  FG_CHK(copy_out(x1_out, X1, (size_t)rows, st));
  FG_CHK(copy_out(u_out, U, (size_t)rows, st));
  // ---- the three ops, from the layer's output back; each op's dY is the dX of the op behind it
  const long gF = 2L * DM * F + F + 3 * DM;
  FG_CHK(launch_ffn_block_grad(U, DM, dY, lddy, fw[0], fw[1], fw[2], fw[3], fw[4], fw[5], rows, F, ws, w.f, grads, dU, DM, st));
  FG_CHK(launch_attn_block_grad(X1, DM, Mem, ldm, key_pad, dU, DM, cw[0], cw[1], cw[2], cw[3], cw[4], cw[5], B, L, Lk, ws, w.a, grads + gF,
                                dX1, DM, dMem, lddm, accumulate_dmem, st));
  return launch_self_attn_block_grad(X0, ldx, dX1, DM, sw[0], sw[1], sw[2], sw[3], sw[4], sw[5], B, T, A, mask_mode, ws, w.s, grads + gF + AG_NGRADS,
                                     dX0, lddx0, st);
}

// ---- the op as a C ABI entry (include/ctrlsim.h)
extern "C" int64_t ctrlsim_decoder_layer_grad_workspace_bytes(int B, int T, int A, int Lk, int F) {
  if (!decoder_layer_grad_dims_ok(B, T, A, Lk, F)) return CTRLSIM_EINVAL;
  return (int64_t)decoder_layer_grad_carve(0, B, T, A, Lk, F).bytes;
}
extern "C" int ctrlsim_decoder_layer_grad(const float* X0, int ldx, const float* Mem, int ldm, const uint8_t* key_pad, const float* dY, int lddy,
                                          const float* const* tensors, int B, int T, int A, int Lk, int F, int mask_mode, void* workspace,
                                          float* grads, float* dX0, int lddx0, float* dMem, int lddm, int accumulate_dmem, float* x1_out,
                                          float* u_out, hipStream_t stream) {
  if (!decoder_layer_grad_dims_ok(B, T, A, Lk, F) || !workspace) return CTRLSIM_EINVAL;
  return launch_decoder_layer_grad(X0, ldx, Mem, ldm, key_pad, dY, lddy, tensors, B, T, A, Lk, F, mask_mode, static_cast<char*>(workspace),
                                   decoder_layer_grad_carve(0, B, T, A, Lk, F), grads, dX0, lddx0, dMem, lddm, accumulate_dmem, x1_out,
                                   u_out, stream);
}
