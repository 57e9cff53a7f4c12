// The f32-input MFMA tile product of the gradient files (head_grad.hip, ffn_grad.hip): C[z] (+)= A B over k in [z kchunk, (z + 1) kchunk)
// with exact fp32 operands and fp32 accumulation (v_mfma_f32_32x32x2_f32), and the LayerNorm row both files recompute.  Everything
// here has internal linkage: one set of instantiations per including file.
#pragma once
#include "launchers.h"

#define HG_LS 68                 // LDS row stride of a 16 x 64 operand tile (floats): 16-byte aligned rows

namespace {

// A(m, k) = A[m sam + k sak], B(k, n) = B[k sbk + n sbn], one stride of each being 1 (template: which).  64 x 64 output tile per
// workgroup, four waves of 32 x 32; operands staged k-major in LDS so that a lane's MFMA operand (row = lane & 31, k = lane >> 5) is
// one conflict-free dword read.  Everything out of range reads as zero.  R / ldr: the residual rows of the HG_EPI_RES epilogue.
struct HgGemm {
  const float* A; long sam, sak; const float* B; long sbk, sbn; float* C; long ldc, slab; const float* bias;
  int M, N, K, kchunk, beta;
  const float* R = nullptr; long ldr = 0;
};
// what leaves the accumulator (template parameter of the kernel):
//   HG_EPI_PLAIN  C = acc + bias (+ C if beta)
//   HG_EPI_RELU   C = max(acc + bias, 0)
//   HG_EPI_RES    C = acc + bias + R(m, n); C may be R itself (each thread reads the element it writes)
//   HG_EPI_MASK   C = C > 0 ? acc : 0, in place: the ReLU's backward over the stored activation, read and overwritten by the same thread
enum { HG_EPI_PLAIN = 0, HG_EPI_RELU = 1, HG_EPI_RES = 2, HG_EPI_MASK = 3 };

__device__ __forceinline__ bool hg_al16(const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// one thread's four elements of a 16 (k) x 64 (x) tile whose CONTIGUOUS dimension is k: x = t >> 2, k = 4 (t & 3) ..
__device__ __forceinline__ void hg_load_kc(const float* P, long sx, int x0, int X, int k0, int kend, int t, float (&v)[4]) {
  const int x = x0 + (t >> 2), k = k0 + 4 * (t & 3);
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (x >= X) return;
  const float* p = P + (long)x * sx + k;
  if (k + 3 < kend && hg_al16(p)) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k + i < kend) v[i] = p[i];
  }
}
// ... whose contiguous dimension is x: k = t >> 4, x = 4 (t & 15) ..
__device__ __forceinline__ void hg_load_xc(const float* P, long sk, int x0, int X, int k0, int kend, int t, float (&v)[4]) {
  const int k = k0 + (t >> 4), x = x0 + 4 * (t & 15);
  v[0] = v[1] = v[2] = v[3] = 0.f;
  if (k >= kend || x >= X) return;
  const float* p = P + (long)k * sk + x;
  if (x + 3 < X && hg_al16(p)) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x + i < X) v[i] = p[i];
  }
}
__device__ __forceinline__ void hg_store_kc(float* S, int t, const float (&v)[4]) {
  const int x = t >> 2, k = 4 * (t & 3);
#pragma unroll
  for (int i = 0; i < 4; ++i) S[(k + i) * HG_LS + x] = v[i];
}
__device__ __forceinline__ void hg_store_xc(float* S, int t, const float (&v)[4]) {
  float* s = S + (t >> 4) * HG_LS + 4 * (t & 15);
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = v[i];
}

template <bool A_KC, bool B_KC, int EPI>
__global__ __launch_bounds__(256) void hg_gemm_kernel(HgGemm g) {
  __shared__ __attribute__((aligned(16))) float As[16 * HG_LS];
  __shared__ __attribute__((aligned(16))) float Bs[16 * HG_LS];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, l31 = lane & 31, half = lane >> 5;
  const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64, z = blockIdx.z;
  const int kbeg = z * g.kchunk, kend = min(g.K, kbeg + g.kchunk);
  const int wm = wave & 1, wn = wave >> 1;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float va[4], vb[4];
  auto gload = [&](int k0) {
    if (A_KC) hg_load_kc(g.A, g.sam, m0, g.M, k0, kend, t, va); else hg_load_xc(g.A, g.sak, m0, g.M, k0, kend, t, va);
    if (B_KC) hg_load_kc(g.B, g.sbn, n0, g.N, k0, kend, t, vb); else hg_load_xc(g.B, g.sbk, n0, g.N, k0, kend, t, vb);
  };
  if (kbeg < kend) gload(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += 16) {
    if (A_KC) hg_store_kc(As, t, va); else hg_store_xc(As, t, va);
    if (B_KC) hg_store_kc(Bs, t, vb); else hg_store_xc(Bs, t, vb);
    __syncthreads();
    if (k0 + 16 < kend) gload(k0 + 16);                // the next tile's loads are in flight during the products
    const float* as = As + half * HG_LS + wm * 32 + l31;
    const float* bs = Bs + half * HG_LS + wn * 32 + l31;
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[2 * s * HG_LS], bs[2 * s * HG_LS], acc, 0, 0, 0);
    __syncthreads();
  }
  const int n = n0 + wn * 32 + l31;
  if (n >= g.N) return;
  const float bv = g.bias ? g.bias[n] : 0.f;
  float* C = g.C + (long)z * g.slab;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + mfma_row(r, half);
    if (m < g.M) {
      float* p = C + (long)m * g.ldc + n;
      float v = acc[r] + bv;
      if (EPI == HG_EPI_PLAIN) { if (g.beta) v += *p; }
      else if (EPI == HG_EPI_RELU) v = fmaxf(v, 0.f);
      else if (EPI == HG_EPI_RES) v += g.R[(long)m * g.ldr + n];
      else v = *p > 0.f ? acc[r] : 0.f;
      *p = v;
    }
  }
}

template <bool A_KC, bool B_KC, int EPI>
int hg_gemm_t(const HgGemm& g, hipStream_t st) {
  if (g.M <= 0 || g.N <= 0 || g.K <= 0) return CTRLSIM_OK;
  const int nz = (g.K + g.kchunk - 1) / g.kchunk;
  if (nz > 65535 || (g.N + 63) / 64 > 65535) return CTRLSIM_EINVAL;
  const dim3 grid((g.M + 63) / 64, (g.N + 63) / 64, nz);
  hipLaunchKernelGGL((hg_gemm_kernel<A_KC, B_KC, EPI>), grid, dim3(256), 0, st, g);
  return ctrlsim_launch_status();
}

// ---- LayerNorm(256) of one row held by a wave, lane l = columns 4 l .. 4 l + 3
__device__ __forceinline__ void hg_ln_row(const float (&x)[4], float (&xh)[4], float& rstd) {
  const float mean = wave_sum((x[0] + x[1]) + (x[2] + x[3])) * (1.0f / DM);
  float d[4], q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) { d[i] = x[i] - mean; q += d[i] * d[i]; }
  const float var = wave_sum(q) * (1.0f / DM);
  rstd = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
  for (int i = 0; i < 4; ++i) xh[i] = d[i] * rstd;
}

}  // namespace
