// The row-sum machinery the gradient files of the post-LN sublayers share (ffn_grad.hip, attn_grad.hip): the LayerNorm backward with its
// block partials, column-sum partials and their fixed-order float64 second stage, and the slab adder of the products that sum over rows.
// No float atomics anywhere: identical bits from run to run.  Internal linkage, like hg_gemm.h: one set of instantiations per including file.
#pragma once
#include "hg_gemm.h"

#define FG_KS 1024               // rows per partial slab of a product that sums over rows
#define FG_CS_ROWS 128           // rows per partial of db1's column sum
#define FG_LN_ROWS 64            // rows per workgroup of the LayerNorm backward

namespace {

__device__ __forceinline__ void fg_load4(const float* p, float (&v)[4]) {
  if (hg_al16(p)) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p);
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = p[i];
  }
}

// dY -> dS [rows, 256]; part[block][3][256] = this block's sums over its rows of (dY xhat, dY, dS): dgamma, dbeta, db2
__global__ __launch_bounds__(256) void fg_ln_bwd_kernel(const float* __restrict__ S, const float* __restrict__ gamma,
                                                        const float* __restrict__ dY, long lddy, float* __restrict__ dS, int rows,
                                                        float* __restrict__ part) {
  __shared__ float red[4][3][DM];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float gq[4];
  fg_load4(gamma + 4 * lane, gq);
  float sg[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f}, sz[4] = {0.f, 0.f, 0.f, 0.f};
  const long r0 = (long)blockIdx.x * FG_LN_ROWS + wave * (FG_LN_ROWS / 4);
  for (int j = 0; j < FG_LN_ROWS / 4; ++j) {
    const long row = r0 + j;
    if (row >= rows) break;                            // (wave-uniform)
    const f32x4 sq = *reinterpret_cast<const f32x4*>(S + row * DM + 4 * lane);
    const float x[4] = {sq[0], sq[1], sq[2], sq[3]};
    float dq[4], xh[4], rstd, dxh[4], s1 = 0.f, s2 = 0.f;
    fg_load4(dY + row * lddy + 4 * lane, dq);
    hg_ln_row(x, xh, rstd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sg[i] += dq[i] * xh[i];
      sb[i] += dq[i];
      dxh[i] = dq[i] * gq[i];
      s1 += dxh[i];
      s2 += dxh[i] * xh[i];
    }
    const float c1 = wave_sum(s1) * (1.0f / DM), c2 = wave_sum(s2) * (1.0f / DM);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = rstd * (dxh[i] - c1 - xh[i] * c2);
      sz[i] += o[i];
    }
    *reinterpret_cast<f32x4*>(dS + row * DM + 4 * lane) = o;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    red[wave][0][4 * lane + i] = sg[i];
    red[wave][1][4 * lane + i] = sb[i];
    red[wave][2][4 * lane + i] = sz[i];
  }
  __syncthreads();
  const int c = threadIdx.x;
#pragma unroll
  for (int q = 0; q < 3; ++q)
    part[((long)blockIdx.x * 3 + q) * DM + c] = (red[0][q][c] + red[1][q][c]) + (red[2][q][c] + red[3][q][c]);
}

// part[block][n] = sums over FG_CS_ROWS rows each of P [rows, ld]
__global__ __launch_bounds__(256) void fg_colsum_kernel(const float* __restrict__ P, long ld, int rows, int n, float* __restrict__ part) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const int r0 = blockIdx.y * FG_CS_ROWS, r1 = min(rows, r0 + FG_CS_ROWS);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += P[(long)r * ld + c];
  part[(long)blockIdx.y * n + c] = s;
}

// out[c] = sum_k part[k stride + c], k < npart, for n columns: a workgroup owns 16 columns, its 16 row groups q take k = q, q + 16, ..;
// every thread four independent float64 sums (k, k + 16, k + 32, k + 48 of a round of 64), added in a fixed order, then the row groups
// by a fixed tree in LDS
__global__ __launch_bounds__(256) void fg_colreduce_kernel(const float* __restrict__ part, int npart, long stride, int n,
                                                           float* __restrict__ out) {
  __shared__ double red[16][16];
  const int cl = threadIdx.x & 15, q = threadIdx.x >> 4, c = blockIdx.x * 16 + cl;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (c < n) {
    for (int k = q; k < npart; k += 64) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (k + 16 * u < npart) s[u] += (double)part[(long)(k + 16 * u) * stride + c];
    }
  }
  red[q][cl] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
#pragma unroll
  for (int w = 8; w >= 1; w >>= 1) {
    if (q < w) red[q][cl] += red[q + w][cl];
    __syncthreads();
  }
  if (q == 0 && c < n) out[c] = (float)red[0][cl];
}

// out[e] = (beta ? out[e] : 0) + sum of the slabs in slab order (float64)
__global__ __launch_bounds__(256) void fg_slab_add_kernel(const float* __restrict__ slab, int nslab, long n, float* __restrict__ out, int beta) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double s = 0.0;
  for (int k = 0; k < nslab; ++k) s += (double)slab[(long)k * n + e];
  out[e] = (float)(beta ? (double)out[e] + s : s);
}

inline size_t fg_up(size_t n) { return (n + 255) & ~size_t(255); }

#define FG_CHK(...) do { int _e = (__VA_ARGS__); if (_e != 0) return _e; } while (0)

}  // namespace
