// The head-tile helpers the attention backward files share (attn_grad.hip, self_attn_grad.hip): a 64 x 32 head tile staged in LDS, a
// lane's fragment of a row's 32 head columns, and the transposed store of a wave's 32 x 32 accumulator tile.  Internal linkage, like
// hg_gemm.h: one set of instantiations per including file.
#pragma once
#include "fg_reduce.h"

#define AG_P 36                  // LDS row stride of a 64 x 32 head tile (floats): 16-byte aligned rows

namespace {

constexpr float AG_RS = 0.17677669529663687f;                      // 1 / sqrt(32)
constexpr float AG_SCALE = 0.17677669529663687f * 1.4426950408889634f;   // log2(e) / sqrt(32): scores live in the log2 domain

// 64 rows x 32 columns of P (rows r0 .., the columns P points at); rows at or beyond R read as zero.  256 threads.
__device__ __forceinline__ void ag_stage(const float* __restrict__ P, long ld, int r0, int R, float* T, int tid) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = tid + 256 * i, r = idx >> 3, c = (idx & 7) * 4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r0 + r < R) v = *reinterpret_cast<const f32x4*>(P + (long)(r0 + r) * ld + c);
    *reinterpret_cast<f32x4*>(T + r * AG_P + c) = v;
  }
}
// a lane's 16 of a row's 32 head columns: element (j, c) = column 8 j + 4 half + c (p already points at 4 half) — the k slots of the
// sixteen MFMA steps that sum over the head dimension
__device__ __forceinline__ void ag_frag(const float* p, f32x4 (&f)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) f[j] = *reinterpret_cast<const f32x4*>(p + 8 * j);
}
// v[r] = T[y = mfma_row(r, half)][x = lane & 31] of a wave's tile, times scale -> out[x ld + y] for x < nx, through the wave's patch ot
__device__ __forceinline__ void ag_store_t(const float (&v)[16], float scale, float* ot, float* __restrict__ out, long ld, int nx, int l31,
                                           int half) {
#pragma unroll
  for (int r = 0; r < 16; ++r) ot[l31 * 33 + mfma_row(r, half)] = v[r] * scale;
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int x = 2 * i + half;
    if (x < nx) out[(long)x * ld + l31] = ot[x * 33 + l31];
  }
  __builtin_amdgcn_wave_barrier();
}

}  // namespace
