// The attention backward's core, stated once for the ops that use it (attn_grad.hip and scene_attn_grad.hip under a key-padding mask,
// self_attn_grad.hip under the multi-agent causal mask; decoder_layer_grad.hip and encoder_layer_grad.hip drive them): the head-tile
// helpers, the three kernels as templates over a MASK POLICY, and the host steps the launchers share.  Internal linkage, like hg_gemm.h:
// one set of instantiations per including file — ag_fwd_kernel / ag_dq_kernel / ag_dkv_kernel<AgPadMask> (ag_pad_mask.h) in attn_grad.hip
// and scene_attn_grad.hip, <SaCausalMask> in self_attn_grad.hip.
//
// THE CORE.  One wave = a 32 x 32 tile of scores.  ag_fwd / ag_dq: a workgroup = 128 queries of one (context, head), the query on the
// lane (S^T = K Q^T as attention.hip), so that max, sum, delta and the statistics are lane-local and the score registers are the B
// operand of the next product (O^T += V^T P^T, dQ^T += K^T dSc^T).  ag_dkv: a workgroup = 64 keys of one (context, head), the KEY on the
// lane (S = Q K^T), walking the query blocks of its context in order with dV^T and dK^T in registers; waves 0, 1 take the even, waves
// 2, 3 the odd 32-query blocks and are added in that order at the end.  A key tile has one owner: no partial slabs, no atomics.
// Tiles are staged against the context's real row counts (Lq, Lk), never against a policy's tile range: a row inside the context is data.
//
// A MASK POLICY is passed by value beside the operands; it carries the op's launch parameters and, once set_query / set_key has run, the
// lane's own state.  It supplies exactly
//   REVERSE                    query blocks of ag_fwd / ag_dq walked from the last to the first (the longest key ranges first)
//   KeyTile, stage_keys        the 64 staged keys' metadata in LDS (ag_fwd, ag_dq);  QueryTile, stage_queries: the 64 queries' (ag_dkv)
//   set_query, set_key         the lane's query (clamped to the context); the lane's key and the first key of its wave
//   key_end(q)                 one past the last key that queries up to q see: the key loops of a wave and of a workgroup end there
//   first_query(kb), beyond(q) ag_dkv: the first query block that sees keys from kb on; the wave's keys lie wholly beyond queries up to q
//   band(q)                    the first key that not every query from q on sees: a 32-key tile wholly below it is FULL, the mask is not
//                              evaluated there (AG_NO_BAND: no tile ever is)
//   score(tile, s, jj)         ag_fwd: the score of (lane's query, staged key jj), -inf where masked — its exp2 is exactly 0
//   key_visible(tile, jj)      ag_dq: that pair is visible;  query_visible(tile, q): ag_dkv, (staged query q, lane's key) — P is selected
//                              to exactly 0 where not
#pragma once
#include "fg_reduce.h"

#define AG_P 36                  // LDS row stride of a 64 x 32 head tile (floats): 16-byte aligned rows

namespace {

constexpr int AG_NO_BAND = -0x7fffffff - 1;                        // a policy's band() where no tile is ever wholly visible
constexpr float AG_RS = 0.17677669529663687f;                      // 1 / sqrt(32)
constexpr float AG_SCALE = 0.17677669529663687f * 1.4426950408889634f;   // log2(e) / sqrt(32): scores live in the log2 domain

// Where the operands of one launch live: context 0 of the launch, head 0.  Q / dQ rows have ldq floats; K | V and dK | dV are halves of
// the same rows of ldk floats in both ops (V = KV + 256: a lane's K and V addresses differ by a constant); dO, O [contexts Lq, 256] and
// the statistics [contexts Lq, 8] are dense.
struct AgOperands {
  const float *Q, *KV, *dO;
  float *O, *dQ, *dKV, *smax, *slog, *delta;
  int ldq, ldk, Lq, Lk;
};

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

// ---- O [rows, 256] and the statistics (max, log2 of the sum; log2 domain) of every (row, head)
template <class Mask>
__global__ __launch_bounds__(256) void ag_fwd_kernel(const AgOperands a, Mask m) {
  __shared__ __attribute__((aligned(16))) float Ks[64 * AG_P];
  __shared__ __attribute__((aligned(16))) float Vs[64 * AG_P];
  __shared__ typename Mask::KeyTile mt;
  __shared__ float ot[4][32 * 33];
  const int Lq = a.Lq, Lk = a.Lk;
  const int b = blockIdx.z, h = blockIdx.y, qb = (Mask::REVERSE ? gridDim.x - 1 - blockIdx.x : blockIdx.x) * 128;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const float NEG_INF = -__builtin_inff();
  const int qw = qb + wave * 32, qi = qw + l31, qrow = qi < Lq ? qi : Lq - 1;
  const bool active = qw < Lq;                            // (wave-uniform, like everything derived from qw below)
  m.set_query(b, qrow, Lk);
  const int kend_w = m.key_end(qw + 31, Lq, Lk), kend_b = m.key_end(qb + 127, Lq, Lk), band_w = m.band(min(qw, Lq - 1));
  const float* kvb = a.KV + (long)b * Lk * a.ldk + h * HD;
  f32x4 qf[4];
  ag_frag(a.Q + ((long)b * Lq + qrow) * a.ldq + h * HD + half * 4, qf);
#pragma unroll
  for (int j = 0; j < 4; ++j) qf[j] *= AG_SCALE;
  float oacc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
  float m_run = NEG_INF, l_run = 0.f;
  for (int k0 = 0; k0 < kend_b; k0 += 64) {
    __syncthreads();                                     // the previous tile has been read
    ag_stage(kvb, a.ldk, k0, Lk, Ks, tid);
    ag_stage(kvb + DM, a.ldk, k0, Lk, Vs, tid);
    m.stage_keys(mt, k0, Lk, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int j0 = k0 + sub * 32;
      if (!active || j0 >= kend_w) continue;             // (the barriers are outside)
      const bool full = j0 + 31 < band_w;
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
      const float* kr = Ks + (sub * 32 + l31) * AG_P + half * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 kf = *reinterpret_cast<const f32x4*>(kr + j * 8);
#pragma unroll
        for (int c = 0; c < 4; ++c) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[c], qf[j][c], s, 0, 0, 0);
      }
      float sc[16], tmax = NEG_INF;
      if (full) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = s[r];
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = m.score(mt, s[r], sub * 32 + mfma_row(r, half));
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, sc[r]);
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
      const float m_new = fmaxf(m_run, tmax);
      const float m_use = (m_new == NEG_INF) ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);   // m_run = -inf -> 0
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[r] = __builtin_amdgcn_exp2f(sc[r] - m_use);
        psum += sc[r];
      }
      psum += __shfl_xor(psum, 32, 64);
      l_run = l_run * alpha + psum;
      m_run = m_new;
      f32x16 o;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = oacc[r] * alpha;
      const float* vr = Vs + (sub * 32) * AG_P + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[mfma_row(r, half) * AG_P], sc[r], o, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[r] = o[r];
    }
  }
  if (!active) return;                                    // (no barrier follows)
  const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;     // every key masked: O = 0
  ag_store_t(oacc, inv, ot[wave], a.O + ((long)b * Lq + qw) * DM + h * HD, DM, Lq - qw, l31, half);
  if (half == 0 && qi < Lq) {
    const long e = ((long)b * Lq + qi) * NHEAD + h;
    a.smax[e] = l_run > 0.f ? m_run : 0.f;                 // finite in every case: a masked key's P is exp2(-inf - finite) = 0
    a.slog[e] = l_run > 0.f ? log2f(l_run) : 0.f;
  }
}

// ---- delta [rows, 8] = sum_keys P o dP and dQ = sum_keys dSc K / sqrt(32); P = exp2(s - max - log2sum), dP = dO V^T, dSc = P o (dP - delta)
template <class Mask>
__global__ __launch_bounds__(256) void ag_dq_kernel(const AgOperands a, Mask m) {
  __shared__ __attribute__((aligned(16))) float Ks[64 * AG_P];
  __shared__ __attribute__((aligned(16))) float Vs[64 * AG_P];
  __shared__ typename Mask::KeyTile mt;
  __shared__ float ot[4][32 * 33];
  const int Lq = a.Lq, Lk = a.Lk;
  const int b = blockIdx.z, h = blockIdx.y, qb = (Mask::REVERSE ? gridDim.x - 1 - blockIdx.x : blockIdx.x) * 128;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int qw = qb + wave * 32, qi = qw + l31, qrow = qi < Lq ? qi : Lq - 1;
  const bool active = qw < Lq;
  m.set_query(b, qrow, Lk);
  const int kend_w = m.key_end(qw + 31, Lq, Lk), kend_b = m.key_end(qb + 127, Lq, Lk), band_w = m.band(min(qw, Lq - 1));
  const long row = (long)b * Lq + qrow;
  const float* kvb = a.KV + (long)b * Lk * a.ldk + h * HD;
  f32x4 qf[4], dof[4];
  ag_frag(a.Q + row * a.ldq + h * HD + half * 4, qf);
  ag_frag(a.dO + row * DM + h * HD + half * 4, dof);
#pragma unroll
  for (int j = 0; j < 4; ++j) qf[j] *= AG_SCALE;
  const float mq = a.smax[row * NHEAD + h], lq = a.slog[row * NHEAD + h];
  float dl = 0.f;
  float dq[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) dq[r] = 0.f;
  // two passes over the key tiles: delta = sum_keys P dP first, from the very P and dP (bit for bit) that the second pass takes it from
  // again — where one key holds nearly all of a row's weight, dSc = P (dP - delta) is a difference of nearly equal numbers, and the
  // rounding of dP cancels in it only if delta carries the same rounding (rowsum(dO o O), the same number in exact arithmetic, does
  // not: measured at one key per query, 19 times float32 autograd's error in dX instead of exactly 0)
  for (int pass = 0; pass < 2; ++pass) {
  for (int k0 = 0; k0 < kend_b; k0 += 64) {
    __syncthreads();
    ag_stage(kvb, a.ldk, k0, Lk, Ks, tid);
    ag_stage(kvb + DM, a.ldk, k0, Lk, Vs, tid);
    m.stage_keys(mt, k0, Lk, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int j0 = k0 + sub * 32;
      if (!active || j0 >= kend_w) continue;
      const bool full = j0 + 31 < band_w;
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
      const float* kr = Ks + (sub * 32 + l31) * AG_P + half * 4;
      const float* vq = Vs + (sub * 32 + l31) * AG_P + half * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 kf = *reinterpret_cast<const f32x4*>(kr + j * 8);
        const f32x4 vf = *reinterpret_cast<const f32x4*>(vq + j * 8);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[c], qf[j][c], s, 0, 0, 0);        // S^T  = K Q^T
          dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[c], dof[j][c], dp, 0, 0, 0);     // dP^T = V dO^T
        }
      }
      float dsc[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) dsc[r] = __builtin_amdgcn_exp2f((s[r] - mq) - lq);      // P
      if (!full) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dsc[r] = m.key_visible(mt, sub * 32 + mfma_row(r, half)) ? dsc[r] : 0.f;
      }
      if (pass == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dl += dsc[r] * dp[r];
        continue;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) dsc[r] *= dp[r] - dl;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = dq[r];
      const float* kt = Ks + (sub * 32) * AG_P + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kt[mfma_row(r, half) * AG_P], dsc[r], acc, 0, 0, 0);   // dQ^T += K^T dSc^T
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[r] = acc[r];
    }
  }
  if (pass == 0) {
    dl += __shfl_xor(dl, 32, 64);
    if (half == 0 && qi < Lq) a.delta[row * NHEAD + h] = dl;
  }
  }
  if (!active) return;
  ag_store_t(dq, AG_RS, ot[wave], a.dQ + ((long)b * Lq + qw) * a.ldq + h * HD, a.ldq, Lq - qw, l31, half);
}

// ---- dK = sum_queries dSc^T Q / sqrt(32) and dV = sum_queries P^T dO: one workgroup per (context, head, 64 keys)
template <class Mask>
__global__ __launch_bounds__(256) void ag_dkv_kernel(const AgOperands a, Mask m) {
  __shared__ __attribute__((aligned(16))) float Qs[64 * AG_P];
  __shared__ __attribute__((aligned(16))) float Ds[64 * AG_P];
  __shared__ float sm[64], sl[64], sd[64];
  __shared__ typename Mask::QueryTile mt;
  __shared__ float red[2][2 * 16 * 64];                 // [key half][dV, dK]: the odd query blocks' sums; then the wave's transpose patch
  const int Lq = a.Lq, Lk = a.Lk;
  const int b = blockIdx.z, h = blockIdx.y, kb = blockIdx.x * 64;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int ksub = wave & 1, qsub = wave >> 1;
  const int j0 = kb + ksub * 32, key = j0 + l31, krow = key < Lk ? key : Lk - 1;
  const bool active = j0 < Lk;
  m.set_key(b, j0, key, Lk);
  f32x4 kf[4], vf[4];
  const float* kp = a.KV + ((long)b * Lk + krow) * a.ldk + h * HD + half * 4;
  ag_frag(kp, kf);
  ag_frag(kp + DM, vf);
  const float* Qb = a.Q + (long)b * Lq * a.ldq + h * HD;
  const float* Db = a.dO + (long)b * Lq * DM + h * HD;
  float dv[16], dk[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dv[r] = 0.f; dk[r] = 0.f; }
  for (int q0 = m.first_query(kb); q0 < Lq; q0 += 64) {
    __syncthreads();
    ag_stage(Qb, a.ldq, q0, Lq, Qs, tid);
    ag_stage(Db, DM, q0, Lq, Ds, tid);
    if (tid < 64) {
      const int q = q0 + tid;
      const long e = ((long)b * Lq + (q < Lq ? q : Lq - 1)) * NHEAD + h;
      sm[tid] = q < Lq ? a.smax[e] : __builtin_inff();   // a query beyond Lq: P = exp2(0 - inf) = 0
      sl[tid] = q < Lq ? a.slog[e] : 0.f;
      sd[tid] = q < Lq ? a.delta[e] : 0.f;
    }
    m.stage_queries(mt, q0, tid);
    __syncthreads();
    const int qlo = q0 + qsub * 32;
    if (!active || qlo >= Lq) continue;                 // (wave-uniform; the barriers above are outside)
    if (m.beyond(qlo + 31, Lq)) continue;               // the keys lie wholly beyond what these queries see
    const bool full = j0 + 31 < m.band(qlo);
    f32x16 s, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
    const float* qr = Qs + (qsub * 32 + l31) * AG_P + half * 4;
    const float* dr = Ds + (qsub * 32 + l31) * AG_P + half * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 qv = *reinterpret_cast<const f32x4*>(qr + j * 8);
      const f32x4 dv4 = *reinterpret_cast<const f32x4*>(dr + j * 8);
      qv *= AG_SCALE;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[c], kf[j][c], s, 0, 0, 0);          // S  = Q K^T
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(dv4[c], vf[j][c], dp, 0, 0, 0);       // dP = dO V^T
      }
    }
    float pr[16], dsc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = qsub * 32 + mfma_row(r, half);
      float p = __builtin_amdgcn_exp2f((s[r] - sm[q]) - sl[q]);
      if (!full) p = m.query_visible(mt, q) ? p : 0.f;
      pr[r] = p;
      dsc[r] = p * (dp[r] - sd[q]);
    }
    f32x16 av, ak;
#pragma unroll
    for (int r = 0; r < 16; ++r) { av[r] = dv[r]; ak[r] = dk[r]; }
    const float* qt = Qs + (qsub * 32) * AG_P + l31;
    const float* dt = Ds + (qsub * 32) * AG_P + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      av = __builtin_amdgcn_mfma_f32_32x32x2f32(dt[mfma_row(r, half) * AG_P], pr[r], av, 0, 0, 0);    // dV^T += dO^T P
      ak = __builtin_amdgcn_mfma_f32_32x32x2f32(qt[mfma_row(r, half) * AG_P], dsc[r], ak, 0, 0, 0);   // dK^T += Q^T dSc
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { dv[r] = av[r]; dk[r] = ak[r]; }
  }
  __syncthreads();
  if (qsub == 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      red[ksub][r * 64 + lane] = dv[r];
      red[ksub][1024 + r * 64 + lane] = dk[r];
    }
  }
  __syncthreads();
  if (qsub == 0 && active) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dv[r] += red[ksub][r * 64 + lane];
      dk[r] += red[ksub][1024 + r * 64 + lane];
    }
    __builtin_amdgcn_wave_barrier();
    float* out = a.dKV + ((long)b * Lk + j0) * a.ldk + h * HD;
    ag_store_t(dk, AG_RS, red[ksub], out, a.ldk, Lk - j0, l31, half);
    ag_store_t(dv, 1.0f, red[ksub], out + DM, a.ldk, Lk - j0, l31, half);
  }
}

// ---- the host steps the two ops' launchers share

// contexts per chunk of query rows: whole contexts, at most 8192 rows where a context has no more
inline int ag_chunk_contexts(int B, int L) {
  const int cc = 8192 / L;
  return cc < 1 ? 1 : cc > B ? B : cc;
}

// `grads` of either op: in_proj_weight [768, 256], in_proj_bias [768], out_proj.weight [256, 256], out_proj.bias, norm weight, norm bias
constexpr long AG_NGRADS = 4L * DM * DM + 6 * DM;
struct AgGrads { float *Win, *bin, *Wo, *bo, *g, *be; };
inline AgGrads ag_grads(float* grads) {
  AgGrads g;
  g.Win = grads; g.bin = g.Win + 3L * DM * DM; g.Wo = g.bin + 3 * DM; g.bo = g.Wo + (long)DM * DM; g.g = g.bo + DM; g.be = g.g + DM;
  return g;
}

// Steps 3 to 6 of a chunk of nr rows: S = Xc + O Wo^T + bo; dS = LayerNorm backward of dYc, its block partials (dY xhat, dY, dS) behind
// the cursor nln; dWo (+)= dS^T O by slabs; dO = dS Wo, over S
inline int ag_out_proj_bwd(const float* Xc, int ldx, const float* dYc, int lddy, const float* O, const float* Wo, const float* bo,
                           const float* gamma, float* S, float* dS, float* slab, float* gWo, int nr, int acc, float* pln, long& nln,
                           hipStream_t st) {
  const long wsz = (long)DM * DM;
  FG_CHK(hg_gemm_t<true, true, HG_EPI_RES>(HgGemm{O, DM, 1, Wo, 1, DM, S, DM, 0, bo, nr, DM, DM, DM, 0, Xc, ldx}, st));
  const int nb = (nr + FG_LN_ROWS - 1) / FG_LN_ROWS;
  hipLaunchKernelGGL(fg_ln_bwd_kernel, dim3(nb), dim3(256), 0, st, S, gamma, dYc, (long)lddy, dS, nr, pln + nln * 3 * DM);
  nln += nb;
  FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{dS, 1, DM, O, DM, 1, slab, DM, wsz, nullptr, DM, DM, nr, FG_KS, 0}, st));
  hipLaunchKernelGGL(fg_slab_add_kernel, dim3((unsigned)((wsz + 255) / 256)), dim3(256), 0, st, slab, (nr + FG_KS - 1) / FG_KS, wsz, gWo, acc);
  return hg_gemm_t<true, false, HG_EPI_PLAIN>(HgGemm{dS, DM, 1, Wo, DM, 1, S, DM, 0, nullptr, nr, DM, DM, DM, 0}, st);
}

// behind the chunks: the LayerNorm backward's partial rows [3][256] = (dY xhat, dY, dS) -> dgamma, dbeta, dbo
inline void ag_ln_reduce(const float* pln, long nln, const AgGrads& g, hipStream_t st) {
  float* const col3[3] = {g.g, g.be, g.bo};
  for (int q = 0; q < 3; ++q)
    hipLaunchKernelGGL(fg_colreduce_kernel, dim3(DM / 16), dim3(256), 0, st, pln + q * DM, (int)nln, 3L * DM, DM, col3[q]);
}

}  // namespace
