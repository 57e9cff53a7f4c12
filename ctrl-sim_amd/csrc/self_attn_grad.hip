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
//   2. O and the statistics                           sa_fwd_kernel
//   3. S = X + O Wo^T + bo                            (HG_EPI_RES)
//   4. dS = LayerNorm backward of dY; partials (dY xhat, dY, dS): dg, dbe, dbo
//   5. dWo (+)= dS^T O            6. dO = dS Wo, over S
//   7. delta and dQ -> dQKV[:, 0:256]                 sa_dq_kernel
//   8. dK | dV      -> dQKV[:, 256:768]               sa_dkv_kernel
//   9. dWin (+)= dQKV^T X  (one product)       10. dbin partials       11. dX = dS + dQKV Win  (one product with K = 768, HG_EPI_RES)
// hg_gemm.h serves all of them without a new epilogue.
//
// THE ATTENTION CORE is attn_grad.hip's (one wave = a 32 x 32 tile of scores; sa_fwd / sa_dq: 128 queries of one (context, head) per
// workgroup, the query on the lane; sa_dkv: 64 keys per workgroup, the key on the lane, waves 0, 1 the even and waves 2, 3 the odd
// 32-query blocks, added in that order) with the mask's structure on top.  With A3 = 3A keys per timestep, a wave's 32 queries span the
// timesteps t_lo .. t_hi, and a 32-key tile [j0, j0 + 32) is
//   skipped    where j0 >= (t_hi + 1) A3: wholly beyond the last visible key — about half of the score matrix is never computed; the
//              workgroup's tile loops end at its last query's band (sa_fwd, sa_dq) or begin at its first key's (sa_dkv);
//   unmasked   in mode 0 where j0 + 31 < t_lo A3: wholly below the first timestep row of the wave's queries, every pair visible;
//   masked     otherwise: the closed form per pair, from the pair's (t, a, k) — the tile's 64 keys' (sa_fwd, sa_dq) or 64 queries'
//              (sa_dkv) triples are computed once per tile into LDS, the lane's own once per kernel.
// Mode 1 evaluates the closed form in EVERY visited tile (below the band visibility depends on the agent pair: no tile of 32 keys is
// wholly visible once A >= 2); its work is the same MFMA count as mode 0's, the mask costs VALU only.
#include "ag_tile.h"
#include "../../include/ctrlsim.h"

namespace {

// (tq, aq, kq): the query's triple; tj and akj = 4 a_j + k_j: the key's.  A key at or beyond L has t_j >= T: never visible.
__device__ __forceinline__ bool sa_visible(int mode, int tq, int aq, int kq, int tj, int akj) {
  const int kj = akj & 3;
  const bool same = (akj >> 2) == aq, state = kj == 0;
  return tj < tq ? (mode == 0 || same || state) : (tj == tq && ((same && kj <= kq) || state));
}
// the 64 tokens i0 .. of a tile: timestep and 4 a + k
__device__ __forceinline__ void sa_triples(int i0, int A, int A3, int* tt, int* tak, int tid) {
  if (tid < 64) {
    const int i = i0 + tid;
    tt[tid] = i / A3;
    tak[tid] = (((i / 3) % A) << 2) | (i % 3);
  }
}

// ---- 2. O [rows, 256] and the statistics of every (row, head)
__global__ __launch_bounds__(256) void sa_fwd_kernel(const float* __restrict__ QKV, float* __restrict__ O, float* __restrict__ smax,
                                                     float* __restrict__ slog, int L, int A, int mode) {
  __shared__ __attribute__((aligned(16))) float Ks[64 * AG_P];
  __shared__ __attribute__((aligned(16))) float Vs[64 * AG_P];
  __shared__ int kt[64], kak[64];
  __shared__ float ot[4][32 * 33];
  const int b = blockIdx.z, h = blockIdx.y, qb = (gridDim.x - 1 - blockIdx.x) * 128, A3 = 3 * A;   // the longest key ranges first
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const float NEG_INF = -__builtin_inff();
  const int qw = qb + wave * 32, qi = qw + l31, qrow = qi < L ? qi : L - 1;
  const int tq = qrow / A3, aq = (qrow / 3) % A, kq = qrow % 3;
  const bool active = qw < L;                                       // (wave-uniform, like everything derived from qw below)
  const int band_w = (min(qw, L - 1) / A3) * A3;                    // the first key of the wave's first timestep
  const int kend_w = min(L, (min(qw + 31, L - 1) / A3 + 1) * A3);   // one past the wave's last visible key
  const int kend_b = min(L, (min(qb + 127, L - 1) / A3 + 1) * A3);  // ... the workgroup's
  const float* base = QKV + (long)b * L * (3 * DM) + h * HD;
  f32x4 qf[4];
  ag_frag(base + (long)qrow * (3 * DM) + half * 4, qf);
#pragma unroll
  for (int j = 0; j < 4; ++j) qf[j] *= AG_SCALE;
  float oacc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
  float m_run = NEG_INF, l_run = 0.f;
  for (int k0 = 0; k0 < kend_b; k0 += 64) {
    __syncthreads();                                     // the previous tile has been read
    ag_stage(base + DM, 3 * DM, k0, L, Ks, tid);
    ag_stage(base + 2 * DM, 3 * DM, k0, L, Vs, tid);
    sa_triples(k0, A, A3, kt, kak, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int j0 = k0 + sub * 32;
      if (!active || j0 >= kend_w) continue;             // (the barriers are outside)
      const bool full = mode == 0 && j0 + 31 < band_w;
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
        for (int r = 0; r < 16; ++r) {
          const int jj = sub * 32 + mfma_row(r, half);
          sc[r] = sa_visible(mode, tq, aq, kq, kt[jj], kak[jj]) ? s[r] : NEG_INF;      // selected by index: exp2 below gives exactly 0
        }
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
  const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;     // (every row sees itself: l_run > 0)
  ag_store_t(oacc, inv, ot[wave], O + ((long)b * L + qw) * DM + h * HD, DM, L - qw, l31, half);
  if (half == 0 && qi < L) {
    const long e = ((long)b * L + qi) * NHEAD + h;
    smax[e] = l_run > 0.f ? m_run : 0.f;
    slog[e] = l_run > 0.f ? log2f(l_run) : 0.f;
  }
}

// ---- 7. delta [rows, 8] and dQ -> dQKV[:, 0:256]
__global__ __launch_bounds__(256) void sa_dq_kernel(const float* __restrict__ QKV, const float* __restrict__ dO, const float* __restrict__ smax,
                                                    const float* __restrict__ slog, float* __restrict__ delta, float* __restrict__ dQKV,
                                                    int L, int A, int mode) {
  __shared__ __attribute__((aligned(16))) float Ks[64 * AG_P];
  __shared__ __attribute__((aligned(16))) float Vs[64 * AG_P];
  __shared__ int kt[64], kak[64];
  __shared__ float ot[4][32 * 33];
  const int b = blockIdx.z, h = blockIdx.y, qb = (gridDim.x - 1 - blockIdx.x) * 128, A3 = 3 * A;   // the longest key ranges first
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int qw = qb + wave * 32, qi = qw + l31, qrow = qi < L ? qi : L - 1;
  const int tq = qrow / A3, aq = (qrow / 3) % A, kq = qrow % 3;
  const bool active = qw < L;
  const int band_w = (min(qw, L - 1) / A3) * A3;
  const int kend_w = min(L, (min(qw + 31, L - 1) / A3 + 1) * A3);
  const int kend_b = min(L, (min(qb + 127, L - 1) / A3 + 1) * A3);
  const long row = (long)b * L + qrow;
  const float* base = QKV + (long)b * L * (3 * DM) + h * HD;
  f32x4 qf[4], dof[4];
  ag_frag(base + (long)qrow * (3 * DM) + half * 4, qf);
  ag_frag(dO + row * DM + h * HD + half * 4, dof);
#pragma unroll
  for (int j = 0; j < 4; ++j) qf[j] *= AG_SCALE;
  const float mq = smax[row * NHEAD + h], lq = slog[row * NHEAD + h];
  float dl = 0.f;
  float dq[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) dq[r] = 0.f;
  // two passes over the key tiles, as attn_grad.hip's ag_dq_kernel: delta = sum_keys P dP first, from the very P and dP (bit for bit) that
  // the second pass takes dSc = P (dP - delta) from
  for (int pass = 0; pass < 2; ++pass) {
  for (int k0 = 0; k0 < kend_b; k0 += 64) {
    __syncthreads();
    ag_stage(base + DM, 3 * DM, k0, L, Ks, tid);
    ag_stage(base + 2 * DM, 3 * DM, k0, L, Vs, tid);
    sa_triples(k0, A, A3, kt, kak, tid);
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int j0 = k0 + sub * 32;
      if (!active || j0 >= kend_w) continue;
      const bool full = mode == 0 && j0 + 31 < band_w;
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
        for (int r = 0; r < 16; ++r) {
          const int jj = sub * 32 + mfma_row(r, half);
          dsc[r] = sa_visible(mode, tq, aq, kq, kt[jj], kak[jj]) ? dsc[r] : 0.f;
        }
      }
      if (pass == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) dl += dsc[r] * dp[r];
        continue;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) dsc[r] *= dp[r] - dl;
      f32x16 a;
#pragma unroll
      for (int r = 0; r < 16; ++r) a[r] = dq[r];
      const float* ktile = Ks + (sub * 32) * AG_P + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) a = __builtin_amdgcn_mfma_f32_32x32x2f32(ktile[mfma_row(r, half) * AG_P], dsc[r], a, 0, 0, 0);   // dQ^T += K^T dSc^T
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[r] = a[r];
    }
  }
  if (pass == 0) {
    dl += __shfl_xor(dl, 32, 64);
    if (half == 0 && qi < L) delta[row * NHEAD + h] = dl;
  }
  }
  if (!active) return;
  ag_store_t(dq, AG_RS, ot[wave], dQKV + ((long)b * L + qw) * (3 * DM) + h * HD, 3 * DM, L - qw, l31, half);
}

// ---- 8. dK | dV -> dQKV[:, 256:768]: one workgroup per (context, head, 64 keys)
__global__ __launch_bounds__(256) void sa_dkv_kernel(const float* __restrict__ QKV, const float* __restrict__ dO, const float* __restrict__ smax,
                                                     const float* __restrict__ slog, const float* __restrict__ delta, float* __restrict__ dQKV,
                                                     int L, int A, int mode) {
  __shared__ __attribute__((aligned(16))) float Qs[64 * AG_P];
  __shared__ __attribute__((aligned(16))) float Ds[64 * AG_P];
  __shared__ float sm[64], sl[64], sd[64];
  __shared__ int qt[64], qak[64];
  __shared__ float red[2][2 * 16 * 64];                 // [key half][dV, dK]: the odd query blocks' sums; then the wave's transpose patch
  const int b = blockIdx.z, h = blockIdx.y, kb = blockIdx.x * 64, A3 = 3 * A;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int ksub = wave & 1, qsub = wave >> 1;
  const int j0 = kb + ksub * 32, key = j0 + l31, krow = key < L ? key : L - 1;
  const int tk = key / A3, akk = (((key / 3) % A) << 2) | (key % 3);     // (a key at or beyond L: t >= T, visible to no query)
  const bool active = j0 < L;
  const int tk0 = j0 / A3;                              // the first timestep of the wave's keys
  f32x4 kf[4], vf[4];
  const float* base = QKV + (long)b * L * (3 * DM) + h * HD;
  ag_frag(base + (long)krow * (3 * DM) + DM + half * 4, kf);
  ag_frag(base + (long)krow * (3 * DM) + 2 * DM + half * 4, vf);
  const float* Db = dO + (long)b * L * DM + h * HD;
  float dv[16], dk[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dv[r] = 0.f; dk[r] = 0.f; }
  // query blocks wholly before the first key's timestep see none of these keys (a multiple of 64: even / odd blocks keep their waves)
  for (int q0 = (((kb / A3) * A3) / 64) * 64; q0 < L; q0 += 64) {
    __syncthreads();
    ag_stage(base, 3 * DM, q0, L, Qs, tid);
    ag_stage(Db, DM, q0, L, Ds, tid);
    if (tid < 64) {
      const int q = q0 + tid;
      const long e = ((long)b * L + (q < L ? q : L - 1)) * NHEAD + h;
      sm[tid] = q < L ? smax[e] : __builtin_inff();      // a query beyond L: P = exp2(0 - inf) = 0
      sl[tid] = q < L ? slog[e] : 0.f;
      sd[tid] = q < L ? delta[e] : 0.f;
    }
    sa_triples(q0, A, A3, qt, qak, tid);
    __syncthreads();
    const int qlo = q0 + qsub * 32;
    if (!active || qlo >= L) continue;                  // (wave-uniform; the barriers above are outside)
    if (tk0 > min(qlo + 31, L - 1) / A3) continue;      // the keys lie wholly beyond the last timestep of these queries
    const bool full = mode == 0 && j0 + 31 < (qlo / A3) * A3;
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
      if (!full) p = sa_visible(mode, qt[q], qak[q] >> 2, qak[q] & 3, tk, akk) ? p : 0.f;
      pr[r] = p;
      dsc[r] = p * (dp[r] - sd[q]);
    }
    f32x16 av, ak;
#pragma unroll
    for (int r = 0; r < 16; ++r) { av[r] = dv[r]; ak[r] = dk[r]; }
    const float* qtile = Qs + (qsub * 32) * AG_P + l31;
    const float* dtile = Ds + (qsub * 32) * AG_P + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      av = __builtin_amdgcn_mfma_f32_32x32x2f32(dtile[mfma_row(r, half) * AG_P], pr[r], av, 0, 0, 0);    // dV^T += dO^T P
      ak = __builtin_amdgcn_mfma_f32_32x32x2f32(qtile[mfma_row(r, half) * AG_P], dsc[r], ak, 0, 0, 0);   // dK^T += Q^T dSc
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
    float* out = dQKV + ((long)b * L + j0) * (3 * DM) + h * HD;
    ag_store_t(dk, AG_RS, red[ksub], out + DM, 3 * DM, L - j0, l31, half);
    ag_store_t(dv, 1.0f, red[ksub], out + 2 * DM, 3 * DM, L - j0, l31, half);
  }
}

}  // namespace

// Workspace behind `base`: the chunk buffers Q | K | V and dQ | dK | dV [chunk rows, 768], O, S (then dO), dS [chunk rows, 256], the three
// statistics [chunk rows, 8], the product slabs of one chunk, and the column-sum partials
SelfAttnGradWs self_attn_grad_carve(size_t base, int B, int L) {
  SelfAttnGradWs w;
  size_t off = fg_up(base);
  auto take = [&](size_t n) { const size_t o = off; off += fg_up(n); return o; };
  int cc = 8192 / L;
  cc = cc < 1 ? 1 : cc > B ? B : cc;
  w.chunk_ctx = cc;
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

int launch_self_attn_block_grad(const float* X, int ldx, const float* dY, int lddy, const float* Win, const float* bin, const float* Wo,
                                const float* bo, const float* gamma, const float* beta, int B, int T, int A, int mask_mode, char* ws,
                                const SelfAttnGradWs& w, float* grads, float* dX, int lddx, hipStream_t st) {
  (void)beta;                                          // the backward of a LayerNorm does not read its bias
  if (!X || !dY || !Win || !bin || !Wo || !bo || !gamma || !ws || !grads || B < 1 || T < 1 || A < 1 || (mask_mode != 0 && mask_mode != 1) ||
      3L * T * A > 0x7fffffffL / (3 * DM) || (long)B * 3 * T * A > 0x7fffffffL / (3 * DM) || ldx < DM || lddy < DM || (dX && lddx < DM) ||
      w.chunk_ctx < 1 || (reinterpret_cast<uintptr_t>(ws) & 15))
    return CTRLSIM_EINVAL;
  const int L = 3 * T * A;
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *QKV = f(w.QKV), *dQKV = f(w.dQKV), *O = f(w.O), *S = f(w.S), *dS = f(w.dS), *slab = f(w.slab);
  float *pln = f(w.part_ln), *pcs = f(w.part_cs);
  const long crows = (long)w.chunk_ctx * L, nstat = crows * NHEAD, wsz = (long)DM * DM;
  float *smax = f(w.stat), *slog = smax + nstat, *delta = slog + nstat, *dO = S;
  float *gWin = grads, *gbin = gWin + 3 * wsz, *gWo = gbin + 3 * DM, *gbo = gWo + wsz, *gg = gbo + DM, *gbe = gg + DM;
  const unsigned nadd = (unsigned)((wsz + 255) / 256);
  long nln = 0, ncs = 0;
  for (int c0 = 0; c0 < B; c0 += w.chunk_ctx) {
    const int nc = B - c0 < w.chunk_ctx ? B - c0 : w.chunk_ctx, nr = nc * L;
    const int acc = c0 > 0, nslab = (nr + FG_KS - 1) / FG_KS;
    const long r0 = (long)c0 * L;
    const float* Xc = X + r0 * ldx;
    const float* dYc = dY + r0 * lddy;
    const dim3 gq((L + 127) / 128, NHEAD, nc), gk((L + 63) / 64, NHEAD, nc);
    // 1. Q | K | V      2. O, statistics      3. S = X + O Wo^T + bo
    FG_CHK(hg_gemm_t<true, true, HG_EPI_PLAIN>(HgGemm{Xc, ldx, 1, Win, 1, DM, QKV, 3 * DM, 0, bin, nr, 3 * DM, DM, DM, 0}, st));
    hipLaunchKernelGGL(sa_fwd_kernel, gq, dim3(256), 0, st, QKV, O, smax, slog, L, A, mask_mode);
    FG_CHK(hg_gemm_t<true, true, HG_EPI_RES>(HgGemm{O, DM, 1, Wo, 1, DM, S, DM, 0, bo, nr, DM, DM, DM, 0, Xc, ldx}, st));
    // 4. dY -> dS, partials of dg, dbe, dbo
    const int nb = (nr + FG_LN_ROWS - 1) / FG_LN_ROWS;
    hipLaunchKernelGGL(fg_ln_bwd_kernel, dim3(nb), dim3(256), 0, st, S, gamma, dYc, (long)lddy, dS, nr, pln + nln * 3 * DM);
    nln += nb;
    // 5. dWo (+)= dS^T O      6. dO = dS Wo, over S
    FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{dS, 1, DM, O, DM, 1, slab, DM, wsz, nullptr, DM, DM, nr, FG_KS, 0}, st));
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3(nadd), dim3(256), 0, st, slab, nslab, wsz, gWo, acc);
    FG_CHK(hg_gemm_t<true, false, HG_EPI_PLAIN>(HgGemm{dS, DM, 1, Wo, DM, 1, dO, DM, 0, nullptr, nr, DM, DM, DM, 0}, st));
    // 7. delta, dQ      8. dK | dV
    hipLaunchKernelGGL(sa_dq_kernel, gq, dim3(256), 0, st, QKV, dO, smax, slog, delta, dQKV, L, A, mask_mode);
    hipLaunchKernelGGL(sa_dkv_kernel, gk, dim3(256), 0, st, QKV, dO, smax, slog, delta, dQKV, L, A, mask_mode);
    // 9. dWin (+)= dQKV^T X      10. dbin partials      11. dX = dS + dQKV Win
    FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{dQKV, 1, 3 * DM, Xc, ldx, 1, slab, DM, 3 * wsz, nullptr, 3 * DM, DM, nr, FG_KS, 0}, st));
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3(3 * nadd), dim3(256), 0, st, slab, nslab, 3 * wsz, gWin, acc);
    const int ncb = (nr + FG_CS_ROWS - 1) / FG_CS_ROWS;
    hipLaunchKernelGGL(fg_colsum_kernel, dim3(3, ncb), dim3(256), 0, st, dQKV, 3L * DM, nr, 3 * DM, pcs + ncs * 3 * DM);
    ncs += ncb;
    if (dX)
      FG_CHK(hg_gemm_t<true, false, HG_EPI_RES>(HgGemm{dQKV, 3 * DM, 1, Win, DM, 1, dX + r0 * lddx, lddx, 0, nullptr, nr, DM, 3 * DM, 3 * DM, 0,
                                                       dS, DM}, st));
  }
  if (nln > w.nln || ncs > w.ncs) return CTRLSIM_EINVAL;
  float* const col3[3] = {gg, gbe, gbo};               // the LayerNorm backward's partial rows are [3][256]: (dY xhat, dY, dS)
  for (int q = 0; q < 3; ++q)
    hipLaunchKernelGGL(fg_colreduce_kernel, dim3(DM / 16), dim3(256), 0, st, pln + q * DM, (int)nln, 3L * DM, DM, col3[q]);
  hipLaunchKernelGGL(fg_colreduce_kernel, dim3(3 * DM / 16), dim3(256), 0, st, pcs, (int)ncs, 3L * DM, 3 * DM, gbin);
  return ctrlsim_launch_status();
}

// Step 2 alone, for decoder_layer_grad.hip's recompute of the sublayer's output: O [nc L, 256] and the statistics [nc L, 8] of nc contexts
int launch_self_attn_fwd_stats(const float* QKV, float* O, float* smax, float* slog, int nc, int L, int A, int mask_mode, hipStream_t st) {
  hipLaunchKernelGGL(sa_fwd_kernel, dim3((L + 127) / 128, NHEAD, nc), dim3(256), 0, st, QKV, O, smax, slog, L, A, mask_mode);
  return ctrlsim_launch_status();
}

// ---- the op as a C ABI entry (include/ctrlsim.h)
namespace {
bool sa_dims_ok(int B, int T, int A) {
  return B >= 1 && T >= 1 && A >= 1 && 3L * T * A <= 0x7fffffffL / (3 * DM) && (long)B * 3 * T * A <= 0x7fffffffL / (3 * DM);
}
}  // namespace
extern "C" int64_t ctrlsim_self_attn_block_grad_workspace_bytes(int B, int T, int A) {
  if (!sa_dims_ok(B, T, A)) return CTRLSIM_EINVAL;
  return (int64_t)self_attn_grad_carve(0, B, 3 * T * A).bytes;
}
extern "C" int ctrlsim_self_attn_block_grad_chunk_contexts(int B, int T, int A) {
  if (!sa_dims_ok(B, T, A)) return CTRLSIM_EINVAL;
  return self_attn_grad_carve(0, B, 3 * T * A).chunk_ctx;
}
extern "C" int ctrlsim_self_attn_block_grad(const float* X, int ldx, const float* dY, int lddy, const float* in_proj_weight,
                                            const float* in_proj_bias, const float* out_proj_weight, const float* out_proj_bias,
                                            const float* gamma, const float* beta, int B, int T, int A, int mask_mode, void* workspace,
                                            float* grads, float* dX, int lddx, hipStream_t stream) {
  if (!sa_dims_ok(B, T, A) || !beta || !workspace) return CTRLSIM_EINVAL;
  return launch_self_attn_block_grad(X, ldx, dY, lddy, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, gamma, beta, B, T, A,
                                     mask_mode, static_cast<char*>(workspace), self_attn_grad_carve(0, B, 3 * T * A), grads, dX, lddx, stream);
}
