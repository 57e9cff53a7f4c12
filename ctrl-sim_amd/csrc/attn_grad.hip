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
// THE ATTENTION CORE.  One wave = a 32 x 32 tile of scores.  ag_fwd / ag_dq: a workgroup = 128 queries of one (context, head), the query
// on the lane (S^T = K Q^T as attention.hip), so that max, sum, delta and the statistics are lane-local and the score registers are the B
// operand of the next product (O^T += V^T P^T, dQ^T += K^T dSc^T).  ag_dkv: a workgroup = 64 keys of one (context, head), the KEY on the
// lane (S = Q K^T), walking all query blocks of its context in order with dV^T and dK^T in registers; waves 0, 1 take the even, waves
// 2, 3 the odd 32-query blocks and are added in that order at the end.  A key tile has one owner: no partial slabs, no atomics.
// Padded keys and keys at or beyond Lk are excluded by index: their P is exactly 0, so their dK, dV and dMem rows are exactly 0.
//
// SUMS OVER ROWS as ffn_grad.hip (fg_reduce.h): slabs of 1024 rows added in slab order in float64, chunks in stream order; column sums
// through partials and one fixed-order float64 reduction.  Identical bits from run to run, whatever the workspace held.
#include "ag_tile.h"
#include "../../include/ctrlsim.h"

#define AG_KVROWS 8192           // memory rows per pass of dWk | dWv

namespace {

// ---- 2. O [rows, 256] and the statistics of every (row, head).  Q, O and the statistics are chunk-local (context b of the chunk is
// context c0 + b of KV / key_pad).
__global__ __launch_bounds__(256) void ag_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ KV,
                                                     const unsigned char* __restrict__ key_pad, float* __restrict__ O,
                                                     float* __restrict__ smax, float* __restrict__ slog, int Lq, int Lk, int c0) {
  __shared__ __attribute__((aligned(16))) float Ks[64 * AG_P];
  __shared__ __attribute__((aligned(16))) float Vs[64 * AG_P];
  __shared__ float bias[64];
  __shared__ float ot[4][32 * 33];
  const int b = blockIdx.z, h = blockIdx.y, qb = blockIdx.x * 128;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const float NEG_INF = -__builtin_inff();
  const int qi = qb + wave * 32 + l31, qrow = qi < Lq ? qi : Lq - 1;
  f32x4 qf[4];
  ag_frag(Q + ((long)b * Lq + qrow) * DM + h * HD + half * 4, qf);
#pragma unroll
  for (int j = 0; j < 4; ++j) qf[j] *= AG_SCALE;
  const float* kvb = KV + (long)(c0 + b) * Lk * (2 * DM) + h * HD;
  const unsigned char* pad = key_pad ? key_pad + (long)(c0 + b) * Lk : nullptr;
  float oacc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) oacc[r] = 0.f;
  float m_run = NEG_INF, l_run = 0.f;
  for (int k0 = 0; k0 < Lk; k0 += 64) {
    __syncthreads();                                     // the previous tile has been read
    ag_stage(kvb, 2 * DM, k0, Lk, Ks, tid);
    ag_stage(kvb + DM, 2 * DM, k0, Lk, Vs, tid);
    if (tid < 64) bias[tid] = (k0 + tid < Lk && !(pad && pad[k0 + tid])) ? 0.f : NEG_INF;
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= Lk) continue;
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
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sc[r] = s[r] + bias[sub * 32 + mfma_row(r, half)];
        tmax = fmaxf(tmax, sc[r]);
      }
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
  const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;     // every key padded: O = 0
  const int nq = Lq - (qb + wave * 32);                    // (<= 0: nothing to store)
  ag_store_t(oacc, inv, ot[wave], O + ((long)b * Lq + qb + wave * 32) * DM + h * HD, DM, nq, l31, half);
  if (half == 0 && qi < Lq) {
    const long e = ((long)b * Lq + qi) * NHEAD + h;
    smax[e] = l_run > 0.f ? m_run : 0.f;                   // finite in every case: a padded key's P is exp2(-inf - finite) = 0
    slog[e] = l_run > 0.f ? log2f(l_run) : 0.f;
  }
}

// ---- 7. delta [rows, 8] and dQ [rows, 256]
__global__ __launch_bounds__(256) void ag_dq_kernel(const float* __restrict__ Q, const float* __restrict__ KV,
                                                    const unsigned char* __restrict__ key_pad, const float* __restrict__ dO, const float* __restrict__ smax,
                                                    const float* __restrict__ slog, float* __restrict__ delta, float* __restrict__ dQ,
                                                    int Lq, int Lk, int c0) {
  __shared__ __attribute__((aligned(16))) float Ks[64 * AG_P];
  __shared__ __attribute__((aligned(16))) float Vs[64 * AG_P];
  __shared__ float bias[64];
  __shared__ float ot[4][32 * 33];
  const int b = blockIdx.z, h = blockIdx.y, qb = blockIdx.x * 128;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const float NEG_INF = -__builtin_inff();
  const int qi = qb + wave * 32 + l31, qrow = qi < Lq ? qi : Lq - 1;
  const long row = (long)b * Lq + qrow;
  f32x4 qf[4], dof[4];
  ag_frag(Q + row * DM + h * HD + half * 4, qf);
  ag_frag(dO + row * DM + h * HD + half * 4, dof);
#pragma unroll
  for (int j = 0; j < 4; ++j) qf[j] *= AG_SCALE;
  const float mq = smax[row * NHEAD + h], lq = slog[row * NHEAD + h];
  float dl = 0.f;
  const float* kvb = KV + (long)(c0 + b) * Lk * (2 * DM) + h * HD;
  const unsigned char* pad = key_pad ? key_pad + (long)(c0 + b) * Lk : nullptr;
  float dq[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) dq[r] = 0.f;
  // two passes over the key tiles: delta = sum_keys P dP first, from the very P and dP (bit for bit) that the second pass takes it from
  // again — where one key holds nearly all of a row's weight, dSc = P (dP - delta) is a difference of nearly equal numbers, and the
  // rounding of dP cancels in it only if delta carries the same rounding (rowsum(dO o O), the same number in exact arithmetic, does
  // not: measured at one key per query, 19 times float32 autograd's error in dX instead of exactly 0)
  for (int pass = 0; pass < 2; ++pass) {
  for (int k0 = 0; k0 < Lk; k0 += 64) {
    __syncthreads();
    ag_stage(kvb, 2 * DM, k0, Lk, Ks, tid);
    ag_stage(kvb + DM, 2 * DM, k0, Lk, Vs, tid);
    if (tid < 64) bias[tid] = (k0 + tid < Lk && !(pad && pad[k0 + tid])) ? 0.f : NEG_INF;
    __syncthreads();
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      if (k0 + sub * 32 >= Lk) continue;
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
      for (int r = 0; r < 16; ++r) dsc[r] = __builtin_amdgcn_exp2f(((s[r] + bias[sub * 32 + mfma_row(r, half)]) - mq) - lq);      // P
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
      const float* kt = Ks + (sub * 32) * AG_P + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) a = __builtin_amdgcn_mfma_f32_32x32x2f32(kt[mfma_row(r, half) * AG_P], dsc[r], a, 0, 0, 0);   // dQ^T += K^T dSc^T
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[r] = a[r];
    }
  }
  if (pass == 0) {
    dl += __shfl_xor(dl, 32, 64);
    if (half == 0 && qi < Lq) delta[row * NHEAD + h] = dl;
  }
  }
  const int nq = Lq - (qb + wave * 32);
  ag_store_t(dq, AG_RS, ot[wave], dQ + ((long)b * Lq + qb + wave * 32) * DM + h * HD, DM, nq, l31, half);
}

// ---- 8. dK | dV [B Lk, 512] rows of the chunk's contexts: one workgroup per (context, head, 64 keys)
__global__ __launch_bounds__(256) void ag_dkv_kernel(const float* __restrict__ Q, const float* __restrict__ KV,
                                                     const unsigned char* __restrict__ key_pad, const float* __restrict__ dO,
                                                     const float* __restrict__ smax, const float* __restrict__ slog,
                                                     const float* __restrict__ delta, float* __restrict__ dKV, int Lq, int Lk, int c0) {
  __shared__ __attribute__((aligned(16))) float Qs[64 * AG_P];
  __shared__ __attribute__((aligned(16))) float Ds[64 * AG_P];
  __shared__ float sm[64], sl[64], sd[64];
  __shared__ float red[2][2 * 16 * 64];                 // [key half][dV, dK]: the odd query blocks' sums; then the wave's transpose patch
  const int b = blockIdx.z, h = blockIdx.y, kb = blockIdx.x * 64;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int ksub = wave & 1, qsub = wave >> 1;
  const int key = kb + ksub * 32 + l31, krow = key < Lk ? key : Lk - 1;
  const bool kvalid = key < Lk && !(key_pad && key_pad[(long)(c0 + b) * Lk + krow]);
  f32x4 kf[4], vf[4];
  const float* kp = KV + ((long)(c0 + b) * Lk + krow) * (2 * DM) + h * HD + half * 4;
  ag_frag(kp, kf);
  ag_frag(kp + DM, vf);
  const float* Qb = Q + (long)b * Lq * DM + h * HD;
  const float* Db = dO + (long)b * Lq * DM + h * HD;
  float dv[16], dk[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { dv[r] = 0.f; dk[r] = 0.f; }
  for (int q0 = 0; q0 < Lq; q0 += 64) {
    __syncthreads();
    ag_stage(Qb, DM, q0, Lq, Qs, tid);
    ag_stage(Db, DM, q0, Lq, Ds, tid);
    if (tid < 64) {
      const int q = q0 + tid;
      const long e = ((long)b * Lq + (q < Lq ? q : Lq - 1)) * NHEAD + h;
      sm[tid] = q < Lq ? smax[e] : __builtin_inff();     // a query beyond Lq: P = exp2(0 - inf) = 0
      sl[tid] = q < Lq ? slog[e] : 0.f;
      sd[tid] = q < Lq ? delta[e] : 0.f;
    }
    __syncthreads();
    if (q0 + qsub * 32 >= Lq) continue;                 // (wave-uniform; the barriers above are outside)
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
      const float p = kvalid ? __builtin_amdgcn_exp2f((s[r] - sm[q]) - sl[q]) : 0.f;
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
  if (qsub == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dv[r] += red[ksub][r * 64 + lane];
      dk[r] += red[ksub][1024 + r * 64 + lane];
    }
    __builtin_amdgcn_wave_barrier();
    const int nk = Lk - (kb + ksub * 32);
    float* out = dKV + ((long)(c0 + b) * Lk + kb + ksub * 32) * (2 * DM) + h * HD;
    ag_store_t(dk, AG_RS, red[ksub], out, 2 * DM, nk, l31, half);
    ag_store_t(dv, 1.0f, red[ksub], out + DM, 2 * DM, nk, l31, half);
  }
}

}  // namespace

// Workspace behind `base`: K | V and dK | dV of all contexts [B Lk, 512], the chunk buffers Q, O, S (then dO), dS, dQ [chunk rows, 256] and
// the three statistics [chunk rows, 8], the product slabs of one chunk / one pass over the memory rows, and the column-sum partials
AttnGradWs attn_grad_carve(size_t base, int B, int Lq, int Lk) {
  AttnGradWs w;
  size_t off = fg_up(base);
  auto take = [&](size_t n) { const size_t o = off; off += fg_up(n); return o; };
  int cc = 8192 / Lq;
  cc = cc < 1 ? 1 : cc > B ? B : cc;
  w.chunk_ctx = cc;
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

int launch_attn_block_grad(const float* X, int ldx, const float* Mem, int ldm, const unsigned char* key_pad, const float* dY, int lddy,
                           const float* Win, const float* bin, const float* Wo, const float* bo, const float* gamma, const float* beta,
                           int B, int Lq, int Lk, char* ws, const AttnGradWs& w, float* grads, float* dX, int lddx, float* dMem, int lddm,
                           int accumulate_dmem, hipStream_t st) {
  (void)beta;                                          // the backward of a LayerNorm does not read its bias
  if (!X || !Mem || !dY || !Win || !bin || !Wo || !bo || !gamma || !ws || !grads || B < 1 || Lq < 1 || Lk < 1 ||
      (long)B * Lq > 0x7fffffffL / DM || (long)B * Lk > 0x7fffffffL / (2 * DM) || ldx < DM || ldm < DM || lddy < DM || (dX && lddx < DM) ||
      (dMem && lddm < DM) || w.chunk_ctx < 1 || (reinterpret_cast<uintptr_t>(ws) & 15))
    return CTRLSIM_EINVAL;
  auto f = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *KV = f(w.KV), *dKV = f(w.dKV), *Q = f(w.Q), *O = f(w.O), *S = f(w.S), *dS = f(w.dS), *dQ = f(w.dQ), *slab = f(w.slab);
  float *pln = f(w.part_ln), *pcq = f(w.part_cq), *pck = f(w.part_ck);
  const long crows = (long)w.chunk_ctx * Lq, nstat = crows * NHEAD, wsz = (long)DM * DM;
  float *smax = f(w.stat), *slog = smax + nstat, *delta = slog + nstat, *dO = S;
  float *gWin = grads, *gbin = gWin + 3 * wsz, *gWo = gbin + 3 * DM, *gbo = gWo + wsz, *gg = gbo + DM, *gbe = gg + DM;
  const int rowsk = B * Lk;
  const unsigned nadd = (unsigned)((wsz + 255) / 256);
  // K | V = Mem (Wk; Wv)^T + (bk; bv)
  FG_CHK(hg_gemm_t<true, true, HG_EPI_PLAIN>(HgGemm{Mem, ldm, 1, Win + wsz, 1, DM, KV, 2 * DM, 0, bin + DM, rowsk, 2 * DM, DM, DM, 0}, st));
  long nln = 0, ncq = 0, nck = 0;
  for (int c0 = 0; c0 < B; c0 += w.chunk_ctx) {
    const int nc = B - c0 < w.chunk_ctx ? B - c0 : w.chunk_ctx, nr = nc * Lq;
    const int acc = c0 > 0, nslab = (nr + FG_KS - 1) / FG_KS;
    const long r0 = (long)c0 * Lq;
    const float* Xc = X + r0 * ldx;
    const float* dYc = dY + r0 * lddy;
    const dim3 gq((Lq + 127) / 128, NHEAD, nc), gk((Lk + 63) / 64, NHEAD, nc);
    // 1. Q      2. O, statistics      3. S = X + O Wo^T + bo
    FG_CHK(hg_gemm_t<true, true, HG_EPI_PLAIN>(HgGemm{Xc, ldx, 1, Win, 1, DM, Q, DM, 0, bin, nr, DM, DM, DM, 0}, st));
    hipLaunchKernelGGL(ag_fwd_kernel, gq, dim3(256), 0, st, Q, KV, key_pad, O, smax, slog, Lq, Lk, c0);
    FG_CHK(hg_gemm_t<true, true, HG_EPI_RES>(HgGemm{O, DM, 1, Wo, 1, DM, S, DM, 0, bo, nr, DM, DM, DM, 0, Xc, ldx}, st));
    // 4. dY -> dS, partials of dg, dbe, dbo
    const int nb = (nr + FG_LN_ROWS - 1) / FG_LN_ROWS;
    hipLaunchKernelGGL(fg_ln_bwd_kernel, dim3(nb), dim3(256), 0, st, S, gamma, dYc, (long)lddy, dS, nr, pln + nln * 3 * DM);
    nln += nb;
    // 5. dWo (+)= dS^T O      6. dO = dS Wo, over S
    FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{dS, 1, DM, O, DM, 1, slab, DM, wsz, nullptr, DM, DM, nr, FG_KS, 0}, st));
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3(nadd), dim3(256), 0, st, slab, nslab, wsz, gWo, acc);
    FG_CHK(hg_gemm_t<true, false, HG_EPI_PLAIN>(HgGemm{dS, DM, 1, Wo, DM, 1, dO, DM, 0, nullptr, nr, DM, DM, DM, 0}, st));
    // 7. delta, dQ      8. dK | dV of these contexts
    hipLaunchKernelGGL(ag_dq_kernel, gq, dim3(256), 0, st, Q, KV, key_pad, dO, smax, slog, delta, dQ, Lq, Lk, c0);
    hipLaunchKernelGGL(ag_dkv_kernel, gk, dim3(256), 0, st, Q, KV, key_pad, dO, smax, slog, delta, dKV, Lq, Lk, c0);
    // 9. dWq (+)= dQ^T X      10. dbq partials      11. dX = dS + dQ Wq
    FG_CHK(hg_gemm_t<false, false, HG_EPI_PLAIN>(HgGemm{dQ, 1, DM, Xc, ldx, 1, slab, DM, wsz, nullptr, DM, DM, nr, FG_KS, 0}, st));
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3(nadd), dim3(256), 0, st, slab, nslab, wsz, gWin, acc);
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
    hipLaunchKernelGGL(fg_slab_add_kernel, dim3(2 * nadd), dim3(256), 0, st, slab, nslab, 2 * wsz, gWin + wsz, k0 > 0);
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
  float* const col3[3] = {gg, gbe, gbo};               // the LayerNorm backward's partial rows are [3][256]: (dY xhat, dY, dS)
  for (int q = 0; q < 3; ++q)
    hipLaunchKernelGGL(fg_colreduce_kernel, dim3(DM / 16), dim3(256), 0, st, pln + q * DM, (int)nln, 3L * DM, DM, col3[q]);
  hipLaunchKernelGGL(fg_colreduce_kernel, dim3(DM / 16), dim3(256), 0, st, pcq, (int)ncq, (long)DM, DM, gbin);
  hipLaunchKernelGGL(fg_colreduce_kernel, dim3(2 * DM / 16), dim3(256), 0, st, pck, (int)nck, 2L * DM, 2 * DM, gbin + DM);
  return ctrlsim_launch_status();
}

// Step 2 alone, for decoder_layer_grad.hip's recompute of the sublayer's output: O [nc Lq, 256] and the statistics [nc Lq, 8] of the nc
// contexts from c0 on (Q, O and the statistics chunk-local, K | V and key_pad of all contexts)
int launch_attn_fwd_stats(const float* Q, const float* KV, const unsigned char* key_pad, float* O, float* smax, float* slog, int nc, int Lq,
                          int Lk, int c0, hipStream_t st) {
  hipLaunchKernelGGL(ag_fwd_kernel, dim3((Lq + 127) / 128, NHEAD, nc), dim3(256), 0, st, Q, KV, key_pad, O, smax, slog, Lq, Lk, c0);
  return ctrlsim_launch_status();
}

// ---- the op as a C ABI entry (include/ctrlsim.h)
extern "C" int64_t ctrlsim_attn_block_grad_workspace_bytes(int B, int Lq, int Lk) {
  if (B < 1 || Lq < 1 || Lk < 1 || (long)B * Lq > 0x7fffffffL / DM || (long)B * Lk > 0x7fffffffL / (2 * DM)) return CTRLSIM_EINVAL;
  return (int64_t)attn_grad_carve(0, B, Lq, Lk).bytes;
}
extern "C" int ctrlsim_attn_block_grad_chunk_contexts(int B, int Lq, int Lk) {
  if (B < 1 || Lq < 1 || Lk < 1) return CTRLSIM_EINVAL;
  return attn_grad_carve(0, B, Lq, Lk).chunk_ctx;
}
extern "C" int ctrlsim_attn_block_grad(const float* X, int ldx, const float* Mem, int ldm, const uint8_t* key_pad, const float* dY, int lddy,
                                       const float* in_proj_weight, const float* in_proj_bias, const float* out_proj_weight,
                                       const float* out_proj_bias, const float* gamma, const float* beta, int B, int Lq, int Lk,
                                       void* workspace, float* grads, float* dX, int lddx, float* dMem, int lddm, hipStream_t stream) {
  if (B < 1 || Lq < 1 || Lk < 1 || !beta || !workspace || (long)B * Lq > 0x7fffffffL / DM || (long)B * Lk > 0x7fffffffL / (2 * DM))
    return CTRLSIM_EINVAL;
  return launch_attn_block_grad(X, ldx, Mem, ldm, key_pad, dY, lddy, in_proj_weight, in_proj_bias, out_proj_weight, out_proj_bias, gamma, beta,
                                B, Lq, Lk, static_cast<char*>(workspace), attn_grad_carve(0, B, Lq, Lk), grads, dX, lddx, dMem, lddm, 0, stream);
}
