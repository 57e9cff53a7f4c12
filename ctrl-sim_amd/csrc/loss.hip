// Open-loop evaluation (teacher-forced loss of a logged window): what CtRLSim.compute_loss (models/ctrl_sim.py:48-189) computes from the
// logits of every head, without the logits.
//
//   head_ce_kernel   (a) the last Linear of an MLP head (256 -> V) with a cross-entropy epilogue: per row and softmax the log-sum-exp
//                        and the target's logit leave as two floats; nothing of size V is written.  TWO-fp16-PLANE SCHEME ONLY, like
//                        inproj_rs_kernel (gemm_bf16x6.hip) whose structure it has: three bf16 planes would need 192 registers for a
//                        wave's row fragments.  An engine on the three-plane scheme takes (c).
//   row_lse_kernel   (c) the same two floats from logits in memory (ctrlsim_forward_all's tensors, or a chunk of rows the generic
//                        GEMM just wrote): one wave per row, max pass + sum pass.
//   loss_ctx_kernel  (b) per context the masked float64 sums and counts behind loss_actions, loss_rtg_goal / _veh / _road and loss_state
//   loss_total_kernel    and their total over the batch.  TWO STAGES, no atomics: a context's ten numbers are reduced by a fixed tree
//                        inside its workgroup, the batch total by a fixed tree over the contexts — identical bits from run to run.
//
// This file is compiled once per operand split (build.py: SPLIT_SRCS); the kernels that do not depend on the split, (b) and (c), are
// compiled in the two-plane build only and live outside the scheme namespace.
#include "split.h"
#include "launchers.h"

// one (lse, target logit) pair per row and softmax: LT[row][4][2]; softmax 0 = actions, 1..3 = return components goal / veh / road
#define LT_STRIDE 8

namespace SPLIT_NS {

#if CTRLSIM_F16X3
// ---- (a) Row-stationary Linear(256 -> 32 nb) with an online-softmax epilogue.
// A wave keeps 32 rows as split operand fragments in registers (128 VGPRs) for the life of a 256-row job; the weight streams through a
// four-slot LDS ring by LDS-DMA as 32 KB blocks of 32 output columns (pack.py:row_blocks layout; pack.py:head_ce_image pads / permutes
// the head's rows), 48 MFMAs per block and wave into a fresh accumulator, D^T = W_blk . X^T: a LANE OWNS ONE ROW and holds 16 of the
// block's 32 columns (register r <-> column (r & 3) + 8 (r >> 2) + 4 half; the lane 32 further on holds the other 16).  The epilogue of a
// block stores nothing: the lane updates a running (max, sum) over its 16 columns and keeps the target's logit when it meets its
// column; the two half-rows are combined ONCE per softmax (one cross-lane exchange), after the softmax's last block.
// The nb blocks are nsm softmaxes of bps blocks each with `valid` real columns (action head: 1 x 32 blocks, 1000 of 1024; return head:
// 3 x 11 blocks, 350 of 352, component-major).  Pad columns are masked BY COLUMN INDEX (their weights and bias are zeros, not -inf).
// Counted wait: the only vector-memory requests in flight at the end of a block are this block's CE_PIECES DMA pieces (for the block
// two ahead) — so "at most CE_PIECES outstanding" means the next block has landed — and, behind a softmax's last block, the wave's
// result store: the block after it drains the counter instead of counting.
constexpr int CE_BLK = NPL * 16 * 2 * 32 * 8;        // 16-bit elements of one weight block (32 columns x 256 k x 2 planes = 32 KB)
constexpr int CE_RING = 4;
constexpr int CE_PIECES = CE_BLK / (512 * 8);        // 16-byte-per-thread DMA pieces of a block (4)
constexpr int CE_MAXB = 40;                          // column blocks of the largest head (1280 columns)
constexpr int CE_PF = 2;                             // LDS fragment prefetch distance in k-steps
#define CE_LDS_BYTES (CE_RING * CE_BLK * 2 + CE_MAXB * 32 * 4)

__global__ __launch_bounds__(512, 2) void head_ce_kernel(const float* __restrict__ A, int lda, const op_t* __restrict__ Wb,
                                                         const float* __restrict__ bias, const int* __restrict__ tgt, int tgt_stride,
                                                         long tgt_shift, long tgt_rows, int M, int nb, int bps, int valid,
                                                         float* __restrict__ LT, int sm0) {
  static_assert(NPL == 2 && CE_PIECES == 4, "the counted vmcnt wait below assumes 4 DMA pieces per block");
  extern __shared__ __attribute__((aligned(16))) op_t ce_ring[];
  float* const bs = reinterpret_cast<float*>(ce_ring + CE_RING * CE_BLK);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l31 = lane & 31, half = lane >> 5;
  const int n_jobs = (M + 255) / 256;
  if ((int)blockIdx.x >= n_jobs) return;
  for (int i = tid; i < nb * 32; i += 512) bs[i] = bias[i];
  auto dma_piece = [&](int blk, int slot, int j) {
    const op_t* src = Wb + (size_t)blk * CE_BLK + (j * 512 + tid) * 8;
    op_t* dst = ce_ring + slot * CE_BLK + (j * 512 + wave * 64) * 8;       // wave-uniform LDS base (+ 16 B per lane)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  };
#pragma unroll
  for (int j = 0; j < CE_PIECES; ++j) dma_piece(0, 0, j);
#pragma unroll
  for (int j = 0; j < CE_PIECES; ++j) dma_piece(1 % nb, 1, j);
  int nxt = 2 % nb;                                   // column block two phases ahead (every job walks blocks 0 .. nb-1: the ring never idles)
  int slot = 0;
  bool first = true;
  for (int job = blockIdx.x; job < n_jobs; job += gridDim.x) {
    const int row = job * 256 + wave * 32 + l31;
    opx8 xT[16][NPL];
    {
      // the wave's 32 rows: 32 raw 16-byte loads per lane (k-step ks: k = 16 ks + 8 half .. + 7), converted in order as they land
      f32x4 raw[32];
      const float* xp = A + (size_t)(row < M ? row : M - 1) * lda + half * 8;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        raw[2 * ks] = *reinterpret_cast<const f32x4*>(xp + ks * 16);
        raw[2 * ks + 1] = *reinterpret_cast<const f32x4*>(xp + ks * 16 + 4);
      }
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const f32x4 x0 = raw[2 * ks], x1 = raw[2 * ks + 1];
        const float xs[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
        split_frag(xs, xT[ks]);
      }
    }
    // (the row loads above were waited for with everything older complete: this wave's pieces of the first two blocks have landed)
    if (first) {                                      // blocks 0 and 1 are in LDS for every wave, the bias vector is visible
      __builtin_amdgcn_s_waitcnt(0x0070);
      __syncthreads();
      first = false;
    }
    const long trow = (long)row + tgt_shift;
    int sm = 0, cbs = 0;                              // softmax of the current block, block index inside it
    int t = -1;
    float m_run = -INFINITY, s_run = 0.f, t_logit = -INFINITY;
    bool stored = false;                              // the previous block ended a softmax: its result store is in flight
    for (int cb = 0; cb < nb; ++cb) {
      if (cbs == 0) {
        t = (row < M && trow < tgt_rows) ? tgt[trow * tgt_stride + sm] : -1;
        m_run = -INFINITY; s_run = 0.f; t_logit = -INFINITY;
      }
      const op_t* w1 = ce_ring + slot * CE_BLK + (half * 32 + l31) * 8;    // [p][ks][half][col][8]
      const int nslot = (slot + 2) & 3;
      f32x16 acc;
      {
        const float* bp = bs + cb * 32 + 4 * half;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + 8 * g);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[4 * g + j] = bv[j] * WSCALE;
        }
      }
      {
        opx8 wf[CE_PF + 1][NPL];
        auto ld1 = [&](int ks, opx8 (&f)[NPL]) {
#pragma unroll
          for (int pp = 0; pp < NPL; ++pp) f[pp] = *reinterpret_cast<const opx8*>(w1 + ((pp * 16 + ks) * 2) * 32 * 8);
        };
#pragma unroll
        for (int i = 0; i < CE_PF; ++i) ld1(i, wf[i]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          if (ks + CE_PF < 16) ld1(ks + CE_PF, wf[(ks + CE_PF) % (CE_PF + 1)]);
          if (ks < CE_PIECES) dma_piece(nxt, nslot, ks);
          const int c = ks % (CE_PF + 1);
          SPLIT_TERMS(acc, wf[c], xT[ks])
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // the NEXT block (requested during the previous block) must have landed for every wave before anyone reads it; this block's slot is
      // overwritten two phases from now, behind two barriers
      if (stored) __builtin_amdgcn_s_waitcnt(0x0070);  // (behind a result store: drain, whatever order loads and stores retire in)
      else __builtin_amdgcn_s_waitcnt(0x0070 | CE_PIECES);  // vmcnt <= 4, lgkmcnt 0
      stored = false;
      __builtin_amdgcn_s_barrier();
      // ---- epilogue: online softmax over this lane's 16 columns of the block
      {
        const int c0 = cbs * 32 + 4 * half;
        float v[16], vmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int col = c0 + (r & 3) + 8 * (r >> 2);
          v[r] = col < valid ? acc[r] * WSCALE_INV : -INFINITY;
          vmax = fmaxf(vmax, v[r]);
          if (col == t) t_logit = v[r];
        }
        if (vmax > -INFINITY) {                        // (a lane whose 16 columns are all padding keeps its pair)
          const float m_new = fmaxf(m_run, vmax);
          float s = s_run * expf(m_run - m_new);
#pragma unroll
          for (int r = 0; r < 16; ++r) s += expf(v[r] - m_new);
          s_run = s; m_run = m_new;
        }
      }
      if (++cbs == bps) {
        // combine the two half-rows (lanes l and l + 32) and store: once per softmax
        const float m_o = __shfl_xor(m_run, 32), s_o = __shfl_xor(s_run, 32), t_o = __shfl_xor(t_logit, 32);
        const float mm = fmaxf(m_run, m_o);
        const float ss = s_run * expf(m_run - mm) + s_o * expf(m_o - mm);
        if (half == 0 && row < M) {
          float2 o;
          o.x = mm + logf(ss);
          o.y = fmaxf(t_logit, t_o);                   // -inf when the target is no column of this softmax
          *reinterpret_cast<float2*>(LT + (size_t)row * LT_STRIDE + (sm0 + sm) * 2) = o;
        }
        cbs = 0; ++sm;
        stored = true;
      }
      slot = (slot + 1) & 3;
      nxt = nxt + 1 == nb ? 0 : nxt + 1;
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0070);                 // the pieces requested for blocks nobody will read: landed before the LDS is released
}

int launch_head_ce(const float* A, int lda, const void* Wblk, const float* bias, const int* tgt, int tgt_stride, long tgt_shift,
                   long tgt_rows, int M, int nsm, int bps, int valid, float* LT, int sm0, hipStream_t st) {
  if (M <= 0) return CTRLSIM_OK;
  const int nb = nsm * bps;
  if (!A || !Wblk || !bias || !tgt || !LT || (lda & 3) || nsm < 1 || sm0 < 0 || sm0 + nsm > 4 || bps < 1 || nb < 2 || nb > CE_MAXB ||
      valid > bps * 32 || valid <= (bps - 1) * 32)
    return CTRLSIM_EINVAL;
  static const int cus = [] {
    int dev = 0, n = 0;
    return (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
  }();
  static const bool attr_ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&head_ce_kernel),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, CE_LDS_BYTES) == hipSuccess;
  if (!attr_ok) return CTRLSIM_EINVAL;
  const int n_jobs = (M + 255) / 256;
  prof_before(PROF_GEMM, st);
  hipLaunchKernelGGL(head_ce_kernel, dim3(n_jobs < cus ? n_jobs : cus), dim3(512), CE_LDS_BYTES, st, A, lda,
                     static_cast<const op_t*>(Wblk), bias, tgt, tgt_stride, tgt_shift, tgt_rows, M, nb, bps, valid, LT, sm0);
  prof_after(PROF_GEMM, 2.0 * (double)M * nb * 32 * (double)DM, st,
             4.0 * (double)M * DM + 8.0 * (double)M * nsm + 2.0 * NPL * (double)nb * 32 * DM, PKIND_GEMM_PLAIN);
  return ctrlsim_launch_status();
}
#else
int launch_head_ce(const float*, int, const void*, const float*, const int*, int, long, long, int, int, int, int, float*, int, hipStream_t) {
  return 1;                                            // two-fp16-plane scheme only: the caller takes the from-memory path
}
#endif

}  // namespace SPLIT_NS

#if CTRLSIM_F16X3
// ---- (c) log-sum-exp and target logit of rows of logits in memory.  Softmax s of row i is the elements L[i * ld + e * estride + s],
// e < n (action head: estride 1; return head of the reference, bin-major / component-minor, policies/policy.py:108-127: estride 3).
__global__ __launch_bounds__(256) void row_lse_kernel(const float* __restrict__ L, long ld, int n, int estride, int nsm,
                                                      const int* __restrict__ tgt, int tgt_stride, long tgt_shift, long tgt_rows, long row0,
                                                      int M, float* __restrict__ LT, int sm0) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;
  const float* p = L + i * ld;
  const long row = row0 + i, trow = row + tgt_shift;
  for (int s = 0; s < nsm; ++s) {
    float mx = -INFINITY;
    for (int e = lane; e < n; e += 64) mx = fmaxf(mx, p[(long)e * estride + s]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int e = lane; e < n; e += 64) sum += expf(p[(long)e * estride + s] - mx);
    sum = wave_sum(sum);
    if (lane == 0) {
      const int t = trow < tgt_rows ? tgt[trow * tgt_stride + s] : -1;
      float2 o;
      o.x = mx + logf(sum);
      o.y = (t >= 0 && t < n) ? p[(long)t * estride + s] : -INFINITY;
      *reinterpret_cast<float2*>(LT + (size_t)row * LT_STRIDE + (sm0 + s) * 2) = o;
    }
  }
}

int launch_row_lse(const float* L, long ld, int n, int estride, int nsm, const int* tgt, int tgt_stride, long tgt_shift, long tgt_rows,
                   long row0, int M, float* LT, int sm0, hipStream_t st) {
  if (M <= 0) return CTRLSIM_OK;
  if (!L || !tgt || !LT || n < 1 || estride < 1 || nsm < 1 || sm0 < 0 || sm0 + nsm > 4) return CTRLSIM_EINVAL;
  hipLaunchKernelGGL(row_lse_kernel, dim3((M + 3) / 4), dim3(256), 0, st, L, ld, n, estride, nsm, tgt, tgt_stride, tgt_shift, tgt_rows, row0,
                     M, LT, sm0);
  return ctrlsim_launch_status();
}

// ---- (b) masked sums and counts of one context (models/ctrl_sim.py:48-189), float64.
// Terms: 0 loss_actions, 1 loss_rtg_goal, 2 loss_rtg_veh, 3 loss_rtg_road, 4 loss_state; per term (sum, count).  The caller's means:
// terms 0-3 sum / count (x loss_action_coef for term 0), term 4 sum / (100 * 2 * count).
//   mask(tt, a) = exist[tt, a] (x moving[a] under supervise_moving): actions and returns (:73-107).  Trajeglish (shift != 0, :50-67):
//   the logits of step tt are scored against the action of step tt + 1 — LT already holds that target — under mask(tt + 1, a).
//   state (:114-148): prediction slot j of step tt is the position at step tt + 1 + j, masked where that runs past the window or the
//   agent does not exist there (x moving under supervise_moving); local_frame (:151-187): targets translated to the agent's position
//   at step tt and rotated by minus its yaw, and — as in the reference — NO moving mask.
struct LossArgs {
  const float* LT; const float* exist; const unsigned char* moving; const float* st12; const float* fut; float* row_nll;
  double* per_ctx; int Tq, A, nfut, has_rtg, shift, supervise_moving, local_frame;
};
__global__ __launch_bounds__(256) void loss_ctx_kernel(LossArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tq = a.Tq, A = a.A, n = Tq * A;
  const float* ex = a.exist + (size_t)b * n;
  const float* st = a.st12 + (size_t)b * n * 12;
  const unsigned char* mv = a.moving ? a.moving + (size_t)b * A : nullptr;
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0.0;
  for (int i = tid; i < n; i += 256) {
    const int tt = i / A, ag = i - tt * A;
    const size_t row = (size_t)b * n + i;
    const double mov = (a.supervise_moving && mv) ? (double)(mv[ag] != 0) : 1.0;
    const float* lt = a.LT + row * LT_STRIDE;
    double nll[4];                                    // (the difference of the two floats is taken in float64: one rounding less)
#pragma unroll
    for (int s = 0; s < 4; ++s) nll[s] = (s == 0 || a.has_rtg) ? (double)lt[2 * s] - (double)lt[2 * s + 1] : 0.0;
    if (a.row_nll) {
#pragma unroll
      for (int s = 0; s < 4; ++s) a.row_nll[row * 4 + s] = (float)nll[s];
    }
    const double m_here = (double)ex[i] * mov;
    // actions
    {
      const double m = a.shift ? (tt + 1 < Tq ? (double)ex[i + A] * mov : 0.0) : m_here;
      if (m != 0.0) { acc[0] += nll[0] * m; acc[1] += m; }
    }
    if (a.has_rtg && m_here != 0.0) {
#pragma unroll
      for (int s = 1; s < 4; ++s) { acc[2 * s] += nll[s] * m_here; acc[2 * s + 1] += m_here; }
    }
    if (a.fut) {
      const float* pr = a.fut + row * (size_t)(2 * a.nfut);
      const double ox = st[(size_t)i * 12], oy = st[(size_t)i * 12 + 1];
      double cy = 1.0, sy = 0.0;
      if (a.local_frame) { const double yaw = (double)st[(size_t)i * 12 + 4]; cy = cos(-yaw); sy = sin(-yaw); }
      const double mstate = a.local_frame ? 1.0 : mov;
      for (int j = 0; j < a.nfut && tt + 1 + j < Tq; ++j) {
        const int i2 = i + (1 + j) * A;
        const double m = (double)ex[i2] * mstate;
        if (m == 0.0) continue;
        double tx = st[(size_t)i2 * 12], ty = st[(size_t)i2 * 12 + 1];
        if (a.local_frame) {
          const double dx = tx - ox, dy = ty - oy;
          tx = cy * dx - sy * dy; ty = sy * dx + cy * dy;
        }
        const double ex_ = (double)pr[2 * j] - tx, ey_ = (double)pr[2 * j + 1] - ty;
        acc[8] += (ex_ * ex_ + ey_ * ey_) * m; acc[9] += m;
      }
    }
  }
  // fixed tree: lanes of a wave, then the four waves in order
  __shared__ double red[4][10];
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o);
    if ((tid & 63) == 0) red[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < 10) a.per_ctx[(size_t)b * 10 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
// sums[k] += the per-context values of k over the batch: wave k, lanes stride over the contexts, fixed shuffle tree
__global__ __launch_bounds__(640) void loss_total_kernel(const double* __restrict__ per_ctx, int B, double* __restrict__ sums) {
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double v = 0.0;
  for (int b = lane; b < B; b += 64) v += per_ctx[(size_t)b * 10 + k];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o);
  if (lane == 0) sums[k] += v;
}

int launch_loss_reduce(const float* LT, const float* exist, const unsigned char* moving, const float* st12, const float* fut, float* row_nll,
                       double* per_ctx, double* sums, int B, int Tq, int A, int nfut, int has_rtg, int shift, int supervise_moving,
                       int local_frame, hipStream_t st) {
  if (B <= 0) return CTRLSIM_OK;
  if (!LT || !exist || !st12 || !per_ctx || !sums || Tq < 1 || A < 1 || (fut && nfut < 1)) return CTRLSIM_EINVAL;
  LossArgs a{LT, exist, moving, st12, fut, row_nll, per_ctx, Tq, A, nfut, has_rtg, shift, supervise_moving, local_frame};
  hipLaunchKernelGGL(loss_ctx_kernel, dim3(B), dim3(256), 0, st, a);
  hipLaunchKernelGGL(loss_total_kernel, dim3(1), dim3(640), 0, st, per_ctx, B, sums);
  return ctrlsim_launch_status();
}
#endif
