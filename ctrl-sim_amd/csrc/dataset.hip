// Offline-RL dataset generation on the device (gfx950): what the reference computes between a rolled logged scene and the
// `*_physics.pkl` dictionary CtRL-Sim is trained on and its evaluators read back — float64, one launch set for a whole batch.
//
// Reference:
//   data/generate_offline_rl_dataset.py:17-144   every logged vehicle pushed through the simulator; one compute_reward row per vehicle and step
//   utils/sim.py:83-141                          compute_reward: goal-reached latch, heading / speed targets, shaped terms, collision flags
//   datasets/rl_waymo/dataset.py:187-237         compute_dist_to_nearest_road_edge_rewards / compute_dist_to_nearest_vehicle_rewards
//   utils/data.py:152-290                        compute_distance_to_road_edge: the SIGNED distance to the nearest road-edge polyline
//   datasets/rl_waymo/dataset.py:240-275 +
//   datasets/rl_waymo/dataset_ctrl_sim.py:92-97  compute_rewards (five components) and the reverse cumulative sum: returns-to-go
// Host forms the tests compare with: rewards.signed_distance_to_road_edges, metrics.compute_rewards / nearest_vehicle_distance as
// ingest.preprocess_scene uses them, ingest.load_preprocessed.  Arithmetic follows their NumPy expressions operation by operation (no
// FMA contraction); division and square root are correctly rounded on both sides, np's float `%` is fmod plus the divisor's sign.
//
// edge_distance_kernel — one thread per (vehicle, step) point, 256 points of ONE scene per workgroup.  The scene's road-edge segments
// stream through LDS in stages of EDGE_STAGE segments: thread k of the workgroup prepares segment k of the stage (start, direction,
// squared length, and the flags that do not depend on the query point: first / last segment of its polyline, convexity of both
// corners, cyclic polyline), then every lane walks the stage reading the same LDS address (a broadcast).  Each lane carries the state of
// the polyline it is in across stages, so a polyline may straddle any number of them.  Strict `<` in visiting order gives np.argmin's
// first-index tie-breaks, within a polyline (over distances) and across polylines (over |signed distance|).
#include "common.h"
#include "../../include/ctrlsim.h"

#pragma clang fp contract(off)

namespace {

constexpr int EDGE_STAGE = 256;     // segments per LDS stage = threads per workgroup (tests/test_gpu_datagen.py states it)
enum { SEG_FIRST = 1, SEG_LAST = 2, SEG_CVX_BEFORE = 4, SEG_CVX_AFTER = 8, SEG_CYCLIC = 16 };

__device__ __forceinline__ double clipd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// utils/geometry.py:3-12 as kinematics.angle_sub evaluates it: d = (target - current) % 2 pi; d > pi -> -(2 pi - d)
__device__ __forceinline__ double angle_sub(double current, double target) {
  const double two_pi = 2.0 * 3.141592653589793;
  double d = fmod(target - current, two_pi);
  if (d != 0.0) { if (d < 0.0) d += two_pi; } else d = 0.0;
  return d > 3.141592653589793 ? -(two_pi - d) : d;
}

// CT = coordinate type of the point and segment tables: float = the simulator's (points = rows of hist_states [S,N,T1,8], P = N * T),
// double = plain tables (points xy [S,P,2]; ctrlsim_dataset_edge_distance_f64).  Both are widened to float64 before the first operation
template <typename CT>
__global__ __launch_bounds__(EDGE_STAGE) void edge_distance_kernel(int P, int T, int T1, int E, int PE, int blocks_per_scene,
                                                                   const CT* __restrict__ pts, const double* __restrict__ exist,
                                                                   const CT* __restrict__ edges, const int* __restrict__ poly_off,
                                                                   double* __restrict__ out) {
  __shared__ double s_x0[EDGE_STAGE], s_y0[EDGE_STAGE], s_sx[EDGE_STAGE], s_sy[EDGE_STAGE], s_den[EDGE_STAGE];
  __shared__ int s_fl[EDGE_STAGE];
  const int s = blockIdx.x / blocks_per_scene, tid = threadIdx.x;
  const int i0 = (blockIdx.x - s * blocks_per_scene) * EDGE_STAGE + tid;      // point of the scene: vehicle i / T, step i % T
  const bool in_range = i0 < P;
  const int i = in_range ? i0 : 0;
  double x, y, ex = 1.0;
  if constexpr (sizeof(CT) == sizeof(float)) {
    const int v = i / T, t = i - v * T;
    const CT* row = pts + (((size_t)s * (P / T) + v) * T1 + t) * 8;
    x = row[0]; y = row[1]; ex = row[7];
  } else {
    const CT* q = pts + ((size_t)s * P + i) * 2;
    x = q[0]; y = q[1];
  }
  if (exist) ex = exist[(size_t)s * P + i];
  const bool active = in_range && ex != 0.0;
  const CT* eg = edges + (size_t)s * E * 4;
  const int* off = poly_off + (size_t)s * (PE + 1);
  // segments of the scene: the end of its offset table, never beyond the table the caller described
  int n_seg = (E > 0 && PE > 0) ? off[PE] : 0;
  n_seg = n_seg < 0 ? 0 : (n_seg > E ? E : n_seg);

  double best = __builtin_inf();            // signed distance of the first polyline of minimum |signed distance|
  // the polyline the walk is in: first-minimum segment so far (squared distance seen, distance, which side of the segment the foot
  // fell, its n, the n before and after it, its flags), n of the polyline's first and of the previous segment
  double bd2 = __builtin_inf(), bd = __builtin_inf();
  int bcls = 1, bn = 0, bnp = 0, bnn = 0, bfl = 0, n0 = 0, n_prev = 0;
  bool pend = false;                        // the minimum sits on the previous segment: this segment's n is its n_next

  for (int base = 0; base < n_seg; base += EDGE_STAGE) {
    const int cnt = n_seg - base < EDGE_STAGE ? n_seg - base : EDGE_STAGE;
    __syncthreads();                        // the previous stage has been read by every lane
    if (tid < cnt) {
      const int e = base + tid;
      // polyline of segment e: the last p with off[p] <= e (empty polylines repeat an offset and are stepped over)
      int lo = 0, hi = PE;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= e) lo = mid; else hi = mid;
      }
      int a = off[lo], b = off[lo + 1];
      b = b > n_seg ? n_seg : b;
      if (!(a >= 0 && a <= e && e < b)) { a = e; b = e + 1; }      // a table that is not a partition: the segment stands alone
      const int ep = e == a ? b - 1 : e - 1, en = e == b - 1 ? a : e + 1;
      const double x0 = (double)eg[e * 4], y0 = (double)eg[e * 4 + 1], sx = (double)eg[e * 4 + 2] - x0, sy = (double)eg[e * 4 + 3] - y0;
      const double psx = (double)eg[ep * 4 + 2] - (double)eg[ep * 4], psy = (double)eg[ep * 4 + 3] - (double)eg[ep * 4 + 1];
      const double nsx = (double)eg[en * 4 + 2] - (double)eg[en * 4], nsy = (double)eg[en * 4 + 3] - (double)eg[en * 4 + 1];
      const double cx = (double)eg[a * 4] - (double)eg[(b - 1) * 4 + 2], cy = (double)eg[a * 4 + 1] - (double)eg[(b - 1) * 4 + 3];
      int f = (e == a ? SEG_FIRST : 0) | (e == b - 1 ? SEG_LAST : 0);
      if (psx * sy - psy * sx > 0.0) f |= SEG_CVX_BEFORE;          // is_locally_convex, utils/data.py:273-275 (the padding wraps around)
      if (sx * nsy - sy * nsx > 0.0) f |= SEG_CVX_AFTER;
      if (cx * cx + cy * cy < 1.0) f |= SEG_CYCLIC;                // _CYCLIC_MAP_FEATURE_TOLERANCE_M2
      s_x0[tid] = x0; s_y0[tid] = y0; s_sx[tid] = sx; s_sy[tid] = sy; s_den[tid] = sx * sx + sy * sy;
      s_fl[tid] = f;
    }
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < cnt; ++j) {
      const double sx = s_sx[j], sy = s_sy[j], den = s_den[j];
      const int f = s_fl[j];
      const double px = x - s_x0[j], py = y - s_y0[j];
      const double num = px * sx + py * sy, crs = px * sy - py * sx;
      const int n = (crs > 0.0) - (crs < 0.0);
      // clip(nan_to_num(num / den), 0, 1): 0 for num <= 0 (and for 0 / 0), 1 for num >= den; the quotient only in between
      double r = 0.0;
      if (num > 0.0) r = num >= den ? 1.0 : num / den;
      const double qx = px - sx * r, qy = py - sy * r;
      const double d2 = qx * qx + qy * qy;
      if (f & SEG_FIRST) {
        // a new polyline: nothing of the previous one's first-minimum state survives
        bd2 = __builtin_inf(); bd = __builtin_inf();
        bcls = 1; bn = 0; bnp = 0; bnn = 0; bfl = f;
        pend = false;
        n0 = n; n_prev = n;
      }
      if (pend) { bnn = n; pend = false; }
      if (d2 < bd2) {
        // (the square root is monotonic: a segment can only be a new first minimum of the distances where its square is smaller)
        bd2 = d2;
        const double d = sqrt(d2);
        if (d < bd) {
          bd = d;
          bcls = num < 0.0 ? 0 : ((num < den || den == 0.0) ? 1 : 2);        // rel_t < 0 | rel_t < 1 | else
          bn = n; bnp = n_prev; bfl = f;
          pend = true;
        }
      }
      n_prev = n;
      if (f & SEG_LAST) {
        const bool cyc = (bfl & SEG_CYCLIC) != 0;
        const int np_ = (bfl & SEG_FIRST) ? (cyc ? n : n0) : bnp;
        const int nn_ = (bfl & SEG_LAST) ? (cyc ? n0 : n) : bnn;
        int sg = bn;
        if (bcls == 0) sg = (bfl & SEG_CVX_BEFORE) ? max(bn, np_) : min(bn, np_);
        if (bcls == 2) sg = (bfl & SEG_CVX_AFTER) ? max(bn, nn_) : min(bn, nn_);
        const double val = (double)sg * bd;
        if (fabs(val) < fabs(best)) best = val;
        pend = false;
      }
    }
  }
  if (in_range) out[(size_t)s * P + i] = active ? best : 0.0;
}

// every term of a compute_reward row that depends on its own step only, and the two distance rewards.  ag_rewards[.., 0] and [.., 3]
// leave as (now, shaped term), NOT yet latched or masked: reward_latch_kernel finishes them
__global__ __launch_bounds__(256) void reward_rows_kernel(int N, int T, int T1, int blocks_per_scene, const float* __restrict__ hist_states,
                                                          const unsigned char* __restrict__ coll, const double* __restrict__ exist,
                                                          const double* __restrict__ goals4, const double* __restrict__ edge_dist,
                                                          ctrlsim_dataset_cfg c, double* __restrict__ ag_rewards,
                                                          double* __restrict__ veh_veh, double* __restrict__ veh_edge) {
  const int s = blockIdx.x / blocks_per_scene;
  const int i = (blockIdx.x - s * blocks_per_scene) * 256 + threadIdx.x;
  if (i >= N * T) return;
  const int v = i / T, t = i - v * T;
  const size_t sv = (size_t)s * N + v;
  const float* row = hist_states + (sv * T1 + t) * 8;
  const float* row0 = hist_states + sv * T1 * 8;
  const double x = row[0], y = row[1], vx = row[2], vy = row[3], h = row[4];
  const double ex = exist[sv * T + t];
  const double* g = goals4 + sv * 4;
  const double gx = g[0] - x, gy = g[1] - y, dist = sqrt(gx * gx + gy * gy);
  const double gx0 = g[0] - (double)row0[0], gy0 = g[1] - (double)row0[1];
  double norm0 = sqrt(gx0 * gx0 + gy0 * gy0);
  if (norm0 == 0.0) norm0 = 1.0;
  const double gh = g[2], gs = g[3];
  const double speed = sqrt(vx * vx + vy * vy);
  double* r = ag_rewards + (sv * T + t) * 8;
  r[0] = dist < c.pos_tol ? 1.0 : 0.0;
  r[1] = (fabs(angle_sub(gh, h)) < c.heading_tol ? 1.0 : 0.0) * ex;
  r[2] = (fabs(gs - speed) < c.speed_tol ? 1.0 : 0.0) * ex;
  r[3] = c.shaped_scaling * (1.0 - dist / norm0) / c.reward_scaling;
  r[4] = c.shaped_scaling * (1.0 - fabs(speed - gs) / 40.0) / c.reward_scaling * ex;
  r[5] = c.shaped_scaling * (1.0 - fabs(angle_sub(h, gh)) / (2.0 * 3.141592653589793)) / c.reward_scaling * ex;
  const unsigned char* cl = coll + (sv * T1 + t) * 2;
  r[6] = (double)cl[0] * ex;
  r[7] = (double)cl[1] * ex;
  // nearest existing other vehicle (dataset.py:202-237): 0 when this one is absent or alone
  double m = __builtin_inf();
  if (ex != 0.0) {
    for (int u = 0; u < N; ++u) {
      if (u == v || exist[((size_t)s * N + u) * T + t] == 0.0) continue;
      const float* ru = hist_states + (((size_t)s * N + u) * T1 + t) * 8;
      const double dx = x - (double)ru[0], dy = y - (double)ru[1];
      m = fmin(m, dx * dx + dy * dy);
    }
  }
  const double nd = m < __builtin_inf() ? sqrt(m) * ex * ex : 0.0;
  veh_veh[sv * T + t] = clipd(nd, 0.0, c.max_veh_dist) / c.max_veh_dist * ex;
  veh_edge[sv * T + t] = ex != 0.0 ? -edge_dist[sv * T + t] / c.edge_scale * ex : 0.0;
}

// the goal-reached latch over t (utils/sim.py:99-104, 116-120), one lane per vehicle: once the goal was reached the flag stays 1 and the
// shaped term takes its maximum; then the row's existence
__global__ __launch_bounds__(256) void reward_latch_kernel(int n, int T, const double* __restrict__ exist, ctrlsim_dataset_cfg c,
                                                           double* __restrict__ ag_rewards) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool achieved = false;
  for (int t = 0; t < T; ++t) {
    double* r = ag_rewards + ((size_t)i * T + t) * 8;
    const double ex = exist[(size_t)i * T + t];
    const bool now = r[0] != 0.0;
    const double r0 = achieved ? 1.0 : r[0], r3 = achieved ? c.shaped_scaling / c.reward_scaling : r[3];
    r[0] = r0 * ex;
    r[3] = r3 * ex;
    achieved = achieved || now;
  }
}

// compute_rewards + the reverse cumulative sum (ingest.load_preprocessed), one lane per vehicle walking its steps from the last one
// backwards: rtg[t] = rtg[t + 1] + reward[t], np.cumsum's order on the reversed axis
__global__ __launch_bounds__(256) void rtg_scan_kernel(int n, int T, const double* __restrict__ ag_rewards,
                                                       const double* __restrict__ veh_veh, const double* __restrict__ veh_edge,
                                                       const double* __restrict__ exist, ctrlsim_dataset_cfg c,
                                                       double* __restrict__ rtgs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int t = T - 1; t >= 0; --t) {
    const double* r = ag_rewards + ((size_t)i * T + t) * 8;
    const double ex = exist[(size_t)i * T + t], veh = veh_veh[(size_t)i * T + t], edge = veh_edge[(size_t)i * T + t];
    double a[5];
    a[0] = r[0] * c.goal_mult;
    if (!c.remove_shaped_goal) a[0] = a[0] + (clipd(r[3], c.shaped_min, c.shaped_max) - c.shaped_max) * (1.0 / c.shaped_max);
    a[1] = r[1] + r[5];
    a[2] = r[2] + r[4];
    a[3] = c.remove_shaped_veh ? -1.0 * r[6] * c.veh_mult : veh - r[6] * c.veh_mult;
    a[4] = c.remove_shaped_edge ? -1.0 * r[7] * c.edge_mult : clipd(fabs(edge) * c.edge_scale, 0.0, 5.0) / 5.0 - r[7] * c.edge_mult;
    double* o = rtgs + ((size_t)i * T + t) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double ak = a[k] * ex;
      acc[k] = t == T - 1 ? ak : acc[k] + ak;
      o[k] = acc[k];
    }
  }
}

// (S, N, T) of a batch: the point count of a scene and the grid of one-workgroup-per-256-points kernels must fit an int
bool dataset_dims_ok(int S, int N, int T) {
  if (S < 0 || N < 1 || N > 64 || T < 1) return false;
  const long pts = (long)N * T, blocks = (pts + 255) / 256;
  return pts <= 0x7fffffffL - 256 && blocks * (long)S <= 0x7fffffffL && (long)S * N <= 0x7fffffffL - 256;
}

}  // namespace

namespace {

template <typename CT>
int launch_edge_distance(int S, int P, int T, int T1, int E, int PE, const CT* pts, const double* exist, const CT* edges,
                         const int* poly_off, double* out, hipStream_t st) {
  if (S == 0) return CTRLSIM_OK;
  if (!poly_off) PE = 0;                    // (E = 0: no segment is read, and no offset)
  const int bps = (P + EDGE_STAGE - 1) / EDGE_STAGE;
  hipLaunchKernelGGL(edge_distance_kernel<CT>, dim3((unsigned)(S * bps)), dim3(EDGE_STAGE), 0, st, P, T, T1, E, PE, bps, pts, exist, edges,
                     poly_off, out);
  return ctrlsim_launch_status();
}

}  // namespace

extern "C" int ctrlsim_dataset_edge_distance(int S, int N, int T, int T1, int E, int PE, const float* hist_states, const double* exist,
                                             const float* edges, const int* poly_off, double* out, hipStream_t st) {
  if (!dataset_dims_ok(S, N, T) || T > T1 || E < 0 || E > 0x1fffffff || PE < 0 || !hist_states || !out ||
      (E > 0 && (!edges || !poly_off)))
    return CTRLSIM_EINVAL;
  return launch_edge_distance<float>(S, N * T, T, T1, E, PE, hist_states, exist, edges, poly_off, out, st);
}

extern "C" int ctrlsim_dataset_edge_distance_f64(int S, int P, int E, int PE, const double* xy, const double* exist, const double* edges,
                                                 const int* poly_off, double* out, hipStream_t st) {
  if (S < 0 || P < 1 || E < 0 || E > 0x1fffffff || PE < 0 || !xy || !out || (E > 0 && (!edges || !poly_off))) return CTRLSIM_EINVAL;
  if (P > 0x7fffffff - 256 || ((long)P + 255) / 256 * (long)S > 0x7fffffffL) return CTRLSIM_EINVAL;
  return launch_edge_distance<double>(S, P, 1, 1, E, PE, xy, exist, edges, poly_off, out, st);
}

extern "C" int ctrlsim_dataset_rtgs(int S, int N, int T, const double* ag_rewards, const double* veh_veh, const double* veh_edge,
                                    const double* exist, const ctrlsim_dataset_cfg* cfg, double* rtgs, hipStream_t st) {
  if (!dataset_dims_ok(S, N, T) || !ag_rewards || !veh_veh || !veh_edge || !exist || !cfg || !rtgs) return CTRLSIM_EINVAL;
  if (S == 0) return CTRLSIM_OK;
  const int n = S * N;
  hipLaunchKernelGGL(rtg_scan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, T, ag_rewards, veh_veh, veh_edge, exist, *cfg,
                     rtgs);
  return ctrlsim_launch_status();
}

extern "C" int ctrlsim_dataset_rewards(int S, int N, int T, int T1, const float* hist_states, const uint8_t* coll, const double* exist,
                                       const double* goals4, const double* edge_dist, const ctrlsim_dataset_cfg* cfg,
                                       double* ag_rewards, double* veh_veh, double* veh_edge, double* rtgs, hipStream_t st) {
  if (!dataset_dims_ok(S, N, T) || T > T1 || !hist_states || !coll || !exist || !goals4 || !edge_dist || !cfg || !ag_rewards || !veh_veh ||
      !veh_edge || !rtgs)
    return CTRLSIM_EINVAL;
  if (S == 0) return CTRLSIM_OK;
  const int bps = (N * T + 255) / 256, n = S * N;
  hipLaunchKernelGGL(reward_rows_kernel, dim3((unsigned)(S * bps)), dim3(256), 0, st, N, T, T1, bps, hist_states, coll, exist, goals4,
                     edge_dist, *cfg, ag_rewards, veh_veh, veh_edge);
  int rc = ctrlsim_launch_status();
  if (rc != CTRLSIM_OK) return rc;
  hipLaunchKernelGGL(reward_latch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, T, exist, *cfg, ag_rewards);
  rc = ctrlsim_launch_status();
  if (rc != CTRLSIM_OK) return rc;
  return ctrlsim_dataset_rtgs(S, N, T, ag_rewards, veh_veh, veh_edge, exist, cfg, rtgs, st);
}
