// Open-loop training windows for B (scene, first step, origin agent) triples, cut from a device-resident dataset (gfx950).
// -ffp-contract=off.
//
// Reference (host NumPy, float64; restated in ingest.training_window) -> what this kernel replaces:
//   datasets/rl_waymo/dataset_ctrl_sim.py:99-160  training-mode get_data: return normalisation (components goal position, vehicle,
//                                                 road edge), moving ids, the window cut [t0, t0 + T), discretisation
//   datasets/rl_waymo/dataset.py:278-319          select_relevant_agents at window index 0: the A nearest of the filtered agents
//                                                 (those that exist at dataset step 0) within the distance threshold, slots in
//                                                 ascending agent order, the remaining slots padded BEFORE the transforms
//   datasets/rl_waymo/dataset.py:390-428          normalize_scene: SE(2) frame of the origin agent at window index 0, the nearest-P
//                                                 polylines (argsort of the max existing-point distance) or all of them and padding
//   utils/geometry.py:14-19,30-47                 angle_sub_tensor, apply_se2_transform
// The outputs are a ctrlsim_ctx in the layout ctrlsim_forward_loss reads (the one build_context_kernel of context.hip writes for the
// rollout), plus moving [B,A] u8 and status [B] i32.  All geometry is float64 as in the reference, rounded once to float32 on store.
//
// One workgroup of WIN_THREADS threads per window:
//   select   the first wave, one lane per vehicle (N <= 64): the triple is checked, the filtered set / the selection are ballots, the
//            rank in np.argsort(dist) a counted compare over lane shuffles (ties to the lower index), the slot a popcount; the frame
//            (rot, cos, sin, translation) is evaluated once and left in LDS for the block
//   agents   threads over (window step, slot): state row, existence, action token, the three return bins; then time steps and goals
//   roads    the phases of build_context_kernel, written again here for float64 sources and a per-scene polyline count (context.hip is
//            on the rollout's hot path and stays as it is): WIN_LPP neighbouring lanes take consecutive points of a polyline and reduce
//            their key by shuffles, rank[p] by counted compares in LDS, a wave gathers each output row
// A triple that cannot be served (status != 0) reads NOTHING of the dataset: its window is all padding (zero states with types -1,
// the token of the zero action, zero returns, zero time steps, zero polylines with types -1, nothing moving).
#include "launchers.h"
#include "../../include/ctrlsim.h"

#pragma clang fp contract(off)

namespace {

#define WIN_TWO_PI 6.283185307179586476925286766559
#define WIN_PI 3.14159265358979323846
constexpr int WIN_THREADS = 512;
constexpr int WIN_LPP = 16;      // lanes per polyline in the key sweep
static_assert(WIN_THREADS % 64 == 0 && 64 % WIN_LPP == 0, "whole waves, whole shuffle groups inside a wave");

__device__ __forceinline__ double win_mod_2pi(double a) {   // numpy/python float %: result takes the divisor's sign
  double m = fmod(a, WIN_TWO_PI);
  if (m != 0.0) { if (m < 0.0) m += WIN_TWO_PI; } else { m = 0.0; }
  return m;
}
__device__ __forceinline__ double win_angle_sub(double current, double target) {   // utils/geometry.py:14-19
  double d = win_mod_2pi(target - current);
  if (d > WIN_PI) d = -(WIN_TWO_PI - d);
  return d;
}
__device__ __forceinline__ double win_clip(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

struct WindowIn {
  const double* ag_data;      // [S,N,Td,8]
  const double* actions;      // [S,N,Td,2]
  const double* rtgs;         // [S,N,Td,5]
  const double* goals5;       // [S,N,5]
  const double* types;        // [S,N,5]
  const double* road_points;  // [S,Pmax,NP,3]
  const double* road_types;   // [S,Pmax,8]
  const int* n_polys;         // [S]
  const int* win_scn;         // [B]
  const int* win_t0;
  const int* win_agent;
};

// LDS, all of it dynamic (the base stays 16-byte aligned): double key[Pmax], double frame[6], then int rank[Pmax], sel[P], gid_of[64],
// mov_of[64], head[4] = {status, selected vehicles, polylines of the scene, -}
__global__ __launch_bounds__(WIN_THREADS) void window_build_kernel(int S, int N, int Td, int T, int A, int Pmax, int P, int NP, WindowIn in,
                                                                   ctrlsim_window_cfg c, CtxOut o, unsigned char* __restrict__ moving,
                                                                   int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double win_lds[];
  double* key = win_lds;
  double* frame = key + Pmax;
  int* rank = reinterpret_cast<int*>(frame + 6);
  int* sel = rank + Pmax;
  int* gid_of = sel + P;
  int* mov_of = gid_of + 64;
  int* head = mov_of + 64;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int s = in.win_scn[b], t0 = in.win_t0[b], wa = in.win_agent[b];        // the same for every thread of the block
  int st0 = CTRLSIM_WINDOW_OK;
  if (s < 0 || s >= S) st0 = CTRLSIM_WINDOW_SCENE;
  else if (t0 < 0 || t0 > Td - T) st0 = CTRLSIM_WINDOW_STEP;

  // ---- select: the first wave, one lane per vehicle
  if (tid < 64) {
    const bool live = st0 == CTRLSIM_WINDOW_OK && tid < N;
    bool fil = false, mov = false;
    double x = 0.0, y = 0.0, yaw = 0.0, ex = 0.0;
    if (live) {
      const double* row0 = in.ag_data + ((size_t)s * N + tid) * Td * 8;         // dataset step 0: the filter and the moving mask
      const double* rw = row0 + (size_t)t0 * 8;                                 // the window's first step
      const double* g = in.goals5 + ((size_t)s * N + tid) * 5;
      fil = row0[7] != 0.0;
      const double mx = row0[0] - g[0], my = row0[1] - g[1];
      mov = sqrt(mx * mx + my * my) > c.moving_threshold;
      x = rw[0]; y = rw[1]; yaw = rw[4]; ex = rw[7];
    }
    const unsigned long long F = __ballot(fil);
    const unsigned long long below = (tid == 0) ? 0ull : (~0ull >> (64 - tid));
    int st = st0;
    if (st == CTRLSIM_WINDOW_OK && (wa < 0 || wa >= __popcll(F))) st = CTRLSIM_WINDOW_AGENT;
    // the origin vehicle: the filtered agent of index wa (exactly one lane answers when the index is in range)
    const unsigned long long O = __ballot(fil && __popcll(F & below) == wa);
    const int org = (st == CTRLSIM_WINDOW_OK && O) ? __ffsll((long long)O) - 1 : 0;
    const double ox = __shfl(x, org, 64), oy = __shfl(y, org, 64), oyaw = __shfl(yaw, org, 64), oex = __shfl(ex, org, 64);
    const int omov = __shfl((int)mov, org, 64);
    if (st == CTRLSIM_WINDOW_OK && oex != 1.0) st = CTRLSIM_WINDOW_ABSENT;
    if (st == CTRLSIM_WINDOW_OK && !omov) st = CTRLSIM_WINDOW_STILL;
    const bool ok = st == CTRLSIM_WINDOW_OK;
    // select_relevant_agents over the filtered agents
    const double dx = ox - x, dy = oy - y;
    const double d = (ok && fil) ? sqrt(dx * dx + dy * dy) : __builtin_inf();
    int rk = 0;                                         // position in np.argsort(dist), ties to the lower index
    for (int i = 0; i < N; ++i) {
      const double di = __shfl(d, i, 64);
      rk += (di < d || (di == d && i < tid)) ? 1 : 0;
    }
    const unsigned long long ids = __ballot(ok && fil && rk < A && d < c.agent_dist_threshold);
    if ((ids >> tid) & 1ull) {
      const int slot = __popcll(ids & below);
      gid_of[slot] = tid;
      mov_of[slot] = mov ? 1 : 0;
    }
    if (tid == 0) {
      // normalize_scene's frame (dataset.py:392-396); a refused window keeps the identity at the origin: padding stays zero
      double rot = 0.0, cr = 1.0, sr = 0.0, tx = 0.0, ty = 0.0;
      if (ok) {
        const double sgn = (-oyaw > 0.0) ? 1.0 : ((-oyaw < 0.0) ? -1.0 : 0.0);
        rot = (WIN_PI / 2) + sgn * fabs(oyaw);
        cr = cos(rot); sr = sin(rot); tx = ox; ty = oy;
      }
      frame[0] = rot; frame[1] = cr; frame[2] = sr; frame[3] = tx; frame[4] = ty;
      int np_ = ok ? in.n_polys[s] : 0;
      np_ = np_ < 0 ? 0 : (np_ > Pmax ? Pmax : np_);    // rows beyond the table the caller described are never read
      head[0] = st; head[1] = __popcll(ids); head[2] = np_;
      status[b] = st;
    }
  }
  __syncthreads();
  const double rot = frame[0], cr = frame[1], sr = frame[2], tx = frame[3], ty = frame[4];
  const bool ok = head[0] == CTRLSIM_WINDOW_OK;
  const int n_ids = head[1], P_all = head[2];

  // ---- agents
  // padded slots: zero state rows (their transform is the transform of zero), zero action -> its token, zero returns (dataset.py:284-288)
  const double a0z = (win_clip(0.0, c.min_accel, c.max_accel) - c.min_accel) / (c.max_accel - c.min_accel);
  const double a1z = (win_clip(0.0, c.min_steer, c.max_steer) - c.min_steer) / (c.max_steer - c.min_steer);
  const int zero_tok = (int)(rint(a0z * (double)(c.accel_discretization - 1)) * (double)c.steer_discretization +
                             rint(a1z * (double)(c.steer_discretization - 1)));
  const int zero_rtg = c.continuous_rtg ? __float_as_int(0.f) : 0;
  for (int k = tid; k < T * A; k += WIN_THREADS) {
    const int tt = k / A, slot = k - tt * A;
    double raw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float ty5[5] = {-1.f, -1.f, -1.f, -1.f, -1.f};
    int tok = zero_tok, rb[3] = {zero_rtg, zero_rtg, zero_rtg};
    if (slot < n_ids) {
      const size_t sv = (size_t)s * N + gid_of[slot];
      const size_t at = sv * Td + (size_t)(t0 + tt);
      const double* row = in.ag_data + at * 8;
#pragma unroll
      for (int q = 0; q < 8; ++q) raw[q] = row[q];
#pragma unroll
      for (int q = 0; q < 5; ++q) ty5[q] = (float)in.types[sv * 5 + q];
      // discretize_actions: the expressions of replay.hip's replay_token (clip, scale, round half to even)
      const double* ac = in.actions + at * 2;
      const double a0 = (win_clip(ac[0], c.min_accel, c.max_accel) - c.min_accel) / (c.max_accel - c.min_accel);
      const double a1 = (win_clip(ac[1], c.min_steer, c.max_steer) - c.min_steer) / (c.max_steer - c.min_steer);
      tok = (int)(rint(a0 * (double)(c.accel_discretization - 1)) * (double)c.steer_discretization +
                  rint(a1 * (double)(c.steer_discretization - 1)));
      // returns: components goal position, vehicle, road edge, clipped and normalised (dataset_ctrl_sim.py:99-107)
      const double* rt = in.rtgs + at * 5;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double lo = c.rtg_lo[q], hi = c.rtg_hi[q];
        const double r = (win_clip(rt[q == 0 ? 0 : q + 2], lo, hi) - lo) / (hi - lo);
        rb[q] = c.continuous_rtg ? __float_as_int((float)r) : (int)rint(r * (double)(c.rtg_discretization - 1));
      }
    }
    const double px = raw[0] - tx, py = raw[1] - ty;
    const size_t ro = ((size_t)b * T + tt) * A + slot;
    float* so = o.st12 + ro * 12;
    so[0] = (float)(cr * px + (-sr) * py);
    so[1] = (float)(sr * px + cr * py);
    so[2] = (float)(cr * raw[2] + (-sr) * raw[3]);
    so[3] = (float)(sr * raw[2] + cr * raw[3]);
    so[4] = (float)win_angle_sub(raw[4], -rot);
    so[5] = (float)raw[5];
    so[6] = (float)raw[6];
#pragma unroll
    for (int q = 0; q < 5; ++q) so[7 + q] = ty5[q];
    o.exist[ro] = (float)raw[7];
    o.act_tok[ro] = tok;
    o.rtg_bin[ro * 3] = rb[0]; o.rtg_bin[ro * 3 + 1] = rb[1]; o.rtg_bin[ro * 3 + 2] = rb[2];
  }
  for (int tt = tid; tt < T; tt += WIN_THREADS) o.tstep[(size_t)b * T + tt] = ok ? t0 + tt : 0;
  // goals (constant in time), the moving mask, the slot's agent-id row (open-loop contexts number their slots 0 .. A-1)
  for (int slot = tid; slot < A; slot += WIN_THREADS) {
    double gr[5] = {0, 0, 0, 0, 0};
    if (slot < n_ids) {
      const double* gp = in.goals5 + ((size_t)s * N + gid_of[slot]) * 5;
#pragma unroll
      for (int q = 0; q < 5; ++q) gr[q] = gp[q];
    }
    const double px = gr[0] - tx, py = gr[1] - ty;
    float* go = o.goal5 + ((size_t)b * A + slot) * 5;
    go[0] = (float)(cr * px + (-sr) * py);
    go[1] = (float)(sr * px + cr * py);
    go[2] = (float)(cr * gr[2] + (-sr) * gr[3]);
    go[3] = (float)(sr * gr[2] + cr * gr[3]);
    go[4] = (float)win_angle_sub(gr[4], -rot);
    moving[(size_t)b * A + slot] = (unsigned char)(slot < n_ids ? mov_of[slot] : 0);
    if (o.slot_gid) o.slot_gid[(size_t)b * A + slot] = slot;
  }

  // ---- roads
  const int rowd = NP * 3;                             // values of one polyline
  const double* rsrc = in.road_points + (size_t)(ok ? s : 0) * Pmax * rowd;     // (P_all = 0 when refused: never dereferenced)
  if (P_all > P) {
    // keys: the trip count is the same for every thread, so that all lanes of a wave meet at the shuffles
    const int sub = tid & (WIN_LPP - 1), grp = tid / WIN_LPP;
    for (int p0 = 0; p0 < P_all; p0 += WIN_THREADS / WIN_LPP) {
      const int p = p0 + grp;
      double mxd = 0.0;
      if (p < P_all) {
        const double* pl = rsrc + (size_t)p * rowd;
#pragma unroll 4
        for (int q = sub; q < NP; q += WIN_LPP) {
          const double px = pl[q * 3] - tx, py = pl[q * 3 + 1] - ty;
          const double x = cr * px + (-sr) * py, y = sr * px + cr * py;
          const double dd = sqrt(x * x + y * y) * pl[q * 3 + 2];
          if (dd > mxd) mxd = dd;
        }
      }
#pragma unroll
      for (int off = WIN_LPP / 2; off > 0; off >>= 1) {
        const double other = __shfl_xor(mxd, off, 64);
        if (other > mxd) mxd = other;
      }
      if (sub == 0 && p < P_all) { key[p] = mxd; rank[p] = 0; }
    }
    __syncthreads();
    // rank: item (h, p) counts the polylines q of range h that come before p (ascending key, ties to the lower index)
    const int H = P_all >= WIN_THREADS ? 1 : (WIN_THREADS + P_all - 1) / P_all;
    const int span = (P_all + H - 1) / H;
    for (int k = tid; k < P_all * H; k += WIN_THREADS) {
      const int h = k / P_all, p = k - h * P_all;
      const int q0 = h * span, q1 = min(P_all, q0 + span);
      const double d = key[p];
      int before = 0;
#pragma unroll 8
      for (int q = q0; q < q1; ++q) {
        const double dq = key[q];
        before += (dq < d || (dq == d && q < p)) ? 1 : 0;
      }
      if (before) atomicAdd(&rank[p], before);
    }
    __syncthreads();
    for (int p = tid; p < P_all; p += WIN_THREADS) {
      const int r = rank[p];
      if (r < P) sel[r] = p;
    }
    __syncthreads();
  }
  const int n_live = P_all > P ? P : P_all;
  for (int r = tid >> 6; r < P; r += WIN_THREADS / 64) {          // a wave per output row
    float* po = o.road_pts + ((size_t)b * P + r) * rowd;
    if (r < n_live) {
      const int p = P_all > P ? sel[r] : r;
      const double* pl = rsrc + (size_t)p * rowd;
#pragma unroll 4
      for (int f = tid & 63; f < rowd; f += 64) {
        const int q = f / 3, cc = f - q * 3;
        const double px = pl[q * 3] - tx, py = pl[q * 3 + 1] - ty;
        // cc == 0: cr * px + (-sr) * py, cc == 1: sr * px + cr * py — the same products and sum as written out
        const double ca = cc == 0 ? cr : sr, cb_ = cc == 0 ? -sr : cr;
        const float xy = (float)(ca * px + cb_ * py);
        po[f] = cc == 2 ? (float)pl[f] : xy;
      }
    } else {
      for (int f = tid & 63; f < rowd; f += 64) po[f] = 0.f;
    }
  }
  for (int k = tid; k < P * 8; k += WIN_THREADS) {
    const int r = k >> 3, cc = k & 7;
    float v = -1.f;
    if (r < n_live) {
      const int p = P_all > P ? sel[r] : r;
      v = (float)in.road_types[((size_t)s * Pmax + p) * 8 + cc];
    }
    o.road_types[((size_t)b * P + r) * 8 + cc] = v;
  }
}

}  // namespace

int launch_window_build(int B, int S, int N, int Td, int T, int A, int Pmax, int P, int NP, const double* ag_data, const double* actions,
                        const double* rtgs, const double* goals5, const double* types, const double* road_points,
                        const double* road_types, const int* n_polys, const int* win_scn, const int* win_t0, const int* win_agent,
                        const ctrlsim_window_cfg& cfg, CtxOut o, unsigned char* moving, int* status, hipStream_t st) {
  if (B == 0) return CTRLSIM_OK;
  if (B < 0 || S < 1 || N < 1 || N > 64 || T < 1 || Td < T || A < 1 || A > 64 || Pmax < 0 || P < 1 || NP < 1) return CTRLSIM_EINVAL;
  if (!ag_data || !actions || !rtgs || !goals5 || !types || !n_polys || !win_scn || !win_t0 || !win_agent || !moving || !status ||
      (Pmax > 0 && (!road_points || !road_types)))
    return CTRLSIM_EINVAL;
  if (!o.st12 || !o.exist || !o.goal5 || !o.act_tok || !o.rtg_bin || !o.tstep || !o.road_pts || !o.road_types) return CTRLSIM_EINVAL;
  if (cfg.rtg_discretization < 2 || cfg.accel_discretization < 2 || cfg.steer_discretization < 2) return CTRLSIM_EINVAL;
  // every index of the kernel is a size_t product; the counts themselves must fit an int
  if ((long)T * A > 0x7fffffffL || (long)NP * 3 > 0x7fffffffL || (long)P * 8 > 0x7fffffffL) return CTRLSIM_EINVAL;
  const size_t shm = (size_t)Pmax * (sizeof(double) + sizeof(int)) + 6 * sizeof(double) + ((size_t)P + 64 + 64 + 4) * sizeof(int);
  if (shm > 64 * 1024) return CTRLSIM_EINVAL;
  const WindowIn in{ag_data, actions, rtgs, goals5, types, road_points, road_types, n_polys, win_scn, win_t0, win_agent};
  hipLaunchKernelGGL(window_build_kernel, dim3((unsigned)B), dim3(WIN_THREADS), shm, st, S, N, Td, T, A, Pmax, P, NP, in, cfg, o, moving,
                     status);
  return ctrlsim_launch_status();
}

extern "C" int ctrlsim_window_build(int B, int S, int N, int Td, int T, int A, int Pmax, int P, int NP, const double* ag_data,
                                    const double* actions, const double* rtgs, const double* goals5, const double* types,
                                    const double* road_points, const double* road_types, const int* n_polys, const int* win_scn,
                                    const int* win_t0, const int* win_agent, const ctrlsim_window_cfg* cfg, const ctrlsim_ctx* out,
                                    uint8_t* moving, int* status, hipStream_t st) {
  if (!cfg || !out) return CTRLSIM_EINVAL;
  const CtxOut o{out->st12, out->exist, out->goal5, out->act_tok, out->rtg_bin, out->tstep, out->slot_gid, out->road_pts, out->road_types};
  return launch_window_build(B, S, N, Td, T, A, Pmax, P, NP, ag_data, actions, rtgs, goals5, types, road_points, road_types, n_polys,
                             win_scn, win_t0, win_agent, *cfg, o, moving, status, st);
}
