// Device-side log replay (gfx950): who drives a vehicle at step t — the policy or its log — decided and carried out per vehicle on the
// device, so that a partially controlled logged scene rolls inside RolloutEngine.run() without a host round trip per step.  One thread
// per vehicle, float64, two kernels per step:
//
//   replay_latch_kernel     existence of step t = the log's flag, latched at 0 once it was 0
//                           evaluators/policy_evaluator.py:118-121 (update_vehicle_data_dict: `if t > 0 and existence[-1] == 0: ex = 0`),
//                           with the speed read-back of the same function (veh.getSpeed()) as an optional per-step record
//   replay_actions_kernel   the (acceleration, steering) pair of step t, the simulator's `exists` flag and the action-history token:
//                           evaluators/policy_evaluator.py:534-540  vehicles_to_evaluate from t >= history_steps - 1: policy.act, else
//                                                                   apply_gt_action
//                           policies/autoregressive_policy.py:256-274  act: the sampled token undiscretised; a vehicle that does not exist
//                                                                   any more is parked; a vehicle no context answers for gets (0, 0)
//                           datasets/rl_waymo/dataset.py:322-338    undiscretize_actions / discretize_actions
//                           evaluators/evaluator.py:160-193         apply_gt_action: valid iff the log holds this step and the next one and
//                                                                   the vehicle has not been latched out; else (0, 0) and parked
//                           nocturne/bicycle_model.py:51-109        BicycleModel.backward: the inverse bicycle model against the next
//                                                                   logged state (with utils/geometry.py:3-12 angle_sub)
// Arithmetic follows the NumPy expressions of ctrlsim_amd/kinematics.py and ctrlsim_amd/discretize.py operation by operation (no FMA
// contraction; `%` as NumPy defines it for floats: fmod, then the divisor's sign), so that everything but the arctangent — a library
// function on both sides — gives the host's bits (ctrlsim_amd/replay.py is the host form the tests compare with).
//
// Both kernels serve a scene whose vehicles are driven by up to CTRLSIM_MAX_ROLES policy ROLES (planner, adversary, ...), each role with
// a policy view of the scene (the _views entry points); one policy and a `controlled` flag per vehicle (the plain entry points) is the
// case R = 1 without view arrays.
#include "launchers.h"
#include "../../include/ctrlsim.h"

#pragma clang fp contract(off)

namespace {

struct ReplayDisc {          // cfgs/dataset/waymo/base.yaml:13-16,41-42
  double min_accel, max_accel, min_steer, max_steer;
  int n_accel, n_steer;
};

// The pair of step t for vehicle i: the policy's token (by_policy; tok < 0 = no context answers for the vehicle) or the inverse bicycle
// model against the next logged state.  -> alive (the simulator's `exists` flag)
__device__ __forceinline__ bool replay_pair(int i, int t, int T1, double dt, bool by_policy, int tok, double ex,
                                            const double* __restrict__ log, const float* __restrict__ hist_states,
                                            const float* __restrict__ phys, const ReplayDisc& dz, double& accel, double& steer) {
  accel = 0.0;
  steer = 0.0;
  bool alive;
  if (by_policy) {
    alive = ex != 0.0;
    if (alive && tok >= 0) {                               // undiscretize_actions: the expressions of csrc/sim.hip's token path
      accel = (double)(tok / dz.n_steer) / (double)(dz.n_accel - 1);
      steer = (double)(tok % dz.n_steer) / (double)(dz.n_steer - 1);
      accel = accel * (dz.max_accel - dz.min_accel) + dz.min_accel;
      steer = steer * (dz.max_steer - dz.min_steer) + dz.min_steer;
    }
  } else {
    const double* cur = log + ((size_t)i * (T1 + 1) + t) * 6;
    const double* nx = cur + 6;
    alive = cur[4] != 0.0 && nx[4] != 0.0 && !(t > 0 && ex == 0.0);
    if (alive) {
      const float* row = hist_states + ((size_t)i * T1 + t) * 8;
      const double p_th = (double)row[4], p_v = (double)phys[(size_t)i * 20 + 16];
      const double n_th = nx[2], n_v = nx[3], n_len = nx[5];
      const double two_pi = 2.0 * 3.141592653589793;
      accel = (n_v - p_v) / dt;
      double d = fmod(n_th - p_th, two_pi);                 // angle_sub(current = prev, target = next)
      if (d != 0.0) { if (d < 0.0) d += two_pi; } else d = 0.0;
      if (d > 3.141592653589793) d = -(two_pi - d);
      const double w = d / dt;
      const double c = 2.0 * n_len * w / (n_v + p_v + 1e-10);
      steer = atan(2.0 * c / sqrt(4.0 - c * c));
      if (steer != steer) steer = 0.0;
      steer = fmin(fmax(steer, -0.7), 0.7);
    }
  }
  return alive;
}

// discretize_actions: clip, scale, round half to even
__device__ __forceinline__ int replay_token(double accel, double steer, const ReplayDisc& dz) {
  const double a0 = (fmin(fmax(accel, dz.min_accel), dz.max_accel) - dz.min_accel) / (dz.max_accel - dz.min_accel);
  const double a1 = (fmin(fmax(steer, dz.min_steer), dz.max_steer) - dz.min_steer) / (dz.max_steer - dz.min_steer);
  const double tokf = rint(a0 * (double)(dz.n_accel - 1)) * (double)dz.n_steer + rint(a1 * (double)(dz.n_steer - 1));
  return (int)tokf;
}

// ---- policy roles: S scenes, S * R policy views (view s * R + r = role r's picture of scene s, an ordinary engine scenario for
// the grouping, context, forward and sampling kernels).  The simulator runs on the scene; its state row, the latched existence and
// the applied action's token travel into every view of the scene, and a vehicle takes the token its own role's view sampled
// (evaluators/planner_adversary_evaluator.py:497-546: two policies, one scene, a common state and applied-action history).
__global__ __launch_bounds__(256) void replay_latch_kernel(int n, int N, int R, int t, int T1, const double* __restrict__ log,
                                                           const float* __restrict__ phys, double* __restrict__ exist_hist,
                                                           float* __restrict__ hist_states, float* __restrict__ speed_hist,
                                                           float* __restrict__ view_states) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double e = log[((size_t)i * (T1 + 1) + t) * 6 + 4];
  if (t > 0) e = e * (exist_hist[(size_t)i * T1 + t - 1] != 0.0 ? 1.0 : 0.0);
  exist_hist[(size_t)i * T1 + t] = e;
  float* row = hist_states + ((size_t)i * T1 + t) * 8;
  row[7] = (float)e;
  if (speed_hist) speed_hist[(size_t)i * T1 + t] = phys[(size_t)i * 20 + 16];
  if (!view_states) return;
  float4 lo = *reinterpret_cast<const float4*>(row), hi = *reinterpret_cast<const float4*>(row + 4);
  hi.w = (float)e;
  const int s = i / N, v = i - s * N;
  for (int r = 0; r < R; ++r) {
    float* dst = view_states + ((((size_t)s * R + r) * N + v) * T1 + t) * 8;
    *reinterpret_cast<float4*>(dst) = lo;
    *reinterpret_cast<float4*>(dst + 4) = hi;
  }
}

// who drives vehicle i: a policy role (>= 0) or the log (-1).  A `controlled` flag is role 0 of one policy
__device__ __forceinline__ int replay_role(const int* __restrict__ role, int i) { return role[i]; }
__device__ __forceinline__ int replay_role(const unsigned char* __restrict__ controlled, int i) { return controlled[i] ? 0 : -1; }

template <typename Who>
__global__ __launch_bounds__(256) void replay_actions_kernel(int n, int N, int R, int t, int T1, int Tmax, int history_steps, double dt,
                                                             const double* __restrict__ log, const Who* __restrict__ who,
                                                             const double* __restrict__ exist_hist,
                                                             const float* __restrict__ hist_states, const float* __restrict__ phys,
                                                             const int* __restrict__ act_now, ReplayDisc dz,
                                                             double* __restrict__ act_f64, unsigned char* __restrict__ exists,
                                                             int* __restrict__ hist_tok, int* __restrict__ view_tok) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = i / N, v = i - s * N;
  const double ex = exist_hist[(size_t)i * T1 + t];
  const int r = replay_role(who, i);
  const bool by_policy = r >= 0 && t >= history_steps - 1;
  // the token of the vehicle's OWN role's view (R = 1, role 0: act_now[i]); a role index the views do not hold answers like a view
  // without a context for it
  const int tok = (by_policy && r < R) ? act_now[((size_t)s * R + r) * N + v] : -1;
  double accel, steer;
  const bool alive = replay_pair(i, t, T1, dt, by_policy, tok, ex, log, hist_states, phys, dz, accel, steer);
  act_f64[(size_t)i * 2 + 0] = accel;
  act_f64[(size_t)i * 2 + 1] = steer;
  exists[i] = alive ? 1 : 0;
  const int token = replay_token(accel, steer, dz);
  hist_tok[(size_t)i * Tmax + t] = token;
  if (!view_tok) return;
  for (int q = 0; q < R; ++q) view_tok[(((size_t)s * R + q) * N + v) * Tmax + t] = token;
}

}  // namespace

int launch_replay_latch_views(int S, int N, int R, int t, int T1, const double* log, const float* phys, double* exist_hist,
                              float* hist_states, float* speed_hist, float* view_states, hipStream_t st) {
  if (S <= 0) return CTRLSIM_OK;
  if (N < 1 || R < 1 || R > CTRLSIM_MAX_ROLES || t < 0 || t >= T1 || !log || !exist_hist || !hist_states || (speed_hist && !phys))
    return CTRLSIM_EINVAL;
  const long n = (long)S * N;
  if (n * R > 0x7fffffffL - 256) return CTRLSIM_EINVAL;
  if (view_states == hist_states) view_states = nullptr;     // R = 1 on the scene's own tensors: nothing to copy
  if (!view_states && R != 1) return CTRLSIM_EINVAL;
  hipLaunchKernelGGL(replay_latch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int)n, N, R, t, T1, log, phys, exist_hist,
                     hist_states, speed_hist, view_states);
  return ctrlsim_launch_status();
}

int launch_replay_latch(int S, int N, int t, int T1, const double* log, const float* phys, double* exist_hist, float* hist_states,
                        float* speed_hist, hipStream_t st) {
  return launch_replay_latch_views(S, N, 1, t, T1, log, phys, exist_hist, hist_states, speed_hist, nullptr, st);
}

namespace {

// `who` = role [S,N] int32 or controlled [S,N] uint8 (replay_role)
template <typename Who>
int launch_actions(int S, int N, int R, int t, int T1, int Tmax, int history_steps, double dt, const double* log, const Who* who,
                   const double* exist_hist, const float* hist_states, const float* phys, const int* act_now, const double* disc6,
                   double* act_f64, unsigned char* exists, int* hist_tok, int* view_tok, hipStream_t st) {
  if (S <= 0) return CTRLSIM_OK;
  if (N < 1 || R < 1 || R > CTRLSIM_MAX_ROLES || t < 0 || t >= Tmax || t + 1 >= T1 || !log || !who || !exist_hist || !hist_states ||
      !phys || !act_now || !disc6 || !act_f64 || !exists || !hist_tok)
    return CTRLSIM_EINVAL;
  const long n = (long)S * N;
  if (n * R > 0x7fffffffL - 256) return CTRLSIM_EINVAL;
  if (view_tok == hist_tok) view_tok = nullptr;
  if (!view_tok && R != 1) return CTRLSIM_EINVAL;
  const ReplayDisc dz{disc6[0], disc6[1], disc6[2], disc6[3], (int)disc6[4], (int)disc6[5]};
  if (dz.n_accel < 2 || dz.n_steer < 2) return CTRLSIM_EINVAL;
  hipLaunchKernelGGL(replay_actions_kernel<Who>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int)n, N, R, t, T1, Tmax,
                     history_steps, dt, log, who, exist_hist, hist_states, phys, act_now, dz, act_f64, exists, hist_tok, view_tok);
  return ctrlsim_launch_status();
}

}  // namespace

int launch_replay_actions(int S, int N, int t, int T1, int Tmax, int history_steps, double dt, const double* log,
                          const unsigned char* controlled, const double* exist_hist, const float* hist_states, const float* phys,
                          const int* act_now, const double* disc6, double* act_f64, unsigned char* exists, int* hist_tok,
                          hipStream_t st) {
  return launch_actions(S, N, 1, t, T1, Tmax, history_steps, dt, log, controlled, exist_hist, hist_states, phys, act_now, disc6, act_f64,
                        exists, hist_tok, nullptr, st);
}

int launch_replay_actions_views(int S, int N, int R, int t, int T1, int Tmax, int history_steps, double dt, const double* log,
                                const int* role, const double* exist_hist, const float* hist_states, const float* phys,
                                const int* act_now, const double* disc6, double* act_f64, unsigned char* exists, int* hist_tok,
                                int* view_tok, hipStream_t st) {
  return launch_actions(S, N, R, t, T1, Tmax, history_steps, dt, log, role, exist_hist, hist_states, phys, act_now, disc6, act_f64, exists,
                        hist_tok, view_tok, st);
}
