"""Host form (NumPy float64) of the device-side log replay of csrc/replay.hip — what the tests compare the kernels with.

A logged scene hands some vehicles to the policy (`controlled`, from step history_steps - 1) and replays every other vehicle's
log through the inverse bicycle model (evaluators/policy_evaluator.py:534-540, evaluators/evaluator.py:160-193).  Two phases
per step t, the same two the engine queues around its launches (include/ctrlsim.h: ctrlsim_replay_latch / _actions):

  latch    existence of step t = the log's flag, 0 for good once it was 0     (policy_evaluator.py:118-121)
  actions  (accel, steer), the simulator's `exists` flag and the action-history token of step t

Arrays: log [..., T1 + 1, 6] = x, y, heading, speed, exist, length (zero rows past the end of a vehicle's log),
controlled [...] bool, exist_t / exist_prev [...] float64.  Built from kinematics.bicycle_backward and discretize.*, the
functions the per-scenario loop calls; the host-driven batched route (PolicyEvaluator._roll_batch) calls latch / actions themselves.
"""
import numpy as np

from . import discretize as dz
from .kinematics import bicycle_backward


def log_array(gt_data_dicts, N, T1):
    """The logs of S scenes, gt_data_dicts[k][v]["traj"] = rows of x, y, heading, speed, exist, ..., length, as [S, N, T1 + 1, 6]
    (T1 = steps + 1; one row more: step t looks at t + 1): a longer log is truncated, zero rows (existence 0) past the end of a shorter one."""
    log = np.zeros((len(gt_data_dicts), N, T1 + 1, 6))
    for k, gtd in enumerate(gt_data_dicts):
        for v in range(N):
            tr = np.asarray(gtd[v]["traj"], np.float64)
            n = min(len(tr), T1 + 1)
            log[k, v, :n, :5] = tr[:n, :5]
            log[k, v, :n, 5] = tr[:n, -1]
    return log


def latch(log, t, exist_prev=None):
    """Existence of step t: log[..., t, 4] at t = 0, log[..., t, 4] * (exist_prev != 0) afterwards."""
    log = np.asarray(log, np.float64)
    if t == 0:
        return log[..., 0, 4].copy()
    return log[..., t, 4] * (np.asarray(exist_prev, np.float64) != 0)


def latch_all(log, T1):
    """exist_hist [..., T1]: the latch run over rows 0 .. T1 - 1."""
    log = np.asarray(log, np.float64)
    out = np.zeros(log.shape[:-2] + (T1,))
    for t in range(T1):
        out[..., t] = latch(log, t, out[..., t - 1] if t else None)
    return out


def actions(log, controlled, exist_t, t, history_steps, heading, speed, act_now, dt, w):
    """Step t for every vehicle -> (act [..., 2] float64, alive [...] bool, token [...] int32).
    heading / speed: the vehicles' current heading (history row t) and speed, any float type (widened to float64 as the kernel does);
    act_now: the sampled tokens, < 0 = no context answers for the vehicle; w = cfg.dataset.waymo."""
    log = np.asarray(log, np.float64)
    ctrl = np.asarray(controlled).astype(bool)
    ex = np.asarray(exist_t, np.float64)
    toks = np.asarray(act_now)
    a = np.zeros(ctrl.shape)
    st = np.zeros(ctrl.shape)
    alive = np.ones(ctrl.shape, bool)
    by_policy = ctrl & (t >= history_steps - 1)
    # policy.act (autoregressive_policy.py:256-274)
    und = dz.undiscretize_actions(np.maximum(toks, 0), w)
    live = by_policy & (ex != 0)
    a[live] = np.where(toks[live] >= 0, und[live][:, 0], 0.0)
    st[live] = np.where(toks[live] >= 0, und[live][:, 1], 0.0)
    alive[by_policy & (ex == 0)] = False
    # apply_gt_action (evaluators/evaluator.py:160-193)
    rep = ~by_policy
    ok = rep & (log[..., t, 4] != 0) & (log[..., t + 1, 4] != 0) & ~((t > 0) & (ex == 0))
    if ok.any():
        nxt = np.concatenate([log[..., t + 1, :4][ok], log[..., t + 1, 5][ok][:, None]], 1)
        zero = np.zeros(int(ok.sum()))
        prev = np.stack([zero, zero, np.asarray(heading)[ok].astype(np.float64), np.asarray(speed)[ok].astype(np.float64)], 1)
        a[ok], st[ok] = bicycle_backward(nxt, prev, dt)      # (the model reads heading and speed of the current state only)
    alive[rep & ~ok] = False
    act = np.stack([a, st], -1)
    return act, alive, dz.discretize_actions(act, w).astype(np.int32)


# ---- policy roles (include/ctrlsim.h: ctrlsim_replay_latch_views / _actions_views): a scene [..., N] has R policy views
# [..., R, N]; role [..., N] int = -1 (the log drives the vehicle) or the view whose policy drives it
def latch_views(log, t, exist_prev, state_row, view_states):
    """The latch of step t on a scene and its views.  state_row [..., N, 8] float32 = the row the simulator wrote;
    view_states [..., R, N, T1, 8] float32 is updated in place: row t of every view <- the scene's row, existence column latched.
    -> (exist_t [..., N] float64, the scene's row with the latched existence column)."""
    ex = latch(log, t, exist_prev)
    row = np.array(state_row, np.float32)
    row[..., 7] = ex.astype(np.float32)
    view_states[..., t, :] = row[..., None, :, :]
    return ex, row


def actions_views(log, role, exist_t, t, history_steps, heading, speed, act_now_views, dt, w):
    """Step t of a scene with roles -> (act [..., N, 2], alive [..., N], token [..., N]) as actions(): role >= 0 stands for
    `controlled`, and vehicle v of role r takes act_now_views[..., r, v] — the token its own role's view sampled (< 0, or a role the
    views do not hold: nobody answers, (0, 0)).  The token goes into the scene's action history and every view's."""
    role = np.asarray(role)
    toks = np.asarray(act_now_views)
    R = toks.shape[-2]
    ok = (role >= 0) & (role < R)
    own = np.take_along_axis(toks, np.clip(role, 0, R - 1)[..., None, :], axis=-2)[..., 0, :]
    return actions(log, role >= 0, exist_t, t, history_steps, heading, speed, np.where(ok, own, -1), dt, w)


def merge_cat_log(log, adv, traj, history_steps):
    """The log of a scene whose adversary `adv` follows a fixed trajectory (PlannerAdversaryEvaluator.apply_adv_traj,
    planner_adversary_evaluator.py:163-199) instead of a policy: a copy of log [N, T1 + 1, 6] in which the adversary's rows
    >= history_steps take x, y, heading and speed = hypot(vx, vy) from traj [>= T1, 5] = x, y, vx, vy, yaw (rows beyond the trajectory
    keep the log's).  Existence and length stay the log's, so the replay branch (role -1) decides validity and latches exactly as
    apply_adv_traj does, and reaches for the trajectory from step history_steps - 1 on, as the loop does."""
    out = np.array(log, np.float64)
    traj = np.asarray(traj, np.float64)
    n = min(out.shape[-2], len(traj))
    hs = int(history_steps)
    if n > hs:
        out[adv, hs:n, 0] = traj[hs:n, 0]
        out[adv, hs:n, 1] = traj[hs:n, 1]
        out[adv, hs:n, 2] = traj[hs:n, 4]
        out[adv, hs:n, 3] = np.sqrt(traj[hs:n, 2] ** 2 + traj[hs:n, 3] ** 2)
    return out


def token_margin(act, w):
    """Distance of the scaled (accel, steer) of discretize_actions from the nearest half-integer, [..., 2]: where it is tiny, a last-bit
    difference of the pair may round to the neighbouring bin."""
    a = np.asarray(act, np.float64)
    a0 = (np.clip(a[..., 0], w.min_accel, w.max_accel) - w.min_accel) / (w.max_accel - w.min_accel) * (w.accel_discretization - 1)
    a1 = (np.clip(a[..., 1], w.min_steer, w.max_steer) - w.min_steer) / (w.max_steer - w.min_steer) * (w.steer_discretization - 1)
    v = np.stack([a0, a1], -1)
    return np.abs(v - np.floor(v) - 0.5)
