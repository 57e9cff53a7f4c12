"""GPU: policy roles per vehicle (RolloutEngine.set_roles) — the _views entries of csrc/replay.hip against their host form, run() with
roles against R ordinary single-policy engines stepped by the host, scheduling invariance, R = 1 against set_log alone, and the
planner-vs-adversary evaluator's cfg.eval_planner_adversary.device_replay route against its stepwise route and the reference fixture."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import cfg_of, golden  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402
from replay_utils import ULP, _ulps, _disc6, _cut_logs, host_driven, assert_rollouts_agree  # noqa: E402
from ctrlsim_amd import _lib, replay, scenarios  # noqa: E402
from ctrlsim_amd.engine import RolloutEngine  # noqa: E402
from ctrlsim_amd.models import CtRLSim  # noqa: E402
from ctrlsim_amd.policies import AutoregressivePolicy  # noqa: E402
from ctrlsim_amd.evaluators import PlannerAdversaryEvaluator  # noqa: E402
from ctrlsim_amd.evaluators.planner_adversary_evaluator import PLANNER_KEYS, ADVERSARY_KEYS, pick_ego_adversary  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------- (a) kernels
@pytest.mark.parametrize("t,hsteps", [(0, 3), (2, 3), (4, 3)])
def test_views_kernels_match_the_host_form(t, hsteps):
    w = cfg_of("loop").dataset.waymo
    S, N, R, T1 = 8, 64, 3, 6
    Tmax = T1 - 1
    rs = np.random.RandomState(70 + t)
    log = np.zeros((S, N, T1 + 1, 6))
    log[..., 0] = rs.uniform(-100, 100, (S, N, T1 + 1))
    log[..., 1] = rs.uniform(-100, 100, (S, N, T1 + 1))
    log[..., 2] = rs.uniform(-np.pi, np.pi, (S, N, 1)) + rs.uniform(-0.15, 0.15, (S, N, T1 + 1))
    log[..., 3] = rs.uniform(0.5, 25.0, (S, N, 1)) + rs.uniform(-0.4, 0.4, (S, N, T1 + 1))
    log[..., 4] = (rs.uniform(size=(S, N, T1 + 1)) < 0.93).astype(np.float64)
    log[..., 5] = rs.uniform(3.0, 7.0, (S, N, 1))
    role = rs.randint(-1, R, (S, N)).astype(np.int32)
    role[1][role[1] == 2] = -1                             # a scene with an unused role
    exist_prev = (rs.uniform(size=(S, N)) < 0.85).astype(np.float64)          # latched-out vehicles
    heading = (log[:, :, t, 2] + rs.uniform(-0.02, 0.02, (S, N))).astype(np.float32)
    speed = (log[:, :, t, 3] + rs.uniform(-0.3, 0.3, (S, N))).astype(np.float32)
    toks_v = rs.randint(0, 1000, (S, R, N)).astype(np.int32)
    toks_v[rs.uniform(size=(S, R, N)) < 0.1] = -1
    # ---- device
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    eh = np.zeros((S, N, T1))
    if t > 0:
        eh[:, :, t - 1] = exist_prev
    hs = rs.uniform(-5, 5, (S, N, T1, 8)).astype(np.float32)
    hs[:, :, t, 4] = heading
    hs[:, :, t, 7] = 1.0
    phys = np.zeros((S, N, 20), np.float32)
    phys[:, :, 16] = speed
    log_d, role_d, eh_d, hs_d, phys_d = dev(log), dev(role), dev(eh), dev(hs), dev(phys)
    sp_d = torch.zeros(S, N, T1, device=DEV)
    vs_d = torch.full((S * R, N, T1, 8), -3.0, device=DEV)
    vt_d = torch.full((S * R, N, Tmax), -5, dtype=torch.int32, device=DEV)
    tok_d = dev(toks_v.reshape(S * R, N))
    act_d = torch.full((S, N, 2), 7.0, dtype=torch.float64, device=DEV)
    ex_d = torch.full((S, N), 9, dtype=torch.uint8, device=DEV)
    ht_d = torch.full((S, N, Tmax), -5, dtype=torch.int32, device=DEV)
    _lib.check(lib.ctrlsim_replay_latch_views(S, N, R, t, T1, p(log_d), p(phys_d), p(eh_d), p(hs_d), p(sp_d), p(vs_d), st), "latch_views")
    _lib.check(lib.ctrlsim_replay_actions_views(S, N, R, t, T1, Tmax, hsteps, 0.1, p(log_d), p(role_d), p(eh_d), p(hs_d), p(phys_d),
                                                p(tok_d), _disc6(w), p(act_d), p(ex_d), p(ht_d), p(vt_d), st), "actions_views")
    torch.cuda.synchronize()
    # ---- host form
    vs_h = np.full((S, R, N, T1, 8), -3.0, np.float32)
    ex, row = replay.latch_views(log, t, exist_prev if t > 0 else None, hs[:, :, t], vs_h)
    act, alive, tok = replay.actions_views(log, role, ex, t, hsteps, heading, speed, toks_v, 0.1, w)
    # ---- existence, `exists`, accel, tokens: the host's bits; steer: the device arctangent
    assert np.array_equal(eh_d.cpu().numpy()[:, :, t], ex)
    hs_out = hs_d.cpu().numpy()
    assert np.array_equal(hs_out[:, :, t], row)
    hs_ref = hs.copy(); hs_ref[:, :, t, 7] = ex
    assert np.array_equal(hs_out, hs_ref)                                  # the scene: only the existence column of row t
    assert np.array_equal(sp_d.cpu().numpy()[:, :, t], speed)
    assert np.array_equal(ex_d.cpu().numpy(), alive.astype(np.uint8))
    a_d = act_d.cpu().numpy()
    assert np.array_equal(a_d[..., 0].view(np.int64), act[..., 0].view(np.int64)), "accel is not bit-equal"
    u = _ulps(a_d[..., 1], act[..., 1])
    print(f"t={t}: {u.size} rows, largest steer distance {u.max():.1f} ulp ({int((u > 0).sum())} rows differ)")
    assert u.max() <= ULP
    ht = ht_d.cpu().numpy()
    assert np.array_equal(ht[:, :, t], tok)
    assert (np.delete(ht, t, axis=2) == -5).all()
    # ---- every view holds the scene's state row and token column, and nothing else was written
    vs = vs_d.cpu().numpy().reshape(S, R, N, T1, 8)
    vt = vt_d.cpu().numpy().reshape(S, R, N, Tmax)
    for r in range(R):
        assert np.array_equal(vs[:, r, :, t], hs_out[:, :, t]) and np.array_equal(vt[:, r, :, t], ht[:, :, t])
    assert np.array_equal(vs, vs_h)
    assert (np.delete(vs, t, axis=3) == -3.0).all() and (np.delete(vt, t, axis=3) == -5).all()
    # ---- the inputs reach every branch
    by_policy = (role >= 0) & (t >= hsteps - 1)
    own = np.take_along_axis(toks_v, np.clip(role, 0, R - 1)[:, None, :], 1)[:, 0]
    assert (role == -1).sum() > 50 and not (role[1] == 2).any() and (ex == 0).sum() > 20
    if t >= hsteps - 1:
        assert (by_policy & (ex != 0) & (own >= 0)).sum() > 100 and (by_policy & (ex != 0) & (own < 0)).sum() > 5
        assert (by_policy & (ex == 0)).sum() > 5
        live = by_policy & (ex != 0) & (own >= 0)
        assert np.array_equal(tok[live], own[live])
    else:
        assert (alive & (role >= 0)).sum() > 100          # history steps: the log drives the roles' vehicles too


# ---------------------------------------------------------------------------------------------------------------- engine
TILTS2 = np.array([[10.0, 10.0, 10.0], [0.0, -10.0, 0.0]])
TILTS3 = np.array([[10.0, 10.0, 10.0], [0.0, -10.0, 0.0], [-5.0, 5.0, -5.0]])


def _model(cfg):
    return CtRLSim(cfg, seed=0, device=DEV)


def _scenes(cfg, model, S, N, seed, cut=None):
    """S synthetic scenes with their stand-in logs -> (scenes, log [S,N,T1+1,6])."""
    T = cfg.nocturne.steps
    scns = [scenarios.make_scenario(seed, k, n_agents=N, n_polylines=14, n_points=model.dims.NP, extent=40.0) for k in range(S)]
    gtds = [scenarios.standin_log(scn, T, cfg.nocturne.dt) for scn in scns]
    if cut is not None:
        gtds = [{v: {"traj": cut(k, v, np.asarray(gtd[v]["traj"], np.float64).copy())} for v in range(N)} for k, gtd in enumerate(gtds)]
    return scns, replay.log_array(gtds, N, T + 1)


def _role_order(role_row, log_s, r):
    """A role's processing order: its vehicles by decreasing logged length (AutoregressivePolicy._open_session's rule on the
    ascending list of the role's vehicles)."""
    mine = np.nonzero(role_row == r)[0]
    lengths = np.array([int(log_s[v, :, 4].sum()) for v in mine])
    return mine[np.argsort(lengths)[::-1]].astype(np.int32) if len(mine) else np.zeros(0, np.int32)


def _new_engine(cfg, model, tilt=(0.0, 0.0, 0.0), **kw):
    pol = cfg.eval.policy
    return RolloutEngine(model.cfg, model.weights, DEV, max_ctx=64, seed=int(cfg.eval.seed), tilt=tilt,
                         temperature=pol.action_temperature, nucleus=pol.nucleus_sampling, top_p=pol.nucleus_threshold, model=model.hip, **kw)


def _oracle(cfg, model, scns, log, role, tilts, hsteps, noise=None):
    """R ordinary single-policy engines on the same scenes, stepped by the host (replay_utils.host_driven, as
    tests/test_gpu_replay.py::_host_driven steps one).  No code of the roles feature is used.
    noise(t) -> (noise_rtg [S*R,N,3,bins], noise_act [S*R,N,V]): explicit sampling noise per view row; engine r takes rows r::R."""
    T = cfg.nocturne.steps
    S, N = role.shape
    R = len(tilts)
    engs = []
    for r in range(R):
        mine = []
        for k, scn in enumerate(scns):
            s2 = copy.copy(scn)
            s2.eval_order = _role_order(role[k], log[k], r)
            mine.append(s2)
        e = _new_engine(cfg, model, tilt=tuple(tilts[r]), lanes=1)
        e.load_scenarios(mine, steps=T)
        engs.append(e)
    mutual = np.zeros(S, bool)

    def meet(t, engs):                                     # ego (role 0) and adversary (role 1) in each other's context
        if R != 2 or t < hsteps - 1:
            return
        members = [(e.n_groups.cpu().numpy(), e.grp_focal.cpu().numpy(), e.grp_ids.cpu().numpy().astype(np.uint64)) for e in engs]   # context slots
        for k in range(S):
            ego, adv = int(np.nonzero(role[k] == 0)[0][0]), int(np.nonzero(role[k] == 1)[0][0])
            sees = []
            for (ng, gf, gm), me, other in ((members[0], ego, adv), (members[1], adv, ego)):
                g = [i for i in range(ng[k]) if gf[k, i] == me]
                sees.append(bool(g) and bool((int(gm[k, g[0]]) >> other) & 1))
            mutual[k] |= all(sees)
    out = host_driven(engs, log, role, hsteps, cfg.nocturne.dt, cfg.dataset.waymo, noise=noise, after_policy_step=meet)
    out["mutual"] = mutual
    return out


def _first_difference(a, b, name):
    diff = np.argwhere(a != b)
    if len(diff) == 0:
        return f"{name} identical"
    tmin = diff[:, 3].min()
    s, r, v, _ = diff[diff[:, 3] == tmin][0]
    return f"{len(diff)} {name} differ; first at scene {s}, role {r}, vehicle {v}, step {tmin}: {a[s, r, v, tmin]} vs {b[s, r, v, tmin]}"


def _assert_roles_rollout_agrees(host, devr, what):
    assert np.array_equal(host["sampled_roles"], devr["sampled_roles"]), _first_difference(host["sampled_roles"], devr["sampled_roles"], "sampled tokens")
    assert np.array_equal(host["own_ctx"] >= 0, devr["own_ctx"] >= 0)
    assert_rollouts_agree(host, devr, what, ("tokens", "rtg_bins_roles", "existence", "coll"))


def _roles_cfg():
    cfg = cfg_of("loop")                                   # context length 8, 20 steps: the window slides
    cfg.nocturne.history_steps = 3
    cfg.eval.seed = 9
    return cfg


def _two_role_case(cfg, model, S=16, N=10):
    scns, log = _scenes(cfg, model, S, N, seed=31)
    role = -np.ones((S, N), np.int32)
    for k, scn in enumerate(scns):
        ego, adv = pick_ego_adversary(scn)
        role[k, ego], role[k, adv] = 0, 1
    return scns, log, role


def _three_role_case(cfg, model, S=16, N=10):
    """Role 0 drives vehicles 0 and 1 (1 leaves its log: at k % 5 == 0 during the K/V-cached steps, else after them), role 1 vehicle 2
    (leaves after row 11), role 2 vehicle 5 — except in scene 3, where role 2 has no vehicle."""
    scns, log = _scenes(cfg, model, S, N, seed=31, cut=_cut_logs)
    role = -np.ones((S, N), np.int32)
    role[:, [0, 1]] = 0
    role[:, 2] = 1
    role[:, 5] = 2
    role[3, 5] = -1
    return scns, log, role


def _rolled(cfg, model, scns, log, role, tilts, how="run", **kw):
    T, hs = cfg.nocturne.steps, cfg.nocturne.history_steps
    S = len(scns)
    eng = _new_engine(cfg, model, **kw)
    eng.load_scenarios(scns, steps=T)
    eng.set_log(log, role >= 0, hs)
    eng.set_roles(role, tilts)
    if how == "jobs":
        eng.run_jobs([(0, S // 3), (S // 3, S)])
    elif how == "step":
        for t in range(T):
            eng.step(t)
    elif callable(how):
        eng.run(noise_fn=how)
    else:
        eng.run()
    return eng, eng.results()


def _views_follow_the_scene(eng):
    R = eng.R
    vs = eng._pv.hist_states.cpu().numpy().reshape(eng.S, R, eng.N, eng.steps + 1, 8)
    vt = eng._pv.hist_tok.cpu().numpy().reshape(eng.S, R, eng.N, eng.steps)
    hs, ht = eng.hist_states.cpu().numpy(), eng.hist_tok.cpu().numpy()
    return all(np.array_equal(vs[:, r], hs) and np.array_equal(vt[:, r], ht) for r in range(R))


def test_run_with_two_roles_equals_single_policy_engines_stepped_by_the_host():
    cfg = _roles_cfg()
    model = _model(cfg)
    scns, log, role = _two_role_case(cfg, model)
    hs = cfg.nocturne.history_steps
    host = _oracle(cfg, model, scns, log, role, TILTS2, hs)
    eng, devr = _rolled(cfg, model, scns, log, role, TILTS2)
    assert devr["rtg_bins_roles"].shape == (16, 2, 10, 20, 3) and devr["sampled_roles"].shape == (16, 2, 10, 20)
    _assert_roles_rollout_agrees(host, devr, "16 scenes, ego + adversary")
    assert _views_follow_the_scene(eng)
    # the inputs exercise the feature: the two roles' RTGs differ, and ego and adversary meet in each other's contexts
    assert not np.array_equal(host["rtg_bins_roles"][:, 0], host["rtg_bins_roles"][:, 1])
    print(f"scenes with ego and adversary in each other's context: {int(host['mutual'].sum())} of 16")
    assert host["mutual"].any()
    ego = role == 0
    assert (host["sampled_roles"][:, 0][ego][:, hs - 1:] >= 0).all() and (host["sampled_roles"][:, 1][role == 1][:, hs - 1:] >= 0).all()
    # the merged token of the driving role
    drive = np.where(role[:, :, None] >= 0, np.take_along_axis(devr["sampled_roles"], np.clip(role, 0, 1)[:, None, :, None], 1)[:, 0], -1)
    assert np.array_equal(devr["sampled"], drive)
    assert np.array_equal(devr["tokens"][ego][:, hs - 1:], devr["sampled"][ego][:, hs - 1:])


def test_run_with_three_roles_and_vehicles_that_leave_equals_the_host_stepping():
    cfg = _roles_cfg()
    model = _model(cfg)
    scns, log, role = _three_role_case(cfg, model)
    hs = cfg.nocturne.history_steps
    host = _oracle(cfg, model, scns, log, role, TILTS3, hs)
    # the cuts do what they are there for: a role-driven vehicle leaves during the K/V-cached steps (t < 8), others after them
    ex = host["existence"]
    assert ex[0, 1, 6] == 1 and ex[0, 1, 7] == 0 and ex[1, 1, 7] == 1 and ex[1, 1, 8] == 0 and ex[0, 2, 11] == 1 and ex[0, 2, 12] == 0
    assert (role[3] == 2).sum() == 0 and (host["own_ctx"][3, 2] < 0).all() and (host["own_ctx"][2, 2] >= 0).any()
    eng, devr = _rolled(cfg, model, scns, log, role, TILTS3)
    _assert_roles_rollout_agrees(host, devr, "16 scenes, three roles, vehicles that leave")
    assert _views_follow_the_scene(eng)
    assert not np.array_equal(host["rtg_bins_roles"][:, 0], host["rtg_bins_roles"][:, 1])


def test_explicit_noise_is_taken_per_view_row():
    """run(noise_fn=...) / step(t, noise_rtg, noise_act) under roles: row s * R + r of the noise belongs to role r of scene s."""
    cfg = _roles_cfg()
    model = _model(cfg)
    scns, log, role = _two_role_case(cfg, model, S=4)
    hs, d = cfg.nocturne.history_steps, model.dims
    rs = np.random.RandomState(2)
    draws = [(dev(rs.exponential(size=(8, 10, 3, d.R)).astype(np.float32)), dev(rs.exponential(size=(8, 10, d.V)).astype(np.float32)))
             for _ in range(cfg.nocturne.steps)]
    noise = lambda t: draws[t]
    host = _oracle(cfg, model, scns, log, role, TILTS2, hs, noise=noise)
    eng, devr = _rolled(cfg, model, scns, log, role, TILTS2, how=noise, lanes=1)
    _assert_roles_rollout_agrees(host, devr, "4 scenes, explicit noise")
    _, drawn = _rolled(cfg, model, scns, log, role, TILTS2, lanes=1)
    assert not np.array_equal(drawn["sampled_roles"], devr["sampled_roles"])          # (the explicit noise was what decided the races)


KEYS = ("tokens", "rtg_bins", "states", "coll", "n_groups", "applied", "existence", "sampled", "rtg_bins_roles", "sampled_roles", "own_ctx",
        "n_groups_roles")


def test_roles_rollout_does_not_depend_on_the_schedule():
    cfg = _roles_cfg()
    model = _model(cfg)
    scns, log, role = _three_role_case(cfg, model)
    T, hs = cfg.nocturne.steps, cfg.nocturne.history_steps
    case = (cfg, model, scns, log, role, TILTS3)
    base_eng, base = _rolled(*case, lanes=1)
    assert set(KEYS) == set(base)
    runs = {"default lanes": _rolled(*case)[1], "three lanes": _rolled(*case, lanes=3)[1],
            "run_jobs over two ranges": _rolled(*case, how="jobs", lanes=2)[1], "no K/V cache": _rolled(*case, lanes=1, use_cache=False)[1],
            "step()": _rolled(*case, how="step", lanes=1)[1]}
    base_eng.reset()
    base_eng.run()
    runs["a second reset() + run()"] = base_eng.results()
    for name, r in runs.items():
        for k in KEYS:
            assert np.array_equal(base[k], r[k]), (name, k)
    # roles detached: the engine rolls what a fresh engine with the same log rolls
    base_eng.set_roles(None)
    base_eng.reset()
    plain = base_eng.run().results()
    assert "rtg_bins_roles" not in plain
    fresh = _new_engine(cfg, model, lanes=1)
    fresh.load_scenarios(scns, steps=T)
    fresh.set_log(log, role >= 0, hs)
    ref = fresh.run().results()
    assert set(plain) == set(ref)
    for k in ref:
        assert np.array_equal(plain[k], ref[k]), k
    assert not np.array_equal(ref["tokens"], base["tokens"])


def test_one_role_equals_set_log_alone():
    cfg = _roles_cfg()
    model = _model(cfg)
    S, N = 16, 10
    scns, log = _scenes(cfg, model, S, N, seed=31, cut=_cut_logs)
    T, hs = cfg.nocturne.steps, cfg.nocturne.history_steps
    ctrl = np.zeros((S, N), bool)
    ctrl[:, [0, 1, 2, 5, 7]] = True
    role = np.where(ctrl, 0, -1)
    tilt = (2.0, -5.0, 5.0)
    scns = [copy.copy(s) for s in scns]
    for k, s in enumerate(scns):                           # the controlled vehicles in the order a role's view processes them
        s.eval_order = _role_order(role[k], log[k], 0)
    plain = _new_engine(cfg, model, tilt=tilt)
    plain.load_scenarios(scns, steps=T)
    plain.set_log(log, ctrl, hs)
    order = plain.eval_order.cpu().numpy()
    a = plain.run().results()
    eng = _new_engine(cfg, model)
    eng.load_scenarios(scns, steps=T)
    eng.set_log(log, ctrl, hs)
    eng.set_roles(role, [tilt])
    # the scene is its own view: the engine's tensors, with the role's order and tilt rows beside (not in place of) the engine's own
    assert eng._pv.hist_rtg is eng.hist_rtg and eng._pv.act_now is eng.act_now and eng.tilt_scn is None
    assert np.array_equal(eng._pv.eval_order.cpu().numpy(), order) and np.array_equal(eng.eval_order.cpu().numpy(), order)
    b = eng.run().results()
    assert set(a) < set(b) and (a["sampled"][ctrl][:, hs - 1:] >= 0).any()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(b["rtg_bins_roles"][:, 0], a["rtg_bins"]) and np.array_equal(b["sampled_roles"][:, 0], a["sampled"])


@pytest.mark.parametrize("R", [1, 2])
def test_a_new_batch_after_roles_rolls_what_a_fresh_engine_rolls(R):
    """load_scenarios detaches the roles for good: after roles with their own tilt (R = 1: the scene is its own view) a LARGER batch
    without a log rolls under the engine's uniform tilt, bit for bit what a fresh engine rolls; so does a logged one."""
    cfg = _roles_cfg()
    model = _model(cfg)
    T, hs = cfg.nocturne.steps, cfg.nocturne.history_steps
    scns, log = _scenes(cfg, model, 12, 10, seed=31)
    small, small_log = scns[:4], log[:4]
    role = -np.ones((4, 10), np.int32)
    role[:, 0] = 0
    if R == 2:
        role[:, 2] = 1
    tilt = (2.0, -5.0, 5.0)
    eng = _new_engine(cfg, model, tilt=tilt, lanes=1)
    eng.load_scenarios(small, steps=T)
    eng.set_log(small_log, role >= 0, hs)
    eng.set_roles(role, TILTS2[:R])
    eng.run().results()
    own_order = eng.eval_order
    eng.load_scenarios(scns, steps=T)                      # 12 scenes after 4
    assert eng.role is None and eng.R == 1 and eng._pv is eng and eng.tilt_scn is None and eng.eval_order is not own_order
    a = eng.run().results()
    fresh = _new_engine(cfg, model, tilt=tilt, lanes=1)
    fresh.load_scenarios(scns, steps=T)
    b = fresh.run().results()
    assert set(a) == set(b) and "applied" not in a
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    # the uniform tilt is what decided: the roles' tilt gives other RTGs on these scenes
    other = _new_engine(cfg, model, tilt=tuple(TILTS2[0]), lanes=1)
    other.load_scenarios(scns, steps=T)
    assert not np.array_equal(other.run().results()["rtg_bins"], b["rtg_bins"])
    # ... and a log attached to the new batch rolls as on the fresh engine, roles gone; set_roles(None) after R = 1 leaves the engine's own
    # order and tilt as they were
    ctrl = np.zeros((12, 10), bool)
    ctrl[:, [0, 2, 5]] = True
    for e in (eng, fresh):
        e.reset()
        e.set_log(log, ctrl, hs)
    eng.set_roles(np.where(ctrl, 0, -1), [TILTS2[0]])
    eng.set_roles(None)
    assert eng.tilt_scn is None and eng._pv is eng
    a, b = eng.run().results(), fresh.run().results()
    for k in b:
        assert np.array_equal(a[k], b[k]), k


def test_set_roles_refusals():
    cfg = _roles_cfg()
    model = _model(cfg)
    scns, log, role = _two_role_case(cfg, model, S=2)
    T, hs = cfg.nocturne.steps, cfg.nocturne.history_steps
    eng = _new_engine(cfg, model)
    eng.load_scenarios(scns, steps=T)
    with pytest.raises(RuntimeError, match="set_log"):
        eng.set_roles(role, TILTS2)                        # roles without a log
    eng.set_log(log, role >= 0, hs)
    with pytest.raises(ValueError, match="role index 1"):
        eng.set_roles(role, TILTS2[:1])                    # a role index >= R
    with pytest.raises(ValueError, match="at most 4"):
        eng.set_roles(role, np.zeros((5, 3)))
    eng.set_roles(role, TILTS2)
    with pytest.raises(ValueError, match="per view row"):
        eng.step(0, noise_rtg=torch.zeros(2, 10, 3, 4, device=DEV))
    assert eng.R == 2 and eng.set_log(None, None).role is None and eng.R == 1
    eng.set_log(log, role >= 0, hs).set_roles(role, np.zeros((4, 3)))
    assert eng.R == 4
    eng.load_scenarios(scns, steps=T)
    assert eng.role is None and eng._pv is eng
    # the Decision-Transformer reward ledger keeps the step-by-step route: set_log refuses it, and so does set_roles
    import ctrlsim_amd.spec as spec
    import ctrlsim_amd.weights as weights
    cfg3 = cfg_of("loop", variant="decision_transformer")
    dt = RolloutEngine(cfg3, weights.generate(spec.Dims(cfg3), 0), DEV, max_ctx=32, seed=1)
    dt.load_scenarios(scns, steps=T)
    with pytest.raises(AssertionError, match="ledger"):
        dt.set_log(log, role >= 0, hs)
    dt.device_ledger = False                               # (the plugin surface's setting: the host feeds the RTG rows — per scene too)
    dt.set_log(log, role >= 0, hs)
    with pytest.raises(RuntimeError, match="Decision-Transformer"):
        dt.set_roles(role, TILTS2)
    assert dt.role is None and dt._pv is dt


# ---------------------------------------------------------------------------------------------------------------- (e) evaluator
def _role_policy(cfg, model, pol, key_dict, name=None):
    tilt_dict = {"tilt": True, "goal_tilt": pol.goal_tilt, "veh_veh_tilt": pol.veh_veh_tilt, "veh_edge_tilt": pol.veh_edge_tilt}
    return AutoregressivePolicy(cfg=cfg, model_path="", model=model, use_rtg=pol.use_rtg, predict_rtgs=pol.predict_rtgs,
                                discretize_rtgs=pol.discretize_rtgs, real_time_rewards=pol.real_time_rewards,
                                privileged_return=pol.privileged_return, max_return=pol.max_return, min_return=pol.min_return,
                                key_dict=key_dict, tilt_dict=tilt_dict, name=name or pol.model,
                                action_temperature=pol.action_temperature, nucleus_sampling=pol.nucleus_sampling,
                                nucleus_threshold=pol.nucleus_threshold)


METRIC_KEYS = ["ego_goal", "ego_prog", "ego_cr", "ego_cr_w_adv", "ego_or", "ego_fde", "ego_ade", "ego_accel", "ego_jerk",
               "ego_steer_rate", "adv_coll_speed", "adv_lin_jsd", "adv_ang_jsd", "adv_acc_jsd", "nearest_dist_jsd"]


@pytest.mark.parametrize("tag", ["a", "b"])
def test_planner_vs_adversary_device_route_matches_reference_fixture(tag):
    """The assertions of tests/test_gpu_facade.py::test_planner_vs_adversary_matches_reference_fixture with
    cfg.eval_planner_adversary.device_replay on."""
    g = golden("planner_adversary")
    rc = g[f"{tag}_recipe"]
    cfg = cfg_of("loop")
    cfg.eval.seed = int(rc[5])
    pa = cfg.eval_planner_adversary
    pa.seed, pa.history_steps = int(rc[5]), int(rc[6])
    pa["synthetic"] = dict(num_scenarios=int(rc[1]) + 1, n_agents=int(rc[2]), n_polylines=int(rc[3]), seed=int(rc[0]),
                           extent=float(rc[4]))
    pa["device_replay"] = True
    model = CtRLSim(cfg, seed=0, device=DEV)
    planner = _role_policy(cfg, model, pa.planner, PLANNER_KEYS)
    adversary = _role_policy(cfg, model, pa.adversary, ADVERSARY_KEYS)
    ev = PlannerAdversaryEvaluator(cfg, planner, adversary)
    m, lines = ev.evaluate_planner_adversary()
    assert ev.device_replay_scenes == int(rc[1]) + 1       # the engine route ran
    assert list(m) == METRIC_KEYS
    assert all(np.isfinite(v) for k, v in m.items() if k != "adv_coll_speed") and len(lines) == 15
    vdd = ev.last_vehicle_data_dict                        # the last scenario evaluated = the fixture's
    n, steps = int(rc[2]), 20
    ego, adv = [int(v) for v in g[f"{tag}_ego_adv"]]
    assert (ev.ego_vehicle, ev.adversary_vehicle) == (ego, adv)
    acts = np.array([[vdd[v]["acceleration"][t], vdd[v]["steering"][t]] for v in range(n) for t in range(steps)]).reshape(n, steps, 2)
    ref = g[f"{tag}_actions"]
    hs = int(rc[6])
    for v in (ego, adv):                                   # policy-driven: the same tokens -> the same bin centres
        np.testing.assert_allclose(acts[v, hs - 1:], ref[v, hs - 1:], atol=1e-9, rtol=0)
    np.testing.assert_allclose(acts, ref, atol=2e-3, rtol=0)   # replayed: inverse bicycle model of float32 states / dt
    st = g[f"{tag}_states"]
    xs = np.array([[vdd[v]["position"][t]["x"] for t in range(steps + 1)] for v in range(n)])
    ys = np.array([[vdd[v]["position"][t]["y"] for t in range(steps + 1)] for v in range(n)])
    hd = np.array([[vdd[v]["heading"][t] for t in range(steps + 1)] for v in range(n)])
    np.testing.assert_allclose(xs, st[:, :, 0], atol=1e-4, rtol=0)
    np.testing.assert_allclose(ys, st[:, :, 1], atol=1e-4, rtol=0)
    np.testing.assert_allclose(hd, st[:, :, 4], atol=1e-4, rtol=0)
    cv = np.array([[vdd[v]["reward"][t][6] for t in range(steps + 1)] for v in range(n)])
    assert np.array_equal(cv, g[f"{tag}_coll"][..., 0].astype(float))
    for role, r in (("planner", 0), ("adversary", 1)):
        rt = np.array([[vdd[v][f"{role}_rtgs"][t] for t in range(steps)] for v in range(n)])
        np.testing.assert_allclose(rt, g[f"{tag}_rtg_cont"][r], atol=1e-9, rtol=0)


def _pa_cfg(flag):
    cfg = cfg_of("loop")
    cfg.eval.seed = 4
    pa = cfg.eval_planner_adversary
    pa.seed, pa.history_steps = 4, 3
    pa["synthetic"] = dict(num_scenarios=6, n_agents=8, n_polylines=12, seed=19, extent=30.0)
    pa["device_replay"] = flag
    return cfg


def _shifted_adv_traj(scn, gt_data_dict, ego, adv):
    """The adversary's log shifted 1 m sideways: rows x, y, vx, vy, yaw."""
    tr = np.asarray(gt_data_dict[adv]["traj"], np.float64)
    h, v = tr[:, 2], tr[:, 3]
    return np.stack([tr[:, 0] - np.sin(h), tr[:, 1] + np.cos(h), v * np.cos(h), v * np.sin(h), h], 1)


def _both_routes(cat=False, other_model=False):
    out = []
    for flag in (False, True):
        cfg = _pa_cfg(flag)
        pa = cfg.eval_planner_adversary
        model = CtRLSim(cfg, seed=0, device=DEV)
        planner = _role_policy(cfg, model, pa.planner, PLANNER_KEYS)
        adv_model = CtRLSim(cfg, seed=0, device=DEV) if other_model else model
        adversary = _role_policy(cfg, adv_model, pa.adversary, ADVERSARY_KEYS, name="cat" if cat else None)
        ev = PlannerAdversaryEvaluator(cfg, planner, adversary)
        m, lines = ev.evaluate_planner_adversary(adv_traj_fn=_shifted_adv_traj if cat else None)
        out.append((m, ev.last_vehicle_data_dict, ev))
    return out


def _assert_routes_agree(off, on, what):
    (m0, v0, ev0), (m1, v1, ev1) = off, on
    assert not hasattr(ev0, "device_replay_scenes") and ev1.device_replay_scenes == 6
    assert list(m0) == METRIC_KEYS and list(m1) == METRIC_KEYS
    for k in METRIC_KEYS:
        print(f"  {what} {k}: stepwise {m0[k]!r}, device {m1[k]!r}")
    for k in METRIC_KEYS:
        if np.isnan(m0[k]) or np.isnan(m1[k]):
            assert np.isnan(m0[k]) and np.isnan(m1[k]), k
        else:
            assert abs(m0[k] - m1[k]) <= 1e-9 * abs(m0[k]), (k, m0[k], m1[k])
    assert (ev0.ego_vehicle, ev0.adversary_vehicle) == (ev1.ego_vehicle, ev1.adversary_vehicle)
    assert set(v0) == set(v1)
    for v in v0:                                           # the last scene's dict: same schema, same list lengths
        assert set(v0[v]) == set(v1[v]), (v, set(v0[v]) ^ set(v1[v]))
        for key in v0[v]:
            assert isinstance(v1[v][key], list) == isinstance(v0[v][key], list) and isinstance(v1[v][key], dict) == isinstance(v0[v][key], dict), (v, key)
            if isinstance(v0[v][key], list):
                assert len(v1[v][key]) == len(v0[v][key]), (v, key, len(v1[v][key]), len(v0[v][key]))


def test_planner_adversary_device_route_equals_the_stepwise_route():
    off, on = _both_routes()
    _assert_routes_agree(off, on, "policies")
    v0, v1 = off[1], on[1]
    ego, adv = on[2].ego_vehicle, on[2].adversary_vehicle
    for v in v0:                                           # tokens of both policies, existence and both RTG histories: identical
        for key in ("existence", "timestep", "gt_speed", "gt_acceleration"):
            assert np.array_equal(np.asarray(v0[v][key], np.float64), np.asarray(v1[v][key], np.float64)), (v, key)
        assert np.array_equal(np.array(v0[v]["planner_rtgs"]), np.array(v1[v]["planner_rtgs"])), v
        assert np.array_equal(np.array(v0[v]["adversary_rtgs"]), np.array(v1[v]["adversary_rtgs"])), v
    for v in (ego, adv):
        assert np.array_equal(np.asarray(v0[v]["acceleration"][2:], np.float64), np.asarray(v1[v]["acceleration"][2:], np.float64))


def test_planner_adversary_device_route_with_a_fixed_adversary_trajectory():
    off, on = _both_routes(cat=True)
    _assert_routes_agree(off, on, "cat")
    v0, v1 = off[1], on[1]
    adv = on[2].adversary_vehicle
    assert all(len(v1[v]["adversary_rtgs"]) == 0 for v in v1)
    # the adversary follows the shifted trajectory, not its log
    p, g = v1[adv]["position"][10], v1[adv]["gt_position"][10]
    assert 0.5 < np.hypot(p["x"] - g["x"], p["y"] - g["y"]) < 2.0
    np.testing.assert_allclose([q["x"] for q in v1[adv]["position"]], [q["x"] for q in v0[adv]["position"]], rtol=0, atol=1e-4)


def test_policies_on_different_model_objects_keep_the_stepwise_route():
    cfg = _pa_cfg(True)
    pa = cfg.eval_planner_adversary
    pa["synthetic"]["num_scenarios"] = 1
    model, model2 = CtRLSim(cfg, seed=0, device=DEV), CtRLSim(cfg, seed=0, device=DEV)
    planner = _role_policy(cfg, model, pa.planner, PLANNER_KEYS)
    adversary = _role_policy(cfg, model2, pa.adversary, ADVERSARY_KEYS)
    ev = PlannerAdversaryEvaluator(cfg, planner, adversary)
    assert not ev._device_route_applies()
    same = PlannerAdversaryEvaluator(cfg, planner, _role_policy(cfg, model, pa.adversary, ADVERSARY_KEYS))
    assert same._device_route_applies()
    m, _ = ev.evaluate_planner_adversary()
    assert not hasattr(ev, "device_replay_scenes") and planner._session is not None      # the stepwise loop drove the policy objects
    assert list(m) == METRIC_KEYS
