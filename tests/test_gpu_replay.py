"""GPU: device-side log replay — the kernels of csrc/replay.hip through the C ABI against their host form (ctrlsim_amd/replay.py),
RolloutEngine.run() with a log attached against the host-driven stepping of PolicyEvaluator._roll_batch, scheduling invariance of a
logged batch, and the evaluator's cfg.eval.device_replay route."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import cfg_of, golden  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402
from replay_utils import ULP, _ulps, _disc6, _cut_logs, engine_of as _engine, host_driven, assert_rollouts_agree  # noqa: E402
from ctrlsim_amd import _lib, spec, replay  # noqa: E402
from ctrlsim_amd.kinematics import bicycle_backward  # noqa: E402  (the fixture test's host check of its narrowed rows)
from ctrlsim_amd.metrics import MetricAccumulators  # noqa: E402
from ctrlsim_amd.models import CtRLSim  # noqa: E402
from ctrlsim_amd.policies import AutoregressivePolicy  # noqa: E402
from ctrlsim_amd.evaluators import PolicyEvaluator  # noqa: E402


def _device_step(log, ctrl, exist_prev, t, T1, hsteps, heading32, speed32, toks, dt, w):
    """One latch + actions call pair through the C ABI on [S, N] vehicles -> dict of what the kernels wrote."""
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    S, N = ctrl.shape
    Tmax = T1 - 1
    log_d = dev(log)
    ctrl_d = dev(ctrl.astype(np.uint8))
    eh = np.zeros((S, N, T1))
    if t > 0:
        eh[:, :, t - 1] = exist_prev
    eh_d = dev(eh)
    hs = np.zeros((S, N, T1, 8), np.float32)
    hs[:, :, t, 4] = heading32
    hs[:, :, t, 7] = 1.0                                   # what the simulator wrote (its `exists` flag): the latch overwrites it
    hs_d = dev(hs)
    phys = np.zeros((S, N, 20), np.float32)
    phys[:, :, 16] = speed32
    phys_d = dev(phys)
    sp_d = torch.zeros(S, N, T1, device=DEV)
    tok_d = dev(toks.astype(np.int32))
    act_d = torch.full((S, N, 2), 7.0, dtype=torch.float64, device=DEV)
    ex_d = torch.full((S, N), 9, dtype=torch.uint8, device=DEV)
    ht_d = torch.full((S, N, Tmax), -5, dtype=torch.int32, device=DEV)
    _lib.check(lib.ctrlsim_replay_latch(S, N, t, T1, p(log_d), p(phys_d), p(eh_d), p(hs_d), p(sp_d), st), "replay_latch")
    _lib.check(lib.ctrlsim_replay_actions(S, N, t, T1, Tmax, hsteps, dt, p(log_d), p(ctrl_d), p(eh_d), p(hs_d), p(phys_d), p(tok_d),
                                          _disc6(w), p(act_d), p(ex_d), p(ht_d), st), "replay_actions")
    torch.cuda.synchronize()
    ht = ht_d.cpu().numpy()
    assert (np.delete(ht, t, axis=2) == -5).all()          # only column t of the action history is written
    return dict(exist=eh_d.cpu().numpy()[:, :, t], exist_col=hs_d.cpu().numpy()[:, :, t, 7], speed=sp_d.cpu().numpy()[:, :, t],
                act=act_d.cpu().numpy(), alive=ex_d.cpu().numpy(), tok=ht[:, :, t], hs=hs_d.cpu().numpy(), hs_in=hs)


def _compare_step(out, log, ctrl, exist_prev, t, hsteps, heading32, speed32, toks, dt, w, what):
    ex = replay.latch(log, t, exist_prev)
    act, alive, tok = replay.actions(log, ctrl, ex, t, hsteps, heading32, speed32, toks, dt, w)
    assert np.array_equal(out["exist"], ex), what
    assert np.array_equal(out["exist_col"], ex.astype(np.float32)), what
    assert np.array_equal(out["speed"], speed32), what
    other = np.ones(8, bool); other[7] = False             # the latch touches the existence column only
    assert np.array_equal(out["hs"][..., other], out["hs_in"][..., other]), what
    assert np.array_equal(out["alive"], alive.astype(np.uint8)), what
    assert np.array_equal(out["act"][..., 0].view(np.int64), act[..., 0].view(np.int64)), f"{what}: accel is not bit-equal"
    u = _ulps(out["act"][..., 1], act[..., 1])
    print(f"{what}: {act[..., 0].size} rows, largest steer distance {u.max():.1f} ulp ({int((u > 0).sum())} rows differ)")
    assert u.max() <= ULP, (what, u.max())
    # tokens: equal wherever the scaled pair lies more than 1e-9 from a half-integer — and wherever device and host hold the same
    # bits of the pair anyway (the pair (0, 0) of a parked vehicle / an unanswered token lies EXACTLY on a half-integer of both
    # discretisations: round-half-even of identical bits is identical)
    margin = replay.token_margin(act, w).min(-1)
    same_bits = (out["act"].view(np.int64) == act.view(np.int64)).all(-1)
    dropped = (margin <= 1e-9) & ~same_bits
    assert dropped.mean() <= 0.01, (what, dropped.mean())
    assert np.array_equal(out["tok"][~dropped], tok[~dropped]), what
    return act, alive, tok, margin


def _random_rows(S, N, T1, t, seed):
    """[S, N] vehicles at step t of a T1-row rollout: random logs around the vehicles' current states, the edge rows in scene 0."""
    rs = np.random.RandomState(seed)
    log = np.zeros((S, N, T1 + 1, 6))
    log[..., 0] = rs.uniform(-100, 100, (S, N, T1 + 1))
    log[..., 1] = rs.uniform(-100, 100, (S, N, T1 + 1))
    log[..., 2] = rs.uniform(-np.pi, np.pi, (S, N, 1)) + rs.uniform(-0.15, 0.15, (S, N, T1 + 1))
    log[..., 3] = rs.uniform(0.5, 25.0, (S, N, 1)) + rs.uniform(-0.4, 0.4, (S, N, T1 + 1))
    log[..., 4] = (rs.uniform(size=(S, N, T1 + 1)) < 0.93).astype(np.float64)
    log[..., 5] = rs.uniform(3.0, 7.0, (S, N, 1))
    log[..., T1, :] = np.where(rs.uniform(size=(S, N, 1)) < 0.1, 0.0, log[..., T1, :])
    ctrl = rs.uniform(size=(S, N)) < 0.5
    exist_prev = (rs.uniform(size=(S, N)) < 0.9).astype(np.float64)
    heading = (log[:, :, t, 2] + rs.uniform(-0.02, 0.02, (S, N))).astype(np.float32)
    speed = (log[:, :, t, 3] + rs.uniform(-0.3, 0.3, (S, N))).astype(np.float32)
    toks = rs.randint(0, 1000, (S, N)).astype(np.int32)
    toks[rs.uniform(size=(S, N)) < 0.05] = -1
    # ---- edge rows (scene 0): uncontrolled, alive, rows t and t + 1 logged unless said otherwise
    e = np.arange(12)
    ctrl[0, e] = False
    exist_prev[0, e] = 1.0
    log[0, e, t, 4] = 1.0
    log[0, e, t + 1, 4] = 1.0
    log[0, e, t + 1, 5] = 4.0
    heading[0, e] = 0.0
    log[0, e, t + 1, 2] = 0.01
    speed[0, e] = 8.0
    log[0, e, t + 1, 3] = 8.0
    # 0: speeds summing to exactly -1e-10 (denominator 0 -> C = inf -> NaN -> 0); 1: summing to about 0 (huge C)
    speed[0, 0], log[0, 0, t + 1, 3] = 0.0, -1e-10
    speed[0, 1], log[0, 1, t + 1, 3] = np.float32(1e-7), -1e-7
    # 2: |C| > 2 (the square root of a negative number); 3: |C| = 2 up to rounding
    speed[0, 2], log[0, 2, t + 1, 3], log[0, 2, t + 1, 2] = 0.5, 0.5, 1.0
    speed[0, 3], log[0, 3, t + 1, 3], log[0, 3, t + 1, 2] = 10.0, 10.0, 0.5
    # 4, 5: heading wraps across +-pi, both ways; 6: a difference of exactly 0
    heading[0, 4], log[0, 4, t + 1, 2] = np.float32(3.1), -3.1
    heading[0, 5], log[0, 5, t + 1, 2] = np.float32(-3.1), 3.1
    heading[0, 6], log[0, 6, t + 1, 2] = 0.25, 0.25
    # 7, 8: steer beyond +-0.7
    log[0, 7, t + 1, 2], log[0, 8, t + 1, 2] = 0.3, -0.3
    # 9: the next log row is missing; 10: token -1 on a controlled vehicle; 11: a controlled vehicle that stopped existing (parked)
    log[0, 9, t + 1, 4] = 0.0
    ctrl[0, 10], toks[0, 10] = True, -1
    ctrl[0, 11], exist_prev[0, 11] = True, 0.0
    return log, ctrl, exist_prev, heading, speed, toks


@pytest.mark.parametrize("t,hsteps", [(1, 2), (0, 1), (2, 4)])
def test_replay_kernels_match_the_host_form(t, hsteps):
    w = cfg_of("loop").dataset.waymo
    S, N, T1 = 64, 64, 4                                   # 4096 rows
    log, ctrl, exist_prev, heading, speed, toks = _random_rows(S, N, T1, t, seed=11 + t)
    out = _device_step(log, ctrl, exist_prev, t, T1, hsteps, heading, speed, toks, 0.1, w)
    act, alive, tok, margin = _compare_step(out, log, ctrl, exist_prev, t, hsteps, heading, speed, toks, 0.1, w, f"random rows t={t}")
    # the chosen inputs drop no row from the token comparison: the only components within 1e-9 of a half-integer are exact zeros
    # (accel = 0 and steer = 0 ARE bin edges: 9.5 of 19, 24.5 of 49) — written as literals or atan(0) on both sides, hence compared as
    # identical bits in _compare_step
    # (the hand-made edge rows are not random inputs: row 0's accel of -1e-9 sits 9.5e-10 from a bin edge on purpose of its speeds)
    m2 = replay.token_margin(act, w)
    m2[0, :12] = 0.5
    assert not ((m2 <= 1e-9) & (act != 0)).any()
    # the edge rows did what they were made for
    ex = replay.latch(log, t, exist_prev)
    by_policy = t >= hsteps - 1
    assert act[0, 0, 1] == 0.0 and act[0, 2, 1] == 0.0 and alive[0, 0] and alive[0, 2]
    assert abs(act[0, 3, 1]) == 0.7 and act[0, 7, 1] == 0.7 and act[0, 8, 1] == -0.7
    assert 0 < act[0, 4, 1] < 0.7 and -0.7 < act[0, 5, 1] < 0 and act[0, 6, 1] == 0.0
    assert not alive[0, 9] and (act[0, 9] == 0).all()
    if by_policy:
        assert alive[0, 10] == (ex[0, 10] != 0) and (act[0, 10] == 0).all() and tok[0, 10] == spec.ZERO_ACTION_TOKEN
    if by_policy and t > 0:
        assert not alive[0, 11] and (act[0, 11] == 0).all()
    # all three branches are populated
    bp = ctrl & by_policy
    assert (not by_policy or (bp & (ex != 0) & (toks >= 0)).sum() > 100) and (~bp & alive).sum() > 500 and (~alive).sum() > 100


def test_replay_kernel_reproduces_the_reference_inverse_bicycle_fixture():
    """tests/golden/bicycle_backward.npz (the reference's own BicycleModel.backward) through the kernel, to 1e-12 of the fixture.
    The kernel takes the CURRENT heading and speed from the float32 history row and body state, the fixture's are float64 values no
    float32 holds.  Each fixture row is therefore run as the row with the float32-narrowed current state that asks the model the same
    question: next heading and next speed shifted by the narrowing error (the model works with their differences from the current
    ones) and the length scaled by the ratio of the speed sums (its only other use of the speeds is 2 L w / (v' + v + 1e-10)).  On the
    host these rows reproduce the fixture to 2e-14 (asserted below), so 1e-12 on the device still is the fixture's tolerance."""
    g = golden("bicycle_backward")
    w = cfg_of("loop").dataset.waymo
    nxt, prev = g["nxt"], g["prev"]
    n = len(nxt)
    h32, s32 = prev[:, 2].astype(np.float32), prev[:, 3].astype(np.float32)
    h64, s64 = h32.astype(np.float64), s32.astype(np.float64)
    n2 = nxt.copy()
    n2[:, 2] = nxt[:, 2] + (h64 - prev[:, 2])
    n2[:, 3] = nxt[:, 3] + (s64 - prev[:, 3])
    n2[:, 4] = nxt[:, 4] * ((n2[:, 3] + s64 + 1e-10) / (nxt[:, 3] + prev[:, 3] + 1e-10))
    a_h, s_h = bicycle_backward(n2, np.stack([prev[:, 0], prev[:, 1], h64, s64], 1), 0.1)
    np.testing.assert_allclose(np.stack([a_h, s_h], 1), g["accel_steer"], rtol=0, atol=1e-13)
    log = np.zeros((1, n, 3, 6))
    log[0, :, 0, 4] = 1.0
    log[0, :, 1, :4] = n2[:, :4]
    log[0, :, 1, 4] = 1.0
    log[0, :, 1, 5] = n2[:, 4]
    ctrl = np.zeros((1, n), bool)
    toks = np.full((1, n), -1, np.int32)
    out = _device_step(log, ctrl, None, 0, 2, 1, h32[None], s32[None], toks, 0.1, w)
    _compare_step(out, log, ctrl, None, 0, 1, h32[None], s32[None], toks, 0.1, w, "fixture rows")
    err = np.abs(out["act"][0] - g["accel_steer"])
    print(f"fixture: {n} rows, largest distance from the fixture: accel {err[:, 0].max():.3g}, steer {err[:, 1].max():.3g}")
    np.testing.assert_allclose(out["act"][0], g["accel_steer"], rtol=0, atol=1e-12)
    assert out["alive"].all()


# ---------------------------------------------------------------------------------------------------------------- engine
def _policy(cfg, tilts=(5.0, -10.0, 10.0)):
    model = CtRLSim(cfg, seed=0, device=DEV)
    pol = cfg.eval.policy
    policy = AutoregressivePolicy(cfg=cfg, model_path="", model=model, use_rtg=pol.use_rtg, predict_rtgs=pol.predict_rtgs,
                                  discretize_rtgs=pol.discretize_rtgs, real_time_rewards=pol.real_time_rewards,
                                  privileged_return=pol.privileged_return, max_return=pol.max_return, min_return=pol.min_return,
                                  key_dict={"next_acceleration": "next_acceleration", "next_steering": "next_steering", "rtgs": "rtgs"},
                                  tilt_dict={"tilt": True, "goal_tilt": tilts[0], "veh_veh_tilt": tilts[1], "veh_edge_tilt": tilts[2]},
                                  name=pol.model, action_temperature=pol.action_temperature, nucleus_sampling=pol.nucleus_sampling,
                                  nucleus_threshold=pol.nucleus_threshold)
    return model, policy


def _cfg64(device_replay=None):
    """The scene set of test_batched_evaluator_route_equals_the_per_scenario_route_on_64_scenes (tests/test_gpu_facade.py)."""
    cfg = cfg_of("loop")
    cfg.nocturne.history_steps = 4
    cfg.eval.seed = 5
    cfg.eval["synthetic"] = dict(num_scenarios=64, n_agents=12, n_polylines=14, seed=23, extent=45.0)
    cfg.eval.num_files_to_evaluate = 64 * cfg.eval.partitions
    cfg.eval["batched"] = True
    if device_replay is not None:
        cfg.eval["device_replay"] = device_replay
    return cfg


def _logged_batch(ev, limit=None, cut=None):
    """The batch PolicyEvaluator._evaluate_policy_batched / _roll_batch build (ev._prepare_batch): scenes (goals moved as
    initialize_goal_dict does, eval_order by decreasing log length), gt [S,N,T1+1,6], controlled [S,N], goal dicts, the drawn vehicles.
    cut(k, v, traj) -> traj: shorten / blank a vehicle's log (tests of vehicles that leave)."""
    ev.reset()
    items = []
    for scn, gtd, moving, pre in ev._scenes(ev.synthetic):
        if limit is not None and len(items) == limit:
            break
        to_eval = ev._choose_vehicles(scn, gtd, moving)
        if to_eval:
            items.append((scn, gtd, list(to_eval)))
    if cut is not None:
        for k, (scn, gtd, to_eval) in enumerate(items):
            for v in range(scn.N):
                gtd[v]["traj"] = cut(k, v, np.asarray(gtd[v]["traj"], np.float64).copy())
    b = ev._prepare_batch(items)
    return b.scns, b.gt, b.ctrl, b.goal_dicts, items


def _host_driven(eng, gt, ctrl, hsteps, dt, w):
    """What PolicyEvaluator._roll_batch does per step (replay_utils.host_driven on one engine): policy_step, read-backs, NumPy float64
    actions, uploads, sim_step."""
    out = host_driven([eng], gt, np.where(ctrl, 0, -1), hsteps, dt, w)
    out["sampled"], out["rtg_bins"] = out["sampled_roles"][:, 0], out["rtg_bins_roles"][:, 0]
    return out


def _report_token_difference(a, b, ctrl, hsteps):
    """First sampled token that differs between two rollouts: where, and whether it is a policy-driven one (the margin of the sampling
    race itself stays on the device: rerun the step with explicit noise, engine.step(t, noise_rtg, noise_act), to read it)."""
    diff = np.argwhere(a["sampled"] != b["sampled"])
    if len(diff) == 0:
        return "sampled tokens identical"
    t = diff[:, 2].min()
    s, v, _ = diff[diff[:, 2] == t][0]
    return (f"{len(diff)} sampled tokens differ; first at scene {s}, vehicle {v}, step {t}: {a['sampled'][s, v, t]} vs {b['sampled'][s, v, t]} "
            f"(controlled {bool(ctrl[s, v])}, by policy {bool(ctrl[s, v] and t >= hsteps - 1)}); RTG bins there "
            f"{a['rtg_bins'][s, v, t]} vs {b['rtg_bins'][s, v, t]}; largest state difference before that step "
            f"{np.abs(a['states'][:, :, :t + 1, :7] - b['states'][:, :, :t + 1, :7]).max():.3g}")


def _assert_rollouts_agree(host, devr, ctrl, hsteps, what):
    """The agreement the host-driven and the device-side replay owe each other."""
    assert np.array_equal(host["sampled"], devr["sampled"]), _report_token_difference(host, devr, ctrl, hsteps)
    assert_rollouts_agree(host, devr, what, ("tokens", "rtg_bins", "existence", "coll"))


def test_engine_run_with_a_log_equals_the_host_driven_stepping_on_64_scenes():
    cfg = _cfg64()
    model, policy = _policy(cfg)
    ev = PolicyEvaluator(cfg, policy)
    scns, gt, ctrl, goal_dicts, items = _logged_batch(ev)
    assert ctrl.shape == (64, 12) and (ctrl.sum(1) == 8).all()
    w, T, hs = cfg.dataset.waymo, cfg.nocturne.steps, cfg.nocturne.history_steps
    e0 = _engine(ev, lanes=1)
    e0.load_scenarios(scns, steps=T)
    host = _host_driven(e0, gt, ctrl, hs, cfg.nocturne.dt, w)
    e1 = _engine(ev)
    e1.load_scenarios(scns, steps=T)
    e1.set_log(gt, ctrl, hs)
    devr = e1.run().results()
    assert devr["applied"].shape == (64, 12, T, 2) and devr["existence"].shape == (64, 12, T + 1)
    assert (host["sampled"][ctrl][:, hs - 1:] >= 0).any() and (host["applied"][~ctrl][..., 1] != 0).any()
    _assert_rollouts_agree(host, devr, ctrl, hs, "64 scenes x 12 vehicles")


def _small_logged(cfg_kw=None):
    cfg = cfg_of("loop")
    cfg.nocturne.history_steps = 3
    cfg.eval.seed = 9
    cfg.eval.multi_agent_eval_threshold = 6
    cfg.eval["synthetic"] = dict(num_scenarios=24, n_agents=10, n_polylines=14, seed=31, extent=40.0)
    cfg.eval.num_files_to_evaluate = 24 * cfg.eval.partitions
    model, policy = _policy(cfg, tilts=(2.0, -5.0, 5.0))
    ev = PolicyEvaluator(cfg, policy)
    scns, gt, ctrl, goal_dicts, items = _logged_batch(ev, cut=_cut_logs)
    return cfg, ev, scns, gt, ctrl


KEYS = ("tokens", "rtg_bins", "states", "coll", "applied", "existence", "sampled")


def test_logged_batch_with_vehicles_that_leave_equals_the_host_driven_stepping():
    """The 64-scene set has no vehicle that leaves its log; this one has (controlled and uncontrolled, during the K/V-cached steps and
    after them, dead at t = 0, a flag that comes back): the same agreement."""
    cfg, ev, scns, gt, ctrl = _small_logged()
    w, T, hs = cfg.dataset.waymo, cfg.nocturne.steps, cfg.nocturne.history_steps
    assert ctrl[:, 1].any() and (~ctrl[:, 1]).any() and ctrl.sum(1).max() == 6
    e0 = _engine(ev, lanes=1)
    e0.load_scenarios(scns, steps=T)
    host = _host_driven(e0, gt, ctrl, hs, cfg.nocturne.dt, w)
    assert (host["existence"][:, 1, -1] == 0).all() and (host["existence"][:, 3] == 0).all() and (host["existence"][:, 4, 10:] == 0).all()
    assert (host["states"][:, 1, -1, 0] < -9e5).all()       # parked by the simulator
    e1 = _engine(ev)
    e1.load_scenarios(scns, steps=T)
    e1.set_log(gt, ctrl, hs)
    devr = e1.run().results()
    _assert_rollouts_agree(host, devr, ctrl, hs, "24 scenes with vehicles that leave")


def test_logged_rollout_does_not_depend_on_the_schedule():
    cfg, ev, scns, gt, ctrl = _small_logged()
    T, hs = cfg.nocturne.steps, cfg.nocturne.history_steps
    S = len(scns)

    def rolled(how, **kw):
        eng = _engine(ev, **kw)
        eng.load_scenarios(scns, steps=T)
        eng.set_log(gt, ctrl, hs)
        if how == "jobs":
            eng.run_jobs([(0, S // 3), (S // 3, S)])
        elif how == "step":
            for t in range(T):
                eng.step(t)
        else:
            eng.run()
        r = eng.results()
        r["speed"] = eng.speed_hist.cpu().numpy()
        return eng, r

    base_eng, base = rolled("run", lanes=1)
    assert (base["existence"][:, 1, -1] == 0).all() and (base["sampled"][ctrl][:, hs - 1:] >= 0).any()
    runs = {"default lanes": rolled("run")[1], "two lanes": rolled("run", lanes=2)[1], "three lanes": rolled("run", lanes=3)[1],
            "run_jobs over two ranges": rolled("jobs", lanes=2)[1], "no K/V cache": rolled("run", lanes=1, use_cache=False)[1],
            "no K/V cache, two lanes": rolled("run", lanes=2, use_cache=False)[1], "step()": rolled("step", lanes=1)[1]}
    base_eng.reset()
    base_eng.run()
    r2 = base_eng.results()
    r2["speed"] = base_eng.speed_hist.cpu().numpy()
    runs["a second reset() + run()"] = r2
    for name, r in runs.items():
        for k in KEYS + ("speed",):
            assert np.array_equal(base[k], r[k]), (name, k)
    # the range-safe repeat of check_finite: reset + run of the recorded ranges under the three-plane split rolls the same log again
    eng3 = _engine(ev, lanes=2, split="bf16x6")
    eng3.load_scenarios(scns, steps=T)
    eng3.set_log(gt, ctrl, hs)
    eng3.run()
    assert eng3.check_finite() is False
    a = eng3.results()
    eng3.reset(); eng3.run()
    b = eng3.results()
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["existence"], base["existence"])
    # the log detached: the engine rolls what a fresh engine rolls
    base_eng.set_log(None, None)
    base_eng.reset()
    plain = base_eng.run().results()
    assert "applied" not in plain and "existence" not in plain
    fresh = _engine(ev, lanes=1)
    fresh.load_scenarios(scns, steps=T)
    ref = fresh.run().results()
    for k in ("tokens", "rtg_bins", "states", "coll", "n_groups"):
        assert np.array_equal(plain[k], ref[k]), k
    assert not np.array_equal(ref["tokens"], base["tokens"])


# ---------------------------------------------------------------------------------------------------------------- evaluator
def test_evaluator_device_replay_route():
    out = {}
    for flag in (False, True):
        cfg = _cfg64(device_replay=flag)
        model, policy = _policy(cfg)
        ev = PolicyEvaluator(cfg, policy)
        cap = {}
        if flag:
            inner = ev._roll_batch

            def rolled(items, inner=inner, ev=ev, cap=cap, cfg=cfg):
                inner(items)
                rb = ev.device_replay_readback[-1]
                N = items[0][0].N
                T1 = cfg.nocturne.steps + 1
                goals4 = np.array([[[*np.asarray(gd[v]["pos"], np.float64), float(gd[v]["heading"]), float(gd[v]["speed"])]
                                    for v in range(N)] for gd in rb["goal_dicts"]])
                cap["goals4"] = goals4
                cap["pack"] = ev._batch_engine.metrics_pack(rb["gt"][:, :, :T1, :5], goals4,
                                                            eval_mask=rb["controlled"].astype(np.uint8)).cpu().numpy()
            ev._roll_batch = rolled
        m, lines = ev.evaluate_policy()
        out[flag] = (m, ev.last_vehicle_data_dict, list(ev.vehicles_to_evaluate), ev, cap)
    (m0, v0, e0, ev0, _), (m1, v1, e1, ev1, cap) = out[False], out[True]
    assert ev1.batched_scenes == 64 and ev0.batched_scenes == 64 and e0 == e1 and len(e1) == 8
    assert hasattr(ev0, "batched_timing") and not hasattr(ev0, "device_replay_readback") and len(ev1.device_replay_readback) == 1
    # ---- the metric dict from the route's own read-back arrays
    rb = ev1.device_replay_readback[0]
    cfg = ev1.cfg
    S, N, T1 = rb["states"].shape[:3]
    acc = MetricAccumulators()
    for k in range(S):
        stt = np.zeros((N, T1, 8))
        stt[..., :5] = rb["states"][k, :, :, :5]
        stt[..., 7] = rb["exist"][k]
        g4 = cap["goals4"][k]
        acc.add_scenario(stt, rb["coll"][k].astype(np.float64), rb["accel"][k], rb["gt"][k, :, :T1, :5], g4[:, :2], g4[:, 2], g4[:, 3], cfg,
                         eval_ids=rb["to_eval"][k])
    m_host, _ = acc.compute()
    assert set(m1) == set(m_host)
    for k in m_host:
        assert abs(m_host[k] - m1[k]) <= 1e-12 * max(1.0, abs(m_host[k])), (k, m_host[k], m1[k])
    # ---- the per-scenario schema, and agreement with the step-by-step route
    assert set(v1) == set(v0)
    ulp_max, identical = 0.0, True
    for v in v0:
        assert set(v1[v]) == set(v0[v]), v
        for key in v0[v]:
            assert type(v1[v][key]) is type(v0[v][key]), (v, key)
            if isinstance(v0[v][key], list):
                assert len(v1[v][key]) == len(v0[v][key]), (v, key)
        for key in ("acceleration", "existence", "timestep", "gt_heading", "gt_speed"):
            assert np.array_equal(np.asarray(v0[v][key], np.float64), np.asarray(v1[v][key], np.float64)), (v, key)
        u = _ulps(np.asarray(v0[v]["steering"], np.float64), np.asarray(v1[v]["steering"], np.float64))
        ulp_max = max(ulp_max, float(u.max()))
        assert u.max() <= ULP, (v, u.max())
        for key, get in (("heading", lambda x: x), ("position", lambda p: p["x"]), ("position", lambda p: p["y"]),
                         ("velocity", lambda p: p["x"]), ("velocity", lambda p: p["y"])):
            a = np.array([get(x) for x in v0[v][key]], np.float64)
            b = np.array([get(x) for x in v1[v][key]], np.float64)
            identical = identical and np.array_equal(a, b)
            np.testing.assert_allclose(b, a, rtol=0, atol=1e-4)
        assert np.array_equal(np.array(v0[v]["rtgs"]), np.array(v1[v]["rtgs"])), v       # RTG bins identical
        r0, r1 = np.array(v0[v]["reward"]), np.array(v1[v]["reward"])
        assert np.array_equal(r0[:, [0, 1, 2, 6, 7]], r1[:, [0, 1, 2, 6, 7]]), v          # goal / collision flags identical
        np.testing.assert_allclose(r1, r0, rtol=0, atol=1e-4)
    print(f"last scene: states bit-identical to the step-by-step route: {identical}; largest steering distance {ulp_max:.1f} ulp")
    for k in m0:
        print(f"  {k}: step-by-step {m0[k]!r}, device replay {m1[k]!r}")
    # ---- the device accumulators on the engine the route rolled, against the host accumulators (tolerances of
    # tests/test_gpu_sim_ctx.py::test_device_metric_accumulators_match_host)
    dev_vec, host_vec = cap["pack"], acc.pack()
    assert dev_vec.shape == host_vec.shape
    np.testing.assert_allclose(dev_vec[:10], host_vec[:10], rtol=1e-11, atol=1e-11)
    np.testing.assert_array_equal(dev_vec[10:], host_vec[10:])
    m_dev, _ = MetricAccumulators().unpack(dev_vec).compute()
    for k in m_host:
        np.testing.assert_allclose(m_dev[k], m_host[k], rtol=1e-10, err_msg=k)
