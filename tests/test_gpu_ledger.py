"""ctrlsim_dt_ledger_step (csrc/rewards.hip) call by call against tests/sat_ref.py:ledger_step — the host forms of
ctrlsim_amd/rewards.py, pinned to the reference by tests/golden/dense_reward.npz — in float64, where the rollout test sees it only
after a dozen steps behind the 1e-4 of the float32 positions."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import _lib, spec  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402
import sat_ref  # noqa: E402

EINVAL = -22
S, T1, TMAX = 3, 5, 4
SENT = -7
REMOVE = {"default": None, "none": (0, 0, 0), "veh": (0, 1, 0), "edge": (0, 0, 1), "all": (1, 1, 1)}


def _dt_cfg(w, rew_cfg):
    """ctrlsim_dt_reward_cfg from the configuration (what RolloutEngine._dt_cfg fills in)."""
    c = _lib.DtRewardCfg()
    c.pos_tol = float(rew_cfg["position_target_tolerance"])
    c.shaped_unit = float(rew_cfg.get("shaped_goal_distance_scaling", 1.0)) / float(rew_cfg["reward_scaling"])
    c.goal_mult, c.shaped_min, c.shaped_max = float(w.pos_target_achieved_rew_multiplier), float(w.pos_goal_shaped_min), float(w.pos_goal_shaped_max)
    c.veh_mult, c.max_veh_dist = float(w.veh_veh_collision_rew_multiplier), float(w.max_veh_veh_distance)
    c.edge_mult, c.edge_scale = float(w.veh_edge_collision_rew_multiplier), float(w.dist_to_road_edge_scaling_factor)
    for k, (lo, hi) in enumerate(((w.min_rtg_pos, w.max_rtg_pos), (w.min_rtg_veh, w.max_rtg_veh), (w.min_rtg_road, w.max_rtg_road))):
        c.rtg_lo[k], c.rtg_hi[k] = float(lo), float(hi)
    c.remove_shaped_goal, c.remove_shaped_veh, c.remove_shaped_edge = int(bool(w.remove_shaped_goal)), \
        int(bool(w.remove_shaped_veh_reward)), int(bool(w.remove_shaped_edge_reward))
    return c


def _scene(N, E):
    """Synthetic states / collisions / goals / segment table with the planted cases (see the test's docstring)."""
    rs = np.random.RandomState(100 * N + E)
    f32 = lambda a: np.asarray(a, np.float32)
    states = np.zeros((S, N, T1, 8), np.float32)
    states[..., :2] = f32(rs.uniform(-30, 30, (S, N, T1, 2)))
    states[..., 2:7] = f32(rs.normal(size=(S, N, T1, 5)))
    states[..., 7] = rs.uniform(size=(S, N, T1)) < 0.85
    coll = (rs.uniform(size=(S, N, T1, 2)) < 0.15).astype(np.uint8)
    goals = np.zeros((S, N, 5))
    goals[..., :2] = rs.uniform(-30, 30, (S, N, 2))
    edges = np.zeros((S, E, 4), np.float32)
    a = rs.uniform(-40, 40, (S, E, 2))
    edges[..., :2], edges[..., 2:] = f32(a), f32(a + rs.uniform(-15, 15, (S, E, 2)))
    states[0, 0, :, 7] = 1
    goals[0, 0, :2] = states[0, 0, 0, :2].astype(np.float64)                    # starts exactly on its goal: dist0 == 0
    coll[0, 0, 0] = (1, 0)                                                      # and in a vehicle collision at step 0
    if N == 1:
        states[1, 0, :, 7] = 1
        goals[1, 0, :2] = states[1, 0, 0, :2].astype(np.float64) + (0.3, -0.4)  # within pos_tol (0.5 m of 1.0)
        coll[1, 0, 0] = (0, 1)                                                  # road-edge collision at step 0
        states[2, 0, :, 7] = 0                                                  # a vehicle that does not exist, finite coordinates
    else:
        states[0, 1, :, 7] = 1
        goals[0, 1, :2] = states[0, 1, 0, :2].astype(np.float64) + (0.3, -0.4)
        coll[0, 1, 0] = (0, 1)
        coll[0, 3, 0] = (1, 1)
        states[0, 2, :, 7] = 0                                                  # does not exist, finite coordinates
        states[1, :, :, 7] = 0                                                  # scenario 1: vehicle 0's only neighbours do not exist
        states[1, 0, :, 7] = 1
        states[2, 0, :, :2] = f32(200.0 + rs.uniform(0, 1, (T1, 2)))            # beyond 5 m from every edge (and from every vehicle)
        states[2, 0, :, 7] = 1
        states[2, 1, 2, :2] = states[2, 2, 2, :2] + f32((1.5, 2.0))             # a close pair (2.5 m)
        states[2, 1:3, 2, 7] = 1
    if E == 1:
        edges[1, 0, 2:] = edges[1, 0, :2]                                       # scenario 1: nothing but a zero-length row
        edges[2, 0] = 1e30                                                      # scenario 2: no road edge at all (padding only)
    else:
        edges[0, 60:] = 1e30                                                    # padding rows behind the 64th lane
        edges[1, 66, :2] = states[1, 0, 1, :2] + f32((0.6, 0.8))                # zero-length row 1 m from vehicle (1, 0) at step 1 ...
        edges[1, 66, 2:] = edges[1, 66, :2]
        edges[1, 5, 2:] = edges[1, 5, :2]                                       # ... and another one among the first 64
    return states, coll, goals, edges


def _steer_clear_of_edges(states, edges):
    """The float64 bound holds away from cancellation: every existing vehicle stays >= 1e-3 m from every row (the seeds are chosen so
    that this holds; asserted).  One vehicle is within 5 m of an edge, one beyond."""
    near = min(sat_ref.min_edge_distance(states[s, :, t], edges[s]) for s in range(S) for t in range(TMAX))
    assert near >= 1e-3, near
    return near


@pytest.fixture(scope="module")
def cfg():
    return spec.make_cfg()


@pytest.mark.parametrize("E", [1, 70])
@pytest.mark.parametrize("N", [1, 5, 64])
def test_ledger_steps_match_the_host_form_in_float64(cfg, N, E):
    """Steps t = 0 .. 3 of S = 3 scenarios.  Planted: a vehicle exactly on its goal (dist0 == 0) and one within pos_tol, a vehicle that
    does not exist (finite coordinates), a vehicle whose only neighbours do not exist, padding rows (x0 > 1e29) behind lane 64, a
    zero-length row that is the nearest one, a scenario without road edges, a position beyond 5 m from every edge and ones nearer,
    collisions of both kinds at step 0.  Default switches, no switch, remove_shaped_veh / _edge alone, all three; init_rtg NULL and
    given (values that leave [rtg_lo, rtg_hi] at both ends, at once and within three steps); rtg_raw NULL and given.
    ledger[:, :, 0:10] and rtg_raw: rtol = atol = 1e-12 (chains of < 30 correctly rounded float64 operations on magnitudes <= 100:
    about 3e-13; the min reductions are exact).  hist_rtg: float32 bits within 1 unit in the last place of float32(reference); rows of
    other steps untouched.
    Measured on an MI355X: maximum deviation 0.0 at all six shapes — the kernel evaluates the NumPy expressions operation by operation,
    without FMA contraction, and sqrt / division are correctly rounded on both sides (the test prints the figure)."""
    w0, rew_cfg = cfg.dataset.waymo, cfg.nocturne.rew_cfg
    states, coll, goals, edges = _scene(N, E)
    _steer_clear_of_edges(states, edges)
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    d_states, d_coll, d_goals, d_edges = dev(states), dev(coll), dev(goals), dev(edges)
    rs = np.random.RandomState(N + E)
    init = rs.uniform(-15.0, 100.0, (S, N, 3))
    init[0, 0] = (9.5, 89.5, -9.8)        # on its goal, collided: the goal RTG falls below 0, the vehicle RTG climbs above 90 in three steps
    worst = 0.0
    clipped = np.zeros(2, bool)
    for name, remove in REMOVE.items():
        w = sat_ref.reward_cfg(w0, remove)
        c = _dt_cfg(w, rew_cfg)
        for init_rtg in (None, init):
            for with_raw in (False, True):
                ledger = torch.full((S, N, 10), float(SENT), dtype=torch.float64, device=DEV)
                raw = torch.full((S, N, TMAX, 3), float(SENT), dtype=torch.float64, device=DEV) if with_raw else None
                hist = torch.full((S, N, TMAX, 3), SENT, dtype=torch.int32, device=DEV)
                d_init = dev(init_rtg) if init_rtg is not None else None
                carry = [None] * S
                for t in range(TMAX):
                    _lib.check(lib.ctrlsim_dt_ledger_step(S, N, E, t, T1, TMAX, p(d_states), p(d_coll), p(d_goals), p(d_edges), p(d_init),
                                                          C.byref(c), p(ledger), p(raw), p(hist), st), "dt_ledger_step")
                    torch.cuda.synchronize()
                    got_l, got_h = ledger.cpu().numpy(), hist.cpu().numpy()
                    for s in range(S):
                        (ref_l, ref_raw, ref_n), carry[s] = sat_ref.ledger_step(
                            t, states[s, :, t], coll[s, :, t], goals[s, :, :2], edges[s], w, rew_cfg, carry[s],
                            None if init_rtg is None else init_rtg[s])
                        worst = max(worst, float(np.abs(got_l[s] - ref_l).max()))
                        np.testing.assert_allclose(got_l[s], ref_l, rtol=1e-12, atol=1e-12, err_msg=f"{name} t={t} s={s}")
                        if with_raw:
                            got_r = raw.cpu().numpy()[s]
                            worst = max(worst, float(np.abs(got_r[:, t] - ref_raw).max()))
                            np.testing.assert_allclose(got_r[:, t], ref_raw, rtol=1e-12, atol=1e-12)
                            assert (got_r[:, t + 1:] == SENT).all()
                        ulps = np.abs(got_h[s, :, t].astype(np.int64) - ref_n.astype(np.float32).view(np.int32).astype(np.int64))
                        assert ulps.max() <= 1, (name, t, s, ulps.max())
                        assert (got_h[s, :, t + 1:] == SENT).all()
                        clipped |= [(ref_n == 0.0).any() and (ref_raw < [w.min_rtg_pos, w.min_rtg_veh, w.min_rtg_road]).any(),
                                    (ref_n == 1.0).any() and (ref_raw > [w.max_rtg_pos, w.max_rtg_veh, w.max_rtg_road]).any()]
    assert clipped.all()                                   # the RTG clip was reached at both ends
    print(f"N={N} E={E}: maximum |ledger - float64 host form| = {worst:.3e}")


def test_ledger_refusals(cfg):
    """What the launcher states it refuses, before any launch."""
    lib, st = _lib.lib(), _lib.stream_ptr()
    c = _dt_cfg(sat_ref.reward_cfg(cfg.dataset.waymo), cfg.nocturne.rew_cfg)
    z = torch.zeros(4096, dtype=torch.float64, device=DEV).data_ptr()
    call = lambda N, E, t, T1_, Tmax, edges: lib.ctrlsim_dt_ledger_step(1, N, E, t, T1_, Tmax, z, z, z, edges, None, C.byref(c), z, None, z, st)
    assert call(65, 1, 0, 5, 4, z) == EINVAL
    assert call(4, 1, 4, 6, 4, z) == EINVAL                # t = Tmax
    assert call(4, 1, 2, 2, 4, z) == EINVAL                # T1 = t
    assert call(4, 3, 0, 5, 4, None) == EINVAL             # E > 0 without a segment table
    torch.cuda.synchronize()
