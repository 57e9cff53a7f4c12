"""ctrlsim_metrics_pack (csrc/metrics.hip: the payload of the only collective of a multi-GPU run) called directly on synthetic
arrays, without an engine, against ctrlsim_amd.metrics.MetricAccumulators (pinned to the reference's evaluator by
tests/test_metrics_pinned.py): the shapes, existence patterns and bin-edge values a rollout of 10 vehicles does not produce."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import _lib, spec  # noqa: E402
from ctrlsim_amd.metrics import MetricAccumulators  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402

EINVAL = -22
SHAPES = [(1, 1, 2), (3, 64, 12), (37, 10, 21)]


def _edges():
    E = MetricAccumulators.EDGES
    return np.concatenate([E["lin"], E["ang"], E["accel"], E["nd"]]).astype(np.float64)


def _params(cfg):
    w = cfg.dataset.waymo
    return (C.c_double * 5)(float(cfg.nocturne.rew_cfg["position_target_tolerance"]), w.min_accel, w.max_accel, w.accel_discretization,
                            w.steer_discretization)


def _scene(S, N, T1, hist_steps):
    """float32-representable inputs, so that both sides see the same numbers."""
    rs = np.random.RandomState(S * 1000 + N * 10 + hist_steps)
    f32 = lambda a: np.asarray(a, np.float32)
    h = min(hist_steps, T1 - 1)                                                  # first step that can be evaluated (if any)
    states = np.zeros((S, N, T1, 8), np.float32)
    states[..., :2] = f32(rs.uniform(-60, 60, (S, N, T1, 2)))
    states[..., 2:4] = f32(rs.normal(0, 8, (S, N, T1, 2)))
    states[..., 4] = f32(rs.uniform(-6.5, 6.5, (S, N, T1)))                      # heading / dt beyond +-50 at both ends
    states[..., 5:7] = (4.5, 2.0)
    states[..., 7] = rs.uniform(size=(S, N, T1)) < 0.8
    coll = (rs.uniform(size=(S, N, T1, 2)) < 0.1).astype(np.uint8)
    tok = rs.randint(0, 1000, (S, N, T1 - 1)).astype(np.int32)
    tok[:, :, ::3] = rs.choice([7, 999, 960, 49], (S, N, len(range(0, T1 - 1, 3))))      # acceleration bins 0 and 19: -10 and +10, on edges
    gt = np.zeros((S, N, T1, 5))
    gt[..., :2] = f32(states[..., :2] + f32(rs.normal(0, 2, (S, N, T1, 2))))
    gt[..., 2] = f32(rs.uniform(-6.5, 6.5, (S, N, T1)))
    gt[..., 3] = f32(rs.uniform(0, 35, (S, N, T1)))                              # log speeds beyond 30
    gt[..., 4] = rs.uniform(size=(S, N, T1)) < 0.9
    goals4 = np.zeros((S, N, 4))
    goals4[..., :2] = f32(rs.uniform(-60, 60, (S, N, 2)))
    # ---- values exactly on bin edges (scenario 0, wherever the vehicle is evaluated)
    v_edge = f32([(0, 0), (30, 0), (18, 24), (40, 9), (5, 0), (0, -15)])         # |v| = 0, 30, 30, beyond 30, 5, 15
    hd_edge = f32([-5.0, 5.0, 0.0, 0.25, -0.25, 6.0])                            # / dt = -50, 50 (the inclusive last edge), 0, 2.5, -2.5, beyond
    for k in range(T1):
        states[0, :, k, 2:4] = v_edge[(np.arange(N) + k) % 6]
        states[0, :, k, 4] = hd_edge[(np.arange(N) + k) % 6]
        gt[0, :, k, 2] = hd_edge[(np.arange(N) + 2 * k + 1) % 6]
        gt[0, :, k, 3] = f32([0.0, 30.0, 31.0, 5.0, 2.0, 4.0])[(np.arange(N) + k) % 6]     # steps of 2 / 4 over 2 dt: accelerations beyond the clip
    if N >= 10:
        # ---- existence patterns (scenario 0): exactly one, exactly two evaluated steps, a run with a gap, none
        states[0, :4, :, 7] = 0
        states[0, 0, h, 7] = 1
        states[0, 1, [h, T1 - 1], 7] = 1
        states[0, 2, h:, 7] = 1
        states[0, 2, min(h + 2, T1 - 1), 7] = 0
        states[0, 3, :h, 7] = 1
        # the goal is passed at a step where the vehicle does not exist: the latch runs over all t, evaluated or not
        goals4[0, 1, :2] = states[0, 1, max(h - 1, 0) if h else min(1, T1 - 2), :2].astype(np.float64)
        goals4[0, 4, :2] = states[0, 4, T1 - 1, :2].astype(np.float64) + 0.5      # within the tolerance at the last step only
        states[0, 4, T1 - 1, 7] = 1
        # ---- nearest distances on edges (scenario 1): alone (0), exactly 40 (edge 32), above 40, 2.5 (edge 2)
        states[1, :, :, 7] = 0
        states[1, :4, :, 7] = 1
        states[1, 0, :, :2], states[1, 1, :, :2] = f32((0, 0)), f32((24, 32))
        states[1, 2, :, :2], states[1, 3, :, :2] = f32((500, 500)), f32((501.5, 502))
        gt[1, :4, :, :2] = states[1, :4, :, :2].astype(np.float64) * 2            # log: 80 (beyond 40) and 5.0 (edge 4)
        states[2, :, :, 7] = 0
        states[2, 5, :, 7] = 1                                                    # alone in its scenario: nearest distance 0
    return states, coll, tok, gt, goals4


def _host(cfg, states, coll, tok, gt, goals4, emask):
    w = cfg.dataset.waymo
    acc = MetricAccumulators()
    S, N, T1 = states.shape[:3]
    for s in range(S):
        accel = np.concatenate([(tok[s] // w.steer_discretization) / (w.accel_discretization - 1) * (w.max_accel - w.min_accel)
                                + w.min_accel, np.zeros((N, 1))], 1)
        acc.add_scenario(states[s].astype(np.float64), coll[s], accel, gt[s], goals4[s, :, :2], goals4[s, :, 2], goals4[s, :, 3], cfg,
                         eval_ids=None if emask is None else list(np.where(emask[s])[0]))
    return acc.pack()


def _device(cfg, states, coll, tok, gt, goals4, emask, hist_steps, out=None, sl=slice(None)):
    lib, p = _lib.lib(), _lib.ptr
    S, N, T1 = states[sl].shape[:3]
    if out is None:
        out = torch.zeros(int(lib.ctrlsim_metrics_size()), dtype=torch.float64, device=DEV)
    d = [dev(a[sl]) for a in (states, coll, tok, gt, goals4)]
    d_mask = dev(emask[sl]) if emask is not None else None
    d_edges = dev(_edges())
    _lib.check(lib.ctrlsim_metrics_pack(S, N, T1, T1 - 1, hist_steps, float(cfg.nocturne.dt), p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(d[4]),
                                        p(d_mask), _params(cfg), p(d_edges), p(out), _lib.stream_ptr()), "metrics_pack")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mask", ["null", "random", "one_scenario_off"])
@pytest.mark.parametrize("hist_steps", [0, 3, "T1"])
@pytest.mark.parametrize("S,N,T1", SHAPES)
def test_metrics_pack_matches_the_host_accumulators(S, N, T1, hist_steps, mask):
    """(S, N, T1) = (1, 1, 2): thread = vehicle alone, the shortest rollout; (3, 64, 12): the full 64-entry reduction; (37, 10, 21).
    hist_steps 0, 3 and T1 (nothing is evaluated: the vector stays zero).  Planted: vehicles present at exactly one and exactly two
    evaluated steps (no acceleration sample), at a run with a gap, at no evaluated step; a goal passed while the vehicle does not
    exist; speeds 0 / 30 / beyond, heading / dt -50 / 50 / 0, nearest distances 0 / 40 / beyond, accelerations that land on the edges
    -10 / +10 after the round trip through the discretisation.  Histograms bin for bin; sums and counts at the project's bound for this
    vector (float64 atomics arrive in any order)."""
    hs = T1 if hist_steps == "T1" else hist_steps
    cfg = spec.make_cfg(nocturne__history_steps=hs, nocturne__steps=T1 - 1)
    states, coll, tok, gt, goals4 = _scene(S, N, T1, hs)
    rs = np.random.RandomState(3)
    emask = None if mask == "null" else (rs.uniform(size=(S, N)) < 0.7).astype(np.uint8)
    if mask == "one_scenario_off":
        emask[S // 2] = 0
    host = _host(cfg, states, coll, tok, gt, goals4, emask)
    got = _device(cfg, states, coll, tok, gt, goals4, emask, hs).cpu().numpy()
    assert got.shape == host.shape
    np.testing.assert_array_equal(got[10:], host[10:])
    np.testing.assert_allclose(got[:10], host[:10], rtol=1e-11, atol=1e-11)
    if hs >= T1 or (mask == "one_scenario_off" and S == 1):
        assert not host.any()
    elif N >= 10 and mask == "null":
        assert host[5] > 0 and host[10:].sum() > 0
        e = MetricAccumulators.EDGES
        h = {k: host[o:o + n] for k, o, n in (("acc_gt", 10, 20), ("acc_sim", 30, 20), ("ang_sim", 250, 200), ("lin_sim", 650, 200),
                                              ("nd_gt", 850, 200), ("nd_sim", 1050, 200))}
        # the planted edge values arrived where np.histogram puts them: first bins, the inclusive last edge, the clip values
        assert h["ang_sim"][0] > 0 and h["ang_sim"][199] > 0 and h["ang_sim"][100] > 0
        assert h["lin_sim"][0] > 0 and h["lin_sim"][int(np.searchsorted(e["lin"], 30.0, side="right")) - 1] > 0
        assert h["nd_sim"][0] > 0 and h["nd_sim"][32] > 0 and h["nd_sim"][2] > 0 and h["nd_gt"][32] > 0 and h["nd_gt"][4] > 0
        assert h["acc_sim"][5] > 0 and h["acc_sim"][15] > 0 and h["acc_gt"][5] > 0 and h["acc_gt"][15] > 0


@pytest.mark.parametrize("S,N,T1", SHAPES[1:])
def test_metrics_accumulate_into_a_filled_vector(S, N, T1):
    """Two calls into the same `out` (the second into the first's result) equal one call over the union, and the host."""
    cfg = spec.make_cfg(nocturne__history_steps=3, nocturne__steps=T1 - 1)
    a = _scene(S, N, T1, 3)
    emask = (np.random.RandomState(8).uniform(size=(S, N)) < 0.8).astype(np.uint8)
    whole = _device(cfg, *a, emask, 3).cpu().numpy()
    half = S // 2
    out = _device(cfg, *a, emask, 3, sl=slice(0, half))
    first = out.cpu().numpy().copy()
    assert first.any() and not np.array_equal(first, whole)
    both = _device(cfg, *a, emask, 3, out=out, sl=slice(half, S)).cpu().numpy()
    np.testing.assert_array_equal(both[10:], whole[10:])
    np.testing.assert_allclose(both[:10], whole[:10], rtol=1e-11, atol=1e-11)
    host = _host(cfg, *a, emask)
    np.testing.assert_array_equal(both[10:], host[10:])
    np.testing.assert_allclose(both[:10], host[:10], rtol=1e-11, atol=1e-11)


def test_metrics_refusals():
    lib, st = _lib.lib(), _lib.stream_ptr()
    cfg = spec.make_cfg()
    z = torch.zeros(4096, dtype=torch.float64, device=DEV).data_ptr()
    call = lambda N, T1, edges: lib.ctrlsim_metrics_pack(1, N, T1, max(T1 - 1, 1), 0, 0.1, z, z, z, z, z, None, _params(cfg), edges, z, st)
    assert call(65, 5, z) == EINVAL
    assert call(4, 1, z) == EINVAL
    assert call(4, 5, None) == EINVAL
    torch.cuda.synchronize()
