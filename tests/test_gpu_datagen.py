"""GPU: offline-RL dataset generation — the kernels of csrc/dataset.hip through the C ABI against the reference's own values
(tests/golden/dense_reward.npz, preprocessed.npz) and their float64 host forms, LogReplayer against host-driven stepping, and
datagen.generate end to end against its host-route twin.

Tolerances are the project's precedents for float64 kernels against float64 host forms: rtol = atol = 1e-12 (tests/test_gpu_ledger.py,
tests/test_ingest_pinned.py), atol = 1e-10 for returns-to-go (test_ingest_pinned.py), replay_utils.assert_rollouts_agree for replayed
states.  No point or row is left out of a comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import cfg_of, golden  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402
from replay_utils import ULP, _ulps, _cut_logs, assert_rollouts_agree  # noqa: E402
from ctrlsim_amd import _lib, spec, scenarios, ingest, datagen  # noqa: E402
from ctrlsim_amd.metrics import compute_rewards  # noqa: E402
from ctrlsim_amd.rewards import signed_distance_to_road_edges  # noqa: E402

STAGE = 256          # csrc/dataset.hip: EDGE_STAGE, road-edge segments per LDS stage of the edge-distance kernel
SENT = 7.25          # what the output buffers hold before a call


def _tables(polys_per_scene, dtype):
    """(edges [S,E,4] padded with 1e30 rows, poly_off [S,PE+1]) of a batch, as LogReplayer.load builds them."""
    segs = [[np.concatenate([p[:-1], p[1:]], 1) for p in polys if len(p) > 1] for polys in polys_per_scene]
    segs = [np.concatenate(s) if s else np.zeros((0, 4)) for s in segs]
    E = max(len(s) for s in segs)
    edges = np.full((len(segs), E, 4), 1e30, dtype)
    for k, s in enumerate(segs):
        edges[k, :len(s)] = s
    return edges, datagen.polyline_offsets(polys_per_scene)


def _edge_f32(xy, exist, polys_per_scene, pass_exist=True, pad_rows=2):
    """ctrlsim_dataset_edge_distance on points xy [S,N,T,2] (float32-exact) -> out [S,N,T].  The state rows carry T + pad_rows steps;
    pass_exist: existence as its own array (column 7 of the rows then says 1 everywhere), else in column 7."""
    S, N, T = exist.shape
    T1 = T + pad_rows
    hs = np.full((S, N, T1, 8), 3.0e4, np.float32)
    hs[:, :, :T, :2] = xy
    assert np.array_equal(hs[:, :, :T, :2].astype(np.float64), xy), "the points must be float32 values"
    hs[:, :, :T, 7] = 1.0 if pass_exist else exist
    edges, off = _tables(polys_per_scene, np.float32)
    out = torch.full((S, N, T), SENT, dtype=torch.float64, device=DEV)
    p = _lib.ptr
    hs_d, ex_d, eg_d, off_d = dev(hs), dev(exist), dev(edges), dev(off)
    _lib.check(_lib.lib().ctrlsim_dataset_edge_distance(S, N, T, T1, edges.shape[1], off.shape[1] - 1, p(hs_d), p(ex_d) if pass_exist else None,
                                                        p(eg_d), p(off_d), p(out), _lib.stream_ptr()), "dataset_edge_distance")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _edge_f64(xy, exist, polys_per_scene):
    """ctrlsim_dataset_edge_distance_f64 on xy [S,P,2] float64, polylines float64 -> out [S,P]."""
    S, P = xy.shape[:2]
    edges, off = _tables(polys_per_scene, np.float64)
    out = torch.full((S, P), SENT, dtype=torch.float64, device=DEV)
    p = _lib.ptr
    xy_d, eg_d, off_d = dev(xy), dev(edges), dev(off)
    ex_d = dev(exist) if exist is not None else None
    _lib.check(_lib.lib().ctrlsim_dataset_edge_distance_f64(S, P, edges.shape[1], off.shape[1] - 1, p(xy_d), p(ex_d), p(eg_d), p(off_d),
                                                            p(out), _lib.stream_ptr()), "dataset_edge_distance_f64")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _host_edge(xy, polys):
    with np.errstate(all="ignore"):
        return signed_distance_to_road_edges(np.asarray(xy, np.float64).reshape(-1, 2), polys)


# ---------------------------------------------------------------------------------------------- 1. the reference's own values
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_edge_distance_reproduces_the_reference_fixture(case):
    """tests/golden/dense_reward.npz: RLWaymoDataset.compute_dist_to_nearest_road_edge_rewards of the reference on random points and
    polylines of 12, 2 and 31 points (the last a closed ring) — float64 values that float32 does not hold, hence the float64-table
    entry of the same kernel.  c*_edge_signed is the reward -distance / dist_to_road_edge_scaling_factor * existence."""
    g = golden("dense_reward")
    scale = cfg_of("loop").dataset.waymo.dist_to_road_edge_scaling_factor
    xy, exist = g[f"c{case}_xy"], g[f"c{case}_exist"]
    polys = [g[f"c{case}_poly{k}"] for k in range(int(g[f"c{case}_npoly"]))]
    assert [len(q) for q in polys] == [12, 2, 31]
    got = _edge_f64(xy[None], exist[None], [polys])[0]
    assert (got[exist == 0] == 0).all()
    np.testing.assert_allclose(-got / scale * exist, g[f"c{case}_edge_signed"], rtol=1e-12, atol=1e-12)
    # every point evaluated (existence not given): the reward of the existing ones again, and the host form on all of them
    every = _edge_f64(xy[None], None, [polys])[0]
    assert np.array_equal(every[exist != 0], got[exist != 0])
    np.testing.assert_allclose(-every / scale * exist, g[f"c{case}_edge_signed"], rtol=1e-12, atol=1e-12)
    ref = _host_edge(xy, polys)
    print(f"case {case}: largest deviation from the host form {np.abs(every - ref).max():.3g}")
    np.testing.assert_allclose(every, ref, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------- 2. the host form, one batch
def _walk(rs, n, closed=False):
    """A random polyline of n float32 points; closed: the last point 0.1 m from the first (the cyclic branch)."""
    p = rs.uniform(-50, 50, 2) + np.cumsum(rs.normal(0, 2.5, (n, 2)), axis=0)
    if closed:
        ang = np.sort(rs.uniform(0, 2 * np.pi, n - 1))
        p = np.stack([20 * np.cos(ang), 20 * np.sin(ang)], 1) * rs.uniform(0.8, 1.2, (n - 1, 1)) + rs.uniform(-20, 20, 2)
        p = np.concatenate([p, p[:1] + 0.1])
    return p.astype(np.float32).astype(np.float64)


# hand-made groups of scene 2, each around its own origin (about 1000 m apart, far from the random polylines, no point of one group on
# the line of a segment of another): integer coordinates, feet at dyadic fractions of their segments, integer distances — every
# operation of the signed distance is exact there.
# (origin, polylines relative to it, points relative to it, expected signed distances)
_A, _B = [[0, 0], [8, 0]], [[0, 4], [8, 4]]                          # two parallel polylines running the same way
HAND = [
    ((1000, 0), [_A, _B], [[4, 2]], [-2.0]),                         # midway: the signs are opposite, the first listed wins ...
    ((2000, 64), [_B, _A], [[4, 2]], [2.0]),                         # ... in both orders
    ((3000, 128), [[[0, 8], [0, 0], [8, 0]]], [[2, 3], [-3, -4]], [-2.0, 5.0]),   # a V (right angle): inside; outside, nearest to the apex
    ((4000, 192), [[[0, 0], [8, 0], [8, 8], [0, 8], [0, 0]]], [[4, 1], [-3, -4], [4, -2]], [-1.0, 5.0, 2.0]),   # closed square: inside, outside
                                                                     # a corner (n_prior wraps around: cyclic), outside an edge
    # a repeated point: the zero-length segment comes first and its sign is 0 for EVERY point whose nearest point of the polyline is
    # that start — the whole half plane behind it, whatever else the scene holds (the polyline "wins with distance 0").  It therefore
    # sits at the far left of the scene, with nothing but its own first point behind it
    ((-5000, 0), [[[0, 0], [0, 0], [4, 0]]], [[-1, 1], [2, 1]], [0.0, -1.0]),
    ((6000, 320), [[[0, 0], [10, 0]]], [[12, 0]], [0.0]),            # collinear beyond the end: sign 0 -> 0
    ((7000, 384), [[[0, 50], [10, 50]], [[0, 0], [10, 0]]], [[12, 0]], [0.0]),    # ... also behind a farther polyline listed first
]


def _batch():
    rs = np.random.RandomState(77)
    N, T = 9, 21                                                     # 189 points per scene: one partial workgroup of 256
    lengths = (2, 3, 31, 100)
    s0 = [_walk(rs, 31, closed=True)]
    s1 = [_walk(rs, 2), _walk(rs, 3), _walk(rs, 100)]
    s2 = [_walk(rs, lengths[k % 4], closed=(k % 8 == 2)) for k in range(30)]
    hand_xy, hand_ref = [], []
    for org, polys, pts, want in HAND:
        org = np.asarray(org, np.float64)
        s2 += [np.asarray(q, np.float64) + org for q in polys]
        hand_xy += [np.asarray(q, np.float64) + org for q in pts]
        hand_ref += want
    polys = [s0, s1, s2]
    assert [len(q) for q in polys] == [1, 3, 40]
    assert sum(len(q) for q in s2) > STAGE and sum(len(q) - 1 for q in s2) > 3 * STAGE      # four stages, polylines straddling them
    assert {len(q) for q in s0 + s1 + s2} >= set(lengths)
    xy = rs.uniform(-70, 70, (3, N, T, 2)).astype(np.float32).astype(np.float64)
    exist = (rs.uniform(size=(3, N, T)) < 0.85).astype(np.float64)
    n_hand = len(hand_xy)
    assert n_hand <= T
    xy[2, 0, :n_hand] = hand_xy                                      # scene 2, vehicle 0, its first steps
    exist[2, 0, :n_hand] = 1.0
    return polys, xy, exist, n_hand, np.array(hand_ref)


def test_edge_distance_matches_the_host_form_on_one_batch():
    """S = 3 scenes with 1, 3 and 40 polylines of 2, 3, 31 and 100 points (982 points = 942 segments in the third: four LDS stages of 256
    segments), 9 x 21 points per scene, some absent, the hand-made integer rows in scene 2.  Deviation measured on an MI355X: see the
    printed figure (the kernel evaluates the NumPy expressions operation by operation; 0.0 expected)."""
    polys, xy, exist, n_hand, hand_ref = _batch()
    assert (exist == 0).sum() > 30
    got = _edge_f32(xy, exist, polys)
    assert got.shape == exist.shape and (got[exist == 0] == 0).all()
    ref = np.stack([_host_edge(xy[s], polys[s]).reshape(exist.shape[1:]) for s in range(3)])
    print(f"largest deviation from the host form: {np.abs(got - ref * exist).max():.3g}; both signs: {(ref < 0).sum()} / {(ref > 0).sum()}")
    assert (ref < 0).sum() > 20 and (ref > 0).sum() > 20
    np.testing.assert_allclose(got, ref * exist, rtol=1e-12, atol=1e-12)
    # the integer rows: what the reference's rules say, bit for bit (up to the sign of zero)
    assert np.array_equal(ref[2, 0, :n_hand], hand_ref), "the host form on the hand-made rows"
    assert np.array_equal(got[2, 0, :n_hand], hand_ref)
    # existence read from the state rows' own column instead: the same values
    assert np.array_equal(_edge_f32(xy, exist, polys, pass_exist=False, pad_rows=0), got)


# ---------------------------------------------------------------------------------------------- 3. rewards against the reference
def _export(tag):
    """The same simulated scene the fixture generator exported (oracle/gen_golden.py::export_scene), rebuilt from the recipe
    (as tests/test_ingest_pinned.py does)."""
    cl, gm = golden("closed_loop"), golden("metrics")
    cfg = cfg_of("loop")
    d = spec.Dims(cfg)
    rc = cl[f"{tag}_recipe"]
    scn = scenarios.make_scenario(int(rc[0]), int(rc[1]), n_agents=int(rc[2]), n_polylines=int(rc[3]), n_points=d.NP,
                                  extent=float(rc[4]))
    st, act, rew, ex, goals = cl[f"{tag}_states"], cl[f"{tag}_actions"], gm[f"{tag}_reward"], gm[f"{tag}_existence"], gm[f"{tag}_goal"]
    inv = {v: k for k, v in scenarios.ROAD_TYPES.items()}
    N, T1 = st.shape[:2]
    objs = [{"position": [{"x": float(st[v, t, 0]), "y": float(st[v, t, 1])} for t in range(T1)],
             "velocity": [{"x": float(st[v, t, 2]), "y": float(st[v, t, 3])} for t in range(T1)],
             "heading": [float(st[v, t, 4]) for t in range(T1)], "existence": [float(e) for e in ex[v]],
             "acceleration": [float(act[v, t, 0]) if t < T1 - 1 else 0 for t in range(T1)],
             "steering": [float(act[v, t, 1]) if t < T1 - 1 else 0 for t in range(T1)],
             "reward": [[float(x) for x in rew[v, t]] for t in range(T1)],
             "goal_position": {"x": float(goals[v, 0]), "y": float(goals[v, 1])}, "goal_heading": float(goals[v, 2]),
             "goal_speed": float(goals[v, 3]), "width": float(scn.width[v]), "length": float(scn.length[v]), "type": "vehicle"}
            for v in range(N)]
    roads = [{"geometry": [{"x": float(q[0]), "y": float(q[1])} for q in pl[:int(pl[:, 2].sum())]], "type": inv[int(np.argmax(ty))]}
             for pl, ty in zip(scn.road_points, scn.road_types)]
    return cfg, {"name": "synthetic", "objects": objs, "roads": roads}


def _ref_dict(tag):
    g = golden("preprocessed")
    return {k[len(tag) + 5:]: g[k] for k in g.files if k.startswith(f"{tag}_pkl_")}


def _device_rewards(cfg, ag_data, coll, goals4, polys):
    """Both dataset entries on ONE scene given as the dictionary's float64 states [N,T,8] (float32 values) -> dict of host arrays."""
    N, T = ag_data.shape[:2]
    hs = ag_data.astype(np.float32)
    assert np.array_equal(hs.astype(np.float64), ag_data)
    exist = np.ascontiguousarray(ag_data[None, :, :, 7])
    edges, off = _tables([polys], np.float32)
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    hs_d, cl_d, ex_d, g_d, eg_d, off_d = dev(hs[None]), dev(coll[None].astype(np.uint8)), dev(exist), dev(goals4[None]), dev(edges), dev(off)
    z = lambda *sh: torch.full(sh, SENT, dtype=torch.float64, device=DEV)
    edge, rew, vv, ve, rtg = z(1, N, T), z(1, N, T, 8), z(1, N, T), z(1, N, T), z(1, N, T, 5)
    _lib.check(lib.ctrlsim_dataset_edge_distance(1, N, T, T, edges.shape[1], off.shape[1] - 1, p(hs_d), p(ex_d), p(eg_d), p(off_d), p(edge),
                                                 st), "dataset_edge_distance")
    c = datagen.dataset_cfg(cfg)
    _lib.check(lib.ctrlsim_dataset_rewards(1, N, T, T, p(hs_d), p(cl_d), p(ex_d), p(g_d), p(edge), C.byref(c), p(rew), p(vv), p(ve), p(rtg),
                                           st), "dataset_rewards")
    torch.cuda.synchronize()
    return dict(edge=edge.cpu().numpy()[0], ag_rewards=rew.cpu().numpy()[0], veh_veh_dist_rewards=vv.cpu().numpy()[0],
                veh_edge_dist_rewards=ve.cpu().numpy()[0], rtgs=rtg.cpu().numpy()[0])


def _fixture_inputs(tag):
    g, gm = golden("preprocessed"), golden("metrics")
    cfg, data = _export(tag)
    polys = ingest.roads_to_polylines(data["roads"], cfg.dataset.waymo.max_num_road_pts_per_polyline)[2]
    ag_data = g[f"{tag}_pkl_ag_data"]
    coll = g[f"{tag}_pkl_ag_rewards"][..., 6:8]
    return g, cfg, ag_data, coll, gm[f"{tag}_goal"], polys


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_rewards_and_rtgs_reproduce_the_reference_dictionary(tag):
    """tests/golden/preprocessed.npz: the reference's RLWaymoDatasetCtRLSim.get_data / RLWaymoDataset.get on simulated scenes.  States
    and existence from {tag}_pkl_ag_data, the collision flags of every row from {tag}_pkl_ag_rewards, goals from metrics.npz."""
    g, cfg, ag_data, coll, goals4, polys = _fixture_inputs(tag)
    out = _device_rewards(cfg, ag_data, coll, goals4, polys)
    for k in ("ag_rewards", "veh_edge_dist_rewards", "veh_veh_dist_rewards"):
        print(f"{tag} {k}: largest deviation {np.abs(out[k] - g[f'{tag}_pkl_{k}']).max():.3g}")
        np.testing.assert_allclose(out[k], g[f"{tag}_pkl_{k}"], rtol=1e-12, atol=1e-12, err_msg=k)
    print(f"{tag} rtgs: largest deviation {np.abs(out['rtgs'] - g[f'{tag}_rtgs']).max():.3g}")
    np.testing.assert_allclose(out["rtgs"], g[f"{tag}_rtgs"], rtol=1e-12, atol=1e-10)
    # what the fixtures hold (so that the comparison above means something)
    edge = g[f"{tag}_pkl_veh_edge_dist_rewards"]
    assert (edge < 0).any() and (edge > 0).any()
    if tag == "b":
        assert (ag_data[..., 7] == 0).sum() == 29 and (g["b_pkl_ag_rewards"][..., 0] == 1).any()
    if tag == "c":
        assert (ag_data[..., 7] == 0).sum() == 13 and coll[..., 0].any() and coll[..., 1].any()


@pytest.mark.parametrize("switch", ["remove_shaped_goal", "remove_shaped_veh_reward", "remove_shaped_edge_reward", "none"])
def test_rtgs_honour_the_remove_shaped_switches(switch):
    """Scene c with each switch on alone (remove_shaped_goal is the configuration's default; "none": all three off), against
    ingest.load_preprocessed on the reference's dictionary."""
    g, cfg, ag_data, coll, goals4, polys = _fixture_inputs("c")
    w = cfg.dataset.waymo
    for k in ("remove_shaped_goal", "remove_shaped_veh_reward", "remove_shaped_edge_reward"):
        w[k] = k == switch
    out = _device_rewards(cfg, ag_data, coll, goals4, polys)
    ref = ingest.load_preprocessed(_ref_dict("c"), w)["rtgs"]
    if switch != "remove_shaped_goal":
        assert np.abs(ref - g["c_rtgs"]).max() > 1e-3                 # (the switch changes the returns)
    np.testing.assert_allclose(out["rtgs"], ref, rtol=1e-12, atol=1e-10)


@pytest.mark.parametrize("T", [1, 21, 91])
def test_rtg_scan_alone(T):
    """ctrlsim_dataset_rtgs on random dictionary arrays of 2 scenes x 5 vehicles against ingest.load_preprocessed (np.cumsum on the
    reversed step axis: sequential, as the kernel's walk from the last step backwards)."""
    cfg = cfg_of("loop")
    w = cfg.dataset.waymo
    w.remove_shaped_goal = False
    rs = np.random.RandomState(T)
    S, N = 2, 5
    rew = rs.uniform(-0.3, 0.4, (S, N, T, 8))
    rew[..., [0, 1, 2, 6, 7]] = rs.uniform(size=(S, N, T, 5)) < 0.3
    exist = np.cumprod(rs.uniform(size=(S, N, T)) < 0.97, axis=-1).astype(np.float64)
    rew *= exist[..., None]
    veh, edge = rs.uniform(0, 1, (S, N, T)) * exist, rs.uniform(-0.5, 0.5, (S, N, T)) * exist
    out = torch.full((S, N, T, 5), SENT, dtype=torch.float64, device=DEV)
    p = _lib.ptr
    a = [dev(x) for x in (rew, veh, edge, exist)]
    _lib.check(_lib.lib().ctrlsim_dataset_rtgs(S, N, T, p(a[0]), p(a[1]), p(a[2]), p(a[3]), C.byref(datagen.dataset_cfg(cfg)), p(out),
                                               _lib.stream_ptr()), "dataset_rtgs")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for s in range(S):
        ag = np.zeros((N, T, 8))
        ag[..., 7] = exist[s]
        ref = ingest.load_preprocessed(dict(ag_data=ag, ag_rewards=rew[s], veh_edge_dist_rewards=edge[s], veh_veh_dist_rewards=veh[s],
                                            road_points=None, road_types=None), w)["rtgs"]
        np.testing.assert_allclose(got[s], ref, rtol=1e-12, atol=1e-10)


# ---------------------------------------------------------------------------------------------- 4. / 5. the replayer and generate
STEPS = 24
KEYS = {"idx", "num_agents", "road_points", "road_types", "ag_data", "ag_actions", "ag_types", "last_exist_timesteps",
        "veh_edge_dist_rewards", "veh_veh_dist_rewards", "ag_rewards", "filtered_ag_ids", "ag_goals", "rtgs"}


@pytest.fixture(scope="module")
def logged():
    """5 scenes x 12 vehicles x 24 steps with the four kinds of log cuts of replay_utils._cut_logs; rolled once per route."""
    cfg = cfg_of("loop")
    d = spec.Dims(cfg)
    scns = [scenarios.make_scenario(31, k, n_agents=12, n_polylines=14, n_points=d.NP, extent=40.0) for k in range(5)]
    logs = []
    for k, scn in enumerate(scns):
        lg = scenarios.standin_log(scn, STEPS + 1)
        for v in range(scn.N):
            lg[v]["traj"] = _cut_logs(k, v, lg[v]["traj"].copy())
        logs.append(lg)
    host = datagen.LogReplayer(cfg, DEV).load(scns, logs, STEPS).run_host().results()
    rp = datagen.LogReplayer(cfg, DEV).load(scns, logs, STEPS)
    devr = rp.run().results()
    return dict(cfg=cfg, scns=scns, logs=logs, host=host, dev=devr, log=rp.log_h, goals4=rp.goals4_h)


def test_log_replayer_equals_host_driven_stepping(logged):
    """The host side is LogReplayer.run_host(): NumPy replay.latch / replay.actions around one simulator step per step, as
    replay_utils.host_driven steps an engine.  The replay arithmetic is independent of the kernels, but run_host() shares load() and the
    simulator call with run(): a wrong tensor shape or row count there would go unseen by this
    comparison (the shapes asserted below, the generator's existence rule and the cut checks are what stands against that)."""
    host, devr = logged["host"], logged["dev"]
    assert devr["states"].shape == (5, 12, STEPS + 1, 8) and devr["alive"].shape == (5, 12, STEPS) and devr["applied"].shape == (5, 12, STEPS, 2)
    assert_rollouts_agree(host, devr, "5 scenes x 12 vehicles, nothing controlled", ("tokens", "coll", "existence", "alive"))
    # the dataset's existence is the generator's rule on the log
    assert np.array_equal(devr["alive"], datagen.dataset_existence(logged["log"], STEPS))
    # the cuts did what they were made for: leaves early, leaves later, never there, a flag that drops and comes back
    al = devr["alive"]
    assert (al[:, 1, -1] == 0).all() and (al[:, 2, 10] == 1).all() and (al[:, 2, 11:] == 0).all() and (al[:, 3] == 0).all()
    assert (al[:, 4, 6] == 1).all() and (al[:, 4, 7:] == 0).all() and (al[:, 0] == 1).all()
    assert (devr["existence"][:, 4, 7] == 1).all()          # (the latched log flag still holds where the next row is missing)
    assert (devr["applied"][..., 1] != 0).any()


def test_generate_against_the_host_route_and_its_own_states(logged, tmp_path):
    cfg, scns, logs = logged["cfg"], logged["scns"], logged["logs"]
    w = cfg.dataset.waymo
    dv = datagen.generate(cfg, scns, logs, STEPS, device=DEV)
    hv = datagen.generate_host(cfg, scns, logs, STEPS, device=DEV)
    assert len(dv) == len(hv) == 5
    for k, (d, h) in enumerate(zip(dv, hv)):
        assert set(d) == set(h) == KEYS                                                           # preprocess_scene's keys + rtgs
        for key in d:
            assert np.asarray(d[key]).shape == np.asarray(h[key]).shape and np.asarray(d[key]).dtype == np.asarray(h[key]).dtype, key
        # integer and flag keys
        assert d["idx"] == h["idx"] == k and d["num_agents"] == h["num_agents"] == 12
        assert list(d["filtered_ag_ids"]) == list(h["filtered_ag_ids"])
        for key in ("last_exist_timesteps", "ag_types", "road_points", "road_types"):
            assert np.array_equal(d[key], h[key]), key
        assert np.array_equal(d["ag_data"][..., 5:], h["ag_data"][..., 5:])                       # length, width, existence
        assert np.array_equal(d["ag_rewards"][..., 6:], h["ag_rewards"][..., 6:])                 # the collision flags of every row
        np.testing.assert_allclose(d["ag_goals"], h["ag_goals"], rtol=1e-12, atol=1e-12)
        # states and actions: the rules of the replay comparison
        np.testing.assert_allclose(d["ag_data"][..., :5], h["ag_data"][..., :5], rtol=0, atol=1e-4)
        assert np.array_equal(d["ag_actions"][..., 0].view(np.int64), h["ag_actions"][..., 0].view(np.int64))
        assert _ulps(d["ag_actions"][..., 1], h["ag_actions"][..., 1]).max() <= ULP
        # the reward keys, recomputed by the host forms FROM THE DEVICE ROUTE'S OWN STATES: this isolates the new kernels
        g4 = logged["goals4"][k]
        rows = compute_rewards(d["ag_data"], d["ag_rewards"][..., 6:8], g4[:, :2], g4[:, 2], g4[:, 3], cfg.nocturne.rew_cfg)
        ref = ingest.preprocess_scene(datagen.export_json(f"scene_{k}", scns[k], d, goals4=g4, rewards=rows), w, idx=k)
        for key in ("ag_data", "ag_actions"):
            assert np.array_equal(ref[key], d[key]), key
        np.testing.assert_allclose(ref["ag_goals"], d["ag_goals"], rtol=1e-12, atol=1e-12)
        for key in datagen.REWARD_KEYS:
            print(f"scene {k} {key}: largest deviation {np.abs(d[key] - ref[key]).max():.3g}")
            np.testing.assert_allclose(d[key], ref[key], rtol=1e-12, atol=1e-12, err_msg=key)
        np.testing.assert_allclose(d["rtgs"], ingest.load_preprocessed(ref, w)["rtgs"], rtol=1e-12, atol=1e-10)
    assert any((d["veh_edge_dist_rewards"] < 0).any() for d in dv) and any((d["veh_edge_dist_rewards"] > 0).any() for d in dv)
    # the pickles are what Evaluator.load_preprocessed_data reads: no rtgs inside, the same rtgs out
    names = [f"scene_{k}" for k in range(5)]
    paths = datagen.write_dataset(str(tmp_path), names, dv)
    assert [p.rsplit("/", 1)[1] for p in paths] == [f"{n}_physics.pkl" for n in names]
    import pickle
    for path, d in zip(paths, dv):
        with open(path, "rb") as fh:
            assert "rtgs" not in pickle.load(fh)
        back = ingest.load_preprocessed(path, w)
        np.testing.assert_allclose(back["rtgs"], d["rtgs"], rtol=1e-12, atol=1e-10)
        assert np.array_equal(back["road_points"], d["road_points"])


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    S, N, T, T1, E, PE = 1, 4, 3, 4, 5, 2
    hs, ex = torch.zeros(S, 65, T1, 8, device=DEV), torch.ones(S, 65, T, dtype=torch.float64, device=DEV)
    eg, off = torch.zeros(S, E, 4, device=DEV), torch.tensor([[0, 2, 5]], dtype=torch.int32, device=DEV)
    out = torch.zeros(S, 65, T, dtype=torch.float64, device=DEV)
    call = lambda N=N, T=T, T1=T1, E=E, PE=PE, eg=eg, off=off: lib.ctrlsim_dataset_edge_distance(
        S, N, T, T1, E, PE, p(hs), p(ex), p(eg), p(off), p(out), st)
    assert call() == 0
    assert call(N=65) == -22 and call(N=0) == -22
    assert call(T=T1 + 1) == -22 and call(T=0) == -22
    assert call(eg=None) == -22 and call(off=None) == -22
    assert call(PE=-1) == -22 and call(E=-1) == -22
    assert call(E=0, eg=None, off=None, PE=0) == 0                                # no table, nothing to read
    c = datagen.dataset_cfg(cfg_of("loop"))
    d64 = lambda *sh: torch.zeros(*sh, dtype=torch.float64, device=DEV)
    cl, g4 = torch.zeros(S, N, T1, 2, dtype=torch.uint8, device=DEV), d64(S, N, 4)
    rew, vv, ve, rtg, edge = d64(S, N, T, 8), d64(S, N, T), d64(S, N, T), d64(S, N, T, 5), d64(S, N, T)
    rcall = lambda N=N, T=T, cfgp=C.byref(c), g4=g4: lib.ctrlsim_dataset_rewards(S, N, T, T1, p(hs), p(cl), p(ex), p(g4), p(edge), cfgp, p(rew),
                                                                                   p(vv), p(ve), p(rtg), st)
    assert rcall() == 0
    assert rcall(N=65) == -22 and rcall(T=T1 + 1) == -22 and rcall(cfgp=None) == -22 and rcall(g4=None) == -22
    assert lib.ctrlsim_dataset_rtgs(S, 65, T, p(rew), p(vv), p(ve), p(ex), C.byref(c), p(rtg), st) == -22
    assert lib.ctrlsim_dataset_edge_distance_f64(S, 4, E, -1, p(d64(S, 4, 2)), None, p(d64(S, E, 4)), p(off), p(d64(S, 4)), st) == -22
    torch.cuda.synchronize()


def test_generate_refuses_a_scene_without_road_edges():
    cfg = cfg_of("loop")
    d = spec.Dims(cfg)
    scn = scenarios.make_scenario(31, 0, n_agents=4, n_polylines=6, n_points=d.NP, extent=40.0)
    edge = np.argmax(scn.road_types, axis=1) == scenarios.ROAD_TYPES["road_edge"]
    scn.road_types[edge] = np.eye(8)[scenarios.ROAD_TYPES["lane"]]
    scn.edge_segments = np.zeros((0, 4), np.float32)
    with pytest.raises(ValueError, match="no road-edge polyline"):
        datagen.generate(cfg, [scn], [scenarios.standin_log(scn, 5)], 4, device=DEV)
