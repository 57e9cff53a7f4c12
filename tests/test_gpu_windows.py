"""GPU: the device window build — ctrlsim_window_build (csrc/window.hip) through ctrlsim_amd/windows.py against the reference's own
windows (tests/golden/loss.npz win_*), the host form ingest.training_window on a generated batch, tie cases, the Decision-Transformer
layout, the refusals with the kernel's own guard, OpenLoopEvaluator.evaluate_dataset end to end and two streams at once.

Bounds: integers (tokens, return bins, time steps, types, existence, the moving mask, road types) are exact; st12, goal5 and road_pts are
float64 geometry rounded once to float32 on both sides and compared at atol = 2e-5, rtol = 1e-6 — the bound tests/test_gpu_context_build.py
uses for the same comparison (device sin / cos may differ from libm by an ulp; the products are not contracted on the device, while
np.dot may fuse them).  The rankings are compared only where the host asserts a gap of more than 1e-9 between adjacent keys."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import cfg_of, golden  # noqa: E402
from gpu_utils import DEV  # noqa: E402
from replay_utils import _cut_logs  # noqa: E402
from ctrlsim_amd import spec, scenarios, ingest, datagen, weights  # noqa: E402
from ctrlsim_amd.engine import CtxBuffers, ctx_from_reference_layout  # noqa: E402
from ctrlsim_amd.evaluators import OpenLoopEvaluator  # noqa: E402
from ctrlsim_amd.models import CtRLSim  # noqa: E402
from ctrlsim_amd.windows import DeviceDataset, build_windows, launch_windows  # noqa: E402
import loss_ref  # noqa: E402

ATOL, RTOL = 2e-5, 1e-6
INT_FIELDS = ("act_tok", "rtg_bin", "tstep", "exist", "road_types", "slot_gid")
FLOAT_FIELDS = ("st12", "goal5", "road_pts")
GAP = 1e-9


def pre_of(tag):
    gp = golden("preprocessed")
    pre = {k[len(tag) + 5:]: gp[k] for k in gp.files if k.startswith(f"{tag}_pkl_")}
    pre["filtered_ag_ids"] = [int(i) for i in pre["filtered_ag_ids"]]
    return pre


def flat(wins):
    c = OpenLoopEvaluator.collate(wins)
    return {**c["agent"], **c["map"]}


def host_ctx(d, wins):
    """ctx_from_reference_layout(collate(windows)) as loss_sums prepares it -> {field: array}, moving [B,A] u8."""
    arrs = flat(wins)
    cb = ctx_from_reference_layout(d, arrs, d.T, DEV)
    cb.slot_gid.copy_(torch.arange(d.A, dtype=torch.int32, device=DEV).expand(len(wins), d.A))
    return fetch(cb, len(wins)), (arrs["moving_agent_mask"] != 0).astype(np.uint8)


def fetch(cb, B):
    torch.cuda.synchronize()
    return {f: getattr(cb, f)[:B].cpu().numpy() for f in CtxBuffers.FIELDS}


def compare(got, mv, ref, ref_mv, tag=""):
    """EVERY element of every tensor, padded slots included."""
    for f in INT_FIELDS:
        assert got[f].shape == ref[f].shape and np.array_equal(got[f], ref[f]), f"{tag} {f}"
    assert np.array_equal(got["st12"][..., 7:], ref["st12"][..., 7:]), f"{tag} types"
    assert np.array_equal(np.asarray(mv), ref_mv), f"{tag} moving"
    worst = 0.0
    for f in FLOAT_FIELDS:
        worst = max(worst, float(np.abs(got[f].astype(np.float64) - ref[f]).max()))
        np.testing.assert_allclose(got[f], ref[f], atol=ATOL, rtol=RTOL, err_msg=f"{tag} {f}")
    return worst


def identical(got, ref):
    """Names of the tensors whose bits differ (as integers: NaN patterns and signed zeros count)."""
    return [f for f in CtxBuffers.FIELDS if not np.array_equal(got[f].view(np.int32), ref[f].view(np.int32))]


def ranking_gaps(pre, cfg, origin_t, origin_agent):
    """Smallest gap between adjacent keys of the two rankings of one window as the host form evaluates them: (agents — distances, and the
    distance threshold among them —, polylines — inf when nothing is ranked)."""
    w = cfg.dataset.waymo
    ag = np.asarray(pre["ag_data"], np.float64)
    fil = list(pre["filtered_ag_ids"])
    st = ag[fil, origin_t]
    dist = np.linalg.norm(st[origin_agent, :2].reshape(1, -1) - st[:, :2], axis=-1)
    ga = float(np.diff(np.sort(np.concatenate([dist, [w.agent_dist_threshold]]))).min())
    rp = np.array(pre["road_points"], np.float64)
    if len(rp) <= w.max_num_road_polylines:
        return ga, float("inf")
    yaw = st[origin_agent, 4]
    rot = (np.pi / 2) + np.sign(-yaw) * np.abs(yaw)
    xy = ingest._se2(rp[:, :, :2], st[origin_agent, :2][None, None, :], rot)
    keys = (np.linalg.norm(xy, axis=-1) * rp[:, :, -1]).max(1)
    return ga, float(np.diff(np.sort(keys)).min())


# ---------------------------------------------------------------------------------------------- 1. the reference's own windows
def _golden_window(g, key):
    return {k: g[f"win_{key}_{k}"] for k in ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask",
                                             "road_points", "road_types")}


def test_reference_windows_from_the_reference_dictionaries():
    """tests/golden/loss.npz win_{a0,a1,b0,b1,c0,c1}: what the reference's training-mode get_data returned for the dictionaries of
    preprocessed.npz and the recorded draws.  Scene a (8 agents, 20 polylines > P) is one dataset; b and c (10 agents; 9 < P and
    12 == P polylines) share ONE: per-scene polyline counts, the padding branch, the boundary and rows beyond a scene's count."""
    g = golden("loss")
    cfg = cfg_of("loop")
    d = spec.Dims(cfg)
    pres = {t: pre_of(t) for t in "abc"}
    assert [len(pres[t]["road_points"]) for t in "abc"] == [20, 9, 12] and d.P == 12
    ds_a = DeviceDataset.from_dicts(cfg, [pres["a"]], DEV)
    ds_bc = DeviceDataset.from_dicts(cfg, [pres["b"], pres["c"]], DEV)
    # rows beyond scene b's count hold a pattern the output must never show
    ds_bc.road_points[0, 9:] = 12345.0
    ds_bc.road_types[0, 9:] = 7.0
    for ds, keys, scn in ((ds_a, ("a0", "a1"), (0, 0)), (ds_bc, ("b0", "b1", "c0", "c1"), (0, 0, 1, 1))):
        draws = np.array([g[f"win_{k}_draws"] for k in keys])
        for k, (t0, a0) in zip(keys, draws):
            ga, gp = ranking_gaps(pres[k[0]], cfg, int(t0), int(a0))
            assert ga > GAP and gp > GAP, (k, ga, gp)
        cb, mv = build_windows(ds, scn, draws[:, 0], draws[:, 1])
        got = fetch(cb, len(keys))
        assert (cb.status.cpu().numpy() == 0).all()
        ref, ref_mv = host_ctx(d, [_golden_window(g, k) for k in keys])
        worst = compare(got, mv.cpu().numpy(), ref, ref_mv, "/".join(keys))
        print(f"{'/'.join(keys)}: largest float deviation from the reference's windows {worst:.3g}")


# ---------------------------------------------------------------------------------------------- 2. the host form, a generated batch
STEPS = 24


@pytest.fixture(scope="module")
def generated():
    """3 synthetic scenes x 12 vehicles x 24 steps (14, 9 and 20 polylines against P = 12) rolled by LogReplayer, with the log cuts of
    replay_utils._cut_logs: vehicle 3 is absent at step 0 (filtered index != vehicle id), vehicles 1, 2 and 4 leave at steps 6 .. 11."""
    cfg = cfg_of("loop")
    d = spec.Dims(cfg)
    scns = [scenarios.make_scenario(31, k, n_agents=12, n_polylines=n, n_points=d.NP, extent=40.0) for k, n in enumerate((14, 9, 20))]
    logs = []
    for k, scn in enumerate(scns):
        lg = scenarios.standin_log(scn, STEPS + 1)
        for v in range(scn.N):
            lg[v]["traj"] = _cut_logs(k, v, lg[v]["traj"].copy())
        logs.append(lg)
    rp = datagen.LogReplayer(cfg, DEV).load(scns, logs, STEPS)
    rp.run()
    out = rp.dataset()
    ds = rp.device_dataset(out, scns)
    dicts = datagen.read_back(rp, out, scns)
    return dict(cfg=cfg, d=d, ds=ds, dicts=dicts)


def _all_valid(ds, s, steps):
    fil = ds.filtered[s]
    return [(s, t, a) for t in steps for a in range(len(fil)) if ds.exist_is_one[s, fil[a], t] and ds.moving[s, fil[a]]]


def test_generated_batch_equals_the_host_form_everywhere(generated):
    cfg, d, ds, dicts = (generated[k] for k in ("cfg", "d", "ds", "dicts"))
    w = cfg.dataset.waymo
    assert (ds.S, ds.N, ds.Td, ds.Pmax) == (3, 12, STEPS, 20) and list(ds.n_polys_h) == [14, 9, 20]
    # the wrapped tensors are the dictionaries' arrays, and the tables the host form's
    for s, pre in enumerate(dicts):
        back = ds.scene_dict(s)
        for k in ("ag_data", "ag_actions", "rtgs", "ag_types", "ag_goals", "road_points", "road_types", "last_exist_timesteps"):
            assert np.array_equal(back[k], np.asarray(pre[k], np.float64)), k
        assert back["filtered_ag_ids"] == list(pre["filtered_ag_ids"]) and 3 not in back["filtered_ag_ids"]
        assert ds.max_t[s] == ingest._window_tables(pre, cfg)[4] == STEPS - d.T
        assert ds.choices(s, 7) == ingest.window_choices(pre, cfg, 7)
    triples = [t for s in range(3) for t in _all_valid(ds, s, (0, 5, 8, int(ds.max_t[s])))]
    # what the batch must exercise, asserted on the host
    cuts = beyond = ends = 0
    for s, t0, a in triples:
        pre, fil = dicts[s], ds.filtered[s]
        ga, gp = ranking_gaps(pre, cfg, t0, a)
        assert ga > GAP and gp > GAP, (s, t0, a, ga, gp)
        st = pre["ag_data"][fil, t0]
        dist = np.linalg.norm(st[a, :2] - st[:, :2], axis=-1)
        near = dist < w.agent_dist_threshold
        cuts += near.sum() > d.A                                                  # the ranking cuts
        beyond += (~near).any()                                                   # somebody beyond 60 m
        chosen = np.intersect1d(np.argsort(dist)[:d.A], np.where(near)[0])
        ex = pre["ag_data"][np.asarray(fil)[chosen], t0:t0 + d.T, 7]
        ends += ((ex[:, 0] == 1) & (ex[:, -1] == 0)).any()                        # an existence that ends inside the window
    assert cuts > 0 and beyond > 0 and ends > 0 and any(t0 == ds.max_t[s] for s, t0, _ in triples)
    assert any(fil_a != ds.filtered[s][fil_a] for s, _, fil_a in triples)
    tr = np.array(triples)
    cb, mv = build_windows(ds, tr[:, 0], tr[:, 1], tr[:, 2])
    got = fetch(cb, len(tr))
    assert (cb.status.cpu().numpy() == 0).all()
    wins = [ingest.training_window(dicts[s], cfg, t0, a) for s, t0, a in triples]
    ref, ref_mv = host_ctx(d, wins)
    worst = compare(got, mv.cpu().numpy(), ref, ref_mv, "generated batch")
    print(f"{len(tr)} windows of a generated batch: largest float deviation from the host form {worst:.3g}; tensors with differing bits: "
          f"{identical(got, ref) or 'none'}")


# ---------------------------------------------------------------------------------------------- 3. ties
def _tie_dict(cfg):
    """One hand-made scene: 9 agents, origin = agent 0 at (0, 0); agents 3 and 6 sit at (3, 4) and (-3, 4), both EXACTLY 5 m away, at
    ranks A - 1 and A of the distance order (four agents are nearer, two farther).  16 polylines of which rows 4 and 11 are identical
    (different types) with exactly P - 1 polylines nearer."""
    w = cfg.dataset.waymo
    T, A, P, NP = int(w.train_context_length), int(w.max_num_agents), int(w.max_num_road_polylines), int(w.max_num_road_pts_per_polyline)
    assert (A, P) == (6, 12)
    N, Td = 9, T + 2
    xy = np.array([[0, 0], [1, 0], [0, 2], [3, 4], [-2, 1], [0, -3], [-3, 4], [20, 0], [40, 9]], np.float64)
    # distances: 0, 1, 2, 5, sqrt 5, 3, 5, 20, 41 -> order 0, 1, 2, 4, 5 | 3 = 6 | 7, 8: the tie is at ranks 5 and 6 (A = 6)
    ag = np.zeros((N, Td, 8))
    ag[:, :, :2] = xy[:, None]
    ag[:, :, 2:4] = [1.0, 0.5]
    ag[:, :, 4] = 0.3 + 0.1 * np.arange(N)[:, None]
    ag[:, :, 5:7] = [4.5, 2.0]
    ag[:, :, 7] = 1.0
    goals = np.zeros((N, Td, 5))
    goals[:, :, :2] = xy[:, None] + 30.0
    goals[:, :, 4] = 0.2
    rs = np.random.RandomState(5)
    n_pl = 16
    rp = np.zeros((n_pl, NP, 3))
    radius = np.array([10, 20, 30, 40, 0, 50, 60, 70, 80, 90, 100, 0, 110, 300, 310, 320], np.float64)
    radius[[4, 11]] = 120.0                                                      # 11 polylines nearer, 3 farther
    for p in range(n_pl):
        ang = np.linspace(0.1, 0.5, NP) + 0.05 * (p if p != 11 else 4)
        rp[p, :, 0], rp[p, :, 1], rp[p, :, 2] = radius[p] * np.cos(ang), radius[p] * np.sin(ang), 1.0
    assert np.array_equal(rp[4], rp[11])
    rt = np.eye(8)[rs.randint(3, 8, n_pl)]                                       # types 1 and 2 mark the twins alone
    rt[4], rt[11] = np.eye(8)[1], np.eye(8)[2]
    return dict(ag_data=ag, ag_actions=rs.uniform(-2, 2, (N, Td, 2)), ag_types=np.eye(5)[np.ones(N, int)], ag_goals=goals,
                ag_rewards=rs.uniform(0, 0.1, (N, Td, 8)), veh_edge_dist_rewards=rs.uniform(-0.5, 0.5, (N, Td)),
                veh_veh_dist_rewards=rs.uniform(0, 1, (N, Td)), last_exist_timesteps=np.full(N, Td - 1), road_points=rp, road_types=rt,
                filtered_ag_ids=list(range(N)))


def test_ties_go_to_the_lower_index(monkeypatch):
    cfg = cfg_of("loop")
    d = spec.Dims(cfg)
    pre = _tie_dict(cfg)
    fil_xy = pre["ag_data"][:, 1, :2]
    dist = np.linalg.norm(fil_xy[0] - fil_xy, axis=-1)
    order = np.argsort(dist, kind="stable")
    assert dist[3] == dist[6] == 5.0 and list(order[d.A - 1:d.A + 1]) == [3, 6]
    ds = DeviceDataset.from_dicts(cfg, [pre], DEV)
    cb, mv = build_windows(ds, [0], [1], [0])
    got = fetch(cb, 1)
    # the expectation: the host form with a STABLE argsort (NumPy's default promises nothing about ties)
    real = np.argsort
    monkeypatch.setattr(np, "argsort", lambda a, *args, **kw: real(a, *args, **{**kw, "kind": "stable"}))
    win = ingest.training_window(pre, cfg, 1, 0)
    monkeypatch.undo()
    ref, ref_mv = host_ctx(d, [win])
    compare(got, mv.cpu().numpy(), ref, ref_mv, "ties")
    # said directly: slots = agents 0, 1, 2, 3, 4, 5 (agent 3 and not 6: their headings tell them apart) ...
    rot = np.pi / 2 - pre["ag_data"][0, 1, 4]
    want_heading = [float(ingest._angle_sub(np.float64(pre["ag_data"][v, 1, 4]), -rot)) for v in (0, 1, 2, 3, 4, 5)]
    np.testing.assert_allclose(got["st12"][0, 0, :, 4], want_heading, atol=ATOL)
    # ... and the last output row is polyline 4 (type 1); its twin 11 (type 2) is not in the window
    kinds = np.argmax(got["road_types"][0], axis=1)
    assert kinds[d.P - 1] == 1 and (kinds[:d.P - 1] >= 3).all()


# ---------------------------------------------------------------------------------------------- 4. Decision Transformer
def test_decision_transformer_returns_travel_as_float_bits(generated):
    cfg = cfg_of("loop", variant="decision_transformer")
    d = spec.Dims(cfg)
    assert d.VARIANT == 3
    dicts = generated["dicts"]
    ds = DeviceDataset.from_dicts(cfg, dicts, DEV)
    triples = [ds.choices(s, seed) for s in range(3) for seed in (1, 2)]
    tr = np.array([(s, t0, a) for s, (t0, a) in zip((0, 0, 1, 1, 2, 2), triples)])
    cb, mv = build_windows(ds, tr[:, 0], tr[:, 1], tr[:, 2])
    got = fetch(cb, len(tr))
    wins = [ingest.training_window(dicts[s], cfg, t0, a) for s, t0, a in tr]
    assert all(w["rtgs"].dtype == np.float64 and (w["rtgs"] != np.round(w["rtgs"])).any() for w in wins)      # continuous
    ref, ref_mv = host_ctx(d, wins)
    compare(got, mv.cpu().numpy(), ref, ref_mv, "decision transformer")
    want = np.stack([w["rtgs"] for w in wins]).transpose(0, 2, 1, 3).astype(np.float32)
    assert np.array_equal(got["rtg_bin"].view(np.float32), want)


# ---------------------------------------------------------------------------------------------- 5. refusals and the guard
INT_PATTERN = 0x5A5A5A5A


def _poisoned(d, B):
    cb = CtxBuffers(d, B, DEV)
    for f in CtxBuffers.FIELDS:
        t = getattr(cb, f)
        t.fill_(float("nan") if t.dtype == torch.float32 else INT_PATTERN)
    return cb


def test_refused_triples_raise_on_the_host_and_pad_on_the_device():
    cfg = cfg_of("loop")
    d = spec.Dims(cfg)
    w = cfg.dataset.waymo
    pres = [pre_of("b"), pre_of("c")]
    # scene c's first filtered agent stands on its goal: it exists, but does not move
    still = pres[1]["filtered_ag_ids"][0]
    pres[1]["ag_goals"] = pres[1]["ag_goals"].copy()
    pres[1]["ag_goals"][still, :, :2] = pres[1]["ag_data"][still, 0, :2]
    ds = DeviceDataset.from_dicts(cfg, pres, DEV)
    assert not ds.moving[1, still] and ds.exist_is_one[1, still, 0]
    fil0 = ds.filtered[0]
    gone = [(t, a) for t in range(int(ds.max_t[0]) + 1) for a in range(len(fil0)) if not ds.exist_is_one[0, fil0[a], t] and ds.moving[0, fil0[a]]]
    assert gone, "scene b holds a filtered agent that leaves"
    t_gone, a_gone = gone[0]
    ok = [(0,) + ds.choices(0, 1), (1,) + ds.choices(1, 2), (0,) + ds.choices(0, 3)]
    bad = [((2, 0, 0), 1, "scene 2 outside"), ((-1, 0, 0), 1, "scene -1 outside"),
           ((0, -1, 0), 2, "origin_t -1 outside"), ((0, ds.Td - d.T + 1, 0), 2, "origin_t"), ((1, 10 ** 9, 0), 2, "origin_t"),
           ((0, 0, len(fil0)), 3, "origin_agent"), ((0, 0, -1), 3, "origin_agent -1 outside"),
           ((0, t_gone, a_gone), 4, "must move and exist"), ((1, 0, 0), 5, "must move and exist")]
    for tr, _, msg in bad:
        with pytest.raises(ValueError, match=msg):
            ds.validate(*tr)
        with pytest.raises(ValueError, match=msg):
            build_windows(ds, [ok[0][0], tr[0]], [ok[0][1], tr[1]], [ok[0][2], tr[2]])
    # one launch around validate(): valid and refused triples interleaved, into buffers full of a pattern, one window more than launched
    mixed = [ok[0]] + [b[0] for b in bad[:4]] + [ok[1]] + [b[0] for b in bad[4:]] + [ok[2]]
    want_status = [0] + [b[1] for b in bad[:4]] + [0] + [b[1] for b in bad[4:]] + [0]
    B = len(mixed)
    up = lambda k: torch.tensor([m[k] for m in mixed], dtype=torch.int32, device=DEV)
    cb, mv, status = launch_windows(ds, up(0), up(1), up(2), B, out=_poisoned(d, B + 1))
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == want_status
    full = {f: getattr(cb, f).cpu().numpy() for f in CtxBuffers.FIELDS}
    for f, a in full.items():
        a = a.view(np.int32)
        pat = np.float32("nan").view(np.int32) if getattr(cb, f).dtype == torch.float32 else INT_PATTERN
        assert (a[B] == pat).all(), f"{f}: written beyond the launched windows"
        assert not np.isnan(full[f][:B].astype(np.float64)).any() and not (a[:B] == INT_PATTERN).any(), f"{f}: an element was left unwritten"
    mv = mv.cpu().numpy()
    # the valid windows are what a launch without the refused ones gives, bit for bit
    cb2, mv2 = build_windows(ds, [m[0] for m in ok], [m[1] for m in ok], [m[2] for m in ok], out=_poisoned(d, 3))
    alone = fetch(cb2, 3)
    pos = [i for i, st in enumerate(want_status) if st == 0]
    for f in CtxBuffers.FIELDS:
        assert np.array_equal(full[f][pos].view(np.int32), alone[f].view(np.int32)), f
    assert np.array_equal(mv[pos], mv2.cpu().numpy())
    ref, ref_mv = host_ctx(d, [ingest.training_window(pres[s], cfg, t, a) for s, t, a in ok])
    compare(alone, mv2.cpu().numpy(), ref, ref_mv, "valid among refused")
    # the refused ones are all padding
    from ctrlsim_amd.discretize import discretize_actions
    zero_tok = int(discretize_actions(np.zeros(2), w))
    for i in (i for i, st in enumerate(want_status) if st != 0):
        assert (full["st12"][i][..., :7] == 0).all() and (full["st12"][i][..., 7:] == -1).all()
        assert (full["exist"][i] == 0).all() and (full["goal5"][i] == 0).all() and (full["act_tok"][i] == zero_tok).all()
        assert (full["rtg_bin"][i] == 0).all() and (full["tstep"][i] == 0).all()
        assert (full["road_pts"][i] == 0).all() and (full["road_types"][i] == -1).all() and (mv[i] == 0).all()
        assert np.array_equal(full["slot_gid"][i], np.arange(d.A))


# ---------------------------------------------------------------------------------------------- 6. end to end
def test_evaluate_dataset_equals_evaluate_on_host_built_windows(generated):
    """Seven triples in chunks of 3, 3 and 1 against OpenLoopEvaluator.evaluate on the host-built windows in the same chunks.  Counts are
    exactly equal.  Sums: when the built context tensors are bit-identical to the host's for these inputs (checked and reported here) the
    two routes run the same kernels on the same bits, and the bound is the 1e-12 tests/test_gpu_loss.py uses between batchings of one
    entry point; otherwise its bound against the float64 restatement — (64 + 16) EPS (|lse| + |logit|) per row times the count, 1e-12
    for the state term — with the differing tensors named."""
    cfg, d, ds, dicts = (generated[k] for k in ("cfg", "d", "ds", "dicts"))
    model = CtRLSim(cfg, weights.generate_trained_like(d, 0), device=DEV)
    triples = [(s,) + ds.choices(s, seed) for s, seed in ((0, 1), (1, 2), (2, 3), (0, 4), (1, 5), (2, 6), (0, 7))]
    wins = [ingest.training_window(dicts[s], cfg, t0, a) for s, t0, a in triples]
    ev = OpenLoopEvaluator(cfg, model)
    host = ev.evaluate(wins, batch_size=3)
    devr = ev.evaluate_dataset(ds, triples, batch_size=3)
    assert list(devr) == list(host) and devr["windows"] == host["windows"] == 7 and devr["windows_per_s"] > 0
    assert devr["counts"] == host["counts"] and all(v > 0 for v in host["counts"].values())
    np.testing.assert_array_equal(devr["sums"][:, 1], host["sums"][:, 1])
    tr = np.array(triples)
    cb, mv = build_windows(ds, tr[:, 0], tr[:, 1], tr[:, 2])
    got = fetch(cb, 7)
    ref, ref_mv = host_ctx(d, wins)
    differing = identical(got, ref) + ([] if np.array_equal(mv.cpu().numpy(), ref_mv) else ["moving"])
    print(f"context tensors with bits that differ from the host's: {differing or 'none'}")
    for k in model.loss_keys():
        print(f"   {k}: device route {devr[k]:.12g} host route {host[k]:.12g}")
    if not differing:
        np.testing.assert_allclose(devr["sums"], host["sums"], rtol=1e-12, atol=0)
        return
    names = {f: int((got[f].view(np.int32) != ref[f].view(np.int32)).sum()) for f in differing if f != "moving"}
    data = {"agent": {k: np.stack([w[k] for w in wins]) for k in ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps",
                                                                  "moving_agent_mask")},
            "map": {k: np.stack([w[k] for w in wins]) for k in ("road_points", "road_types")}}
    preds = {k: v.cpu().numpy() for k, v in model(data).items() if v is not None}
    m = cfg.model
    row = loss_ref.loss_sums({**data["agent"], **data["map"]}, preds, R=d.R, C=d.C, supervise_moving=bool(m.get("supervise_moving", True)),
                             local_frame=bool(m.get("local_frame_predictions", False)))["row"]
    ok = np.isfinite(row[..., 0])
    rb = float((80.0 * 2.0 ** -23 * (np.abs(row[..., 0]) + np.abs(row[..., 1])))[ok].max())
    for k in model.loss_keys():
        i = loss_ref.KEYS.index(k)
        s_d, s_h, n = devr["sums"][i, 0], host["sums"][i, 0], host["sums"][i, 1]
        tol = 1e-12 * abs(s_h) if i == 4 else rb * max(n, 1)
        assert abs(s_d - s_h) <= tol, f"{k}: {s_d} against {s_h}, bound {tol}; elements with differing bits per tensor: {names}"


# ---------------------------------------------------------------------------------------------- 7. two streams
def test_two_streams_at_once_equal_the_single_stream_results(generated):
    """Two launches on two streams, different triples, issued back to back: each equals the same launch made alone, bit for bit (the
    ranking keys of a launch live in its own workgroups' LDS, not in a buffer that launches share)."""
    d, ds = generated["d"], generated["ds"]
    sets = [np.array(_all_valid(ds, s, (0, 3, 8))) for s in (0, 2)]
    alone = []
    for tr in sets:
        cb, mv = build_windows(ds, tr[:, 0], tr[:, 1], tr[:, 2])
        alone.append((fetch(cb, len(tr)), mv.cpu().numpy()))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    both = []
    for tr, st in zip(sets, streams):
        with torch.cuda.stream(st):
            both.append(build_windows(ds, tr[:, 0], tr[:, 1], tr[:, 2]))
    torch.cuda.synchronize()
    for tr, (a, amv), (cb, mv) in zip(sets, alone, both):
        b = fetch(cb, len(tr))
        assert not identical(a, b) and np.array_equal(amv, mv.cpu().numpy())
        assert (cb.status.cpu().numpy() == 0).all()
