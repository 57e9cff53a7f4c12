"""ctrlsim_build_context_c (csrc/context.hip: build_context_kernel) through the C ABI against a NumPy float64 restatement kept in this
file: the focal frame, the polyline keys `(norm * exist).max(1)`, a STABLE argsort of them (ascending key, ties to the lower polyline
index — what the kernel's rank rule says; the oracle's np.argsort is not stable, so tie cases are compared with this rule and only the
untied case with oracle/features_oracle.build_contexts), the gather and the agent / goal / timestep rows.  Every source polyline carries
a unique road_types row, so which polyline landed in which output row is visible exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import spec, _lib  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402
import features_oracle as fo  # noqa: E402
import sat_ref  # noqa: E402

FILL = 0xA5                       # byte pattern of every output buffer before a call
ZERO4 = (524, 0, 35, 35)          # placeholder token, zero-RTG bins
FIELDS = ("st12", "exist", "goal5", "act_tok", "rtg_bin", "tstep", "slot_gid", "road_pts", "road_types")
INT_FIELDS = ("act_tok", "rtg_bin", "tstep", "slot_gid")


def _dims(A, T, P, NP):
    return spec.Dims(spec.make_cfg(dataset__waymo__max_num_agents=A, dataset__waymo__train_context_length=T,
                                   dataset__waymo__max_num_road_polylines=P, dataset__waymo__max_num_road_pts_per_polyline=NP))


def make_inputs(seed, S, N, Tmax, P_all, NP, extents):
    """Random scenes: scenario s spreads its vehicles over extents[s] metres (a small extent gives few focal groups, a large one many);
    some vehicles do not exist at some steps; polyline points in a 200 m box with a random existence flag, >= 1 existing point each."""
    rs = np.random.RandomState(seed)
    hs = np.zeros((S, N, Tmax + 1, 8), np.float32)
    for s in range(S):
        hs[s, :, :, 0:2] = (rs.uniform(-extents[s], extents[s], (N, 1, 2)) + rs.normal(0, 0.5, (N, Tmax + 1, 2)).cumsum(1)).astype(np.float32)
    hs[..., 2:4] = rs.normal(0, 3, (S, N, Tmax + 1, 2))
    hs[..., 4] = rs.uniform(-np.pi, np.pi, (S, N, Tmax + 1))
    hs[..., 5] = rs.uniform(4, 5.5, (S, N, 1)); hs[..., 6] = rs.uniform(1.8, 2.3, (S, N, 1))
    hs[..., 7] = rs.uniform(size=(S, N, Tmax + 1)) < 0.9
    hs[:, 0, :, 7] = 1                                   # vehicle 0 always exists: every scenario has a group
    hs[:, 0, 0, 4] = (0.0, -1.0, 2.0, 3.0)[:S] if S <= 4 else rs.uniform(-3, 3, S)     # sign(-yaw) of 0, > 0, < 0
    tok = rs.randint(0, 500, (S, N, Tmax)).astype(np.int32)
    rtg = rs.randint(0, 70, (S, N, Tmax, 3)).astype(np.int32)
    goals = np.concatenate([rs.uniform(-100, 100, (S, N, 2)), rs.normal(0, 3, (S, N, 2)), rs.uniform(-np.pi, np.pi, (S, N, 1))], -1)
    types = np.eye(5, dtype=np.float32)[rs.randint(0, 5, (S, N))]
    roads = np.zeros((S, P_all, NP, 3), np.float32)
    roads[..., :2] = rs.uniform(-100, 100, (S, P_all, NP, 2))
    roads[..., 2] = rs.uniform(size=(S, P_all, NP)) < 0.8
    roads[:, :, 0, 2] = 1
    rtypes = np.zeros((S, P_all, 8), np.float32)         # unique per (scenario, polyline): identifies the source of an output row
    rtypes[..., 0] = np.arange(P_all)[None]; rtypes[..., 1] = np.arange(S)[:, None]
    rtypes[..., 2:] = rs.randint(0, 2, (S, P_all, 6))
    order = np.stack([rs.permutation(N) for _ in range(S)]).astype(np.int32)
    order[:, N - N // 4:] = -1                           # not every vehicle is evaluated
    return dict(hs=hs, tok=tok, rtg=rtg, goals=goals, types=types, roads=roads, rtypes=rtypes, order=order)


class Prepared:
    """Inputs on the device, focal groups and the class-sorted context list of all S scenarios (synchronised)."""

    def __init__(self, inp, A, T, t, sizes):
        lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
        S, N, Tmax1 = inp["hs"].shape[:3]
        self.inp, self.S, self.N, self.Tmax, self.A, self.T, self.t, self.sizes = inp, S, N, Tmax1 - 1, A, T, t, list(sizes)
        self.d = {k: dev(v) for k, v in inp.items()}
        i32 = lambda *s: torch.full(s, -9, dtype=torch.int32, device=DEV)
        self.n_groups, self.grp_focal, self.own_g, self.mem_g = i32(S), i32(S, N), i32(S, N), i32(S, N)
        self.grp_ids = torch.zeros(S, N, dtype=torch.int64, device=DEV)
        members, persist = torch.zeros_like(self.grp_ids), torch.zeros_like(self.grp_ids)
        tilted = torch.zeros(S, N, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ctrlsim_group_build(S, N, A, T, t, Tmax1, 60.0, p(self.d["hs"]), p(self.d["order"]), 1, p(persist), p(self.n_groups),
                                           p(self.grp_focal), p(self.grp_ids), p(members), p(self.own_g), p(self.mem_g), p(tilted), st))
        torch.cuda.synchronize()
        ng = self.n_groups.cpu().numpy()
        ids = self.grp_ids.cpu().numpy().view(np.uint64)
        n_ctx = int(ng.sum())
        self.ctx_scn, self.ctx_grp, row0 = i32(n_ctx + 4), i32(n_ctx + 4), i32(n_ctx + 4)
        sv = [i32(S, N) for _ in range(5)]
        _lib.check(lib.ctrlsim_ctx_index_classes(0, S, N, A, p(self.n_groups), p(self.grp_ids), p(self.own_g), p(self.mem_g), len(sizes),
                                                 (C.c_int * len(sizes))(*sizes), p(self.ctx_scn), p(self.ctx_grp), p(row0), *[p(x) for x in sv], st))
        torch.cuda.synchronize()
        self.n_ctx, self.ng = n_ctx, ng
        self.scn, self.grp = self.ctx_scn.cpu().numpy()[:n_ctx], self.ctx_grp.cpu().numpy()[:n_ctx]
        self.focal = self.grp_focal.cpu().numpy()[self.scn, self.grp]
        self.ids = [[v for v in range(N) if (int(ids[s, g]) >> v) & 1] for s, g in zip(self.scn, self.grp)]
        cls = [sat_ref.size_class(len(i), self.sizes) for i in self.ids]
        assert cls == sorted(cls)                        # the list is sorted by class
        self.B = [cls.count(k) for k in range(len(sizes))]


def per_ctx(A, Tn, P, NP):
    return dict(st12=Tn * A * 12, exist=Tn * A, goal5=A * 5, act_tok=Tn * A, rtg_bin=Tn * A * 3, tstep=Tn, slot_gid=A,
                road_pts=P * NP * 3, road_types=P * 8)


def launch(pr, P, NP, Tq, tt_first, stream=None, pad=2):
    """One ctrlsim_build_context_c call for all classes into pattern-filled buffers of B_k + pad contexts each; no synchronise."""
    lib, p = _lib.lib(), _lib.ptr
    st = _lib.stream_ptr() if stream is None else stream.cuda_stream
    n, Tn, d = len(pr.sizes), Tq - tt_first, pr.d
    bufs = []
    for B, A in zip(pr.B, pr.sizes):
        sz = per_ctx(A, Tn, P, NP)
        bufs.append({k: torch.full(((B + pad) * sz[k] * 4,), FILL, dtype=torch.uint8, device=DEV) for k in FIELDS})
    cs = (_lib.Ctx * n)(*[_lib.Ctx(*(b[k].data_ptr() for k in FIELDS)) for b in bufs])
    P_all = pr.inp["roads"].shape[1]
    _lib.check(lib.ctrlsim_build_context_c(n, (C.c_int * n)(*pr.B), (C.c_int * n)(*pr.sizes), cs, pr.N, pr.T, pr.t, Tq, tt_first,
                                           pr.Tmax + 1, pr.Tmax, P_all, P, NP, p(pr.ctx_scn), p(pr.ctx_grp), p(pr.grp_focal),
                                           p(pr.grp_ids), p(d["hs"]), p(d["tok"]), p(d["rtg"]), p(d["goals"]), p(d["types"]),
                                           p(d["roads"]), p(d["rtypes"]), (C.c_int * 4)(*ZERO4), st))
    return bufs


def fetch(pr, bufs, P, NP, Tn):
    """Per class: dict of arrays [B, ...]; asserts that everything beyond the B contexts of a class kept the fill pattern."""
    out = []
    for B, A, b in zip(pr.B, pr.sizes, bufs):
        sz = per_ctx(A, Tn, P, NP)
        o = {}
        for k in FIELDS:
            raw = b[k].cpu().numpy()
            assert (raw[B * sz[k] * 4:] == FILL).all(), (k, A, "written beyond the class's contexts")
            o[k] = raw[:B * sz[k] * 4].view(np.int32 if k in INT_FIELDS else np.float32).reshape(B, sz[k])
        out.append(o)
    return out


def reference(pr, P, NP, Tq, tt_first):
    """The float64 restatement, per class the same dict of arrays as fetch() (float64 where the kernel rounds to float32)."""
    inp, t, T, Tmax = pr.inp, pr.t, pr.T, pr.Tmax
    w0 = 0 if t < T else t - (T - 1)
    Tn = Tq - tt_first
    out, c = [], 0
    min_gap = np.inf
    for B, A in zip(pr.B, pr.sizes):
        o = dict(st12=np.zeros((B, Tn, A, 12)), exist=np.zeros((B, Tn, A)), goal5=np.zeros((B, A, 5)),
                 act_tok=np.zeros((B, Tn, A), np.int32), rtg_bin=np.zeros((B, Tn, A, 3), np.int32), tstep=np.zeros((B, Tn), np.int32),
                 slot_gid=np.full((B, A), -1, np.int32), road_pts=np.zeros((B, P, NP, 3)), road_types=np.full((B, P, 8), -1.0))
        for b in range(B):
            s, ids, focal = pr.scn[c], pr.ids[c], pr.focal[c]
            c += 1
            n = len(ids)
            f0 = inp["hs"][s, focal, w0].astype(np.float64)
            yaw = f0[4]
            rot = (np.pi / 2) + np.sign(-yaw) * np.abs(yaw)
            cr, sr, tx, ty = np.cos(rot), np.sin(rot), f0[0], f0[1]
            rows = slice(w0 + tt_first, w0 + Tq)
            raw = np.zeros((A, Tn, 8)); raw[:n] = inp["hs"][s, ids, rows].astype(np.float64)
            ty5 = -np.ones((A, 5)); ty5[:n] = inp["types"][s, ids]
            px, py = raw[..., 0] - tx, raw[..., 1] - ty
            st = np.zeros((A, Tn, 12))
            st[..., 0] = cr * px + (-sr) * py; st[..., 1] = sr * px + cr * py
            st[..., 2] = cr * raw[..., 2] + (-sr) * raw[..., 3]; st[..., 3] = sr * raw[..., 2] + cr * raw[..., 3]
            st[..., 4] = fo.angle_sub_array(raw[..., 4], -rot)
            st[..., 5:7] = raw[..., 5:7]; st[..., 7:] = ty5[:, None]
            o["st12"][b] = st.transpose(1, 0, 2); o["exist"][b] = raw[..., 7].T
            gr = np.zeros((A, 5)); gr[:n] = inp["goals"][s, ids]
            gx, gy = gr[:, 0] - tx, gr[:, 1] - ty
            o["goal5"][b] = np.stack([cr * gx + (-sr) * gy, sr * gx + cr * gy, cr * gr[:, 2] + (-sr) * gr[:, 3],
                                      sr * gr[:, 2] + cr * gr[:, 3], fo.angle_sub_array(gr[:, 4], -rot)], -1)
            for to in range(Tn):
                abs_t = w0 + tt_first + to
                o["tstep"][b, to] = abs_t if abs_t <= t else 0
                o["act_tok"][b, to] = ZERO4[0]
                if abs_t < Tmax:
                    o["act_tok"][b, to, :n] = inp["tok"][s, ids, abs_t]; o["rtg_bin"][b, to, :n] = inp["rtg"][s, ids, abs_t]
                else:
                    o["rtg_bin"][b, to, :n] = ZERO4[1:]
            o["slot_gid"][b, :n] = ids
            pts = inp["roads"][s].astype(np.float64)
            rx, ry = pts[..., 0] - tx, pts[..., 1] - ty
            x, y = cr * rx + (-sr) * ry, sr * rx + cr * ry
            P_all = len(pts)
            if P_all > P:
                key = (np.sqrt(x * x + y * y) * pts[..., 2]).max(1)
                keep = np.argsort(key, kind="stable")[:P]
                gaps = np.diff(np.sort(key))
                if (gaps > 0).any():
                    min_gap = min(min_gap, gaps[gaps > 0].min())
            else:
                keep = np.arange(P_all)
            o["road_pts"][b, :len(keep)] = np.stack([x[keep], y[keep], pts[keep, :, 2]], -1)
            o["road_types"][b, :len(keep)] = inp["rtypes"][s, keep]
        out.append({k: v.reshape(B, per_ctx(A, Tn, P, NP)[k]) for k, v in o.items()})
    assert c == pr.n_ctx
    assert min_gap > 1e-9, min_gap                       # no near-tie: a libm ulp in the frame cannot reorder the reference
    return out


def compare(got, ref):
    for k, (g, r) in enumerate(zip(got, ref)):
        for f in INT_FIELDS + ("exist", "road_types"):
            assert np.array_equal(g[f], r[f].astype(g[f].dtype)), (k, f)
        for f in ("st12", "goal5", "road_pts"):
            r32 = r[f].astype(np.float32)
            np.testing.assert_allclose(g[f], r32, atol=2e-5, rtol=1e-6, err_msg=f"class {k} {f}")
            if g[f].size:
                assert (g[f] == r32).mean() >= 0.99, (k, f, (g[f] == r32).mean())


def run(inp, A, T, P, NP, t, Tq=None, tt_first=0, sizes=None):
    sizes = [1, 3, 4, A] if sizes is None else sizes      # class 0 (one slot) is always empty: a context holds its focal vehicle
    Tq = T if Tq is None else Tq
    pr = Prepared(inp, A, T, t, sizes)
    assert pr.B[0] == 0 and sum(b > 0 for b in pr.B) >= 2 and len(set(pr.ng)) > 1, (pr.B, pr.ng)
    bufs = launch(pr, P, NP, Tq, tt_first)
    torch.cuda.synchronize()
    got = fetch(pr, bufs, P, NP, Tq - tt_first)
    ref = reference(pr, P, NP, Tq, tt_first)
    compare(got, ref)
    return pr, got, ref


EXTENTS = (15.0, 60.0, 150.0, 400.0)


@pytest.mark.parametrize("P_all,P,NP", [(12, 12, 10), (7, 12, 10), (13, 12, 10), (67, 12, 10), (203, 40, 100), (203, 40, 17), (512, 200, 100)])
def test_polyline_counts(P_all, P, NP):
    """P_all = P and P_all < P (no selection, zero / -1 padding rows), P + 1, counts that are no multiple of 64 or of the lane groups of
    the key sweep, the bench's 200 of 512; NP = 100 (no multiple of 64), 17 (one over the 16 lanes of a polyline) and 10 (fewer)."""
    d = _dims(6, 8, P, NP)
    inp = make_inputs(P_all + NP, 4, 12, d.T + 8, P_all, d.NP, EXTENTS)
    pr, got, _ = run(inp, d.A, d.T, d.P, d.NP, t=3)
    if P_all < P:
        for g in got:
            rp, rt = g["road_pts"].reshape(-1, P, NP * 3), g["road_types"].reshape(-1, P, 8)
            assert (rp[:, P_all:] == 0).all() and (rt[:, P_all:] == -1).all()


@pytest.mark.parametrize("t,Tq,tt_first", [(0, None, 0), (3, None, 0), (13, None, 0), (5, 6, 4)])
def test_steps_and_window_rows(t, Tq, tt_first):
    """t in {0, 3, T + 5} with the whole window, and one call that emits rows [4, 6) of the window only (the cached steps' form): the
    excluded rows do not exist in the compact outputs, so everything behind the B x Tn rows must keep the fill pattern."""
    d = _dims(6, 8, 12, 10)
    assert d.T + 5 == 13
    inp = make_inputs(5, 4, 12, d.T + 8, 30, d.NP, EXTENTS)
    run(inp, d.A, d.T, d.P, d.NP, t=t, Tq=Tq, tt_first=tt_first)


def test_ties_and_polyline_content():
    """Exact duplicates inside the selection, several polylines without an existing point (key 0: the first rows, in index order), a
    polyline whose only existing point is its last, one whose farthest point does not exist (it contributes 0, not its distance)."""
    d = _dims(6, 8, 40, 100)
    inp = make_inputs(11, 4, 12, d.T + 8, 203, d.NP, EXTENTS)
    r = inp["roads"]
    r[:, 150] = r[:, 20]; r[:, 21] = r[:, 20]; r[:, 199] = r[:, 64]          # duplicates: (20, 21, 150) and (64, 199)
    r[:, [3, 70, 130, 202], :, 2] = 0                                        # no existing point: key 0
    r[:, 90, :, 2] = 0; r[:, 90, -1, 2] = 1                                  # only the last point exists ...
    r[:, 90, -1, :2] = r[:, 20, 0, :2]
    r[:, 91, :, :2] = np.float32(0.25) * r[:, 91, :, :2]                     # a polyline close to the origin ...
    r[:, 91, 37, :2] = (5000.0, -7000.0); r[:, 91, 37, 2] = 0                # ... whose farthest point does not exist
    pr, got, ref = run(inp, d.A, d.T, d.P, d.NP, t=3)
    for g in got:
        src = g["road_types"].reshape(-1, d.P, 8)[:, :, 0]
        assert (src[:, :4] == (3, 70, 130, 202)).all()
    # polyline 90 (only its last point exists, close to the vehicles of the narrow scenes): its key is that point's distance, not 0 —
    # it is selected somewhere, and never among the four leading key-0 rows
    where90 = [np.where(g["road_types"].reshape(-1, d.P, 8)[:, :, 0] == 90)[1] for g in got]
    assert sum(len(w) for w in where90) > 0 and all((w >= 4).all() for w in where90)
    # the far point must not have pushed polyline 91 out everywhere: with its distance as key it would never be selected
    assert any((g["road_types"].reshape(-1, d.P, 8)[:, :, 0] == 91).any() for g in got)


def test_duplicate_pair_straddling_the_selection_edge():
    """Scenarios 0 and 1, first context: the polylines of rank P - 1 and P are made exact duplicates, so the tie-break (lower index)
    decides which of the two is in the selection: the last output row holds the lower index, the higher one is not selected."""
    d = _dims(6, 8, 40, 100)
    inp = make_inputs(12, 4, 12, d.T + 8, 203, d.NP, EXTENTS)
    pr0 = Prepared(inp, d.A, d.T, 3, [1, 3, 4, d.A])
    picked = {}
    for s in (0, 1):
        c = int(np.where(pr0.scn == s)[0][0])
        f0 = inp["hs"][s, pr0.focal[c], 0].astype(np.float64)
        rot = (np.pi / 2) + np.sign(-f0[4]) * np.abs(f0[4])
        pts = inp["roads"][s].astype(np.float64)
        rx, ry = pts[..., 0] - f0[0], pts[..., 1] - f0[1]
        x, y = np.cos(rot) * rx + (-np.sin(rot)) * ry, np.sin(rot) * rx + np.cos(rot) * ry
        order = np.argsort((np.sqrt(x * x + y * y) * pts[..., 2]).max(1), kind="stable")
        a, b = int(order[d.P - 1]), int(order[d.P])
        inp["roads"][s, b] = inp["roads"][s, a]          # the pair now shares the key of rank P - 1
        picked[s] = (c, min(a, b), max(a, b))
    pr, got, ref = run(inp, d.A, d.T, d.P, d.NP, t=3)
    assert np.array_equal(pr.scn, pr0.scn) and np.array_equal(pr.grp, pr0.grp)
    first = np.cumsum([0] + pr.B)
    for s in (0, 1):
        c, lo, hi = picked[s]
        k = int(np.searchsorted(first, c, side="right") - 1)
        src = got[k]["road_types"].reshape(-1, d.P, 8)[c - first[k], :, 0]
        assert src[d.P - 1] == lo and hi not in src, (s, lo, hi, src[-3:])


def test_untied_case_agrees_with_the_oracle():
    """The restatement above against oracle/features_oracle.build_contexts (one scenario, full dims, nearest 200 of 260 polylines, no
    exact ties), then the kernel against the restatement."""
    cfg = spec.make_cfg()
    d, w = spec.Dims(cfg), cfg.dataset.waymo
    N, Tmax, t = 12, d.T + 8, 3
    inp = make_inputs(21, 1, N, Tmax, 260, d.NP, (60.0,))
    inp["order"][0] = np.arange(N)
    inp["hs"][..., 7] = 1
    sizes = [1, 8, 16, d.A]
    pr = Prepared(inp, d.A, d.T, t, sizes)
    bufs = launch(pr, d.P, d.NP, d.T, 0)
    torch.cuda.synchronize()
    got = fetch(pr, bufs, d.P, d.NP, d.T)
    ref = reference(pr, d.P, d.NP, d.T, 0)
    compare(got, ref)
    buf = fo.PolicyBuffers(N, Tmax)
    buf.states[:] = inp["hs"][0, :, :Tmax]; buf.types[:] = inp["types"][0]; buf.goals[:] = inp["goals"][0][:, None]
    buf.persisted = {v: [] for v in range(N)}
    groups, _ = fo.build_contexts(buf, w, t, list(range(N)), inp["roads"][0].astype(np.float64), inp["rtypes"][0])
    assert len(groups) == pr.n_ctx
    by_focal = {g["focal"]: g["data"] for g in groups}
    first = np.cumsum([0] + pr.B)
    for c in range(pr.n_ctx):
        k = int(np.searchsorted(first, c, side="right") - 1)
        A, b, dt = sizes[k], c - first[k], by_focal[int(pr.focal[c])]
        r = ref[k]
        assert np.array_equal(r["road_types"][b].reshape(d.P, 8), dt["road_types"][0])
        np.testing.assert_allclose(r["road_pts"][b].reshape(d.P, d.NP, 3), dt["road_points"][0], atol=1e-9, rtol=0)
        st = r["st12"][b].reshape(d.T, A, 12)
        np.testing.assert_allclose(st[:, :, :7], dt["agent_states"][0][:A, :, :7].transpose(1, 0, 2), atol=1e-9, rtol=0)
        np.testing.assert_allclose(r["goal5"][b].reshape(A, 5), dt["goals"][0][:A], atol=1e-9, rtol=0)


def test_two_streams_at_once_equal_the_single_stream_results():
    """One pair of calls on two streams, different scenarios, issued back to back: each result equals the result of the same call made
    alone, bit for bit (the selection keys of a call live in its own workgroups, not in a buffer that calls share)."""
    d = _dims(6, 8, 200, 100)
    prs = [Prepared(make_inputs(31 + i, 4, 12, d.T + 8, 512, d.NP, EXTENTS), d.A, d.T, 3, [1, 3, 4, d.A]) for i in range(2)]
    alone = []
    for pr in prs:
        b = launch(pr, d.P, d.NP, d.T, 0)
        torch.cuda.synchronize()
        alone.append(b)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    both = [launch(pr, d.P, d.NP, d.T, 0, stream=st) for pr, st in zip(prs, streams)]
    torch.cuda.synchronize()
    for pr, a, b in zip(prs, alone, both):
        for ka, kb in zip(a, b):
            for f in FIELDS:
                assert torch.equal(ka[f], kb[f]), f
        compare(fetch(pr, b, d.P, d.NP, d.T), reference(pr, d.P, d.NP, d.T, 0))
