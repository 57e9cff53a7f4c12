"""ctrlsim_group_build (csrc/context.hip: group_build_kernel) through the C ABI against tests/group_cases.group_ref, the plain restatement
of the loops it replaces: one call per step over all scenarios of a recipe, persist carried on the device, every table compared exactly
(n_groups, grp_focal / grp_ids / grp_members up to n_groups, own_g / mem_g / tilted / persist per vehicle) — integers and masks, no
tolerance.  Every output buffer is filled with a byte pattern before a call and has one scenario row more than the call covers.
tests/test_group_cases_host.py shows on the CPU that the restatement is the reference's and that this comparison tells ten wrong kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import _lib  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402
import group_cases as gc  # noqa: E402

EINVAL = -22                       # csrc/common.h: CTRLSIM_EINVAL
OUTPUTS = [k for k in gc.TABLES if k != "persist"]
TORCH = {np.int32: torch.int32, np.uint64: torch.int64, np.uint8: torch.uint8}


@pytest.fixture(scope="module")
def recipes():
    return {r["name"]: r for r in gc.all_recipes()}


@pytest.fixture(scope="module")
def runs(recipes):
    return {k: gc.run_recipe(r) for k, r in recipes.items()}


def outputs(S, N, fill):
    """Pattern-filled output tables of S + 1 scenarios."""
    o = {}
    for k in OUTPUTS:
        n = (S + 1) if k == "n_groups" else (S + 1) * N
        o[k] = torch.full((n * np.dtype(gc.DTYPES[k]).itemsize,), fill, dtype=torch.uint8, device=DEV).view(TORCH[gc.DTYPES[k]])
    return o


def persist_buffer(masks, N, fill):
    """[S + 1, N] u64 on the device: the incoming sets and a pattern-filled guard row."""
    S = len(masks)
    a = gc.filled((S + 1, N), np.uint64, fill)
    a[:S] = np.array(masks, dtype=np.uint64).reshape(S, N)
    return dev(a.view(np.int64))


def call(rec, t, hs, order, persist, o, S=None, s0=0, over=None):
    """ctrlsim_group_build of scenarios [s0, s0 + S) at step t (`over`: arguments replaced by name); returns the status, does not synchronise."""
    N, Tmax1 = rec["hs"].shape[1:3]
    S = rec["hs"].shape[0] if S is None else S
    a = dict(S=S, N=N, A=rec["A"], T=rec["T"], t=t, Tmax1=Tmax1, hist_states=hs[s0:].data_ptr(), eval_order=order[s0:].data_ptr(),
             persist=persist[s0:].data_ptr(), n_groups=o["n_groups"][s0:].data_ptr())
    a.update({k: o[k][s0 * N:].data_ptr() for k in OUTPUTS if k != "n_groups"})
    a.update(over or {})
    return _lib.lib().ctrlsim_group_build(a["S"], a["N"], a["A"], a["T"], a["t"], a["Tmax1"], rec["thr"], a["hist_states"],
                                          a["eval_order"], rec["has_roads"], a["persist"], a["n_groups"], a["grp_focal"], a["grp_ids"],
                                          a["grp_members"], a["own_g"], a["mem_g"], a["tilted"], _lib.stream_ptr())


def fetch(o, persist, S, N):
    got = {k: o[k].cpu().numpy().view(gc.DTYPES[k]).reshape((S + 1,) if k == "n_groups" else (S + 1, N)) for k in OUTPUTS}
    got["persist"] = persist.cpu().numpy().view(np.uint64).reshape(S + 1, N)
    return got


@pytest.mark.parametrize("name", gc.NAMES)
def test_tables_equal_the_restatement_at_every_step(recipes, runs, name):
    """Every step of the sequence; then the same step again from the same incoming persist into differently patterned buffers: identical
    bits wherever the kernel writes, the other pattern wherever it does not.  hist_states and eval_order are unchanged by the calls."""
    rec, out = recipes[name], runs[name]
    S, N = rec["order"].shape
    hs, order = dev(rec["hs"]), dev(rec["order"])
    persist = persist_buffer([[0] * N] * S, N, gc.FILL)
    for t, row in zip(rec["steps"], out):
        before = persist.clone()
        o = outputs(S, N, gc.FILL)
        _lib.check(call(rec, t, hs, order, persist, o), "group_build")
        again, o2 = persist_buffer(before.cpu().numpy().view(np.uint64)[:S], N, 0x5A), outputs(S, N, 0x5A)
        _lib.check(call(rec, t, hs, order, again, o2), "group_build")
        torch.cuda.synchronize()
        gc.compare_tables(fetch(o, persist, S, N), gc.expected(row, N), f"{name} step {t}")
        gc.compare_tables(fetch(o2, again, S, N), gc.expected(row, N, fill=0x5A), f"{name} step {t}, second call")
    assert np.array_equal(hs.cpu().numpy().view(np.int32), rec["hs"].view(np.int32)) and np.array_equal(order.cpu().numpy(), rec["order"])


@pytest.mark.parametrize("name", ["shapes_noroads", "shapes_noorder", "shapes_batch"])
def test_a_scenario_without_a_group_keeps_its_sets_and_the_pattern(recipes, name):
    """Arbitrary incoming sets: a scenario with no group has n_groups = 0, own_g = mem_g = -1, tilted = 0, persist as it came in, and its
    group rows keep the fill pattern (asserted on the fetched arrays themselves, then everything against the restatement)."""
    rec = recipes[name]
    S, N = rec["order"].shape
    rs = np.random.RandomState(3)
    masks = [[int(rs.randint(0, 1 << N)) for _ in range(N)] for _ in range(S)]
    hs, order = dev(rec["hs"]), dev(rec["order"])
    for t in rec["steps"][:2]:
        persist, o = persist_buffer(masks, N, gc.FILL), outputs(S, N, gc.FILL)
        _lib.check(call(rec, t, hs, order, persist, o), "group_build")
        torch.cuda.synchronize()
        got = fetch(o, persist, S, N)
        ref = [gc.group_ref(rec["hs"][s], rec["order"][s], masks[s], rec["A"], rec["T"], t, rec["thr"], rec["has_roads"]) for s in range(S)]
        empty = [s for s in range(S) if ref[s]["n_groups"] == 0]
        assert len(empty) >= 2
        pat = {k: gc.filled((1,), gc.DTYPES[k])[0] for k in gc.TABLES}
        for s in empty:
            assert got["n_groups"][s] == 0 and (got["own_g"][s] == -1).all() and (got["mem_g"][s] == -1).all() and (got["tilted"][s] == 0).all()
            assert got["persist"][s].tolist() == masks[s], (name, t, s)
            assert all((got[k][s] == pat[k]).all() for k in ("grp_focal", "grp_ids", "grp_members")), (name, t, s)
        gc.compare_tables(got, gc.expected(ref, N), f"{name} step {t}, arbitrary incoming sets")


def test_a_scenario_launched_alone_gives_the_rows_of_the_batch(recipes, runs):
    """Scenarios 0 (nothing evaluated), 5, 146 and 299 of the 300-scenario recipe, each as a call of its own (S = 1, pointers offset)."""
    rec, out = recipes["shapes_batch"], runs["shapes_batch"]
    S, N = rec["order"].shape
    hs, order = dev(rec["hs"]), dev(rec["order"])
    persist = persist_buffer([[0] * N] * S, N, gc.FILL)
    alone = {s: persist_buffer([[0] * N] * S, N, gc.FILL) for s in (0, 5, 146, 299)}
    for t, row in zip(rec["steps"], out):
        o = outputs(S, N, gc.FILL)
        _lib.check(call(rec, t, hs, order, persist, o), "group_build")
        single = {}
        for s, ps in alone.items():
            single[s] = outputs(S, N, gc.FILL)
            _lib.check(call(rec, t, hs, order, ps, single[s], S=1, s0=s), "group_build")
        torch.cuda.synchronize()
        batch = fetch(o, persist, S, N)
        for s in alone:
            got = fetch(single[s], alone[s], S, N)
            exp = gc.expected(row, N)
            for k in gc.TABLES:                               # the lone call wrote scenario s only: everything else is pattern (persist: 0)
                keep = exp[k][s].copy()
                exp[k][:S] = gc.filled(exp[k][:S].shape, gc.DTYPES[k]) if k != "persist" else 0
                exp[k][s] = keep
                assert np.array_equal(got[k][s], batch[k][s]), (t, s, k)
            gc.compare_tables(got, exp, f"shapes_batch step {t}, scenario {s} alone")


@pytest.mark.parametrize("name,sizes", [("ties", [1, 4, 6, 8]), ("threshold", [1, 4, 8, 13])])
@pytest.mark.parametrize("t", [0, 5])
def test_the_slot_order_the_model_sees_is_the_restated_one(recipes, name, sizes, t):
    """The kernel's tables through ctrlsim_ctx_index_classes and ctrlsim_build_context_c as tests/test_gpu_context_build.py feeds them
    (first call of a rollout: no set yet): slot_gid of every context holds group_ref's ids in ascending vehicle index, -1 behind them,
    and `exist` the existence rows of those vehicles."""
    import test_gpu_context_build as cb
    rec = recipes[name]
    S, N, Tmax1 = rec["hs"].shape[:3]
    A, T, P_all, P, NP = rec["A"], rec["T"], 12, 12, 10
    inp = cb.make_inputs(17, S, N, Tmax1 - 1, P_all, NP, (60.0,) * S)
    inp["hs"], inp["order"] = rec["hs"].copy(), rec["order"].copy()
    inp["hs"][:, :, 1::3, 7] = (np.arange(N) % 3 != 1)[None, :, None]          # existence that tells the vehicles apart (rows 1, 4, 7 only)
    ref = [gc.group_ref(inp["hs"][s], inp["order"][s], [0] * N, A, T, t, rec["thr"], 1) for s in range(S)]
    pr = cb.Prepared(inp, A, T, t, sizes)
    assert pr.ng.tolist() == [r["n_groups"] for r in ref]
    bufs = cb.launch(pr, P, NP, T, 0)
    torch.cuda.synchronize()
    got = cb.fetch(pr, bufs, P, NP, T)
    assert sorted(zip(pr.scn.tolist(), pr.grp.tolist())) == [(s, g) for s in range(S) for g in range(ref[s]["n_groups"])]
    w0 = 0 if t < T else t - (T - 1)
    first = np.cumsum([0] + pr.B)
    for c, (s, g) in enumerate(zip(pr.scn, pr.grp)):
        k = int(np.searchsorted(first, c, side="right") - 1)
        ids = gc.bits(ref[s]["grp_ids"][g])
        assert pr.focal[c] == ref[s]["grp_focal"][g] and len(ids) <= sizes[k]
        slot = got[k]["slot_gid"][c - first[k]]
        assert slot.tolist() == ids + [-1] * (sizes[k] - len(ids)), (name, t, s, g)
        ex = np.zeros((T, sizes[k]), np.float32)
        ex[:, :len(ids)] = inp["hs"][s, ids, w0:w0 + T, 7].T
        assert np.array_equal(got[k]["exist"][c - first[k]].reshape(T, sizes[k]), ex), (name, t, s, g)


def test_refusals_launch_nothing(recipes):
    """T < 1, t < 0, t >= Tmax1, N or A outside [1, 64] or a null table: CTRLSIM_EINVAL and every pattern-filled buffer untouched.
    S <= 0 is CTRLSIM_OK and does nothing."""
    rec = recipes["quirk"]
    S, N, Tmax1 = rec["hs"].shape[:3]
    hs, order = dev(rec["hs"]), dev(rec["order"])
    persist, o = persist_buffer([[0x15] * N] * S, N, gc.FILL), outputs(S, N, gc.FILL)
    bad = [dict(T=0), dict(T=-3), dict(t=-1), dict(t=Tmax1), dict(t=Tmax1 + 100), dict(N=0), dict(N=65), dict(A=0), dict(A=65)]
    bad += [{k: None} for k in ["hist_states", "eval_order", "persist"] + OUTPUTS]
    for over in bad:
        assert call(rec, 1, hs, order, persist, o, over=over) == EINVAL, over
    for over in (dict(S=0), dict(S=-1), dict(S=0, T=0, hist_states=None)):
        assert call(rec, 1, hs, order, persist, o, over=over) == 0, over
    torch.cuda.synchronize()
    got = fetch(o, persist, S, N)
    for k in OUTPUTS:
        assert (got[k] == gc.filled((1,), gc.DTYPES[k])[0]).all(), k
    assert (got["persist"][:S] == 0x15).all() and (got["persist"][S] == gc.filled((1,), np.uint64)[0]).all()
    fresh = persist_buffer([[0] * N] * S, N, gc.FILL)
    _lib.check(call(rec, 1, hs, order, fresh, o), "group_build")         # and the same call without a defect is accepted
    torch.cuda.synchronize()
    assert fetch(o, fresh, S, N)["n_groups"][0] == 2
