"""Logit-level parity of the forward entry points the rollout engine calls — ctrlsim_dt_forward_pass1_c / _pass2_c with several size classes,
the two-stream ctrlsim_dt_forward_pass1_c2, the K/V-cached ctrlsim_dt_forward_pass1_cached_c / _a / plain with pass 2 at cached = 1 — against
the CPU oracle, step by step, and against each other.  tests/forward_cases.py holds the recipes, the expected logits and the guarded harness
(NaN logits with spare rows, a 0xFF workspace with a band behind the size the query names); tests/test_forward_paths_host.py proves on the
CPU that one oracle forward per context serves every step and that the faults these tests exist for are visible in their inputs.
Every failure names split, class, context, step, head and the error against its bound."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import cfg_of  # noqa: E402
from ctrlsim_amd import spec, weights, _lib  # noqa: E402
from ctrlsim_amd.engine import HipModel  # noqa: E402
import model_oracle as mo  # noqa: E402
from gpu_utils import DEV  # noqa: E402
from op_cases import split, split_cases  # noqa: E402,F401  (split: the fixture that binds the operand split)
import forward_cases as fc  # noqa: E402
from forward_cases import EINVAL, Harness  # noqa: E402

TOL = 1e-4        # tests/test_gpu_model.py: test_forward_matches_oracle
TOL_ORDER = 2e-5  # the same context in another evaluation order (test_compact_contexts_equal_plain_contexts)
TOL_REL = 1e-5    # x max |logit| at trained-like weights (test_forward_matches_reference_logits_at_trained_like_weights)

_SETUP = {}


def setup_of(name, classes=None):
    """(dims, HipModel, float32 torch weights, weight tag, Recipe) of a recipe of forward_cases.RECIPES, one per process; classes: another
    class list over the same seed (the contexts it shares with the recipe's own list share their oracle forwards)."""
    kind, wkind, wseed, seed, own = fc.RECIPES[name]
    key = (kind, wkind, wseed)
    if key not in _SETUP:
        cfg = cfg_of(kind)
        d = spec.Dims(cfg)
        w = fc.make_weights(d, wkind, wseed)
        _SETUP[key] = (d, HipModel(cfg, w, DEV), w)
    d, model, w = _SETUP[key]
    rk = (name, tuple(classes or own))
    if rk not in _SETUP:
        _SETUP[rk] = fc.teacher_forced(d, seed, list(classes or own), d.T)
    return d, model, mo.as_torch_weights(w), key, _SETUP[rk]


class Guard:
    """The split's non-finite guard pair bound for the body (the `split` fixture binds the scheme without one); must read [0, 0]."""

    def __init__(self, split):
        self.scheme = 1 if split == "f16x3" else 0
        self.pair = torch.zeros(2, dtype=torch.int32, device=DEV)

    def __enter__(self):
        _lib.check(_lib.lib().ctrlsim_bind(self.scheme, self.pair.data_ptr()))
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _lib.lib().ctrlsim_bind(self.scheme, None)
        if exc[0] is None:
            assert self.pair.tolist() == [0, 0], "non-finite rows met by the guard"


def _sub(rec, k):
    """Class k of a recipe as a recipe of its own."""
    return fc.teacher_forced(rec.d, rec.seed, [rec.classes[k]], rec.t_steps)


def _rows(d, classes, k):
    r0 = fc.rows_of(d, classes[:k])
    return slice(r0, r0 + fc.rows_of(d, classes[k:k + 1]))


def _qkv_in_one_kernel(d, classes, Tq):
    """csrc/forward.hip: gemm_kv — the in_proj writes the K / V tile images from its own epilogue only where EVERY class of the batch has
    token-row counts (all rows, regular rows) that are multiples of 4 and at least 32 rows; else Linear + a split pass per class."""
    ok = True
    for _, A in classes:
        ar, rep = fc.areg(d, A), (1 if A < d.A else 0)
        L, Lreg = Tq * 3 * (ar + rep), Tq * 3 * ar
        ok = ok and L % 4 == 0 and Lreg % 4 == 0 and L >= 32
    return ok


FULL_RECOMPUTE = [("loop", 8), ("loop", 3), ("loop", 1), ("full", 32), ("full", 5)]


@split_cases("name,Tq", FULL_RECOMPUTE, FULL_RECOMPUTE)
def test_class_batched_full_recompute_matches_oracle(split, name, Tq):
    """(a) ctrlsim_dt_forward_pass1_c / _pass2_c(cached = 0) with three size classes in one call: every live slot of every context within 1e-4
    of the oracle's plain evaluation of that context; the same classes in separately allocated context tensors (csrc/forward.hip:
    ctx_contiguous() false, the per-class route of the map pooling, the input MLPs and the token assembly) and as three single-class *_a
    calls: bit-identical logits, every kernel being row-independent.
    ONE PAIR IS NOT BIT-IDENTICAL, by design: under the two-fp16-plane scheme the QKV projection of a full pass has two routes (gemm_kv: the
    row-stationary in_proj kernel with the K / V images in its epilogue, or the weight-stationary Linear + a split pass), chosen for the
    whole batch by its classes' row counts (_qkv_in_one_kernel).  At full size with Tq = 5 the 4-slot class has 45 regular rows, so the batch
    takes the second route, as the 4- and 12-slot classes (45 and 165 regular rows) do alone, while the 24-slot class called alone takes
    the first: other kernels, other summation order (measured: 3.6e-6 on the RTG logits, 3.7e-6 on the action logits).  Exactly there — f16x3
    and the route of the class alone differs from the batch's — the
    single-class call is held to 2e-5, the bound for the same context in another evaluation order; everywhere else, and under bf16x6 (one
    tiled kernel on both routes), to equal bits."""
    d, model, tw, wtag, rec = setup_of(name)
    classes, t = rec.classes, Tq - 1
    want_rtg, want_act = fc.oracle_logits(tw, wtag, rec)
    worst, other_route = {}, []
    with Guard(split):
        h = Harness(model, d, classes, Tq, DEV)
        rtg, act = h.full_step(rec, Tq)
        assert h.band_intact(), "the workspace band behind ctrlsim_forward_workspace_bytes_c was written"
        fc.compare(f"{split} pass1_c", d, classes, rtg, want_rtg, t, "rtg", TOL, worst)
        fc.compare(f"{split} pass2_c", d, classes, act, want_act, t, "action", TOL, worst)
        hs = Harness(model, d, classes, Tq, DEV, separate=True)
        rtg_s, act_s = hs.full_step(rec, Tq)
        assert hs.band_intact()
        for k, cl in enumerate(classes):
            sl = _rows(d, classes, k)
            assert np.array_equal(rtg_s[sl], rtg[sl]), f"{split} class {k} {cl} step {t} head rtg: separate context tensors differ from contiguous"
            assert np.array_equal(act_s[sl], act[sl]), f"{split} class {k} {cl} step {t} head action: separate context tensors differ from contiguous"
            h1 = Harness(model, d, [cl], Tq, DEV, form="a")
            rtg_1, act_1 = h1.full_step(_sub(rec, k), Tq)
            assert h1.band_intact()
            if split == "f16x3" and _qkv_in_one_kernel(d, [cl], Tq) != _qkv_in_one_kernel(d, classes, Tq):
                for head, a, b in (("rtg", rtg_1, rtg[sl]), ("action", act_1, act[sl])):
                    diff = float(np.abs(a - b).max())
                    other_route.append(f"class {k} {head} {diff:.3e}")
                    assert diff <= TOL_ORDER, f"{split} class {k} {cl} step {t} head {head}: single-class call vs batch {diff:.3e} > {TOL_ORDER:.1e}"
                continue
            assert np.array_equal(rtg_1, rtg[sl]), f"{split} class {k} {cl} step {t} head rtg: the single-class call differs from the batch"
            assert np.array_equal(act_1, act[sl]), f"{split} class {k} {cl} step {t} head action: the single-class call differs from the batch"
    print(f"   (a) {split} {name} Tq={Tq}: largest error {worst['err']:.3e} ({worst['where']}); separate == contiguous, bit for bit; per-class calls "
          + ("bit for bit" if not other_route else "on another QKV route, differences " + ", ".join(other_route)))


TWO_STREAM = [("loop", 8), ("loop", 3), ("loop", 1), ("full", 32)]


@split_cases("name,Tq", TWO_STREAM, TWO_STREAM)
def test_two_stream_first_pass_equals_the_single_stream_one(split, name, Tq):
    """(b) ctrlsim_dt_forward_pass1_c2 with its few-row tail on a second stream, then pass 2 there behind an event (engine._policy_chunks):
    RTG logits and, from the workspace it left, action logits bit-identical to ctrlsim_dt_forward_pass1_c / _pass2_c on one stream."""
    d, model, tw, wtag, rec = setup_of(name)
    classes = rec.classes
    with Guard(split):
        h = Harness(model, d, classes, Tq, DEV)
        rtg, act = h.full_step(rec, Tq)
        h2 = Harness(model, d, classes, Tq, DEV)
        rtg_2, act_2 = h2.full_step(rec, Tq, stream2=torch.cuda.Stream())
        assert h.band_intact() and h2.band_intact()
    for k, cl in enumerate(classes):
        sl = _rows(d, classes, k)
        assert np.array_equal(rtg_2[sl], rtg[sl]), f"{split} class {k} {cl} step {Tq - 1} head rtg: pass1_c2 differs from pass1_c"
        assert np.array_equal(act_2[sl], act[sl]), f"{split} class {k} {cl} step {Tq - 1} head action: pass 2 after pass1_c2 differs"


def _cached_sequence(split, h, rec, want_rtg, want_act, tol, rel=False, worst=None, steps=None):
    """Steps 0 .. T - 1 of the cached phase on h's one workspace, each compared with the oracle's row t.  -> [(rtg, act)] per step."""
    d, out = rec.d, []
    for t in range(d.T if steps is None else steps):
        rtg, act = h.cached_step(rec, t)
        out.append((rtg, act))
        fc.compare(f"{split} pass1_cached", d, rec.classes, rtg, want_rtg, t, "rtg", tol, worst, rel)
        fc.compare(f"{split} pass2_c cached", d, rec.classes, act, want_act, t, "action", tol, worst, rel)
    assert h.band_intact(), "the workspace band behind ctrlsim_forward_workspace_bytes_c(.., T) was written"
    return out


CACHED = [("tiny", None), ("loop", None), ("full", ((1, 4), (1, 24)))]


@split_cases("name,classes", CACHED, CACHED, ids={"classes": {None: "all", ((1, 4), (1, 24)): "4+24"}})
def test_cached_sequence_matches_oracle_at_every_step(split, name, classes):
    """(c) What engine._chunk_step_cached does, for t = 0 .. T - 1 on ONE workspace: window rows [t - 1, t] with the placeholders in row t,
    ctrlsim_dt_forward_pass1_cached_c, the true bins of step t into hist_rtg, ctrlsim_dt_forward_pass2_c(cached = 1); both heads within 1e-4
    of the oracle's row t at every step.  The cache must carry the RTG rows pass 2 refreshed and the action rows step t + 1 rewrote (the
    recipes hold no placeholder in a true row).  Full size, classes of 4 and 24 slots: the regular rows cross a 64-key tile at steps 1 and
    8, the representative's key region at step 22.  Slots whose existence drops mid-window stay in their contexts.
    tiny (one plain class): also through the *_a and the unsuffixed entries, bit-identical to the class-batched ones."""
    d, model, tw, wtag, rec = setup_of(name, classes and [tuple(c) for c in classes])
    want_rtg, want_act = fc.oracle_logits(tw, wtag, rec)
    worst = {}
    with Guard(split):
        h = Harness(model, d, rec.classes, d.T, DEV)
        seq = _cached_sequence(split, h, rec, want_rtg, want_act, TOL, worst=worst)
        if name == "tiny":
            for form in ("a", "plain"):
                hf = Harness(model, d, rec.classes, d.T, DEV, form=form)
                for t, (rtg, act) in enumerate(_cached_sequence(f"{split} form {form}", hf, rec, want_rtg, want_act, TOL)):
                    assert np.array_equal(rtg, seq[t][0]) and np.array_equal(act, seq[t][1]), f"{split} step {t}: form {form} differs from _c"
    print(f"   (c) {split} {name}: largest error over {d.T} cached steps {worst['err']:.3e} ({worst['where']})")


@split_cases("name", ["loop"], ["loop"])
def test_cached_steps_equal_full_recompute_on_the_device(split, name):
    """(d) At every step of the loop-size cached sequence, ctrlsim_dt_forward_pass1_c / _pass2_c(cached = 0) with Tq = t + 1 on a second
    workspace and the same inputs: the cached logits within 2e-5 of the recomputed ones — the bound for the same context in another
    evaluation order."""
    d, model, tw, wtag, rec = setup_of(name)
    want_rtg, want_act = fc.oracle_logits(tw, wtag, rec)
    big = {"rtg": (0.0, -1), "action": (0.0, -1)}
    with Guard(split):
        h = Harness(model, d, rec.classes, d.T, DEV)
        for t in range(d.T):
            rtg, act = h.cached_step(rec, t)
            h2 = Harness(model, d, rec.classes, t + 1, DEV)
            rtg_f, act_f = h2.full_step(rec, t + 1)
            assert h2.band_intact()
            for head, a, b in (("rtg", rtg, rtg_f), ("action", act, act_f)):
                for k, cl in enumerate(rec.classes):
                    sl = _rows(d, rec.classes, k)
                    diff = float(np.abs(a[sl] - b[sl]).max())
                    if diff > big[head][0]:
                        big[head] = (diff, t)
                    assert diff <= TOL_ORDER, f"{split} class {k} {cl} step {t} head {head}: cached vs recomputed {diff:.3e} > {TOL_ORDER:.1e}"
        assert h.band_intact()
    print(f"   (d) {split}: largest cached-vs-recompute difference rtg {big['rtg'][0]:.3e} (step {big['rtg'][1]}), "
          f"action {big['action'][0]:.3e} (step {big['action'][1]})")


@split_cases("name", ["loop"], ["loop"])
def test_cached_sequence_does_not_depend_on_what_the_workspace_held(split, name):
    """(e) The cached sequence a second time on its workspace poisoned with 0xFF again: every step's logits bit-identical to the first run
    (nothing of the first run's cache, index lists or images may be read before it is rewritten)."""
    d, model, tw, wtag, rec = setup_of(name)
    want_rtg, want_act = fc.oracle_logits(tw, wtag, rec)
    with Guard(split):
        h = Harness(model, d, rec.classes, d.T, DEV)
        first = _cached_sequence(split, h, rec, want_rtg, want_act, TOL)
        h.poison()
        again = _cached_sequence(split, h, rec, want_rtg, want_act, TOL)
    for t, ((r0, a0), (r1, a1)) in enumerate(zip(first, again)):
        assert np.array_equal(r0, r1), f"{split} step {t} head rtg: the second run on a poisoned workspace differs"
        assert np.array_equal(a0, a1), f"{split} step {t} head action: the second run on a poisoned workspace differs"


@split_cases("name", ["loop"], ["loop"])
def test_cached_first_pass_does_not_depend_on_what_the_second_pass_left(split, name):
    """(e) Steps 0 .. 4, then ctrlsim_dt_forward_pass1_cached_c for step 5 twice in a row: bit-identical RTG logits (the re-evaluation rewrites
    the same cache rows with the same values), and the second pass that follows still matches the oracle."""
    d, model, tw, wtag, rec = setup_of(name)
    want_rtg, want_act = fc.oracle_logits(tw, wtag, rec)
    with Guard(split):
        h = Harness(model, d, rec.classes, d.T, DEV)
        _cached_sequence(split, h, rec, want_rtg, want_act, TOL, steps=5)
        rtg, act, rtg_again = h.cached_step(rec, 5, repeat_pass1=True)
        assert h.band_intact()
    assert np.array_equal(rtg, rtg_again), f"{split} step 5 head rtg: the first pass called twice gives two answers"
    fc.compare(f"{split} pass1_cached twice", d, rec.classes, rtg_again, want_rtg, 5, "rtg", TOL)
    fc.compare(f"{split} pass2_c after pass1_cached twice", d, rec.classes, act, want_act, 5, "action", TOL)


@split_cases("name", ["loop"], ["loop"])
def test_the_next_step_reads_the_rows_the_second_pass_left(split, name):
    """(e) The other side of the cache contract, and the proof on the device that these tests see a stale row: at step 3 the second pass is
    handed the placeholder bins instead of the true ones — what a cache row it failed to refresh would hold.  Step 4 does not recompute
    those rows (its context tensors carry the TRUE bins of step 3, and must not be read for them): its RTG logits must be the oracle's on
    the sequence with the returns of step 3 at their placeholder, within 1e-4, and more than 100 x 1e-4 from the true sequence's on a live
    slot of every context."""
    d, model, tw, wtag, rec = setup_of(name)
    want_rtg, want_act = fc.oracle_logits(tw, wtag, rec)
    stale = []
    for src in rec.data:
        v = dict(src, rtgs=src["rtgs"].copy())
        v["rtgs"][:, :, 3] = spec.ZERO_RTG_BINS
        stale.append(v)
    with torch.no_grad():
        outs = [mo.forward(tw, fc.synth_inputs.to_torch(v), d) for v in stale]
    stale_rtg, stale_act = [o["rtg_preds"].numpy() for o in outs], [o["action_preds"].numpy() for o in outs]
    with Guard(split):
        h = Harness(model, d, rec.classes, d.T, DEV)
        _cached_sequence(split, h, rec, want_rtg, want_act, TOL, steps=3)
        h.nan_logits()
        h.fill(rec.at_step(3), 2, 4)
        _lib.check(h.pass1_cached(3), "pass1_cached")
        h.set_bins(stale, 3)
        _lib.check(h.pass2(4, 3, 1), "pass2 cached")
        torch.cuda.synchronize()
        fc.compare(f"{split} pass2_c cached, placeholder bins", d, rec.classes, h.take("act"), stale_act, 3, "action", TOL)
        rtg, act = h.cached_step(rec, 4)
        assert h.band_intact()
    fc.compare(f"{split} pass1_cached after a stale row", d, rec.classes, rtg, stale_rtg, 4, "rtg", TOL)
    fc.compare(f"{split} pass2_c cached after a stale row", d, rec.classes, act, stale_act, 4, "action", TOL)
    r0 = 0
    for k, (B, A) in enumerate(rec.classes):
        ar, lv = fc.areg(d, A), fc.live(d, A)
        g = rtg[r0:r0 + B * ar].reshape(B, ar, -1)
        for b in range(B):
            off = float(np.abs(g[b, :lv] - want_rtg[k][b, :lv, 4]).max())
            assert off > 100 * TOL, f"{split} class {k} {(B, A)} context {b} step 4 head rtg: a stale row moved the logits by {off:.3e} only"
        r0 += B * ar


@split_cases("name", ["loop"], ["loop"])
def test_invalid_arguments_are_refused_and_write_nothing(split, name):
    """(e) t outside [0, T), a class of fewer than 2 or more than d.A slots, more than CTRLSIM_MAX_CLASSES classes, a variant model handed to
    the cached entries: CTRLSIM_EINVAL, the NaN-filled logits untouched."""
    d, model, tw, wtag, rec = setup_of(name)
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    h = Harness(model, d, rec.classes, d.T, DEV)
    h.fill(rec.at_step(0), 0, 1)
    n, m = h.n, model.handle

    def untouched(what):
        torch.cuda.synchronize()
        assert torch.isnan(h.rtg).all() and torch.isnan(h.act).all(), f"{split} {what}: refused, but logits were written"

    for t in (-1, d.T, d.T + 7):
        assert h.pass1_cached(t) == EINVAL, f"{split} pass1_cached_c accepted t = {t}"
        untouched(f"pass1_cached_c t = {t}")
    for Tq in (0, d.T + 1):
        assert h.pass1(Tq) == EINVAL and h.pass2(Tq, 0, 0) == EINVAL and h.pass2(Tq, 0, 1) == EINVAL, f"{split} Tq = {Tq} accepted"
        assert h.pass1(Tq, tail_stream=st) == EINVAL
        untouched(f"Tq = {Tq}")

    def all_entries(n_, Bs, As, cs, what, hm=m):
        calls = {
            "pass1_c": lambda: lib.ctrlsim_dt_forward_pass1_c(hm, n_, Bs, As, cs, 1, p(h.ws), p(h.rtg), None, st),
            "pass1_c2": lambda: lib.ctrlsim_dt_forward_pass1_c2(hm, n_, Bs, As, cs, 1, p(h.ws), p(h.rtg), st, st),
            "pass1_cached_c": lambda: lib.ctrlsim_dt_forward_pass1_cached_c(hm, n_, Bs, As, cs, 0, p(h.ws), p(h.rtg), st),
            "pass2_c": lambda: lib.ctrlsim_dt_forward_pass2_c(hm, n_, Bs, As, cs, 1, 0, d.A, h.Tmax, p(h.ctx_scn), p(h.hist_rtg), p(h.ws),
                                                              p(h.act), 0, st),
            "pass2_c cached": lambda: lib.ctrlsim_dt_forward_pass2_c(hm, n_, Bs, As, cs, 1, 0, d.A, h.Tmax, p(h.ctx_scn), p(h.hist_rtg),
                                                                     p(h.ws), p(h.act), 1, st)}
        for nm, call in calls.items():
            assert call() == EINVAL, f"{split} {nm} accepted {what}"
            untouched(f"{nm} with {what}")

    for bad in (1, 0, d.A + 1):
        As = (C.c_int * n)(*[bad if k == 1 else A for k, (_, A) in enumerate(rec.classes)])
        assert lib.ctrlsim_forward_workspace_bytes_c(C.byref(model.cdims), n, h.Bs, As, d.T) == EINVAL
        all_entries(n, h.Bs, As, h.cs, f"a class of {bad} slots")
    nmax = 17                                                  # CTRLSIM_MAX_CLASSES + 1 (include/ctrlsim.h)
    Bs, As = (C.c_int * nmax)(*([1] * nmax)), (C.c_int * nmax)(*([3] * nmax))
    cs = (_lib.Ctx * nmax)(*([h.cs[0]] * nmax))
    assert lib.ctrlsim_forward_workspace_bytes_c(C.byref(model.cdims), nmax, Bs, As, d.T) == EINVAL
    all_entries(nmax, Bs, As, cs, f"{nmax} classes")
    all_entries(0, h.Bs, h.As, h.cs, "no class")
    # variant models: the own-return mask (dims.variant 4: full recompute only) and the IL baseline (no return tokens at all)
    own = spec.make_cfg(**dict(fc_overrides("loop"), model__attend_own_return_action=True))
    for cfg in (own, cfg_of("loop", variant="il")):
        dv = spec.Dims(cfg)
        mv = HipModel(cfg, weights.generate(dv, 0), DEV)
        one = (C.c_int * 1)(2), (C.c_int * 1)(d.A)
        cached = {
            "pass1_cached_c": lambda: lib.ctrlsim_dt_forward_pass1_cached_c(mv.handle, 1, one[0], one[1], h.cs, 0, p(h.ws), p(h.rtg), st),
            "pass1_cached_a": lambda: lib.ctrlsim_dt_forward_pass1_cached_a(mv.handle, 2, 0, d.A, C.byref(h.cs[0]), p(h.ws), p(h.rtg), st),
            "pass1_cached": lambda: lib.ctrlsim_dt_forward_pass1_cached(mv.handle, 2, 0, C.byref(h.cs[0]), p(h.ws), p(h.rtg), st),
            "pass2_c cached": lambda: lib.ctrlsim_dt_forward_pass2_c(mv.handle, 1, one[0], one[1], h.cs, 1, 0, d.A, h.Tmax, p(h.ctx_scn),
                                                                     p(h.hist_rtg), p(h.ws), p(h.act), 1, st)}
        for nm, call in cached.items():
            assert call() == EINVAL, f"{split} {nm} accepted a model of variant {mv.cdims.variant}"
            untouched(f"{nm} with a model of variant {mv.cdims.variant}")
    assert h.band_intact() and bool((h.ws == 0xFF).all().item()), "a refused call wrote to the workspace"


def fc_overrides(kind):
    from helpers import LOOP, TINY
    return dict({"tiny": TINY, "loop": LOOP, "full": {}}[kind])


@split_cases("name,classes", [("full_trained", None)], [("full_trained", None)], ids={"classes": {None: "4+24"}})
def test_cached_sequence_at_trained_like_weights(split, name, classes):
    """(f) The cached sequence at full size, classes of 4 and 24 slots, with weights.generate_trained_like(d, 1) (|logit| ~ 30) against the
    oracle evaluated in float64, within 1e-5 x max |logit| of each compared context, head and step; the float32 oracle's own distance from
    float64 is held to the same bound (or the recipe is wrong for this test) and printed next to the device's."""
    d, model, tw, wtag, rec = setup_of(name)
    w64 = {k: v.double() for k, v in tw.items()}
    rtg64, act64 = fc.oracle_logits(w64, wtag, rec, torch.float64)
    rtg32, act32 = fc.oracle_logits(tw, wtag, rec)
    ref_worst, worst = {}, {}
    for t in range(d.T):
        for head, w64_, w32_ in (("rtg", rtg64, rtg32), ("action", act64, act32)):
            for k, (B, A) in enumerate(rec.classes):
                lv = fc.live(d, A)
                for b in range(B):
                    scale = float(np.abs(w64_[k][b, :lv, t]).max())
                    assert scale > 15.0, (head, k, b, t, scale)
            # the float32 oracle's rows, laid out as the device's, through the same comparison
            rows = np.concatenate([w32_[k][:, :fc.areg(d, A), t].reshape(-1, w32_[k].shape[-1]) for k, (_, A) in enumerate(rec.classes)])
            fc.compare("float32 oracle vs float64", d, rec.classes, rows, w64_, t, head, TOL_REL, ref_worst, rel=True)
    with Guard(split):
        h = Harness(model, d, rec.classes, d.T, DEV)
        _cached_sequence(split, h, rec, rtg64, act64, TOL_REL, rel=True, worst=worst)
    print(f"   (f) {split}: device vs float64 {worst['ratio']:.3f} of the bound ({worst['err']:.3e}, {worst['where']}); float32 oracle vs float64 "
          f"{ref_worst['ratio']:.3f} of the bound ({ref_worst['err']:.3e}, {ref_worst['where']}); ratio {worst['ratio'] / ref_worst['ratio']:.2f}")
