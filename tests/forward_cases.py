"""What the logit-level tests of the forward entry points share (tests/test_forward_paths_host.py, tests/test_gpu_forward_paths.py): teacher-forced
input recipes for one or several context size classes, the writer of a window of them into CtxBuffers, the oracle's expected logits per step,
and the harness that calls the class-batched / two-stream / K/V-cached entries of include/ctrlsim.h on guarded buffers.

RECIPE.  teacher_forced() draws one synth_inputs.random_context per CONTEXT (seeded by (seed, A_k, index in the class), so that two class
lists that share a context share its oracle forward) with every window step filled, and re-draws every RTG bin equal to the placeholder bin
of its component and every action token equal to the placeholder token: a cache row that kept its placeholder can then never hold the right
value by accident.  Recipe.at_step(t) is what the device sees at step t before sampling: the true rows below t, the engine's placeholders
(spec.ZERO_RTG_BINS, spec.ZERO_ACTION_TOKEN) in the RTG and action columns of row t.

EXPECTED LOGITS.  rtg_preds[:, :, t] / action_preds[:, :, t] of ONE model_oracle.forward over the whole true window: the structured mask lets
the state token of step t see nothing later than the states of step t, and the RTG token of step t nothing but those and its own slot's RTG
token.  tests/test_forward_paths_host.py proves the equality with the truncated, placeholder-carrying sequence, so no GPU test rests on it.

LAYOUT.  A class (B_k, A_k) with A_k < d.A holds contexts of A_k - 1 live agents in the leading A_k slots of the reference layout: the last
slot is a padded one, the representative of all padded slots (csrc/forward.hip: Shape).  A_k == d.A is the plain layout; its contexts have
d.A - 1 live agents.  Logits rows come class after class, context after context, regular slot after regular slot."""
import contextlib
import ctypes as C

import numpy as np
import torch

from ctrlsim_amd import _lib
from ctrlsim_amd.engine import CtxBuffers
from ctrlsim_amd.spec import ZERO_ACTION_TOKEN, ZERO_RTG_BINS
import model_oracle as mo
import synth_inputs

EINVAL = -22
BAND = 4096                  # guard band behind the workspace the size query asks for
PER_SLOT = ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask")


def areg(d, A):
    """Logits rows per context of a class of A slots: the regular slots."""
    return A - 1 if A < d.A else d.A


def live(d, A):
    """Live agents per context of a class of A slots (the slots whose logits are compared)."""
    return A - 1 if A < d.A else d.A - 1


def rows_of(d, classes):
    return sum(B * areg(d, A) for B, A in classes)


# ---------------------------------------------------------------------------------------------------------------- recipes
# name -> (dims preset, weights, weight seed, input seed, classes).  weights: "peaked" = weights.generate_trained_like with the head gain
# PEAKED_GAIN instead of 15 (LayerNorm gains, matrix scales and embedding rows of a trained checkpoint, peaked attention, |logit| <= 6):
# at weights.generate's initialisation the softmax averages its keys, and a whole step's RTG or action rows left at their placeholders move
# the next step's logits by 5e-3 at loop dims, whatever the seed — less than the 100 x 1e-4 tests/test_forward_paths_host.py asks of a
# recipe; these weights move them by 3.2e-2 or more, and the float32 oracle stays 1.3e-5 from the float64 one.  "trained" = the same generator at
# its own gain (|logit| ~ 30), compared relative to max |logit|.
# "full" holds the contexts of both full-size class lists of the GPU tests ([(2, 4), (1, 12), (1, 24)] and [(1, 4), (1, 24)]: a context is
# seeded by its class's slot count and its index, not by the list it stands in).
PEAKED_GAIN = 2.0
RECIPES = {
    "tiny": ("tiny", "peaked", 1, 41, [(2, 4)]),
    "loop": ("loop", "peaked", 1, 42, [(2, 3), (1, 4), (2, 6)]),
    "full": ("full", "peaked", 1, 43, [(2, 4), (1, 12), (1, 24)]),
    "full_trained": ("full", "trained", 1, 43, [(1, 4), (1, 24)]),
}
HOST_RECIPES = {k: RECIPES[k] for k in ("tiny", "loop")}       # the sizes a CPU forward per step and fault is affordable at


def make_weights(d, wkind, wseed):
    from ctrlsim_amd import weights
    return weights.generate_trained_like(d, wseed, logit_gain=PEAKED_GAIN if wkind == "peaked" else 15.0)


def ctx_key(seed, A, b, t_steps):
    return (seed * 10007 + A * 101 + b) * 128 + t_steps


def _true_context(d, cseed, n_agents, t_steps):
    inp = synth_inputs.random_context(d, cseed, B=1, t_fill=t_steps, n_agents=n_agents, n_polys=d.P - 1)
    rs = np.random.RandomState(cseed + 5)
    for c, z in enumerate(ZERO_RTG_BINS):
        col = inp["rtgs"][..., c]
        while (col == z).any():
            col[col == z] = rs.randint(0, d.R, int((col == z).sum()))
    act = inp["actions"]
    while (act == ZERO_ACTION_TOKEN).any():
        act[act == ZERO_ACTION_TOKEN] = rs.randint(0, d.V, int((act == ZERO_ACTION_TOKEN).sum()))
    return inp


class Recipe:
    """classes [(B_k, A_k)]; data[k]: the true inputs of class k in the reference layout with all d.A slots, [B_k, d.A, T, ...];
    keys[k][b]: the seed of context b of class k (the key of its oracle forward)."""

    def __init__(self, d, seed, classes, t_steps):
        assert 1 <= t_steps <= d.T and len({A for _, A in classes}) == len(classes)
        self.d, self.seed, self.classes, self.t_steps = d, seed, list(classes), t_steps
        self.keys = [[ctx_key(seed, A, b, t_steps) for b in range(B)] for B, A in classes]
        self.data = []
        for (B, A), ks in zip(classes, self.keys):
            ctxs = [_true_context(d, k, live(d, A), t_steps) for k in ks]
            self.data.append({f: np.concatenate([c[f] for c in ctxs], 0) for f in ctxs[0]})

    def at_step(self, t):
        """The inputs the device must see at step t before anything is sampled (rows above t are left as they are: no entry reads them)."""
        out = []
        for src in self.data:
            v = dict(src)
            v["rtgs"], v["actions"] = src["rtgs"].copy(), src["actions"].copy()
            v["rtgs"][:, :, t] = ZERO_RTG_BINS
            v["actions"][:, :, t] = ZERO_ACTION_TOKEN
            out.append(v)
        return out

    def context(self, k, b):
        return {f: v[b:b + 1] for f, v in self.data[k].items()}


def teacher_forced(d, seed, classes, t_steps):
    return Recipe(d, seed, classes, t_steps)


_ORACLE = {}


def oracle_context(tw, wtag, d, key, inp, dtype=torch.float32):
    """(rtg_preds, action_preds) [d.A, T, .] of one context, one oracle forward per (weights, dims, context, dtype) and process.
    tw: torch weights already in `dtype`."""
    ck = (wtag, d.A, d.T, d.P, key, dtype)
    if ck not in _ORACLE:
        x = synth_inputs.to_torch(inp)
        if dtype == torch.float64:
            x = {k: (v.double() if v.is_floating_point() else v) for k, v in x.items()}
        with torch.no_grad():
            o = _forward(tw, x, d, dtype)
        _ORACLE[ck] = (o["rtg_preds"][0].numpy(), o["action_preds"][0].numpy())
    return _ORACLE[ck]


@contextlib.contextmanager
def widened(dtype):
    """model_oracle casts its inputs with .float(); in float64 the same plain-torch code runs with those casts widened (oracle/gen_golden.py
    makes the float64 logits of tests/golden/model_trained.npz the same way).  float32: nothing changes."""
    if dtype == torch.float32:
        yield
        return
    orig = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self.double()
    try:
        yield
    finally:
        torch.Tensor.float = orig


def _forward(tw, x, d, dtype):
    with widened(dtype):
        return mo.forward(tw, x, d)


def oracle_logits(tw, wtag, recipe, dtype=torch.float32):
    """-> (rtg[k], act[k]): per class [B_k, d.A, T, R*C] and [B_k, d.A, T, V] of the true sequences."""
    rtg, act = [], []
    for k, (B, A) in enumerate(recipe.classes):
        per = [oracle_context(tw, wtag, recipe.d, recipe.keys[k][b], recipe.context(k, b), dtype) for b in range(B)]
        rtg.append(np.stack([p[0] for p in per]))
        act.append(np.stack([p[1] for p in per]))
    return rtg, act


# ---------------------------------------------------------------------------------------------------------------- context tensors
def _window_arrays(d, src, t0, t1, A):
    """The flat context-tensor contents of one class: window rows [t0, t1) of the leading A slots of `src` (engine.ctx_from_reference_layout's
    expressions, on a window that need not start at 0)."""
    sub = {k: (np.asarray(v)[:, :A] if k in PER_SLOT else np.asarray(v)) for k, v in src.items()}
    st = np.asarray(sub["agent_states"], np.float64)
    B, _, T = st.shape[:3]
    types = np.broadcast_to(np.asarray(sub["agent_types"], np.float64)[:, :, None, :], (B, A, T, 5))
    rt = np.asarray(sub["rtgs"]).transpose(0, 2, 1, 3)[:, t0:t1]
    if d.VARIANT == 3:
        rt = np.ascontiguousarray(rt, np.float32).view(np.int32)
    out = dict(
        st12=(np.concatenate([st[..., :7], types], -1).transpose(0, 2, 1, 3)[:, t0:t1], np.float32),
        exist=(st[..., 7].transpose(0, 2, 1)[:, t0:t1], np.float32),
        goal5=(np.asarray(sub["goals"], np.float64), np.float32),
        act_tok=(np.asarray(sub["actions"]).transpose(0, 2, 1)[:, t0:t1], np.int32),
        rtg_bin=(rt, np.int32),
        tstep=(np.asarray(sub["timesteps"])[:, 0, t0:t1, 0], np.int32),
        slot_gid=(np.broadcast_to(np.arange(A), (B, A)), np.int32),
        road_pts=(np.asarray(sub["road_points"], np.float64), np.float32),
        road_types=(np.asarray(sub["road_types"], np.float64), np.float32))
    return {k: np.ascontiguousarray(a).astype(dt).reshape(-1) for k, (a, dt) in out.items()}


def fill_window(cb, d, data, t0, t1, classes):
    """Window rows [t0, t1) of reference-layout inputs into context tensors.  cb: ONE CtxBuffers — the classes back to back, the packing
    CtxBuffers.class_structs(classes, t1 - t0) addresses — or a LIST of CtxBuffers, one per class, each written from its start (separately
    allocated: csrc/forward.hip's ctx_contiguous() is then false).  data: the inputs of each class (a dict for a single class), rows
    [B_k, >= A_k slots, T, ...]; slot_gid <- 0 .. A_k - 1 per context.  -> the per-class element offsets of every field."""
    data = [data] if isinstance(data, dict) else list(data)
    separate = isinstance(cb, (list, tuple))
    assert len(data) == len(classes) and (not separate or len(cb) == len(classes)) and 0 <= t0 < t1
    off = {f: 0 for f in CtxBuffers.FIELDS}
    offsets = []
    for k, (B, A) in enumerate(classes):
        assert data[k]["agent_states"].shape[0] == B and data[k]["agent_states"].shape[1] >= A
        tgt = cb[k] if separate else cb
        arrays = _window_arrays(d, data[k], t0, t1, A)
        offsets.append(dict(off))
        for f in CtxBuffers.FIELDS:
            buf = getattr(tgt, f).view(-1)
            a = torch.from_numpy(arrays[f])
            assert off[f] + a.numel() <= buf.numel(), (f, k)
            buf[off[f]:off[f] + a.numel()] = a.to(buf.device)
            if not separate:
                off[f] += a.numel()
    return offsets


def alloc_separate(d, classes, device):
    """One CtxBuffers per class, each with room for one context more than the class has: the tensors of a class then never end where an
    allocation of the next class begins, whatever the allocator does."""
    return [CtxBuffers(d, B + 1, device) for B, _ in classes]


def ctx_structs(cb, classes, Tn):
    return [c.struct for c in cb] if isinstance(cb, (list, tuple)) else cb.class_structs(classes, Tn)


# ---------------------------------------------------------------------------------------------------------------- device harness
class Harness:
    """Guarded buffers of one model batch and the calls on them.  The workspace is what ctrlsim_forward_workspace_bytes_c(classes, Tw) asks
    for plus BAND bytes, all 0xFF (NaN as fp32, fp16 and bf16); the logits buffers are NaN with `extra` rows behind the batch's own.
    form: "c" = the class-batched entries, "a" = the single-class *_a entries, "plain" = the entries without a suffix (one class of d.A
    slots)."""

    def __init__(self, model, d, classes, Tw, device, separate=False, form="c", extra=3):
        self.model, self.d, self.classes, self.device, self.form = model, d, list(classes), device, form
        self.lib = _lib.lib()
        n = self.n = len(classes)
        assert form == "c" or (n == 1 and (form == "a" or classes[0][1] == d.A))
        self.Bs = (C.c_int * n)(*[B for B, _ in classes])
        self.As = (C.c_int * n)(*[A for _, A in classes])
        self.Btot = sum(B for B, _ in classes)
        self.cb = alloc_separate(d, classes, device) if separate else CtxBuffers(d, self.Btot, device)
        self.need = int(self.lib.ctrlsim_forward_workspace_bytes_c(C.byref(model.cdims), n, self.Bs, self.As, Tw))
        assert self.need > 0, self.need
        self.ws = torch.empty(self.need + BAND, dtype=torch.uint8, device=device)
        self.poison()
        self.rows = rows_of(d, classes)
        self.rtg = torch.empty(self.rows + extra, d.R * d.C, device=device)
        self.act = torch.empty(self.rows + extra, d.V, device=device)
        self.nan_logits()
        self.ctx_scn = torch.arange(self.Btot, dtype=torch.int32, device=device)
        self.Tmax = d.T
        self.hist_rtg = torch.zeros(self.Btot, d.A, self.Tmax, 3, dtype=torch.int32, device=device)
        self.cs = None

    def poison(self):
        self.ws.fill_(0xFF)

    def nan_logits(self):
        self.rtg.fill_(float("nan"))
        self.act.fill_(float("nan"))

    def fill(self, data, t0, t1):
        fill_window(self.cb, self.d, data, t0, t1, self.classes)
        self.cs = (_lib.Ctx * self.n)(*ctx_structs(self.cb, self.classes, t1 - t0))

    def set_bins(self, data, t):
        """The true RTG bins of step t where ctrlsim_sample_rtg would write them: hist_rtg[context, slot, t]."""
        c0 = 0
        for (B, _), src in zip(self.classes, data):
            self.hist_rtg[c0:c0 + B, :, t] = torch.from_numpy(np.asarray(src["rtgs"][:, :, t]).astype(np.int32)).to(self.device)
            c0 += B

    # every call returns the entry's status; stream: a raw stream handle (default: torch's current stream)
    def pass1(self, Tq, stream=None, tail_stream=None):
        st = _lib.stream_ptr() if stream is None else stream
        p, m, lib = _lib.ptr, self.model.handle, self.lib
        if tail_stream is not None:
            return lib.ctrlsim_dt_forward_pass1_c2(m, self.n, self.Bs, self.As, self.cs, Tq, p(self.ws), p(self.rtg), st, tail_stream)
        if self.form == "a":
            return lib.ctrlsim_dt_forward_pass1_a(m, self.Bs[0], Tq, self.As[0], C.byref(self.cs[0]), p(self.ws), p(self.rtg), None, st)
        if self.form == "plain":
            return lib.ctrlsim_dt_forward_pass1(m, self.Bs[0], Tq, C.byref(self.cs[0]), p(self.ws), p(self.rtg), None, st)
        return lib.ctrlsim_dt_forward_pass1_c(m, self.n, self.Bs, self.As, self.cs, Tq, p(self.ws), p(self.rtg), None, st)

    def pass1_cached(self, t, stream=None):
        st = _lib.stream_ptr() if stream is None else stream
        p, m, lib = _lib.ptr, self.model.handle, self.lib
        if self.form == "a":
            return lib.ctrlsim_dt_forward_pass1_cached_a(m, self.Bs[0], t, self.As[0], C.byref(self.cs[0]), p(self.ws), p(self.rtg), st)
        if self.form == "plain":
            return lib.ctrlsim_dt_forward_pass1_cached(m, self.Bs[0], t, C.byref(self.cs[0]), p(self.ws), p(self.rtg), st)
        return lib.ctrlsim_dt_forward_pass1_cached_c(m, self.n, self.Bs, self.As, self.cs, t, p(self.ws), p(self.rtg), st)

    def pass2(self, Tq, t, cached, stream=None):
        st = _lib.stream_ptr() if stream is None else stream
        p, m, lib, N = _lib.ptr, self.model.handle, self.lib, self.d.A
        if self.form == "a":
            return lib.ctrlsim_dt_forward_pass2_a(m, self.Bs[0], Tq, self.As[0], t, N, self.Tmax, C.byref(self.cs[0]), p(self.ctx_scn),
                                                  p(self.hist_rtg), p(self.ws), p(self.act), cached, st)
        if self.form == "plain":
            return lib.ctrlsim_dt_forward_pass2(m, self.Bs[0], Tq, t, N, self.Tmax, C.byref(self.cs[0]), p(self.ctx_scn),
                                                p(self.hist_rtg), p(self.ws), p(self.act), cached, st)
        return lib.ctrlsim_dt_forward_pass2_c(m, self.n, self.Bs, self.As, self.cs, Tq, t, N, self.Tmax, p(self.ctx_scn),
                                              p(self.hist_rtg), p(self.ws), p(self.act), cached, st)

    def take(self, which):
        """The logits of the batch's own rows (host array) after checking that they are finite and that the rows behind them are still NaN."""
        buf = (self.rtg if which == "rtg" else self.act).cpu().numpy()
        assert np.isfinite(buf[:self.rows]).all(), f"{which} logits: a row of the batch is not finite"
        assert np.isnan(buf[self.rows:]).all(), f"{which} logits: a row beyond the batch's {self.rows} was written"
        return buf[:self.rows].copy()

    def band_intact(self):
        return bool((self.ws[self.need:] == 0xFF).all().item())

    def full_step(self, recipe, Tq, stream2=None):
        """pass1_c / pass2_c(cached = 0) (or the form's entries) at window length Tq on the recipe: -> (rtg, act) logits of step Tq - 1.
        stream2: a torch stream — the two-stream entry, its tail and the second pass there, ordered as engine._policy_chunks does."""
        t = Tq - 1
        data = recipe.at_step(t)
        self.nan_logits()
        self.fill(data, 0, Tq)
        self.set_bins(recipe.data, t)
        if stream2 is None:
            _lib.check(self.pass1(Tq), "pass1")
            _lib.check(self.pass2(Tq, t, 0), "pass2")
        else:
            main = torch.cuda.current_stream()
            stream2.wait_stream(main)                     # (the harness's own fills ran on the main stream)
            _lib.check(self.pass1(Tq, tail_stream=stream2.cuda_stream), "pass1_c2")
            ev = torch.cuda.Event()
            ev.record(main)
            stream2.wait_event(ev)
            _lib.check(self.pass2(Tq, t, 0, stream=stream2.cuda_stream), "pass2")
            main.wait_stream(stream2)
        torch.cuda.synchronize()
        return self.take("rtg"), self.take("act")

    def cached_step(self, recipe, t, repeat_pass1=False):
        """One step of engine._chunk_step_cached on this harness's workspace: window rows [max(t - 1, 0), t] with the placeholders in row t,
        the cached first pass, the true bins of step t into hist_rtg, the second pass with cached = 1.  -> (rtg, act[, rtg of a repeated
        first pass])."""
        t0 = max(t - 1, 0)
        self.nan_logits()
        self.fill(recipe.at_step(t), t0, t + 1)
        _lib.check(self.pass1_cached(t), "pass1_cached")
        torch.cuda.synchronize()
        rtg = self.take("rtg")
        out = [rtg]
        if repeat_pass1:
            self.rtg.fill_(float("nan"))
            _lib.check(self.pass1_cached(t), "pass1_cached (again)")
            torch.cuda.synchronize()
            out.append(self.take("rtg"))
        self.set_bins(recipe.data, t)
        _lib.check(self.pass2(t + 1, t, 1), "pass2 cached")
        torch.cuda.synchronize()
        out.insert(1, self.take("act"))
        return tuple(out)


def compare(tag, d, classes, got, want, t, head, tol, worst=None, rel=False):
    """got [rows, n] (class after class, context after context, regular slot after regular slot) against want[k][b, slot, t] on the live slots
    of every context; rel: tol is relative to max |want| of the context's compared rows.  worst: dict updated with the largest error seen,
    {"err", "where"}.  The failure names class, context, step, head and the error against the bound."""
    r0 = 0
    for k, (B, A) in enumerate(classes):
        ar, lv = areg(d, A), live(d, A)
        g = got[r0:r0 + B * ar].reshape(B, ar, -1)
        for b in range(B):
            ref = want[k][b, :lv, t]
            err = float(np.abs(g[b, :lv].astype(np.float64) - ref).max())
            bound = tol * float(np.abs(ref).max()) if rel else tol
            if worst is not None and err / bound > worst.get("ratio", -1.0):
                worst.update(ratio=err / bound, err=err, where=f"class {k} {(B, A)} context {b} step {t} head {head}")
            assert err <= bound, f"{tag}: class {k} {(B, A)} context {b} step {t} head {head}: max error {err:.3e} > {bound:.3e}"
        r0 += B * ar
