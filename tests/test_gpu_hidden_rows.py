"""GPU tests of the hidden rows the training entries store and their backward starts from: the assembled token rows x0_out[0], the rows
entering every decoder layer x0_out[l], the scene memory mem_out, the last layer's x1_out and u_out, the decoder output x_out
(CtRLSim.loss_and_train_grads_ctx under "heads+decoder" and "heads+last_layer") and the polyline embeddings dbg_seg_emb of
ctrlsim_dt_forward_pass1, against the staged float64 oracle of tests/hidden_cases.py, under both operand splits.  Row order: that file.

BOUND (profiles/hidden_state_parity.md holds every measured ratio; quoted below).  Per tensor kind, absolute:
    max |device - float64| <= K[kind] x e_ref,   e_ref = max |float32 oracle - float64 oracle| on the same compared rows of the batch;
(a) end to end, the oracles start from the raw inputs; (b) stage local, both evaluate ONE stage on the device's own input rows, which names
the kernel at fault and carries no accumulated error.  K[kind] = ceil(1.5 x the worst ratio measured on the MI355X over both splits and all
cases of that kind), one K per kind; no K may exceed 8.  profiles/hidden_state_parity.md, section 2: "tokens 1.42 ((a) tiny init, bf16x6) K 3;
seg 1.65 ((a) loop init, bf16x6) K 3; mem 3.78 ((b) loop init, f16x3, option 3 = 2 and 3; mem_padded 2.78) K 6; layer 2.97 ((b) tiny init,
f16x3, option 3 = 3) K 5; x1 2.22 K 4; u 2.49 ((a) tiny trained, bf16x6) K 4; x_out 2.49 ((b) tiny init, bf16x6, option 3 = 1) K 4".  e_ref is
1.0e-6 .. 2.5e-6 at the initialisation and 1.5e-6 .. 2.8e-5 at trained-like weights (section 3).  No defect was found.

WHAT THE DEVICE HOLDS IN KEY-PADDED AND FILLER ROWS OF mem_out (csrc/embed.hip: assemble_tokens_kernel; csrc/map_encoder.hip; csrc/forward.hip:
scene_side).  Every one of the M scene rows is a QUERY of the scene encoder, padded or not; padding only removes a row from the keys.  A
polyline without a point is pooled over its point 0 alone (map_encoder.py:31, model_oracle.map_encoder), the initial-state row of a slot
absent at step 0 has the source row s_emb x 0 = 0, and the filler rows P + A .. M - 1 have zero source rows.  So the key-padded rows are the
oracle's padded rows (asserted at the bound of mem, against the yardstick of those rows), and a filler row is the oracle's row of a dead slot
of the same context: the same function of the same zero source row (asserted likewise; every recipe context has a dead slot).

WHAT IS NOT OBSERVABLE.  The scene encoder works in place on its source rows, and no tap holds them: neither the polyline rows the training
forward fed it nor the initial-state rows before embed_ln.  dbg_seg_emb of the rollout's first pass is the output of the map encoder's last
Linear through the plain Linear kernel and a row copy; the training forward takes that route too under bf16x6, and under f16x3 a
weight-stationary kernel that stores the rows straight into the source (forward.hip: scene_side) — not the same kernel, so no bit equality is
asserted between them.  dbg_seg_emb is held to the bound of seg; the training forward's polyline rows are held through mem, end to end.
Stage-local mem feeds the scene encoder dbg_seg_emb and the float64 initial-state rows of the inputs."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import _lib  # noqa: E402
from ctrlsim_amd.engine import ctx_from_reference_layout  # noqa: E402
from ctrlsim_amd.models import CtRLSim  # noqa: E402
from gpu_utils import DEV  # noqa: E402
from op_cases import split  # noqa: E402,F401  (the fixture that binds the operand split)
import hidden_cases as hc  # noqa: E402

SPLITS = ["f16x3", "bf16x6"]
# ceil(1.5 x worst measured ratio) per tensor kind; profiles/hidden_state_parity.md, section 2
# worst ratios: tokens 1.42, seg 1.65, mem 3.78, layer 2.97, x1 2.22, u 2.49, x_out 2.49
K = {"tokens": 3, "seg": 3, "mem": 6, "layer": 5, "x1": 4, "u": 4, "x_out": 4}
assert set(K) == set(hc.KINDS) and max(K.values()) <= 8
OPT_ATTN, OPT_GEMM, OPT_FFN_FUSED = 1, 0, 3       # csrc/common.h


def _data(inp):
    return {"agent": {k: inp[k] for k in ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask")},
            "map": {k: inp[k] for k in ("road_points", "road_types")}}


@contextlib.contextmanager
def _bound(split_name, opts=None, guard=None):
    """The split with a guard pair and an option table bound for the calls inside, released on the way out."""
    lib = _lib.lib()
    scheme = 1 if split_name == "f16x3" else 0
    _lib.check(lib.ctrlsim_bind(scheme, guard.data_ptr() if guard is not None else None))
    try:
        if opts:
            n = lib.ctrlsim_option_count()
            vals = (C.c_int * n)(*([-1] * n))
            for i, v in opts.items():
                vals[i] = v
            _lib.check(lib.ctrlsim_bind_options(vals))
            assert all(lib.ctrlsim_get_option(i) == v for i, v in opts.items())
        yield
    finally:
        lib.ctrlsim_bind_options(None)
        lib.ctrlsim_bind(scheme, None)


def _taps(model, d, inp, fill=None):
    """Every hidden tap of the two training entries and dbg_seg_emb of the first pass, as float32 host arrays in the staged oracle's form
    (mem: [B, M, 256] with the filler rows).  fill: a byte every workspace is prefilled with."""
    cb, moving, B = model._ctx_of(_data(inp))
    ws = {}
    for scope in ("heads+decoder", "heads+last_layer"):
        n = model.train_grad_workspace_bytes(B, scope)
        ws[scope] = torch.empty(n, dtype=torch.uint8, device=DEV) if fill is None else torch.full((n,), fill, dtype=torch.uint8, device=DEV)
    rd = model.loss_and_train_grads_ctx(cb, moving, B, x_out=True, mem_out=True, x0_out=True, scope="heads+decoder", workspace=ws["heads+decoder"])
    r3 = model.loss_and_train_grads_ctx(cb, moving, B, x_out=True, u_out=True, x1_out=True, mem_out=True, x0_out=True, scope="heads+last_layer",
                                        workspace=ws["heads+last_layer"])
    x_out, mem, x0 = rd[3], rd[5], rd[7]
    u, x1 = r3[5], r3[8]
    # the rollout's first pass over the same inputs
    cb1 = ctx_from_reference_layout(d, inp, d.T, DEV)
    cb1.slot_gid.copy_(torch.arange(d.A, dtype=torch.int32, device=DEV).expand(B, d.A))
    n = model.hip.workspace_bytes(B, d.T)
    ws1 = torch.empty(n, dtype=torch.uint8, device=DEV) if fill is None else torch.full((n,), fill, dtype=torch.uint8, device=DEV)
    rtg = torch.empty(B, d.A, d.R * d.C, device=DEV)
    seg = torch.full((B, d.P, 256), float("nan"), device=DEV)
    _lib.check(_lib.lib().ctrlsim_dt_forward_pass1(model.hip.handle, B, d.T, C.byref(cb1.struct), ws1.data_ptr(), rtg.data_ptr(), seg.data_ptr(),
                                                   _lib.stream_ptr()), "pass1")
    torch.cuda.synchronize()
    rows = lambda t: t.cpu().numpy().reshape(B, -1, 256)
    assert len(x0) == d.ND and rows(mem).shape[1] == (d.P + d.A + 3) & ~3
    return dict(tokens=rows(x0[0]), x0=[rows(t) for t in x0], mem=rows(mem), x1_last=rows(x1), u_last=rows(u), x_out=rows(x_out), seg=rows(seg))


def _bits(s):
    flat = [s[k] for k in ("mem", "x1_last", "u_last", "x_out", "seg")] + list(s["x0"])
    return [np.ascontiguousarray(t).view(np.int32) for t in flat]


def _model(kind, wkind, own):
    cfg, d = hc.cfg_dims(kind, own)
    return CtRLSim(cfg, dict(hc.make_weights(kind, wkind, own)), device=DEV), d


def _run(split_name, kind, wkind, own=False, opts=None, fill=None):
    """The taps of a preset's recipe under a split and an option table; at trained-like weights with a guard pair bound, which must read
    [0, 0] afterwards: no row left the range of the fp16 planes."""
    model, d = _model(kind, wkind, own)
    guard = torch.zeros(2, dtype=torch.int32, device=DEV) if wkind == "trained" else None
    with _bound(split_name, opts, guard):
        s = _taps(model, d, hc.recipe(kind), fill)
    if guard is not None:
        assert guard.tolist() == [0, 0], "non-finite rows at trained-like weights"
    assert all(np.isfinite(t).all() for t in [s["mem"], s["x1_last"], s["u_last"], s["x_out"], s["seg"]] + s["x0"])
    return s, d


def _judge(tag, err, ref, kinds=hc.KINDS):
    """Prints every figure, then asserts the bound of each kind."""
    bad = []
    for k in kinds:
        ratio = err[k] / ref[k]
        print(f"\nHR|{tag}|{k}|err {err[k]:.3e}|e_ref {ref[k]:.3e}|ratio {ratio:.2f}|K {K[k]}")
        assert np.isfinite(ref[k]) and ref[k] > 0
        if not err[k] <= K[k] * ref[k]:
            bad.append((k, err[k], ref[k], round(ratio, 2)))
    assert not bad, (tag, bad)


E2E = [("tiny", "init", False), ("tiny", "trained", False), ("tiny", "init", True), ("tiny", "trained", True), ("loop", "init", False),
       ("loop", "trained", False), ("full", "trained", False)]


@pytest.mark.parametrize("split", SPLITS, indirect=True)
@pytest.mark.parametrize("kind,wkind,own", E2E, ids=lambda v: {True: "own", False: "plain"}.get(v, v) if isinstance(v, bool) else v)
def test_hidden_rows_end_to_end_against_the_float64_oracle(kind, wkind, own, split):
    """(a) tokens (every row, those of non-existing agents too), seg, mem (the rows that are not key-padded), the rows entering the layers
    1 .. ND-1, the last layer's x1 and u, and x_out against hidden_cases.staged in float64 from the raw inputs.  The key-padded and the filler
    rows of mem: the module docstring.
    profiles/hidden_state_parity.md, section 2: see K above."""
    s, d = _run(split, kind, wkind, own)
    s64 = hc.staged_of(kind, wkind, torch.float64, own)
    ref = hc.yardstick(kind, wkind, own)
    pad = s64["pad"]
    tag = f"a|{split}|{kind}|{wkind}|{'own' if own else 'plain'}"
    _judge(tag, hc.errors(hc.compared(s, pad), hc.compared(s64, pad)), ref)
    # key-padded rows and filler rows of the scene memory
    s32 = hc.staged_of(kind, wkind, torch.float32, own)
    PA, M = d.P + d.A, s["mem"].shape[1]
    e_pad = hc.dist(s32["mem"][pad], s64["mem"][pad])
    err = hc.dist(s["mem"][:, :PA][pad], s64["mem"][pad])
    for b, a in hc.edges(hc.recipe(kind))["dead_between"]:
        for e in range(PA, M):
            err = max(err, hc.dist(s["mem"][b, e], s64["mem"][b, d.P + a]))
    print(f"\nHR|{tag}|mem_padded|err {err:.3e}|e_ref {e_pad:.3e}|ratio {err / e_pad:.2f}|K {K['mem']}")
    assert pad.any() and e_pad > 0 and err <= K["mem"] * e_pad, (err, e_pad)


DEFAULT = None
FUSED = [{OPT_FFN_FUSED: v} for v in range(4)]
F32 = {OPT_GEMM: 0, OPT_ATTN: 0}
LOCAL = ([("tiny", w, o) for w in hc.WEIGHTS for o in FUSED] + [("loop", w, o) for w in hc.WEIGHTS for o in FUSED + [F32]]
         + [("full", "trained", DEFAULT)])
_oid = lambda o: "default" if o is None else "f32" if o is F32 else f"fused{o[OPT_FFN_FUSED]}"


def _stage_local(s, d, kind, wkind, dtype):
    """Every stage on the DEVICE's input rows in `dtype` -> compared()-form dict of what the stage should have produced."""
    tw = hc.torch_weights(hc.make_weights(kind, wkind), dtype)
    s64 = hc.staged_of(kind, wkind, torch.float64)
    pad = torch.from_numpy(s64["pad"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    PA = d.P + d.A
    mem = hc.stage_mem(tw, t(s["seg"]), t(s64["init_rows"]), pad, d, dtype)
    out = {"mem": [mem.numpy()[s64["pad"] == 0]], "layer": []}
    mem_dev = t(s["mem"][:, :PA])
    for l in range(d.ND):
        Y, X1, U = hc.stage_layer(tw, l, t(s["x0"][l]), mem_dev, pad, d)
        if l < d.ND - 1:
            out["layer"].append(Y.numpy())
    out.update(x1=[X1.numpy()], u=[U.numpy()], x_out=[Y.numpy()])
    return out


@pytest.mark.parametrize("split", SPLITS, indirect=True)
@pytest.mark.parametrize("kind,wkind,opts", LOCAL, ids=lambda v: v if isinstance(v, str) else _oid(v))
def test_hidden_rows_stage_by_stage_on_the_devices_own_input_rows(kind, wkind, opts, split):
    """(b) x0[l + 1] against the float64 layer on (x0[l], mem_out, pad); x1_last, u_last and x_out against the last layer on x0[ND-1];
    mem against the scene encoder on (dbg_seg_emb, the initial-state rows).  Yardstick: the same stage in float32 torch on the same device
    rows.  Under every setting of option 3 (the fusion of the out-projection, norm and feed-forward kernels) at tiny and loop, and with
    options 0 and 1 at 0 (the f32-input MFMA kernels) at loop; full dims once, at the defaults.
    profiles/hidden_state_parity.md, section 2: see K above."""
    s, d = _run(split, kind, wkind, opts=opts)
    pad = hc.staged_of(kind, wkind, torch.float64)["pad"]
    got = {k: v for k, v in hc.compared(s, pad).items() if k not in ("tokens", "seg")}
    want = _stage_local(s, d, kind, wkind, torch.float64)
    ref = hc.errors(_stage_local(s, d, kind, wkind, torch.float32), want)
    _judge(f"b|{split}|{kind}|{wkind}|{_oid(opts)}", hc.errors(got, want), ref, kinds=[k for k in hc.KINDS if k in want])


@pytest.mark.parametrize("split", SPLITS, indirect=True)
@pytest.mark.parametrize("kind", ["tiny", "loop"])
def test_hidden_rows_keep_their_bits_whatever_the_workspace_held_and_on_a_second_call(kind, split):
    """(c) every tap bit-identical with the workspaces prefilled with 0x00 and with 0xFF, and in a second identical call."""
    model, d = _model(kind, "trained", False)
    guard = torch.zeros(2, dtype=torch.int32, device=DEV)
    with _bound(split, None, guard):
        runs = [_bits(_taps(model, d, hc.recipe(kind), fill)) for fill in (0x00, 0xFF, 0xFF)]
    assert guard.tolist() == [0, 0]
    names = ["mem", "x1", "u", "x_out", "seg"] + [f"x0[{l}]" for l in range(d.ND)]
    for other, what in ((runs[1], "0xFF against 0x00"), (runs[2], "a second call")):
        for n, a, b in zip(names, runs[0], other):
            assert np.array_equal(a, b), (what, n)


@pytest.mark.parametrize("split", SPLITS, indirect=True)
@pytest.mark.parametrize("kind", ["tiny", "loop"])
def test_rollout_front_end_polyline_embeddings_at_trained_like_weights(kind, split):
    """(d) dbg_seg_emb of ctrlsim_dt_forward_pass1 at trained-like weights on the edge recipes (one point, all points, no point in the middle
    of the list, every road type) against the float64 seg, every polyline row; the window length does not enter: the first pass of a
    one-step window gives the same bits.  (Not bit-equal to the training forward's polyline rows by construction: the module docstring.)"""
    model, d = _model(kind, "trained", False)
    inp = hc.recipe(kind)
    B = hc.PRESETS[kind][1]
    guard = torch.zeros(2, dtype=torch.int32, device=DEV)
    segs = []
    with _bound(split, None, guard):
        for Tq in (d.T, 1):
            cb = ctx_from_reference_layout(d, inp, Tq, DEV)
            cb.slot_gid.copy_(torch.arange(d.A, dtype=torch.int32, device=DEV).expand(B, d.A))
            ws = torch.full((model.hip.workspace_bytes(B, Tq),), 0xFF, dtype=torch.uint8, device=DEV)
            rtg = torch.empty(B, d.A, d.R * d.C, device=DEV)
            seg = torch.full((B, d.P, 256), float("nan"), device=DEV)
            _lib.check(_lib.lib().ctrlsim_dt_forward_pass1(model.hip.handle, B, Tq, C.byref(cb.struct), ws.data_ptr(), rtg.data_ptr(),
                                                           seg.data_ptr(), _lib.stream_ptr()), "pass1")
            torch.cuda.synchronize()
            segs.append(seg.cpu().numpy())
    assert guard.tolist() == [0, 0]
    s64 = hc.staged_of(kind, "trained", torch.float64)
    err = {"seg": hc.dist(segs[0], s64["seg"])}
    _judge(f"d|{split}|{kind}|trained|pass1", err, hc.yardstick(kind, "trained"), kinds=["seg"])
    assert np.array_equal(segs[0].view(np.int32), segs[1].view(np.int32))
