"""GPU tests of the causal self-attention sublayer's backward (csrc/self_attn_grad.hip: ctrlsim_self_attn_block_grad) and of
ctrlsim_forward_loss_grads at scope 3 (heads + the whole last decoder layer), under both operand splits of the forward where a forward is
involved.

ACCURACY BOUND (profiles/self_attn_grad_parity.md holds every measured ratio).  The form of tests/test_gpu_attn_grads.py: for every
gradient tensor T, relative to max |T_f64| (Frobenius: to ||T_f64||),
    e_hip = max |T_hip - T_f64|,   e_ref = max |T_torch_fp32_cpu - T_f64|   (tests/self_attn_grad_ref.py in float64 / float32)
and e_hip <= K max(e_ref, 2^-24), likewise in the Frobenius norm.  K = K_BOUND below: the largest ratio measured on the device rounded
up to a power of two; the specification's ceiling is 16.

EXACT ZEROS catch mask leaks: a masked pair's probability is exactly 0, so a row that no row with a non-zero dY can see, and that has no
dY itself, has a dX of exactly 0."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import spec, weights, _lib  # noqa: E402
from ctrlsim_amd.models import CtRLSim  # noqa: E402
import loss_ref  # noqa: E402
import head_grad_ref as hgr  # noqa: E402
import ffn_grad_ref as fgr  # noqa: E402
import attn_grad_ref as agr  # noqa: E402
import self_attn_grad_ref as sgr  # noqa: E402
from gpu_utils import DEV  # noqa: E402
from helpers import golden  # noqa: E402

K_BOUND = 8.0               # largest measured ratio 5.79 (model case 7, bf16x6, in_proj_bias, Frobenius; profiles/self_attn_grad_parity.md), rounded up
FLOOR = 2.0 ** -24
LOSS_REL = 2.97e-6          # the loss route's own bound (profiles/loss_parity.md section 1; tests/test_gpu_head_grads.py)
FIX_REL = 4 * 1.741e-04     # tests/test_gpu_head_grads.py: FIX_REL
FIXTURE_CAP = 10 * FIX_REL      # the existing form (tests/test_gpu_attn_grads.py): holds where a head's ReLU sits on a kink
FIXTURE_BOUND = 1e-4            # ... and without one; largest measured deviation without a head kink 4.5e-5 (case 7, bf16x6, norm1.bias)
STEP_LOSS_REL = LOSS_REL    # the existing form (tests/test_gpu_ffn_grads.py); measured worst 1.1e-7 (case 3; case 0: 1.0e-7)
SPLITS = ["f16x3", "bf16x6"]
MODEL_CASES = (0, 1, 7)
# (B, T, A): L = 3 (row 0 sees one key); 36 (under one tile); 135 (one past a 128-query block, 27-key bands straddle tile edges); 384 (a
# 192-key band wider than any tile); 9 x 960 (two chunks, 8 + 1 contexts, and a 1024-row slab boundary); 2304 (the model's own size)
SHAPES = [(1, 1, 1), (2, 3, 4), (2, 5, 9), (1, 2, 64), (9, 10, 32), (1, 32, 24)]
MODES = [0, 1]
assert K_BOUND <= 16.0 and FIXTURE_BOUND <= FIXTURE_CAP and STEP_LOSS_REL <= 1e-5


def _split(lib, name):
    _lib.check(lib.ctrlsim_bind(1 if name == "f16x3" else 0, None))


def _check(tag, got, want64, got32, k=K_BOUND):
    """The accuracy bound of the module docstring for one tensor; prints the figures before it asserts."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    assert np.isfinite(got).all(), tag
    assert want64.any(), tag
    e_hip, f_hip = hgr.errors(got, want64)
    e_ref, f_ref = hgr.errors(got32, want64)
    assert np.isfinite([e_ref, f_ref]).all(), tag
    r, rf = e_hip / max(e_ref, FLOOR), f_hip / max(f_ref, FLOOR)
    print(f"   {tag}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {r:.2f} | F: {f_hip:.3e} {f_ref:.3e} ratio {rf:.2f}")
    assert e_hip <= k * max(e_ref, FLOOR), (tag, e_hip, e_ref)
    assert f_hip <= k * max(f_ref, FLOOR), (tag, f_hip, f_ref)
    return max(r, rf)


def _bits(t):
    return t.cpu().numpy().view(np.int32 if t.dtype == torch.float32 else np.int64)


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---- 1. the op
@functools.lru_cache(maxsize=None)
def _trained_like():
    d = spec.Dims(spec.make_cfg())
    w = weights.generate_trained_like(d, 0)
    return [np.asarray(w[k], np.float32) for k in sgr.names(d)]


@functools.lru_cache(maxsize=None)
def _op_inputs(B, T, A):
    return sgr.make_case(B, T, A, 17 + (3 * T * A) % 13, _trained_like())


@functools.lru_cache(maxsize=None)
def _op_case(B, T, A, mode):
    """Seeded inputs of one op shape with their float64 / float32 references in one mask mode (computed once, never written)."""
    X, dY, W = _op_inputs(B, T, A)
    return X, dY, W, sgr.grads(X, dY, T, A, mode, W), sgr.grads(X, dY, T, A, mode, W, dtype=torch.float32)


def _views(grads):
    out, o = [], 0
    for sz, shp in zip(sgr.SIZES, sgr.SHAPE_OF):
        out.append(grads[o:o + sz].view(shp))
        o += sz
    return out


def _run_op(X, dY, T, A, mode, W, ldx=256, lddy=256, lddx=256, want_dX=True, fill=0, alias=False):
    """ctrlsim_self_attn_block_grad on host arrays -> ([six gradient tensors], dX or None) as device tensors.  fill: a byte, or "nan"."""
    lib, st = _lib.lib(), _lib.stream_ptr()
    B = X.shape[0]
    assert X.shape[1] == 3 * T * A

    def padded(a, ld):
        t = torch.full((a.shape[0] * a.shape[1], ld), 7.0, device=DEV)
        t[:, :256] = torch.from_numpy(a.reshape(-1, 256)).to(DEV)
        return t

    Xd, dYd = padded(X, ldx), padded(dY, lddy)
    Wd = [torch.from_numpy(t).to(DEV) for t in W]
    n = int(lib.ctrlsim_self_attn_block_grad_workspace_bytes(B, T, A))
    assert n > 0 and n % 4 == 0
    if fill == "nan":
        ws = torch.full((n // 4,), float("nan"), device=DEV).view(torch.uint8)
    else:
        ws = torch.full((n,), fill, dtype=torch.uint8, device=DEV)
    grads = torch.full((sum(sgr.SIZES),), float("nan"), device=DEV)
    dXd = dYd if alias else torch.full((B * X.shape[1], lddx), 7.0, device=DEV) if want_dX else None
    _lib.check(lib.ctrlsim_self_attn_block_grad(Xd.data_ptr(), ldx, dYd.data_ptr(), lddy, *(t.data_ptr() for t in Wd), B, T, A, mode,
                                                ws.data_ptr(), grads.data_ptr(), dXd.data_ptr() if dXd is not None else None,
                                                lddy if alias else lddx, st), "self_attn_block_grad")
    torch.cuda.synchronize()
    assert torch.equal(Xd[:, :256].cpu(), torch.from_numpy(X.reshape(-1, 256)))                       # inputs intact
    if not alias:
        assert torch.equal(dYd[:, :256].cpu(), torch.from_numpy(dY.reshape(-1, 256)))
    assert all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, b in zip(Wd, W))
    for t in (dXd, Xd, dYd):
        if t is not None and t.shape[1] > 256:
            assert (t[:, 256:] == 7.0).all()                                   # nothing beyond the 256 columns of a row
    return _views(grads), (dXd[:, :256].contiguous() if dXd is not None else None)


def _check_op(got, dX, r64, r32, k=K_BOUND):
    worst = 0.0
    for name, g, a, b in zip(sgr.PARTS, got, r64[0], r32[0]):
        worst = max(worst, _check(name, g.cpu().numpy(), a, b, k))
    if dX is not None:
        worst = max(worst, _check("dX", dX.cpu().numpy().reshape(r64[1].shape), r64[1], r32[1], k))
    print(f"   worst ratio {worst:.2f}")
    return worst


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_self_attn_block_grad_matches_float64_autograd(shape, mode):
    """Every shape of the specification's table in both mask modes: all six tensors and dX against float64 autograd of the same fp32
    inputs.  At (1, 1, 1) row 0 sees one key: its dQ is exactly 0 in float32, so dX row 0 is dS row 0 plus the key / value paths only —
    checked through the bound like everything else (the float32 yardstick has the same zero)."""
    B, T, A = shape
    X, dY, W, r64, r32 = _op_case(B, T, A, mode)
    got, dX = _run_op(X, dY, T, A, mode, W)
    print(f"op B {B} T {T} A {A} (L {3 * T * A}) mode {mode}")
    _check_op(got, dX, r64, r32)


def _zero_case(B, T, A):
    X, _, W = _op_inputs(B, T, A)
    t, a, k = sgr.triples(T, A)
    return X, W, t, a, k, np.random.RandomState(5)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(2, 5, 9), (1, 2, 64), (2, 3, 4)], ids=lambda s: "x".join(map(str, s)))
def test_rows_no_gradient_can_reach_are_exactly_zero(shape, mode):
    """dY non-zero only on agent a0's three rows of the last timestep of context 0: dX rows of every other context are exactly 0; in
    mode 0 the rows (t_last, a != a0, k != 0) are exactly 0 (a0 sees of its own timestep its own tokens and the others' state tokens
    only); in mode 1 the rows (any t, a != a0, k != 0) are.  dY non-zero only at a timestep t0 < T - 1: every dX row with t > t0 is
    exactly 0 (nothing looks ahead in time).  The rows that must receive something do."""
    B, T, A = shape
    X, W, t, a, k, rs = _zero_case(B, T, A)
    L = 3 * T * A
    a0 = A // 2
    dY = np.zeros((B, L, 256), np.float32)
    sel = (t == T - 1) & (a == a0)
    dY[0, sel] = 1e-3 * rs.standard_normal((int(sel.sum()), 256)).astype(np.float32)
    _, dX = _run_op(X, dY, T, A, mode, W)
    dX = dX.cpu().numpy().reshape(B, L, 256)
    assert not dX[1:].any()
    hidden = (a != a0) & (k != 0) & ((t == T - 1) if mode == 0 else (t >= 0))
    assert not dX[0, hidden].any()
    assert dX[0, sel].any(axis=1).all() and dX[0, (t == T - 1) & (k == 0)].any(axis=1).all()
    if T > 1:
        assert dX[0, (t < T - 1) & (a == a0)].any(axis=1).all()
        assert dX[0, (t < T - 1) & ((k == 0) if mode == 1 else (k >= 0))].any(axis=1).all()
        t0 = (T - 1) // 2
        dY = np.zeros((B, L, 256), np.float32)
        dY[:, t == t0] = 1e-3 * rs.standard_normal((B, int((t == t0).sum()), 256)).astype(np.float32)
        _, dX = _run_op(X, dY, T, A, mode, W)
        dX = dX.cpu().numpy().reshape(B, L, 256)
        assert not dX[:, t > t0].any() and dX[:, t == t0].any(axis=2).all()


def test_self_attn_block_grad_one_visible_key_gives_an_exactly_zero_query_gradient():
    """(1, 1, 1) with dY on row 0 only: row 0 sees key 0 alone, P = 1 from the recomputed statistics and dSc = P (dP - delta) = 0 exactly,
    because delta comes from the same P and dP: the query rows of d in_proj_weight and d in_proj_bias are exactly 0, rows 1 and 2 of dX
    too."""
    X, _, W = _op_inputs(1, 1, 1)
    dY = np.zeros((1, 3, 256), np.float32)
    dY[0, 0] = 1e-3 * np.random.RandomState(1).standard_normal(256)
    for mode in MODES:
        got, dX = _run_op(X, dY, 1, 1, mode, W)
        gW, gb = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert not gW[:256].any() and not gb[:256].any() and gW[512:].any() and gb[512:].any()
        dX = dX.cpu().numpy()
        assert not dX[1:].any() and dX[0].any()


def test_self_attn_block_grad_leading_dimensions_null_and_aliased_dx():
    """Leading dimensions 320 / 288 / 272 for X / dY / dX give the bits of the dense call; dX = NULL leaves the six tensors unchanged;
    dX = dY (same leading dimension) gives the same dX."""
    B, T, A = 2, 5, 9
    X, dY, W, r64, r32 = _op_case(B, T, A, 0)
    dense, dX = _run_op(X, dY, T, A, 0, W)
    got, dX2 = _run_op(X, dY, T, A, 0, W, ldx=320, lddy=288, lddx=272)
    _check_op(got, dX2, r64, r32)
    assert _same(dense, got) and _same([dX], [dX2])
    got, none = _run_op(X, dY, T, A, 0, W, want_dX=False)
    assert none is None and _same(dense, got)
    got, dX3 = _run_op(X, dY, T, A, 0, W, lddy=288, alias=True)
    assert _same(dense, got) and _same([dX], [dX3])


def test_self_attn_block_grad_refuses_bad_arguments():
    lib = _lib.lib()
    x = torch.zeros(768 * 256, device=DEV)
    p = x.data_ptr()
    #     X  ldx  dY lddy Win bin Wo bo g  be B  T  A  mode ws grads dX  lddx stream
    ok = [p, 256, p, 256, p, p, p, p, p, p, 1, 1, 2, 0, p, p, None, 256, None]
    for i, v in ((10, 0), (11, 0), (12, 0), (13, 2), (13, -1), (0, None), (2, None), (4, None), (5, None), (6, None), (7, None), (8, None),
                 (9, None), (14, None), (15, None), (1, 255), (3, 255)):
        a = list(ok)
        a[i] = v
        assert lib.ctrlsim_self_attn_block_grad(*a) == -22, i       # CTRLSIM_EINVAL
    a = list(ok)
    a[16], a[17] = p, 255
    assert lib.ctrlsim_self_attn_block_grad(*a) == -22
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert lib.ctrlsim_self_attn_block_grad_workspace_bytes(*bad) < 0 and lib.ctrlsim_self_attn_block_grad_chunk_contexts(*bad) < 0
    assert lib.ctrlsim_self_attn_block_grad_chunk_contexts(9, 10, 32) == 8 and lib.ctrlsim_self_attn_block_grad_chunk_contexts(64, 32, 24) == 3
    assert lib.ctrlsim_self_attn_block_grad_chunk_contexts(2, 32, 128) == 1           # a context of more than 8192 rows: one per chunk


@pytest.mark.parametrize("mode", MODES)
def test_self_attn_block_grad_identical_bits_whatever_the_workspace_held(mode):
    X, dY, W, _, _ = _op_case(9, 10, 32, mode)
    runs = [_run_op(X, dY, 10, 32, mode, W, fill=f) for f in (0x00, 0xFF, "nan")]
    flat = lambda r: list(r[0]) + [r[1]]
    assert _same(flat(runs[0]), flat(runs[1])) and _same(flat(runs[0]), flat(runs[2]))
    assert all(torch.isfinite(x).all() for x in flat(runs[0]))


# ---- 2. through the model
def _data(inp):
    return {"agent": {k: inp[k] for k in ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask")},
            "map": {k: inp[k] for k in ("road_points", "road_types")}}


@functools.lru_cache(maxsize=None)
def _model_case(case):
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    return cfg, d, loss_ref.case_weights(case, d), loss_ref.case_inputs(case, d)


def _mode_of(d):
    return 1 if getattr(d, "MASK_OWN", False) else 0


def _layer_call(model, cb, moving, B, **kw):
    return model.loss_and_train_grads_ctx(cb, moving, B, dX=True, dU=True, x_out=True, u_out=True, dX1=True, dMem=True, x1_out=True, mem_out=True,
                                          dX0=True, x0_out=True, scope="heads+last_layer", **kw)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", MODEL_CASES)
def test_forward_loss_grad_layer_through_the_model(case, split):
    """ctrlsim_forward_loss_grads at scope 3 on fixture cases 0, 1 (tiny) and 7 (full dims, B = 2): everything the scope "heads+ffn+cross"
    returns bit-identical; the six new tensors and dX0 against the float64 sublayer applied to the returned X0 with the returned dX1 as
    dY; the six tensors against the reference's recorded gradients (tests/golden/self_grads.npz: its trunk, its float32).  Measured
    (profiles/self_attn_grad_parity.md): ratios at most 5.79 (case 7, bf16x6); deviation from the recorded gradients at most 4.5e-5 of a
    tensor's largest element in cases 1 and 7, 5.95e-3 in case 0 under f16x3, where one head hidden element sits on a ReLU kink."""
    lib = _lib.lib()
    cfg, d, w, inp = _model_case(case)
    _split(lib, split)
    try:
        model = CtRLSim(cfg, w, device=DEV)
        cb, moving, B = model._ctx_of(_data(inp))
        r2 = model.loss_and_train_grads_ctx(cb, moving, B, dX=True, dU=True, x_out=True, u_out=True, dX1=True, dMem=True, x1_out=True, mem_out=True,
                                            scope="heads+ffn+cross")
        r3 = _layer_call(model, cb, moving, B)
        assert np.array_equal(_bits(r2[0]), _bits(r3[0]))
        old, new = list(r2[1]), sgr.names(d)
        assert list(r3[1]) == old + new and old == hgr.head_names(w) + fgr.names(d) + agr.names(d)
        assert all(np.array_equal(_bits(r2[1][k]), _bits(r3[1][k])) for k in old)
        assert _same(r2[2:10], r3[2:10])                             # dX, dU, x_out, u_out, dX1, dMem, x1_out, mem_out
        dX1, dX0, x0 = r3[6], r3[10], r3[11]
        L = d.T * d.A * 3
        X0, dY = x0.cpu().numpy().reshape(B, L, 256), dX1.cpu().numpy().reshape(B, L, 256)
        W = [np.asarray(w[k], np.float32) for k in new]
        mode = _mode_of(d)
        r64, r32 = sgr.grads(X0, dY, d.T, d.A, mode, W), sgr.grads(X0, dY, d.T, d.A, mode, W, dtype=torch.float32)
        print(f"case {case} {split}: mask mode {mode}")
        _check_op([r3[1][k] for k in new], dX0, r64, r32)
        gf = golden("self_grads")
        P = f"c{case}_"
        worst = 0.0
        got = {k: r3[1][k].cpu().numpy() for k in new}
        for k in new:
            scale = np.abs(got[k]).max()
            if got[k].ndim == 1:
                err = np.abs(got[k] - gf[P + "g_" + k]).max() / scale
            else:
                rows = gf[P + "r_" + k]
                err = np.abs(got[k][rows] - gf[P + "s_" + k]).max() / scale
                csum = np.abs(got[k].astype(np.float64).sum(0) - gf[P + "c_" + k]).max() / (scale * got[k].shape[0])
                nrm = abs(np.linalg.norm(got[k].astype(np.float64)) - float(gf[P + "n_" + k])) / float(gf[P + "n_" + k])
                err = max(err, csum, nrm)
            print(f"   {k} against the reference's recorded gradient: {err:.3e} of max |T|")
            worst = max(worst, err)
        import test_gpu_ffn_grads as tff                   # the rule for head ReLU kinks, unchanged (ffn_grad_ref.KINK_TOL, head_grad_ref.HEADS)
        nk = tff._head_kinks(r3[4].cpu().numpy(), w, d.VARIANT)
        bound = FIXTURE_CAP if nk else FIXTURE_BOUND
        print(f"   worst {worst:.3e} (bound {bound:.3e}: {nk} head hidden elements on a ReLU kink)")
        assert worst <= bound
    finally:
        _split(lib, "f16x3")


@pytest.mark.parametrize("case", [0, 3])
def test_the_entry_equals_the_op_on_its_own_inputs_bit_for_bit(case):
    """Case 0 (dims.variant 0) and case 3 (attend_own_return_action: dims.variant 4): the entry's six tensors and dX0 are the op's on
    (x0_out, dX1) in the model's mask mode, bit for bit — and not the other mode's, which pins the mode selection."""
    cfg, d, w, inp = _model_case(case)
    model = CtRLSim(cfg, w, device=DEV)
    cb, moving, B = model._ctx_of(_data(inp))
    r3 = _layer_call(model, cb, moving, B)
    new = sgr.names(d)
    L = d.T * d.A * 3
    X0, dY = r3[11].cpu().numpy().reshape(B, L, 256), r3[6].cpu().numpy().reshape(B, L, 256)
    W = [np.ascontiguousarray(np.asarray(w[k], np.float32)) for k in new]
    mode = _mode_of(d)
    assert mode == (1 if case == 3 else 0) and model.hip.cdims.variant == (4 if case == 3 else 0)
    got, dX0 = _run_op(X0, dY, d.T, d.A, mode, W)
    assert _same([r3[1][k] for k in new] + [r3[10].view(-1, 256)], got + [dX0])
    other, dX0o = _run_op(X0, dY, d.T, d.A, 1 - mode, W)
    assert not _same([r3[1][new[0]]], [other[0]]) and not _same([r3[10].view(-1, 256)], [dX0o])


def test_baseline_token_layouts_are_refused():
    """The IL model (case 4: two token types per agent-step) has no (t, a, k < 3) mask: CTRLSIM_EINVAL from this entry."""
    cfg, d, w, inp = _model_case(4)
    model = CtRLSim(cfg, w, device=DEV)
    cb, moving, B = model._ctx_of(_data(inp))
    with pytest.raises(RuntimeError):
        model.loss_and_train_grads_ctx(cb, moving, B, scope="heads+last_layer")


def test_scopes_before_this_one_answer_as_before():
    cfg, d, w, inp = _model_case(0)
    model = CtRLSim(cfg, w, device=DEV)
    assert model.train_grad_layout("heads") == model.head_grad_layout()
    l2, t2 = model.train_grad_layout("heads+ffn+cross")
    l3, t3 = model.train_grad_layout("heads+last_layer")
    assert l3[:len(l2)] == l2 and [k for k, _, _ in l3[len(l2):]] == sgr.names(d) and t3 == t2 + sum(sgr.SIZES)
    assert model.train_grad_workspace_bytes(2, "heads+last_layer") > model.train_grad_workspace_bytes(2, "heads+ffn+cross")
    with pytest.raises(ValueError):
        model.loss_and_train_grads_ctx(None, None, 1, dX0=True, scope="heads+ffn+cross")


def test_the_entry_refuses_a_tap_of_a_wider_scope_and_needs_no_taps():
    """The raw ctrlsim_forward_loss_grads call on case 0: scope 1 with taps.dX0[ND-1] set, scope 6 and scope -1 return CTRLSIM_EINVAL and
    launch nothing (zeroed sums, a NaN-poisoned grads buffer and the tap keep their bits); taps = NULL at scope 3 gives the sums and
    gradients of the call with every tap, bit for bit."""
    import ctypes as C
    lib, st = _lib.lib(), _lib.stream_ptr()
    cfg, d, w, inp = _model_case(0)
    model = CtRLSim(cfg, w, device=DEV)
    cb, moving, B = model._ctx_of(_data(inp))
    lc = model.loss_cfg(True)
    coef = float(cfg.model.get("loss_action_coef", 1.0))
    ws = torch.empty(model.train_grad_workspace_bytes(B, "heads+last_layer"), dtype=torch.uint8, device=DEV)
    sums = torch.zeros(5, 2, dtype=torch.float64, device=DEV)
    grads = torch.full((model.train_grad_layout("heads+last_layer")[1],), float("nan"), device=DEV)
    dX0 = torch.full((B * d.T * d.A * 3, 256), 7.0, device=DEV)

    def call(scope, taps):
        return lib.ctrlsim_forward_loss_grads(model.hip.handle, B, d.T, C.byref(cb.struct), _lib.ptr(moving), C.byref(lc), coef, scope,
                                              ws.data_ptr(), sums.data_ptr(), None, grads.data_ptr(), taps, st)

    taps = _lib.TrainTaps()
    taps.dX0[d.ND - 1] = dX0.data_ptr()
    assert call(1, C.byref(taps)) == -22                                   # CTRLSIM_EINVAL
    assert call(6, None) == -22 and call(-1, None) == -22
    torch.cuda.synchronize()
    assert not sums.any() and torch.isnan(grads).all() and (dX0 == 7.0).all()
    assert call(3, None) == 0
    r3 = _layer_call(model, cb, moving, B)
    assert np.array_equal(_bits(sums), _bits(r3[0]))
    assert np.array_equal(_bits(grads), _bits(torch.cat([g.reshape(-1) for g in r3[1].values()])))


# ---- 3. HipModel.update
@pytest.mark.parametrize("split", SPLITS)
def test_update_of_the_sublayer_equals_a_fresh_model_bit_for_bit(split):
    lib = _lib.lib()
    _split(lib, split)
    try:
        cfg, d, w, inp = _model_case(1)
        data = _data(inp)
        model = CtRLSim(cfg, dict(w), device=DEV)
        before = model.hip.flat.clone()
        rs = np.random.RandomState(9)
        names = sgr.names(d)
        pert = lambda ks: {k: (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32) for k in ks}
        new = pert(names)
        for kw in ({}, {"cross": True}):
            with pytest.raises(KeyError):
                model.hip.update(new, **kw)                        # outside the scope "heads+last_layer" the names are refused
        assert torch.equal(before.view(torch.int32), model.hip.flat.view(torch.int32))
        model.hip.update(new, self_attn=True)
        fresh = CtRLSim(cfg, {**w, **new}, device=DEV)
        assert torch.equal(model.hip.flat.view(torch.int32), fresh.hip.flat.view(torch.int32))          # every image re-derived in place
        a, b = model.loss_sums(data)[0].cpu().numpy(), fresh.loss_sums(data)[0].cpu().numpy()
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
        assert not np.array_equal(a.view(np.int64), CtRLSim(cfg, dict(w), device=DEV).loss_sums(data)[0].cpu().numpy().view(np.int64))
        # later updates of the cross-attention sublayer (.selfq#wqp beside the NEW .selfq#wop) and of the feed-forward block
        newc, newf = pert(agr.names(d)), pert(fgr.names(d))
        model.hip.update(newc, cross=True)
        model.hip.update(newf)
        fresh = CtRLSim(cfg, {**w, **new, **newc, **newf}, device=DEV)
        assert torch.equal(model.hip.flat.view(torch.int32), fresh.hip.flat.view(torch.int32))
        snap = model.hip.flat.clone()
        with pytest.raises(FloatingPointError):
            model.hip.update({names[0]: np.full_like(new[names[0]], 1.0e6)}, cross=True, self_attn=True)
        assert torch.equal(snap.view(torch.int32), model.hip.flat.view(torch.int32))                    # nothing written
    finally:
        _split(lib, "f16x3")


# ---- 4. training loop
def _key_pad(cfg, d, inp):
    """tests/test_gpu_attn_grads.py:_key_pad (modules/encoder.py:155-170)."""
    B = np.asarray(inp["agent_states"]).shape[0]
    M = (d.P + d.A + 3) & ~3
    pad = np.ones((B, M), np.uint8)
    if bool(cfg.model.get("use_map", True)):
        pad[:, :d.P] = ~(np.asarray(inp["road_points"])[..., 2] != 0).any(-1)
    if bool(cfg.model.get("encode_initial_state", True)):
        pad[:, d.P:d.P + d.A] = np.asarray(inp["agent_states"])[:, :, 0, 7] == 0
    return pad


def _twin(cfg, d, w, X0, Mem, kp, ctx, kw, steps):
    """torch float64: the heads and the whole last decoder layer on the same (constant) layer inputs X0 and Mem, the same AdamW groups,
    clip and schedule."""
    heads, ffn, cross, new = hgr.head_names(w), fgr.names(d), agr.names(d), sgr.names(d)
    every = heads + ffn + cross + new
    params = {k: torch.nn.Parameter(torch.tensor(np.asarray(w[k]), dtype=torch.float64)) for k in every}
    decay, no_decay = CtRLSim.param_groups(every)
    tr = cfg.train
    opt = torch.optim.AdamW([{"params": [params[k] for k in decay], "weight_decay": tr["weight_decay"]},
                             {"params": [params[k] for k in no_decay], "weight_decay": 0.0}], lr=tr["lr"], weight_decay=tr["weight_decay"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=CtRLSim.lr_lambda(tr))
    mode = _mode_of(d)

    def evaluate():
        now = {k: p.detach().numpy() for k, p in params.items()}
        Ts, Tc, Tf = [now[k] for k in new], [now[k] for k in cross], [now[k] for k in ffn]
        X1 = sgr.forward(X0, d.T, d.A, mode, Ts)
        U = agr.forward(X1, Mem, kp, Tc).reshape(-1, 256)
        _, final, g, dX = hgr.loss_and_grads(fgr.forward(U, Tf), {k: now[k] for k in heads}, ctx, **kw)
        gf, dU = fgr.grads(U, dX, Tf)
        g.update(zip(ffn, gf))
        gc, dX1, _ = agr.grads(X1, Mem, kp, dU.reshape(X1.shape), Tc)
        g.update(zip(cross, gc))
        g.update(zip(new, sgr.grads(X0, dX1, d.T, d.A, mode, Ts)[0]))
        return final, g

    losses = []
    for _ in range(steps):
        final, g = evaluate()
        losses.append(final)
        for k, p in params.items():
            p.grad = torch.from_numpy(g[k])
        torch.nn.utils.clip_grad_norm_(list(params.values()), float(tr["gradient_clip_val"]))
        opt.step()
        sched.step()
    return losses + [evaluate()[0]], {k: p.detach().numpy() for k, p in params.items()}


def _kw(cfg, d):
    m = cfg.model
    return dict(variant=d.VARIANT, coef=float(m.get("loss_action_coef", 1.0)), supervise_moving=bool(m.get("supervise_moving", True)),
                local_frame=bool(m.get("local_frame_predictions", False)))


@pytest.mark.parametrize("case", [0, 3])
def test_five_training_steps_in_scope_heads_last_layer_follow_the_float64_twin(case):
    """training_step / optimizer_step five times on one fixed batch with set_trainable("heads+last_layer"), a model of each mask mode
    (tiny cases: the twin evaluates the whole layer in float64 six times).  Everything upstream of the layer is frozen, so its inputs X0
    and Mem are constant (asserted bit for bit) and a float64 twin can train the four parts on them.  Loss per step within STEP_LOSS_REL
    of the twin's.  Weights: every element within 2 sum_t lr_t sqrt(t) + 5 x 2^-24 |w| of the twin's (part (a) of
    tests/test_gpu_ffn_grads.py's criterion: what AdamW can move an element at all); its part (b) is printed, not asserted, for the
    reason tests/test_gpu_attn_grads.py gives.  Measured: case 0, loss per step within 1.0e-7, max |w - twin| 2.1e-6 at sum lr 1.0e-5,
    496 of 1 781 258 elements beyond part (b); case 3, 1.1e-7, 2.2e-6, 1 139."""
    cfg, d, w, inp = _model_case(case)
    w0 = {k: np.array(v) for k, v in w.items()}
    model = CtRLSim(cfg, dict(w0), device=DEV).set_trainable("heads+last_layer")
    data = _data(inp)
    first = model.loss_and_train_grads(data, x0_out=True, mem_out=True)
    x0, mem = first[11], first[9]
    heads, ffn, cross, new = hgr.head_names(w), fgr.names(d), agr.names(d), sgr.names(d)
    assert list(model.trainable_parameters()) == heads + ffn + cross + new
    assert all(model.trainable_parameters()[k] is model.head_parameters()[k] for k in heads)
    opt, sched = model.configure_optimizers()
    got = []
    for step in range(5):
        got.append(model.training_step(data, step))
        assert all(p.grad is not None for p in model.trainable_parameters().values())
        model.optimizer_step(opt, sched)
    out = model.loss_and_train_grads(data, x0_out=True, mem_out=True)
    got.append(model.final_loss(model.losses_from_sums(out[0].cpu().numpy())))
    assert torch.equal(x0, out[11]) and torch.equal(mem, out[9])                   # everything in front of the layer did not move
    B = np.asarray(inp["agent_states"]).shape[0]
    M = (d.P + d.A + 3) & ~3
    want, w_twin = _twin(cfg, d, w0, x0.cpu().numpy().reshape(B, -1, 256), mem.cpu().numpy().reshape(B, M, 256), _key_pad(cfg, d, inp),
                         hgr.ctx_from_inputs(inp), _kw(cfg, d), 5)
    print(f"case {case}: loss per step {got}\n         twin          {want}")
    print("         relative      " + " ".join(f"{abs(a - b) / abs(b):.3e}" for a, b in zip(got, want)))
    for a, b in zip(got, want):
        assert abs(a - b) <= STEP_LOSS_REL * abs(b)
    assert got[5] < got[0] and want[5] < want[0]
    lrs = [cfg.train["lr"] * CtRLSim.lr_lambda(cfg.train)(t) for t in range(5)]
    worst_case = 2 * sum(lr * np.sqrt(t + 1) for t, lr in enumerate(lrs))
    bulk = 1e-3 * sum(lrs)
    n_all = n_off = 0
    drift = 0.0
    for k, v in w_twin.items():
        have = (model.hip._heads if k in heads else model.hip._ffn if k in ffn else model.hip._cross if k in cross else model.hip._self)[k]
        have = have.astype(np.float64)
        assert np.array_equal(have, np.asarray(model.weights[k], np.float64))
        diff = np.abs(have - v)
        rnd = 5 * FLOOR * np.abs(v)
        assert (diff <= worst_case + rnd).all(), k
        n_all += diff.size
        n_off += int((diff > bulk + rnd).sum())
        drift = max(drift, float(diff.max()))
        assert np.abs(v - np.asarray(w0[k], np.float64)).max() > 0, k
    print(f"   weights after five steps: max |w - twin| {drift:.3e} (sum lr {sum(lrs):.1e}), {n_off} of {n_all} elements beyond the bulk tolerance")


@pytest.mark.parametrize("scope", ["heads", "heads+ffn", "heads+ffn+cross"])
def test_narrower_scopes_leave_the_sublayer_alone(scope):
    """Two training steps in a scope before this one: the six tensors and every image derived from them keep their bits."""
    cfg, d, w, inp = _model_case(0)
    model = CtRLSim(cfg, {k: np.array(v) for k, v in w.items()}, device=DEV).set_trainable(scope)
    data = _data(inp)
    assert not set(sgr.names(d)) & set(model.trainable_parameters())
    off = model.hip._offset
    order = sorted(off.values()) + [model.hip.flat.numel()]
    pre = sgr.layer_prefix(d)
    mine = torch.zeros(model.hip.flat.numel(), dtype=torch.bool, device=DEV)
    for name, o in off.items():
        if name.split("#")[0] in sgr.names(d) or name.startswith(pre + ".selfq#wop"):
            mine[o:order[order.index(o) + 1]] = True
    assert int(mine.sum()) > sum(sgr.SIZES)
    before = model.hip.flat.clone()
    opt, sched = model.configure_optimizers()
    for step in range(2):
        model.training_step(data, step)
        model.optimizer_step(opt, sched)
    assert torch.equal(before.view(torch.int32)[mine], model.hip.flat.view(torch.int32)[mine])
    assert not torch.equal(before.view(torch.int32)[~mine], model.hip.flat.view(torch.int32)[~mine])
