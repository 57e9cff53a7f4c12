"""GPU tests of the decoder layer's backward by recompute (csrc/decoder_layer_grad.hip: ctrlsim_decoder_layer_grad) and of
ctrlsim_forward_loss_grads at scope 4 (heads + every decoder layer), the latter under both operand splits of the forward.

ACCURACY BOUND (profiles/decoder_grad_parity.md holds every measured ratio).  The form of tests/test_gpu_self_attn_grads.py (_check): for
every tensor T, relative to max |T_f64| (Frobenius: to ||T_f64||),
    e_hip = max |T_hip - T_f64|,   e_ref = max |T_torch_fp32_cpu - T_f64|   (tests/layer_grad_ref.py in float64 / float32)
and e_hip <= K max(e_ref, 2^-24), likewise in the Frobenius norm.  The float64 twin and the float32 yardstick use the ReLU on / off
pattern of the evaluation under test (layer_grad_ref.relu_pattern): the op recomputes U in float32, so a hidden pre-activation within
rounding of zero can fall on the other side of the kink than in float64."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import spec, weights, _lib  # noqa: E402
import attn_grad_ref as agr  # noqa: E402
import layer_grad_ref as lgr  # noqa: E402
from gpu_utils import DEV  # noqa: E402
from test_gpu_self_attn_grads import _check, _bits, _same  # noqa: E402

K_LAYER = 6.0               # largest measured ratio 5.10 (model case 7, bf16x6, layer 1, self_attn.out_proj.weight; the op alone: 3.80 at 2x3x4x7x1024,
                            # mode 1, self_attn.out_proj.weight; profiles/decoder_grad_parity.md), rounded up to the next whole number
# (B, T, A, Lk, F), key padding: smallest; odd Lk with a padded tail; tile-edge Lk, odd F, scattered; 384 rows (the 192-key band), a whole
# padded 64-key tile; two chunks (8 + 1 contexts), a slab edge, one context with every key padded; the model's own sizes
SHAPES = [((1, 1, 1, 4, 8), "none"), ((2, 3, 4, 7, 1024), "tail"), ((2, 5, 9, 64, 33), "scattered"), ((1, 2, 64, 65, 1024), "tile"),
          ((9, 10, 32, 12, 1024), "context"), ((1, 32, 24, 224, 1024), "tail")]
MODES = [0, 1]
_ids = lambda s: "x".join(map(str, s[0])) + "-" + s[1]


@functools.lru_cache(maxsize=None)
def _trained_like():
    d = spec.Dims(spec.make_cfg())
    w = weights.generate_trained_like(d, 0)
    return [np.asarray(w[k], np.float32) for k in lgr.names(d.ND - 1)]


@functools.lru_cache(maxsize=None)
def _op_inputs(B, T, A, Lk, F, pad):
    rs = np.random.RandomState(3 + Lk)
    return lgr.make_case(B, T, A, Lk, F, 29 + (3 * T * A + Lk) % 17, _trained_like()) + (agr.make_pad(B, Lk, pad, rs),)


def _dev(a, ld=256):
    a = np.asarray(a, np.float32).reshape(-1, 256)
    t = torch.full((a.shape[0], ld), 7.0, device=DEV)
    t[:, :256] = torch.from_numpy(a).to(DEV)
    return t


def _views(grads, F):
    out, o = [], 0
    for sz, shp in zip(lgr.sizes(F), lgr.shapes(F)):
        out.append(grads[o:o + sz].view(shp))
        o += sz
    return out


def _workspace(n, fill):
    assert n > 0 and n % 4 == 0
    if fill == "nan":
        return torch.full((n // 4,), float("nan"), device=DEV).view(torch.uint8)
    return torch.full((n,), fill, dtype=torch.uint8, device=DEV)


def _run_op(X0, Mem, pad, dY, T, A, F, mode, W, ldx=256, ldm=256, lddy=256, lddx0=256, lddm=256, want_dX0=True, dMem="new", accumulate=0,
            taps=True, fill=0, alias=False):
    """ctrlsim_decoder_layer_grad on host arrays -> ([18 gradient tensors], dX0, dMem, x1_out, u_out) as device tensors (None where not
    asked for).  dMem: "new" (a buffer of 7s), None, or a device tensor [B Lk, lddm] to write / accumulate into.  fill: a byte, or "nan"."""
    lib, st = _lib.lib(), _lib.stream_ptr()
    B, L, Lk = X0.shape[0], X0.shape[1], Mem.shape[1]
    assert L == 3 * T * A
    Xd, Md, dYd = _dev(X0, ldx), _dev(Mem, ldm), _dev(dY, lddy)
    Wd = [torch.from_numpy(t).to(DEV) for t in W]
    ptrs = (ctypes.c_void_p * 18)(*(t.data_ptr() for t in Wd))
    pd = torch.from_numpy(pad).to(DEV) if pad is not None else None
    ws = _workspace(int(lib.ctrlsim_decoder_layer_grad_workspace_bytes(B, T, A, Lk, F)), fill)
    grads = torch.full((sum(lgr.sizes(F)),), float("nan"), device=DEV)
    dXd = dYd if alias else torch.full((B * L, lddx0), 7.0, device=DEV) if want_dX0 else None
    dMd = torch.full((B * Lk, lddm), 7.0, device=DEV) if isinstance(dMem, str) else dMem
    x1 = torch.full((B * L, 256), float("nan"), device=DEV) if taps else None
    u = torch.full((B * L, 256), float("nan"), device=DEV) if taps else None
    p = lambda t: t.data_ptr() if t is not None else None
    _lib.check(lib.ctrlsim_decoder_layer_grad(Xd.data_ptr(), ldx, Md.data_ptr(), ldm, p(pd), dYd.data_ptr(), lddy, ptrs, B, T, A, Lk, F, mode,
                                              ws.data_ptr(), grads.data_ptr(), p(dXd), lddy if alias else lddx0, p(dMd), lddm, accumulate,
                                              p(x1), p(u), st), "decoder_layer_grad")
    torch.cuda.synchronize()
    assert torch.equal(Xd[:, :256].cpu(), torch.from_numpy(X0.reshape(-1, 256)))                      # inputs intact
    assert torch.equal(Md[:, :256].cpu(), torch.from_numpy(Mem.reshape(-1, 256)))
    if not alias:
        assert torch.equal(dYd[:, :256].cpu(), torch.from_numpy(dY.reshape(-1, 256)))
    assert all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, b in zip(Wd, W))
    for t in (dXd, Xd, dYd, Md, dMd):
        if t is not None and t.shape[1] > 256:
            assert (t[:, 256:] == 7.0).all()                                   # nothing beyond the 256 columns of a row
    cut = lambda t: t[:, :256].contiguous() if t is not None else None
    return _views(grads, F), cut(dXd), cut(dMd), x1, u


def _references(X0, Mem, pad, dY, T, A, F, mode, W, got, u_seen):
    """The float64 twin and the float32 yardstick of one op call, under the ReLU pattern the call used (its u_out and db1)."""
    L = X0.shape[1]
    # dY of the feed-forward block is the op's dY; the pattern is read from the U the op computed
    on, nk = lgr.relu_pattern(u_seen.cpu().numpy(), dY, W[0:6], got[1].cpu().numpy())
    on = on.reshape(-1, F)
    r64 = lgr.grads(X0, Mem, pad, dY, T, A, mode, W, relu_on=on)
    r32 = lgr.grads(X0, Mem, pad, dY, T, A, mode, W, dtype=torch.float32, relu_on=on)
    return r64, r32, nk


def _check_layer(got, dX0, dMem, x1, u, r64, r32, k=K_LAYER):
    worst = {}
    for name, g, a, b in zip(lgr.PARTS, got, r64[0], r32[0]):
        worst[name] = _check(name, g.cpu().numpy(), a, b, k)
    for name, g, i in (("dX0", dX0, 1), ("dMem", dMem, 2), ("x1_out", x1, 3), ("u_out", u, 4)):
        if g is not None:
            worst[name] = _check(name, g.cpu().numpy().reshape(r64[i].shape), r64[i], r32[i], k)
    top = max(worst, key=worst.get)
    print(f"   worst ratio {worst[top]:.2f} ({top})")
    return worst[top]


# ---- 1. the op
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_decoder_layer_grad_matches_float64_autograd(shape, mode):
    """Every shape of the specification's table in both mask modes: all 18 tensors, dX0, dMem, x1_out and u_out against float64 autograd
    of the composed layer on the same fp32 inputs; rows of padded keys have a dMem of exactly zero."""
    (B, T, A, Lk, F), padk = shape
    X0, Mem, dY, W, pad = _op_inputs(B, T, A, Lk, F, padk)
    got, dX0, dMem, x1, u = _run_op(X0, Mem, pad, dY, T, A, F, mode, W)
    r64, r32, nk = _references(X0, Mem, pad, dY, T, A, F, mode, W, got, u)
    print(f"op B {B} T {T} A {A} (L {3 * T * A}) Lk {Lk} F {F} pad {padk} mode {mode}: {nk} hidden elements on a ReLU kink")
    _check_layer(got, dX0, dMem, x1, u, r64, r32)
    if pad is not None:
        assert not dMem.cpu().numpy().reshape(B, Lk, 256)[pad.astype(bool)].any()


def _three_ops_by_hand(X0, Mem, pad, dY, T, A, F, mode, W, x1, u):
    """The three public ops on the layer op's own x1_out and u_out -> ([18 tensors], dX0, dMem)."""
    lib, st = _lib.lib(), _lib.stream_ptr()
    B, L, Lk = X0.shape[0], X0.shape[1], Mem.shape[1]
    Xd, Md, dYd = _dev(X0), _dev(Mem), _dev(dY)
    Wd = [torch.from_numpy(t).to(DEV) for t in W]
    pd = torch.from_numpy(pad).to(DEV) if pad is not None else None
    wp = [t.data_ptr() for t in Wd]
    grads = torch.full((sum(lgr.sizes(F)),), float("nan"), device=DEV)
    sz = lgr.sizes(F)
    gF, gA = sum(sz[:6]), sum(sz[6:12])
    dU, dX1, dX0 = (torch.full((B * L, 256), 7.0, device=DEV) for _ in range(3))
    dMem = torch.full((B * Lk, 256), 7.0, device=DEV)
    ws = _workspace(int(lib.ctrlsim_ffn_block_grad_workspace_bytes(B * L, F)), 0x55)
    _lib.check(lib.ctrlsim_ffn_block_grad(u.data_ptr(), 256, dYd.data_ptr(), 256, *wp[0:6], B * L, F, ws.data_ptr(), grads.data_ptr(),
                                          dU.data_ptr(), 256, st), "ffn_block_grad")
    ws = _workspace(int(lib.ctrlsim_attn_block_grad_workspace_bytes(B, L, Lk)), 0x55)
    _lib.check(lib.ctrlsim_attn_block_grad(x1.data_ptr(), 256, Md.data_ptr(), 256, pd.data_ptr() if pd is not None else None, dU.data_ptr(), 256,
                                           *wp[6:12], B, L, Lk, ws.data_ptr(), grads.data_ptr() + 4 * gF, dX1.data_ptr(), 256, dMem.data_ptr(),
                                           256, st), "attn_block_grad")
    ws = _workspace(int(lib.ctrlsim_self_attn_block_grad_workspace_bytes(B, T, A)), 0x55)
    _lib.check(lib.ctrlsim_self_attn_block_grad(Xd.data_ptr(), 256, dX1.data_ptr(), 256, *wp[12:18], B, T, A, mode, ws.data_ptr(),
                                                grads.data_ptr() + 4 * (gF + gA), dX0.data_ptr(), 256, st), "self_attn_block_grad")
    torch.cuda.synchronize()
    return _views(grads, F), dX0, dMem


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=_ids)
def test_decoder_layer_grad_equals_the_three_ops_by_hand(shape):
    """Bit for bit: the 18 tensors, dX0 and dMem equal ctrlsim_ffn_block_grad, ctrlsim_attn_block_grad and ctrlsim_self_attn_block_grad
    called by hand on the op's own x1_out and u_out (mask mode 1 on the two-chunk shape, 0 on the other)."""
    (B, T, A, Lk, F), padk = shape
    mode = 1 if B > 2 else 0
    X0, Mem, dY, W, pad = _op_inputs(B, T, A, Lk, F, padk)
    got, dX0, dMem, x1, u = _run_op(X0, Mem, pad, dY, T, A, F, mode, W)
    g2, dX0b, dMemb = _three_ops_by_hand(X0, Mem, pad, dY, T, A, F, mode, W, x1, u)
    assert _same(got, g2) and _same([dX0, dMem], [dX0b, dMemb])


def test_decoder_layer_grad_accumulates_dmem_in_a_fixed_order():
    """Two calls with different dY into one dMem, the second with accumulate_dmem: bit for bit the float32 sum of the two calls' own
    dMem (one owner per element adds once).  Rows of padded keys: exactly zero without the flag, untouched with it (their prior
    contents, here 3.25 and a float32 denormal, keep their bits)."""
    (B, T, A, Lk, F), padk = SHAPES[1]
    X0, Mem, dY, W, pad = _op_inputs(B, T, A, Lk, F, padk)
    dY2 = np.ascontiguousarray(dY[::-1] * np.float32(0.5))
    _, _, d1, _, _ = _run_op(X0, Mem, pad, dY, T, A, F, 0, W)
    _, _, d2, _, _ = _run_op(X0, Mem, pad, dY2, T, A, F, 0, W)
    padded = torch.from_numpy(pad.astype(bool).reshape(-1)).to(DEV)
    assert padded.any() and not d1[padded].any() and not d2[padded].any() and d1[~padded].any() and d2[~padded].any()
    acc = torch.full((B * Lk, 320), 7.0, device=DEV)
    _run_op(X0, Mem, pad, dY, T, A, F, 0, W, dMem=acc, lddm=320)
    assert np.array_equal(_bits(acc[:, :256].contiguous()), _bits(d1))
    _run_op(X0, Mem, pad, dY2, T, A, F, 0, W, dMem=acc, lddm=320, accumulate=1)
    assert np.array_equal(_bits(acc[:, :256].contiguous()), _bits(d1.cpu() + d2.cpu()))
    prior = torch.full((B * Lk, 256), 3.25, device=DEV)
    prior[:, 1::2] = 1.0e-41
    before = prior.clone()
    _run_op(X0, Mem, pad, dY, T, A, F, 0, W, dMem=prior, accumulate=1)
    assert np.array_equal(_bits(prior[padded]), _bits(before[padded]))
    assert np.array_equal(_bits(prior[~padded]), _bits(before[~padded].cpu() + d1[~padded].cpu()))


@pytest.mark.parametrize("mode", MODES)
def test_decoder_layer_grad_identical_bits_whatever_the_workspace_held(mode):
    (B, T, A, Lk, F), padk = SHAPES[4]
    X0, Mem, dY, W, pad = _op_inputs(B, T, A, Lk, F, padk)
    runs = [_run_op(X0, Mem, pad, dY, T, A, F, mode, W, fill=f) for f in (0x00, 0xFF, "nan")]
    flat = lambda r: list(r[0]) + list(r[1:])
    assert _same(flat(runs[0]), flat(runs[1])) and _same(flat(runs[0]), flat(runs[2]))
    assert all(torch.isfinite(x).all() for x in flat(runs[0]))


def test_decoder_layer_grad_leading_dimensions_null_optionals_and_aliased_dx0():
    """Leading dimensions 320 / 304 / 288 / 272 / 336 for X0 / Mem / dY / dX0 / dMem give the bits of the dense call; every optional
    output NULL leaves the 18 tensors unchanged; dX0 = dY (same leading dimension) gives the same dX0."""
    (B, T, A, Lk, F), padk = SHAPES[2]
    X0, Mem, dY, W, pad = _op_inputs(B, T, A, Lk, F, padk)
    dense = _run_op(X0, Mem, pad, dY, T, A, F, 0, W)
    wide = _run_op(X0, Mem, pad, dY, T, A, F, 0, W, ldx=320, ldm=304, lddy=288, lddx0=272, lddm=336)
    assert _same(dense[0], wide[0]) and _same(dense[1:], wide[1:])
    bare = _run_op(X0, Mem, pad, dY, T, A, F, 0, W, want_dX0=False, dMem=None, taps=False)
    assert bare[1:] == (None, None, None, None) and _same(dense[0], bare[0])
    ali = _run_op(X0, Mem, pad, dY, T, A, F, 0, W, lddy=288, alias=True)
    assert _same(dense[0], ali[0]) and _same(dense[1:], ali[1:])
    nopad = _run_op(X0, Mem, None, dY, T, A, F, 0, W)
    assert not _same(dense[0][6:7], nopad[0][6:7])                              # the padding bytes are read


def test_decoder_layer_grad_refuses_bad_arguments():
    lib = _lib.lib()
    x = torch.zeros(1024 * 256, device=DEV)
    p = x.data_ptr()
    tn = (ctypes.c_void_p * 18)(*([p] * 18))
    #     X0 ldx  Mem ldm key dY lddy tn  B  T  A  Lk F  mode ws grads dX0  lddx0 dMem lddm acc x1   u    stream
    ok = [p, 256, p, 256, None, p, 256, tn, 1, 1, 2, 3, 4, 0, p, p, None, 256, None, 256, 0, None, None, None]
    for i, v in ((0, None), (2, None), (5, None), (7, None), (14, None), (15, None), (1, 255), (3, 255), (6, 255), (8, 0), (9, 0), (10, 0),
                 (11, 0), (12, 0), (13, 2), (13, -1), (8, 1 << 20)):
        a = list(ok)
        a[i] = v
        assert lib.ctrlsim_decoder_layer_grad(*a) == -22, i         # CTRLSIM_EINVAL
    for i in range(18):                                             # each of the 18 tensors is required
        bad = (ctypes.c_void_p * 18)(*([p] * 18))
        bad[i] = None
        a = list(ok)
        a[7] = bad
        assert lib.ctrlsim_decoder_layer_grad(*a) == -22, i
    for i, j in ((16, 17), (18, 19)):                               # a given dX0 / dMem with a leading dimension below 256
        a = list(ok)
        a[i], a[j] = p, 255
        assert lib.ctrlsim_decoder_layer_grad(*a) == -22
    for bad in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (1 << 20, 1, 2, 3, 4)):
        assert lib.ctrlsim_decoder_layer_grad_workspace_bytes(*bad) < 0
    assert 466034 * 6 * 768 >= 2 ** 31 > 466033 * 6 * 768           # B * 3TA * 768 against 2^31 at T = 1, A = 2
    assert lib.ctrlsim_decoder_layer_grad_workspace_bytes(466034, 1, 2, 1, 1) < 0 < lib.ctrlsim_decoder_layer_grad_workspace_bytes(466033, 1, 2, 1, 1)
    torch.cuda.synchronize()


# ---- 2. through the model
from ctrlsim_amd.models import CtRLSim  # noqa: E402
import loss_ref  # noqa: E402
import head_grad_ref as hgr  # noqa: E402
import ffn_grad_ref as fgr  # noqa: E402
import self_attn_grad_ref as sgr  # noqa: E402
from test_gpu_self_attn_grads import _data, _model_case, _mode_of, _split, SPLITS, MODEL_CASES, LOSS_REL, FLOOR  # noqa: E402
from test_gpu_attn_grads import _key_pad, _kw  # noqa: E402

K_STACK = 4.0               # largest measured ratio 3.51 (case 0, f16x3, the last layer; profiles/decoder_grad_parity.md), rounded up
STEP_LOSS_REL = LOSS_REL    # the existing form (tests/test_gpu_ffn_grads.py)


def _both(model, cb, moving, B):
    """("heads+last_layer" with every tap, "heads+decoder" with every tap) on the same contexts."""
    r3 = model.loss_and_train_grads_ctx(cb, moving, B, dX=True, dU=True, x_out=True, u_out=True, dX1=True, dMem=True, x1_out=True, mem_out=True,
                                        dX0=True, x0_out=True, scope="heads+last_layer")
    rd = model.loss_and_train_grads_ctx(cb, moving, B, dX=True, x_out=True, dMem=True, mem_out=True, dX0=True, x0_out=True, scope="heads+decoder")
    return r3, rd


def _layer_weights(w, l):
    return [np.ascontiguousarray(np.asarray(w[k], np.float32)) for k in lgr.names(l)]


def _rows(t, B):
    return t.cpu().numpy().reshape(B, -1, 256)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", MODEL_CASES)
def test_forward_loss_grads_decoder_layer_by_layer(case, split):
    """ctrlsim_forward_loss_grads at scope 4 on fixture cases 0, 1 (tiny, ND 4) and 7 (full dims, B 2, ND 4).  Bit for bit: the loss sums,
    the scope-3 prefix of the gradients, dX, x_out, mem_out, the last layer's dX0 and x0_out equal "heads+last_layer"; for l = ND-2 .. 0
    the layer's 18 tensors and dX0[l] equal ctrlsim_decoder_layer_grad on the entry's own x0_out[l], mem_out and dX0[l + 1]; dMem equals
    the accumulate chain (the last layer's dMem, then each earlier layer added in descending order).  Against float64: every earlier
    layer on those taps (case 7's whole-stack twin takes 48 s of CPU time in float64 alone, so case 7 is checked from layer ND-2's taps
    down, a layer at a time)."""
    lib = _lib.lib()
    cfg, d, w, inp = _model_case(case)
    _split(lib, split)
    try:
        model = CtRLSim(cfg, w, device=DEV)
        cb, moving, B = model._ctx_of(_data(inp))
        r3, rd = _both(model, cb, moving, B)
        s3, g3, dX_3, _, x_3, _, _, dMem_3, _, mem_3, dX0_3, x0_3 = r3
        sd, gd, dX_d, x_d, dMem_d, mem_d, dX0_d, x0_d = rd
        assert np.array_equal(_bits(s3), _bits(sd))
        assert list(gd)[:len(g3)] == list(g3) and list(gd)[len(g3):] == [n for l in range(d.ND - 2, -1, -1) for n in lgr.names(l)]
        assert all(np.array_equal(_bits(g3[k]), _bits(gd[k])) for k in g3)
        assert _same([dX_3, x_3, mem_3, dX0_3, x0_3], [dX_d, x_d, mem_d, dX0_d[d.ND - 1], x0_d[d.ND - 1]])
        assert len(dX0_d) == len(x0_d) == d.ND
        kp = _key_pad(cfg, d, inp)
        mode, M = _mode_of(d), (d.P + d.A + 3) & ~3
        Mem = _rows(mem_d, B)
        chain = dMem_3.clone()
        for l in range(d.ND - 2, -1, -1):
            W = _layer_weights(w, l)
            X0, dY = _rows(x0_d[l], B), _rows(dX0_d[l + 1], B)
            got, dX0, _, x1, u = _run_op(X0, Mem, kp, dY, d.T, d.A, d.F, mode, W, dMem=chain, accumulate=1, fill=0xA5)
            assert _same(got, [gd[k] for k in lgr.names(l)]) and _same([dX0], [dX0_d[l]]), l
            solo = _run_op(X0, Mem, kp, dY, d.T, d.A, d.F, mode, W)
            r64, r32, nk = _references(X0, Mem, kp, dY, d.T, d.A, d.F, mode, W, got, u)
            print(f"case {case} {split} layer {l}: {nk} hidden elements on a ReLU kink")
            _check_layer(got, dX0, solo[2], x1, u, r64, r32)
        assert np.array_equal(_bits(chain), _bits(dMem_d))
        assert not dMem_d.cpu().numpy().reshape(B, M, 256)[kp.astype(bool)].any()
    finally:
        _split(lib, "f16x3")


def _cfg_nd(nd):
    cfg = loss_ref.case_cfg(0)
    cfg.model.num_decoder_layers = nd
    return cfg


def test_one_decoder_layer_is_the_last_layer_scope():
    """ND == 1: the entry is scope 3 — same gradient layout, same bits of everything both return; dX0[0] is the last layer's dX0."""
    cfg = _cfg_nd(1)
    d = spec.Dims(cfg)
    assert d.ND == 1
    model = CtRLSim(cfg, weights.generate(d, 5), device=DEV)
    cb, moving, B = model._ctx_of(_data(loss_ref.make_inputs(d, 31, 2)))
    assert model.train_grad_layout("heads+decoder") == model.train_grad_layout("heads+last_layer")
    r3, rd = _both(model, cb, moving, B)
    assert np.array_equal(_bits(r3[0]), _bits(rd[0])) and list(r3[1]) == list(rd[1])
    assert all(np.array_equal(_bits(r3[1][k]), _bits(rd[1][k])) for k in r3[1])
    assert _same([r3[2], r3[4], r3[7], r3[9], r3[10], r3[11]], [rd[2], rd[3], rd[4], rd[5], rd[6][0], rd[7][0]])
    assert all(torch.isfinite(t).all() for t in (rd[2], rd[4], rd[6][0]))


def test_decoder_entry_refuses_taps_beyond_the_layers_and_models_scope_3_refuses():
    import ctypes as C
    lib, st = _lib.lib(), _lib.stream_ptr()
    cfg, d, w, inp = _model_case(0)
    model = CtRLSim(cfg, w, device=DEV)
    cb, moving, B = model._ctx_of(_data(inp))
    n = model.train_grad_workspace_bytes(B, "heads+decoder")
    assert n > model.train_grad_workspace_bytes(B, "heads+last_layer")
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    sums = torch.zeros(5, 2, dtype=torch.float64, device=DEV)
    grads = torch.empty(model.train_grad_layout("heads+decoder")[1], device=DEV)
    buf = torch.empty(B * d.T * d.A * 3, 256, device=DEV)
    lc = model.loss_cfg()

    def call(m, taps, *, ws_=ws, sums_=sums, grads_=grads):
        return lib.ctrlsim_forward_loss_grads(m.hip.handle, B, d.T, C.byref(cb.struct), _lib.ptr(moving), C.byref(lc), 1.0, 4, _lib.ptr(ws_),
                                              _lib.ptr(sums_), None, _lib.ptr(grads_), C.byref(taps) if taps is not None else None, st)
    for k in ("x0_out", "dX0"):
        t = _lib.TrainTaps()
        getattr(t, k)[d.ND] = buf.data_ptr()
        assert call(model, t) == -22                                       # a tap of a layer the model does not have
    assert call(model, None, ws_=None) == -22 and call(model, None, sums_=None) == -22 and call(model, None, grads_=None) == -22
    assert call(model, None) == 0                                          # taps == NULL: no tap
    torch.cuda.synchronize()
    for other in (4, 5):                                                   # il, trajeglish: baseline token layouts, as scope 3
        cfg2, d2, w2, inp2 = _model_case(other)
        m2 = CtRLSim(cfg2, w2, device=DEV)
        with pytest.raises(RuntimeError):
            m2.loss_and_train_grads(_data(inp2), scope="heads+decoder")
        with pytest.raises(RuntimeError):
            m2.loss_and_train_grads(_data(inp2), scope="heads+last_layer")
    with pytest.raises(ValueError):
        model.loss_and_train_grads_ctx(cb, moving, B, dU=True, scope="heads+decoder")


def _relu_patterns(model, w, d, B, r3, rd, kp, mode):
    """The ReLU on / off pattern every layer's feed-forward block used in the call behind (r3, rd), first layer first."""
    on, nk = [], 0
    Mem = _rows(rd[5], B)
    for l in range(d.ND):
        W = _layer_weights(w, l)
        if l == d.ND - 1:
            u, dY = r3[5], r3[2]                                           # the last layer: scope 3's own U and dX
        else:
            dY = rd[6][l + 1]
            u = _run_op(_rows(rd[7][l], B), Mem, kp, _rows(dY, B), d.T, d.A, d.F, mode, W, want_dX0=False, dMem=None)[4]
        pat, n = lgr.relu_pattern(u.cpu().numpy(), dY.cpu().numpy(), W[0:6], rd[1][lgr.names(l)[1]].cpu().numpy())
        on.append(pat)
        nk += n
    return on, nk


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", [0, 1])
def test_whole_stack_against_a_float64_twin(case, split):
    """The tiny cases: a float64 twin of the ND decoder layers, the heads and the loss, started from the entry's x0_out[0] and mem_out,
    against every decoder gradient, dMem and every dX0 — the float32 yardstick is the same twin in float32.  The twins use the ReLU
    pattern each layer's feed-forward block used on the device.  Where a head's hidden element sits on a ReLU kink (the rule of
    tests/test_gpu_ffn_grads.py: _head_kinks) the float64 heads differentiate another function than the device's: the stack's backward
    then starts from the device's own dX.  The ratio of every layer is printed: it must not grow from layer to layer faster than the
    yardstick's own error does (the ratio IS relative to the yardstick, so a bounded ratio says exactly that)."""
    import test_gpu_ffn_grads as tff
    lib = _lib.lib()
    cfg, d, w, inp = _model_case(case)
    _split(lib, split)
    try:
        model = CtRLSim(cfg, w, device=DEV)
        cb, moving, B = model._ctx_of(_data(inp))
        r3, rd = _both(model, cb, moving, B)
        kp, mode = _key_pad(cfg, d, inp), _mode_of(d)
        on, nk = _relu_patterns(model, w, d, B, r3, rd, kp, mode)
        layers = [_layer_weights(w, l) for l in range(d.ND)]
        X0, Mem = _rows(rd[7][0], B), _rows(rd[5], B)
        vis = torch.from_numpy(sgr.mask(d.T, d.A, mode))
        hk = tff._head_kinks(rd[3].cpu().numpy(), w, d.VARIANT)
        ctx, kw = hgr.ctx_from_inputs(inp), _kw(cfg, d)
        refs = []
        for dtype in (torch.float64, torch.float32):
            with torch.no_grad():
                Y = lgr.stack(torch.tensor(X0, dtype=dtype), torch.tensor(Mem, dtype=dtype), torch.from_numpy(kp.astype(bool)), vis,
                              [[torch.tensor(t, dtype=dtype) for t in W] for W in layers], [torch.tensor(m, dtype=dtype) for m in on])[0]
            if hk:
                dY = rd[2].cpu().numpy().reshape(X0.shape)
            else:
                dY = hgr.loss_and_grads(Y.double().numpy().reshape(-1, 256), w, ctx, dtype=dtype, **kw)[3].reshape(X0.shape)
            refs.append(lgr.stack_grads(X0, Mem, kp, dY, d.T, d.A, mode, layers, dtype=dtype, relu_on=on))
        (g64, dX64, dM64), (g32, dX32, dM32) = refs
        print(f"case {case} {split}: {nk} hidden elements of the layers on a ReLU kink, {hk} of the heads"
              + (" (the stack's backward starts from the device's dX)" if hk else ""))
        worst = {}
        for l in range(d.ND - 1, -1, -1):
            r = [_check(f"layer {l} {p}", rd[1][k].cpu().numpy(), a, b, K_STACK) for p, k, a, b in zip(lgr.PARTS, lgr.names(l), g64[l], g32[l])]
            r.append(_check(f"layer {l} dX0", _rows(rd[6][l], B), dX64[l], dX32[l], K_STACK))
            worst[l] = max(r)
        r = _check("dMem", _rows(rd[4], B), dM64, dM32, K_STACK)
        print("   worst ratio per layer, last first: " + " ".join(f"{l}: {worst[l]:.2f}" for l in sorted(worst, reverse=True)) + f"; dMem {r:.2f}")
    finally:
        _split(lib, "f16x3")


FIX_REL = 4 * 1.741e-04         # tests/test_gpu_head_grads.py: FIX_REL
FIXTURE_CAP = 10 * FIX_REL      # the existing form (tests/test_gpu_self_attn_grads.py): holds where a ReLU sits on a kink
FIXTURE_BOUND = 1e-4            # ... and without one: that file's bound, beside its largest measured deviation 4.5e-5.  Measured here: 4.5e-5
                                # too (case 1, f16x3, layer 0 self_attn.out_proj.bias, one layer element on a kink); with 140 layer elements
                                # on a kink 8.2e-4 (case 7, bf16x6, layer 0 linear1.bias); with a head element on one 9.3e-3 (case 0, f16x3,
                                # layer 1 norm3.weight) and 2.3e-6 (case 0, bf16x6); profiles/decoder_grad_parity.md


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", MODEL_CASES)
def test_decoder_gradients_against_the_references_recorded_ones(case, split):
    """The gradients of the layers 0 .. ND-2, dMem and dX0[0] against what the unmodified reference's backward recorded
    (tests/golden/decoder_grads.part*.npz: its trunk, its float32; tools/gen_golden_decoder_grads.py), with the deviation measure of
    tests/test_gpu_self_attn_grads.py: bias and norm gradients in full, sampled rows, column sums and the Frobenius norm of every matrix,
    relative to the tensor's largest element.  The reference's encoder output has no filler rows: its row b (P + A) + j is row b M + j
    here.  FIXTURE_BOUND holds where no ReLU — of a head or of a layer's feed-forward block — sits on a kink, FIXTURE_CAP where one does
    (the float32 reference and the device then differentiate functions that differ in that element).  A HEAD element on a kink changes
    one row of dX, the gradient every layer's backward starts from: FIXTURE_CAP is what that does to the last layer's tensors
    (tests/test_gpu_self_attn_grads.py: 5.95e-3 measured there, this case and split), and each further layer the changed row is carried
    through adds a contribution of that kind, so layer l is held to (ND - l) FIXTURE_CAP and dMem and dX0[0], which collect all layers,
    to ND FIXTURE_CAP.  That the device's stack is right GIVEN its dX is what test_whole_stack_against_a_float64_twin shows for the same
    case and split."""
    import test_gpu_ffn_grads as tff
    from helpers import golden
    lib = _lib.lib()
    cfg, d, w, inp = _model_case(case)
    _split(lib, split)
    try:
        model = CtRLSim(cfg, w, device=DEV)
        cb, moving, B = model._ctx_of(_data(inp))
        r3, rd = _both(model, cb, moving, B)
        gf = golden("decoder_grads")
        P = f"c{case}_"
        worst, depth = {}, {}
        for l in range(d.ND - 2, -1, -1):
            for k in lgr.names(l):
                got = rd[1][k].cpu().numpy()
                scale = np.abs(got).max()
                if got.ndim == 1:
                    err = np.abs(got - gf[P + "g_" + k]).max() / scale
                else:
                    rows = gf[P + "r_" + k]
                    err = np.abs(got[rows] - gf[P + "s_" + k]).max() / scale
                    csum = np.abs(got.astype(np.float64).sum(0) - gf[P + "c_" + k]).max() / (scale * got.shape[0])
                    nrm = abs(np.linalg.norm(got.astype(np.float64)) - float(gf[P + "n_" + k])) / float(gf[P + "n_" + k])
                    err = max(err, csum, nrm)
                print(f"   {k} against the reference's recorded gradient: {err:.3e} of max |T|")
                worst[k] = err
                depth[k] = d.ND - l
        M, PA = (d.P + d.A + 3) & ~3, d.P + d.A
        for key, got in (("dMem", rd[4].cpu().numpy().reshape(B, M, 256)[:, :PA].reshape(-1, 256)), ("dX0", rd[6][0].cpu().numpy())):
            rows = gf[P + "r_" + key]
            scale = np.abs(got).max()
            err = np.abs(got[rows] - gf[P + "s_" + key]).max() / scale
            nrm = abs(np.linalg.norm(got.astype(np.float64)) - float(gf[P + "n_" + key])) / float(gf[P + "n_" + key])
            print(f"   {key} against the reference's recorded gradient: rows {err:.3e} of max |T|, norm {nrm:.3e}")
            worst[key] = max(err, nrm)
            depth[key] = d.ND
        assert not rd[4].cpu().numpy().reshape(B, M, 256)[:, PA:].any()                       # the filler rows are padded keys
        nk = _relu_patterns(model, w, d, B, r3, rd, _key_pad(cfg, d, inp), _mode_of(d))[1]
        hk = tff._head_kinks(rd[3].cpu().numpy(), w, d.VARIANT)
        top = max(worst, key=worst.get)
        bound = {k: depth[k] * FIXTURE_CAP if hk else FIXTURE_CAP if nk else FIXTURE_BOUND for k in worst}
        print(f"   worst {worst[top]:.3e} ({top}; bound {bound[top]:.3e}: {hk} head and {nk} layer hidden elements on a ReLU kink)")
        for k in worst:
            assert worst[k] <= bound[k], (k, worst[k], bound[k])
    finally:
        _split(lib, "f16x3")


# ---- 3. HipModel.update
@pytest.mark.parametrize("split", SPLITS)
def test_update_of_every_layer_equals_a_fresh_model_bit_for_bit(split):
    lib = _lib.lib()
    _split(lib, split)
    try:
        cfg, d, w, inp = _model_case(1)
        data = _data(inp)
        model = CtRLSim(cfg, dict(w), device=DEV)
        before = model.hip.flat.clone()
        rs = np.random.RandomState(4)
        names = [n for l in range(d.ND) for n in lgr.names(l)] + hgr.head_names(w)
        new = {k: (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32) for k in names}
        for flags in ({}, {"cross": True, "self_attn": True}):
            with pytest.raises(KeyError):
                model.hip.update(new, **flags)                          # without decoder=True the earlier layers' names are refused
            assert torch.equal(before.view(torch.int32), model.hip.flat.view(torch.int32))
        model.hip.update(new, decoder=True)
        fresh = CtRLSim(cfg, {**w, **new}, device=DEV)
        assert torch.equal(model.hip.flat.view(torch.int32), fresh.hip.flat.view(torch.int32))          # every image re-derived in place
        a, b = model.loss_sums(data)[0].cpu().numpy(), fresh.loss_sums(data)[0].cpu().numpy()
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
        assert not np.array_equal(a.view(np.int64), CtRLSim(cfg, dict(w), device=DEV).loss_sums(data)[0].cpu().numpy().view(np.int64))
        one = lgr.names(0)[2]                                           # a later update of one tensor keeps the others' new values
        newer = {one: (new[one] * np.float32(1.01)).astype(np.float32)}
        model.hip.update(newer, decoder=True)
        fresh = CtRLSim(cfg, {**w, **new, **newer}, device=DEV)
        assert torch.equal(model.hip.flat.view(torch.int32), fresh.hip.flat.view(torch.int32))
        snap = model.hip.flat.clone()
        with pytest.raises(FloatingPointError):
            model.hip.update({one: np.full_like(new[one], 1.0e6)}, decoder=True)
        assert torch.equal(snap.view(torch.int32), model.hip.flat.view(torch.int32))                    # nothing written
        with pytest.raises(KeyError):
            model.hip.update({"encoder.transformer_encoder.layers.0.linear1.weight": np.ones((1024, 256), np.float32)}, decoder=True)
    finally:
        _split(lib, "f16x3")


# ---- 4. training loop
def _twin(cfg, d, w, X0, Mem, kp, mode, ctx, kw, steps):
    """torch float64: the ND decoder layers and the heads on the same (constant) stack inputs X0 and Mem, the same AdamW groups, clip and
    schedule."""
    heads = hgr.head_names(w)
    lnames = [lgr.names(l) for l in range(d.ND)]
    every = heads + [k for l in range(d.ND - 1, -1, -1) for k in lnames[l]]
    params = {k: torch.nn.Parameter(torch.tensor(np.asarray(w[k]), dtype=torch.float64)) for k in every}
    decay, no_decay = CtRLSim.param_groups(every)
    tr = cfg.train
    opt = torch.optim.AdamW([{"params": [params[k] for k in decay], "weight_decay": tr["weight_decay"]},
                             {"params": [params[k] for k in no_decay], "weight_decay": 0.0}], lr=tr["lr"], weight_decay=tr["weight_decay"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=CtRLSim.lr_lambda(tr))
    vis, kpt = torch.from_numpy(sgr.mask(d.T, d.A, mode)), torch.from_numpy(kp.astype(bool))

    def evaluate():
        now = {k: p.detach().numpy() for k, p in params.items()}
        layers = [[now[k] for k in lnames[l]] for l in range(d.ND)]
        with torch.no_grad():
            Y = lgr.stack(torch.tensor(X0), torch.tensor(Mem), kpt, vis, [[torch.tensor(t) for t in W] for W in layers])[0].numpy()
        _, final, g, dX = hgr.loss_and_grads(Y.reshape(-1, 256), {k: now[k] for k in heads}, ctx, **kw)
        gl, _, _ = lgr.stack_grads(X0, Mem, kp, dX.reshape(X0.shape), d.T, d.A, mode, layers)
        for l in range(d.ND):
            g.update(zip(lnames[l], gl[l]))
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


def test_five_training_steps_in_scope_heads_decoder_follow_the_float64_twin():
    """training_step / optimizer_step five times on one fixed batch (case 0) with set_trainable("heads+decoder").  The encoder and the
    embeddings are frozen, so the stack's inputs x0_out[0] and mem_out are constant (asserted bit for bit) and a float64 twin can train
    the heads and all ND layers on them.  Loss per step within STEP_LOSS_REL of the twin's; weights: every element within
    2 sum_t lr_t sqrt(t) + 5 x 2^-24 |w| of the twin's (part (a) of tests/test_gpu_ffn_grads.py's criterion), the bulk figure printed."""
    cfg, d, w, inp = _model_case(0)
    w0 = {k: np.array(v) for k, v in w.items()}
    model = CtRLSim(cfg, dict(w0), device=DEV).set_trainable("heads+decoder")
    data = _data(inp)
    first = model.loss_and_train_grads(data, x0_out=True, mem_out=True)
    x0, mem = first[7][0], first[5]
    heads = hgr.head_names(w)
    every = heads + [k for l in range(d.ND - 1, -1, -1) for k in lgr.names(l)]
    assert list(model.trainable_parameters()) == every and len(every) == len(heads) + 18 * d.ND
    assert all(model.trainable_parameters()[k] is model.head_parameters()[k] for k in heads)
    opt, sched = model.configure_optimizers()
    got = []
    for step in range(5):
        got.append(model.training_step(data, step))
        assert all(p.grad is not None for p in model.trainable_parameters().values())
        model.optimizer_step(opt, sched)
    out = model.loss_and_train_grads(data, x0_out=True, mem_out=True)
    got.append(model.final_loss(model.losses_from_sums(out[0].cpu().numpy())))
    assert torch.equal(x0, out[7][0]) and torch.equal(mem, out[5])                  # everything in front of the decoder did not move
    assert not torch.equal(first[7][1], out[7][1])                                 # ... layer 0 did
    B = np.asarray(inp["agent_states"]).shape[0]
    want, w_twin = _twin(cfg, d, w0, _rows(x0, B).astype(np.float64), _rows(mem, B).astype(np.float64), _key_pad(cfg, d, inp), _mode_of(d),
                         hgr.ctx_from_inputs(inp), _kw(cfg, d), 5)
    print(f"loss per step {got}\n twin         {want}")
    print(" relative     " + " ".join(f"{abs(a - b) / abs(b):.3e}" for a, b in zip(got, want)))
    for a, b in zip(got, want):
        assert abs(a - b) <= STEP_LOSS_REL * abs(b)
    assert got[5] < got[0] and want[5] < want[0]
    lrs = [cfg.train["lr"] * CtRLSim.lr_lambda(cfg.train)(t) for t in range(5)]
    worst_case = 2 * sum(lr * np.sqrt(t + 1) for t, lr in enumerate(lrs))
    bulk = 1e-3 * sum(lrs)
    n_all = n_off = 0
    drift = 0.0
    hip = model.hip
    for k, v in w_twin.items():
        have = next(m for m in (hip._heads, hip._ffn, hip._cross, hip._self, hip._early) if k in m)[k].astype(np.float64)
        assert np.array_equal(have, np.asarray(model.weights[k], np.float64))
        diff = np.abs(have - v)
        rnd = 5 * FLOOR * np.abs(v)
        assert (diff <= worst_case + rnd).all(), k
        n_all += diff.size
        n_off += int((diff > bulk + rnd).sum())
        drift = max(drift, float(diff.max()))
        assert np.abs(v - np.asarray(w0[k], np.float64)).max() > 0, k
    print(f"   weights after five steps: max |w - twin| {drift:.3e} (sum lr {sum(lrs):.1e}), {n_off} of {n_all} elements beyond the bulk tolerance")


@pytest.mark.parametrize("scope", list(CtRLSim.SCOPES))
def test_narrower_scopes_leave_the_earlier_layers_alone(scope):
    """Two training steps in each of the four narrower scopes: the 18 tensors of every earlier decoder layer and every image derived from
    them keep their bits; something else moves."""
    cfg, d, w, inp = _model_case(0)
    model = CtRLSim(cfg, {k: np.array(v) for k, v in w.items()}, device=DEV).set_trainable(scope)
    data = _data(inp)
    early = {n for l in range(d.ND - 1) for n in lgr.names(l)}
    assert not early & set(model.trainable_parameters())
    off = model.hip._offset
    order = sorted(off.values()) + [model.hip.flat.numel()]
    pres = tuple(f"decoder.transformer_decoder.layers.{l}." for l in range(d.ND - 1))
    mine = torch.zeros(model.hip.flat.numel(), dtype=torch.bool, device=DEV)
    for name, o in off.items():
        if name.startswith(pres):
            mine[o:order[order.index(o) + 1]] = True
    assert int(mine.sum()) > (d.ND - 1) * sum(lgr.sizes(d.F))
    before = model.hip.flat.clone()
    opt, sched = model.configure_optimizers()
    for step in range(2):
        model.training_step(data, step)
        model.optimizer_step(opt, sched)
    assert torch.equal(before.view(torch.int32)[mine], model.hip.flat.view(torch.int32)[mine])
    assert not torch.equal(before.view(torch.int32)[~mine], model.hip.flat.view(torch.int32)[~mine])
