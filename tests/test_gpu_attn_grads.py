"""GPU tests of the attention sublayer's backward (csrc/attn_grad.hip: ctrlsim_attn_block_grad) and of ctrlsim_forward_loss_grads at scope 2
(heads + the last decoder layer's feed-forward block + its cross-attention sublayer), under both operand splits of the forward where a
forward is involved.

ACCURACY BOUND (profiles/attn_grad_parity.md holds every measured ratio).  The form of tests/test_gpu_ffn_grads.py: for every gradient
tensor T, relative to max |T_f64| (Frobenius: to ||T_f64||),
    e_hip = max |T_hip - T_f64|,   e_ref = max |T_torch_fp32_cpu - T_f64|   (tests/attn_grad_ref.py in float64 / float32)
and e_hip <= K max(e_ref, 2^-24), likewise in the Frobenius norm.  in_proj_bias is ONE tensor: its bk slice (zero in exact arithmetic)
is measured on the scale of the whole.  K = K_BOUND below: the largest ratio measured on the device rounded up to a power of two; the
specification's ceiling is 16.  A tensor that is identically zero in float64 (a batch whose every key is padded: the in_proj gradients,
the out-projection weight's and dMem) must be exactly zero.  Rows of dMem that belong to padded keys are exactly zero."""
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
from gpu_utils import DEV  # noqa: E402
from helpers import golden  # noqa: E402

K_BOUND = 8.0               # largest measured ratio 5.14 (op 2 x 300 x 257, scattered padding, in_proj_weight; profiles/attn_grad_parity.md), rounded up
FLOOR = 2.0 ** -24
LOSS_REL = 2.97e-6          # the loss route's own bound (profiles/loss_parity.md section 1; tests/test_gpu_head_grads.py)
FIX_REL = 4 * 1.741e-04     # tests/test_gpu_head_grads.py: FIX_REL
FIXTURE_CAP = 10 * FIX_REL      # the specification's cap; holds where a head's ReLU sits on a kink (tests/test_gpu_ffn_grads.py)
FIXTURE_BOUND = 1e-4            # twice the largest measured deviation without a head kink (4.7e-5: case 7, f16x3, norm2.weight), one digit
STEP_LOSS_REL = LOSS_REL    # the existing form (tests/test_gpu_ffn_grads.py); measured worst 1.6e-6 (case 7; case 0: 7.7e-8)
SPLITS = ["f16x3", "bf16x6"]
MODEL_CASES = (0, 1, 7)
SHAPES = [(1, 1, 1), (3, 33, 31), (2, 130, 65), (2, 257, 224), (2, 300, 257), (2, 4608, 224)]
SIZES = (768 * 256, 768, 256 * 256, 256, 256, 256)
SHAPE_OF = ((768, 256), (768,), (256, 256), (256,), (256,), (256,))
assert K_BOUND <= 16.0 and FIXTURE_BOUND <= FIXTURE_CAP and STEP_LOSS_REL <= 1e-5


def _split(lib, name):
    _lib.check(lib.ctrlsim_bind(1 if name == "f16x3" else 0, None))


def _check(tag, got, want64, got32, k=K_BOUND):
    """The accuracy bound of the module docstring for one tensor; prints the figures before it asserts."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    assert np.isfinite(got).all(), tag
    if not want64.any():
        print(f"   {tag}: identically zero in float64")
        assert not got.any() and not np.asarray(got32).any(), tag
        return 0.0
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


# ---- 1. the op
@functools.lru_cache(maxsize=None)
def _trained_like():
    d = spec.Dims(spec.make_cfg())
    w = weights.generate_trained_like(d, 0)
    return [np.asarray(w[k], np.float32) for k in agr.names(d)]


@functools.lru_cache(maxsize=None)
def _op_case(B, Lq, Lk, pad):
    """Seeded inputs of one op shape and padding pattern, with their float64 / float32 references (computed once, never written)."""
    X, Mem, dY, T = agr.make_case(B, Lq, Lk, 11 + Lq % 13, _trained_like())
    kp = agr.make_pad(B, Lk, pad, np.random.RandomState(Lk))
    return X, Mem, dY, T, kp, agr.grads(X, Mem, kp, dY, T), agr.grads(X, Mem, kp, dY, T, dtype=torch.float32)


def _run_op(X, Mem, kp, dY, T, ldx=256, ldm=256, lddy=256, lddx=256, lddm=256, want_dX=True, want_dMem=True, fill=0, alias=False):
    """ctrlsim_attn_block_grad on host arrays -> ([six gradient tensors], dX or None, dMem or None) as device tensors."""
    lib, st = _lib.lib(), _lib.stream_ptr()
    B, Lq, Lk = X.shape[0], X.shape[1], Mem.shape[1]

    def padded(a, ld):
        t = torch.full((a.shape[0] * a.shape[1], ld), 7.0, device=DEV)
        t[:, :256] = torch.from_numpy(a.reshape(-1, 256)).to(DEV)
        return t

    Xd, Md, dYd = padded(X, ldx), padded(Mem, ldm), padded(dY, lddy)
    Td = [torch.from_numpy(t).to(DEV) for t in T]
    kpd = torch.from_numpy(kp).to(DEV) if kp is not None else None
    n = int(lib.ctrlsim_attn_block_grad_workspace_bytes(B, Lq, Lk))
    assert n > 0
    ws = torch.full((n,), fill, dtype=torch.uint8, device=DEV)
    grads = torch.full((sum(SIZES),), float("nan"), device=DEV)
    dXd = dYd if alias else torch.full((B * Lq, lddx), 7.0, device=DEV) if want_dX else None
    dMd = torch.full((B * Lk, lddm), 7.0, device=DEV) if want_dMem else None
    _lib.check(lib.ctrlsim_attn_block_grad(Xd.data_ptr(), ldx, Md.data_ptr(), ldm, kpd.data_ptr() if kpd is not None else None,
                                           dYd.data_ptr(), lddy, *(t.data_ptr() for t in Td), B, Lq, Lk, ws.data_ptr(), grads.data_ptr(),
                                           dXd.data_ptr() if dXd is not None else None, lddy if alias else lddx,
                                           dMd.data_ptr() if dMd is not None else None, lddm, st), "attn_block_grad")
    torch.cuda.synchronize()
    assert torch.equal(Xd[:, :256].cpu(), torch.from_numpy(X.reshape(-1, 256))) and torch.equal(Md[:, :256].cpu(), torch.from_numpy(Mem.reshape(-1, 256)))
    if not alias:
        assert torch.equal(dYd[:, :256].cpu(), torch.from_numpy(dY.reshape(-1, 256)))                 # inputs intact
    for t in (dXd, dMd, Xd, Md, dYd):
        if t is not None and t.shape[1] > 256:
            assert (t[:, 256:] == 7.0).all()                                   # nothing beyond the 256 columns of a row
    out, o = [], 0
    for sz, shp in zip(SIZES, SHAPE_OF):
        out.append(grads[o:o + sz].view(shp))
        o += sz
    return out, (dXd[:, :256].contiguous() if dXd is not None else None), (dMd[:, :256].contiguous() if dMd is not None else None)


def _check_op(got, dX, dMem, r64, r32, kp, k=K_BOUND):
    worst = 0.0
    for name, g, a, b in zip(agr.PARTS, got, r64[0], r32[0]):
        worst = max(worst, _check(name, g.cpu().numpy(), a, b, k))
    if dX is not None:
        worst = max(worst, _check("dX", dX.cpu().numpy().reshape(r64[1].shape), r64[1], r32[1], k))
    if dMem is not None:
        dM = dMem.cpu().numpy().reshape(r64[2].shape)
        worst = max(worst, _check("dMem", dM, r64[2], r32[2], k))
        if kp is not None:
            assert not dM[kp.astype(bool)].any()                               # padded keys: exactly zero rows
    print(f"   worst ratio {worst:.2f}")
    return worst


@pytest.mark.parametrize("pad", agr.PADS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_attn_block_grad_matches_float64_autograd(shape, pad):
    """Every shape of the specification's table (one query and one key; under one tile on both axes; one past a query block and a key
    tile; the model's key count; more than four key tiles; 2 x 4608 query rows: a chunk boundary — one context per chunk — and 1024-row
    slab boundaries) under every key-padding pattern.  All six tensors, dX and dMem against float64 autograd of the same fp32 inputs."""
    X, Mem, dY, T, kp, r64, r32 = _op_case(*shape, pad)
    got, dX, dMem = _run_op(X, Mem, kp, dY, T)
    print(f"op B {shape[0]} Lq {shape[1]} Lk {shape[2]} pad {pad}")
    _check_op(got, dX, dMem, r64, r32, kp)


def test_attn_block_grad_leading_dimensions_null_outputs_and_aliased_dx():
    """Leading dimensions 320 / 304 / 288 / 272 / 264 for X / Mem / dY / dX / dMem give the bits of the dense call; dX = NULL or dMem =
    NULL leave everything else unchanged; dX = dY (same leading dimension) gives the same dX."""
    X, Mem, dY, T, kp, r64, r32 = _op_case(2, 130, 65, "scattered")
    dense, dX, dMem = _run_op(X, Mem, kp, dY, T)
    got, dX2, dMem2 = _run_op(X, Mem, kp, dY, T, ldx=320, ldm=304, lddy=288, lddx=272, lddm=264)
    _check_op(got, dX2, dMem2, r64, r32, kp)
    same = lambda a, b: all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    assert same(dense, got) and same([dX, dMem], [dX2, dMem2])
    got, none, dMem3 = _run_op(X, Mem, kp, dY, T, want_dX=False)
    assert none is None and same(dense, got) and same([dMem], [dMem3])
    got, dX4, none = _run_op(X, Mem, kp, dY, T, want_dMem=False)
    assert none is None and same(dense, got) and same([dX], [dX4])
    got, dX5, dMem5 = _run_op(X, Mem, kp, dY, T, lddy=288, alias=True)
    assert same(dense, got) and same([dX, dMem], [dX5, dMem5])


def test_attn_block_grad_refuses_bad_arguments():
    lib = _lib.lib()
    x = torch.zeros(768 * 256, device=DEV)
    p = x.data_ptr()
    #     X  ldx  Mem ldm  pad   dY lddy Win bin Wo bo g  be B  Lq Lk ws grads dX   lddx dMem lddm stream
    ok = [p, 256, p, 256, None, p, 256, p, p, p, p, p, p, 1, 2, 2, p, p, None, 256, None, 256, None]
    for i, v in ((15, 0), (14, 0), (13, 0), (0, None), (2, None), (5, None), (7, None), (8, None), (9, None), (10, None), (11, None), (12, None),
                 (16, None), (17, None), (1, 255), (3, 255), (6, 255)):
        a = list(ok)
        a[i] = v
        assert lib.ctrlsim_attn_block_grad(*a) == -22, i        # CTRLSIM_EINVAL
    a = list(ok)
    a[18], a[19] = p, 255
    assert lib.ctrlsim_attn_block_grad(*a) == -22
    a = list(ok)
    a[20], a[21] = p, 255
    assert lib.ctrlsim_attn_block_grad(*a) == -22
    assert lib.ctrlsim_attn_block_grad_workspace_bytes(0, 4, 4) < 0 and lib.ctrlsim_attn_block_grad_workspace_bytes(4, 0, 4) < 0
    assert lib.ctrlsim_attn_block_grad_workspace_bytes(4, 4, 0) < 0


def test_attn_block_grad_identical_bits_whatever_the_workspace_held():
    X, Mem, dY, T, kp, _, _ = _op_case(2, 257, 224, "tail")
    a = _run_op(X, Mem, kp, dY, T, fill=0xFF)              # NaN bit patterns
    b = _run_op(X, Mem, kp, dY, T, fill=0x00)
    flat = lambda r: list(r[0]) + [r[1], r[2]]
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(flat(a), flat(b)))
    assert all(torch.isfinite(x).all() for x in flat(a))


# ---- 2. through the model
def _data(inp):
    return {"agent": {k: inp[k] for k in ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask")},
            "map": {k: inp[k] for k in ("road_points", "road_types")}}


@functools.lru_cache(maxsize=None)
def _model_case(case):
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    return cfg, d, loss_ref.case_weights(case, d), loss_ref.case_inputs(case, d)


def _key_pad(cfg, d, inp):
    """The scene rows' key-padding bytes restated from the inputs (modules/encoder.py:155-170): a polyline without an existing point, a
    vehicle that does not exist at the window's first step, and the filler rows up to a multiple of four are padded."""
    B = np.asarray(inp["agent_states"]).shape[0]
    M = (d.P + d.A + 3) & ~3
    pad = np.ones((B, M), np.uint8)
    if bool(cfg.model.get("use_map", True)):
        pad[:, :d.P] = ~(np.asarray(inp["road_points"])[..., 2] != 0).any(-1)
    if bool(cfg.model.get("encode_initial_state", True)):
        pad[:, d.P:d.P + d.A] = np.asarray(inp["agent_states"])[:, :, 0, 7] == 0
    return pad


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", MODEL_CASES)
def test_forward_loss_grad_cross_through_the_model(case, split):
    """ctrlsim_forward_loss_grads at scope 2 on fixture cases 0, 1 (tiny) and 7 (full dims, B = 2): loss sums, head and feed-forward gradients,
    dX and dU bit-identical to scope 1; the six new tensors, dX1 and dMem against the float64 sublayer applied to
    the returned X1 / Mem with the returned dU as dY."""
    lib = _lib.lib()
    cfg, d, w, inp = _model_case(case)
    _split(lib, split)
    try:
        model = CtRLSim(cfg, w, device=DEV)
        cb, moving, B = model._ctx_of(_data(inp))
        s1, g1, dXa, dUa, _, _ = model.loss_and_train_grads_ctx(cb, moving, B, dX=True, dU=True, scope="heads+ffn")
        s2, g2, dXb, dUb, _, _, dX1, dMem, x1, mem = model.loss_and_train_grads_ctx(cb, moving, B, dX=True, dU=True, dX1=True, dMem=True,
                                                                                   x1_out=True, mem_out=True, scope="heads+ffn+cross")
        assert np.array_equal(_bits(s1), _bits(s2))
        old, new = list(g1), agr.names(d)
        assert list(g2) == old + new and old == hgr.head_names(w) + fgr.names(d)
        assert all(np.array_equal(_bits(g1[k]), _bits(g2[k])) for k in old)
        assert np.array_equal(_bits(dXa), _bits(dXb)) and np.array_equal(_bits(dUa), _bits(dUb))
        Lq, M = d.T * d.A * 3, (d.P + d.A + 3) & ~3
        kp = _key_pad(cfg, d, inp)
        X1, Mem, dU = x1.cpu().numpy().reshape(B, Lq, 256), mem.cpu().numpy().reshape(B, M, 256), dUb.cpu().numpy().reshape(B, Lq, 256)
        T = [np.asarray(w[k], np.float32) for k in new]
        r64, r32 = agr.grads(X1, Mem, kp, dU, T), agr.grads(X1, Mem, kp, dU, T, dtype=torch.float32)
        print(f"case {case} {split}: {int(kp.sum())} of {kp.size} scene rows padded")
        _check_op([g2[k] for k in new], dX1, dMem, r64, r32, kp)
        # the reference's own numbers (its trunk, its float32): sampled rows, column sums, norms
        gf = golden("cross_grads")
        P = f"c{case}_"
        worst = 0.0
        got = {k: g2[k].cpu().numpy() for k in new}
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
        xo = model.loss_and_train_grads_ctx(cb, moving, B, x_out=True, scope="heads+ffn")[4]
        nk = tff._head_kinks(xo.cpu().numpy(), w, d.VARIANT)
        bound = FIXTURE_CAP if nk else FIXTURE_BOUND
        print(f"   worst {worst:.3e} (bound {bound:.3e}: {nk} head hidden elements on a ReLU kink)")
        assert worst <= bound
    finally:
        _split(lib, "f16x3")


def test_scopes_before_this_one_answer_as_before():
    cfg, d, w, inp = _model_case(0)
    model = CtRLSim(cfg, w, device=DEV)
    assert model.train_grad_layout("heads") == model.head_grad_layout()
    l1, t1 = model.train_grad_layout("heads+ffn")
    l2, t2 = model.train_grad_layout("heads+ffn+cross")
    assert l2[:len(l1)] == l1 and [k for k, _, _ in l2[len(l1):]] == agr.names(d) and t2 == t1 + sum(SIZES)
    assert model.train_grad_workspace_bytes(2, "heads+ffn+cross") > model.train_grad_workspace_bytes(2, "heads+ffn")


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
        rs = np.random.RandomState(4)
        names = agr.names(d)
        new = {k: (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32) for k in names}
        with pytest.raises(KeyError):
            model.hip.update(new)                                   # outside the scope "heads+ffn+cross" the names are refused
        assert torch.equal(before.view(torch.int32), model.hip.flat.view(torch.int32))
        model.hip.update(new, cross=True)
        fresh = CtRLSim(cfg, {**w, **new}, device=DEV)
        assert torch.equal(model.hip.flat.view(torch.int32), fresh.hip.flat.view(torch.int32))          # every image re-derived in place
        a, b = model.loss_sums(data)[0].cpu().numpy(), fresh.loss_sums(data)[0].cpu().numpy()
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
        assert not np.array_equal(a.view(np.int64), CtRLSim(cfg, dict(w), device=DEV).loss_sums(data)[0].cpu().numpy().view(np.int64))
        # a later update of the feed-forward block derives .ffn#wop from the NEW out-projection
        fn = fgr.names(d)
        newf = {k: (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32) for k in fn}
        model.hip.update(newf)
        fresh = CtRLSim(cfg, {**w, **new, **newf}, device=DEV)
        assert torch.equal(model.hip.flat.view(torch.int32), fresh.hip.flat.view(torch.int32))
        snap = model.hip.flat.clone()
        with pytest.raises(FloatingPointError):
            model.hip.update({names[2]: np.full_like(new[names[2]], 1.0e6)}, cross=True)
        assert torch.equal(snap.view(torch.int32), model.hip.flat.view(torch.int32))                    # nothing written
        with pytest.raises(KeyError):
            model.hip.update({f"decoder.transformer_decoder.layers.{d.ND - 1}.norm1.weight": np.ones(256, np.float32)}, cross=True)
    finally:
        _split(lib, "f16x3")


# ---- 4. training loop
def _twin(cfg, d, w, X1, Mem, kp, ctx, kw, steps):
    """torch float64: the heads, the feed-forward block and the cross-attention sublayer on the same (constant) sublayer inputs X1 and
    Mem, the same AdamW groups, clip and schedule."""
    heads, ffn, new = hgr.head_names(w), fgr.names(d), agr.names(d)
    params = {k: torch.nn.Parameter(torch.tensor(np.asarray(w[k]), dtype=torch.float64)) for k in heads + ffn + new}
    decay, no_decay = CtRLSim.param_groups(heads + ffn + new)
    tr = cfg.train
    opt = torch.optim.AdamW([{"params": [params[k] for k in decay], "weight_decay": tr["weight_decay"]},
                             {"params": [params[k] for k in no_decay], "weight_decay": 0.0}], lr=tr["lr"], weight_decay=tr["weight_decay"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=CtRLSim.lr_lambda(tr))

    def evaluate():
        now = {k: p.detach().numpy() for k, p in params.items()}
        Tc, Tf = [now[k] for k in new], [now[k] for k in ffn]
        U = agr.forward(X1, Mem, kp, Tc).reshape(-1, 256)
        _, final, g, dX = hgr.loss_and_grads(fgr.forward(U, Tf), {k: now[k] for k in heads}, ctx, **kw)
        gf, dU = fgr.grads(U, dX, Tf)
        g.update(zip(ffn, gf))
        g.update(zip(new, agr.grads(X1, Mem, kp, dU.reshape(X1.shape), Tc)[0]))
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


@pytest.mark.parametrize("case", [0, 7])
def test_five_training_steps_in_scope_heads_ffn_cross_follow_the_float64_twin(case):
    """training_step / optimizer_step five times on one fixed batch with set_trainable("heads+ffn+cross").  Everything upstream of the
    sublayer is frozen, so its inputs X1 and Mem are constant (asserted bit for bit) and a float64 twin can train the three parts on
    them.  Loss per step within STEP_LOSS_REL of the twin's.  Weights: every element within 2 sum_t lr_t sqrt(t) + 5 x 2^-24 |w| of the
    twin's (part (a) of tests/test_gpu_ffn_grads.py's criterion: what AdamW can move an element at all).  Its part (b) — all but 1e-3 of
    the elements within 1e-3 sum_t lr_t — is printed, not asserted: AdamW divides every element's step by that element's own gradient
    history, so an element whose gradient is at float32 rounding level moves by a full lr per step in a direction the rounding chooses,
    in the twin and on the device alike.  The feed-forward block has few such elements (a dead hidden unit's gradient is exactly zero
    in both); this sublayer has them by construction — the bk slice of in_proj_bias is zero in exact arithmetic, and the key side
    P o (dP - delta) is a difference of nearly equal numbers wherever one key holds a row's weight.  Measured: case 0, 14 219 of 1 517 578
    elements (0.94 %) beyond part (b), largest difference 6.0e-6 with sum lr 1.0e-5, loss per step within 7.7e-8; case 7, 3 350 of
    1 531 970 (0.22 %), 7.1e-6, 1.6e-6."""
    cfg, d, w, inp = _model_case(case)
    w0 = {k: np.array(v) for k, v in w.items()}
    model = CtRLSim(cfg, dict(w0), device=DEV).set_trainable("heads+ffn+cross")
    data = _data(inp)
    first = model.loss_and_train_grads(data, x1_out=True, mem_out=True)
    x1, mem = first[8], first[9]
    heads, ffn, new = hgr.head_names(w), fgr.names(d), agr.names(d)
    assert list(model.trainable_parameters()) == heads + ffn + new
    assert all(model.trainable_parameters()[k] is model.head_parameters()[k] for k in heads)
    opt, sched = model.configure_optimizers()
    got = []
    for step in range(5):
        got.append(model.training_step(data, step))
        assert all(p.grad is not None for p in model.trainable_parameters().values())
        model.optimizer_step(opt, sched)
    out = model.loss_and_train_grads(data, x1_out=True, mem_out=True)
    got.append(model.final_loss(model.losses_from_sums(out[0].cpu().numpy())))
    assert torch.equal(x1, out[8]) and torch.equal(mem, out[9])                    # everything in front of the sublayer did not move
    B = np.asarray(inp["agent_states"]).shape[0]
    M = (d.P + d.A + 3) & ~3
    want, w_twin = _twin(cfg, d, w0, x1.cpu().numpy().reshape(B, -1, 256), mem.cpu().numpy().reshape(B, M, 256), _key_pad(cfg, d, inp),
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
        have = (model.hip._heads if k in heads else model.hip._ffn if k in ffn else model.hip._cross)[k].astype(np.float64)
        assert np.array_equal(have, np.asarray(model.weights[k], np.float64))
        diff = np.abs(have - v)
        rnd = 5 * FLOOR * np.abs(v)
        assert (diff <= worst_case + rnd).all(), k
        n_all += diff.size
        n_off += int((diff > bulk + rnd).sum())
        drift = max(drift, float(diff.max()))
        assert np.abs(v - np.asarray(w0[k], np.float64)).max() > 0, k
    print(f"   weights after five steps: max |w - twin| {drift:.3e} (sum lr {sum(lrs):.1e}), {n_off} of {n_all} elements beyond the bulk tolerance")


@pytest.mark.parametrize("scope", ["heads", "heads+ffn"])
def test_narrower_scopes_leave_the_sublayer_alone(scope):
    """Two training steps in a scope before this one: the six tensors and every image derived from them keep their bits."""
    cfg, d, w, inp = _model_case(0)
    model = CtRLSim(cfg, {k: np.array(v) for k, v in w.items()}, device=DEV).set_trainable(scope)
    data = _data(inp)
    assert not set(agr.names(d)) & set(model.trainable_parameters())
    off = model.hip._offset
    order = sorted(off.values()) + [model.hip.flat.numel()]
    pre = agr.layer_prefix(d)
    mine = torch.zeros(model.hip.flat.numel(), dtype=torch.bool, device=DEV)
    for name, o in off.items():
        if name.split("#")[0] in agr.names(d) or name.startswith((pre + ".selfq#", pre + ".ffn#wop")):
            mine[o:order[order.index(o) + 1]] = True
    assert int(mine.sum()) > sum(SIZES)
    before = model.hip.flat.clone()
    opt, sched = model.configure_optimizers()
    for step in range(2):
        model.training_step(data, step)
        model.optimizer_step(opt, sched)
    assert torch.equal(before.view(torch.int32)[mine], model.hip.flat.view(torch.int32)[mine])
    assert not torch.equal(before.view(torch.int32)[~mine], model.hip.flat.view(torch.int32)[~mine])
    with pytest.raises(ValueError):
        model.set_trainable("everything")
