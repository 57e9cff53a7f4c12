"""GPU tests of the feed-forward block's backward (csrc/ffn_grad.hip: ctrlsim_ffn_block_grad), of ctrlsim_forward_loss_grads at scope 1 (heads +
the last decoder layer's feed-forward block), of HipModel.update for the block's tensors and of the training loop in scope "heads+ffn",
under both operand splits of the forward where a forward is involved.

ACCURACY BOUND (profiles/ffn_grad_parity.md holds every measured ratio).  The form of tests/test_gpu_head_grads.py: for every gradient
tensor T, relative to max |T_f64|,
    e_hip = max |T_hip - T_f64|,   e_ref = max |T_torch_fp32_cpu - T_f64|   (tests/ffn_grad_ref.py in float64 / float32)
and e_hip <= K max(e_ref, 2^-24), likewise in the Frobenius norm.  K = K_BOUND below: the largest ratio measured on the device rounded
up to a power of two; the specification's ceiling is 16 (four bits for four chained products, two of them recomputed).
Against the reference's OWN recorded gradients (tests/golden/ffn_grads.npz: its trunk, its float32) every tensor is compared relative
to its largest element.  The specification sets the bound at twice the largest deviation measured on the device, rounded up to one
digit, and caps it at 10 x FIX_REL (FIX_REL: the heads' propagated forward-parity bound, tests/test_gpu_head_grads.py).  Measured
(profiles/ffn_grad_parity.md): <= 1.8e-5 everywhere but db1 of case 7 (4.0e-4, both splits) — and case 0 under the two-fp16-plane
split, where all six tensors sit at 1.9e-3 .. 4.9e-3 (9e-7 under the three-bf16-plane split).  That one is a ReLU kink of a HEAD, not an
error: row 74 of the decoder output, hidden unit 123 of predict_future_states, has a LayerNorm output of +4.9e-7 in the default
forward (and, evidently, in the reference) and -2.4e-7 behind this entry's two-kernel last layer, whose output differs from the fused
kernel's by 1e-6; the unit's ReLU passes or blocks, that ROW of dX differs by 1.6 % of max |dX|, and every sum over rows inherits it.
Twice 4.9e-3 is above the cap.  So: FIXTURE_BOUND = 8e-4 (twice 4.0e-4) holds wherever no head has such an element on the returned
decoder output (_head_kinks, float64), and the cap itself, 6.964e-3, where one has."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import golden  # noqa: E402
from ctrlsim_amd import spec, weights, _lib  # noqa: E402
from ctrlsim_amd.models import CtRLSim  # noqa: E402
import loss_ref  # noqa: E402
import head_grad_ref as hgr  # noqa: E402
import ffn_grad_ref as fgr  # noqa: E402
from gpu_utils import DEV  # noqa: E402

K_BOUND = 4.0               # largest measured ratio 3.20 (case 7, f16x3, linear2.weight; profiles/ffn_grad_parity.md), rounded up
K_HEADS = 8.0               # tests/test_gpu_head_grads.py: K_BOUND
FLOOR = 2.0 ** -24
LOSS_REL = 2.97e-6          # the loss route's own bound (profiles/loss_parity.md section 1; tests/test_gpu_head_grads.py)
FIX_REL = 4 * 1.741e-04     # tests/test_gpu_head_grads.py: FIX_REL
FIXTURE_BOUND = 8e-4            # twice the largest measured deviation (4.0e-4: case 7, db1), one digit
FIXTURE_CAP = 10 * FIX_REL      # where a head's ReLU sits on a kink (measured there: 4.93e-3, case 0, f16x3): see the module docstring
EXISTING_CE = 7.428e-07     # tests/test_gpu_loss.py: the bounds of ctrlsim_forward_loss against tests/golden/loss.npz are 4 x these
EXISTING_STATE = 2.978e-08
STEP_LOSS_REL = LOSS_REL    # measured worst 8.0e-7 (case 7): the loss route's bound holds although the decoder output moves
SPLITS = ["f16x3", "bf16x6"]
MODEL_CASES = (0, 1, 7)
assert K_BOUND <= 16.0 and FIXTURE_BOUND <= FIXTURE_CAP and STEP_LOSS_REL <= 1e-5


def _split(lib, name):
    _lib.check(lib.ctrlsim_bind(1 if name == "f16x3" else 0, None))


def _data(inp):
    return {"agent": {k: inp[k] for k in ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask")},
            "map": {k: inp[k] for k in ("road_points", "road_types")}}


def _kw(cfg, d):
    m = cfg.model
    return dict(variant=d.VARIANT, coef=float(m.get("loss_action_coef", 1.0)), supervise_moving=bool(m.get("supervise_moving", True)),
                local_frame=bool(m.get("local_frame_predictions", False)))


def _check(tag, got, want64, got32, k=K_BOUND):
    """The accuracy bound of the module docstring for one tensor; prints the figures before it asserts."""
    got = np.asarray(got, np.float64)
    e_hip, f_hip = hgr.errors(got, want64)
    e_ref, f_ref = hgr.errors(got32, want64)
    print(f"   {tag}: e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {e_hip / max(e_ref, FLOOR):.2f} | F: {f_hip:.3e} {f_ref:.3e} "
          f"ratio {f_hip / max(f_ref, FLOOR):.2f}")
    assert np.isfinite(got).all(), tag
    assert e_hip <= k * max(e_ref, FLOOR), (tag, e_hip, e_ref)
    assert f_hip <= k * max(f_ref, FLOOR), (tag, f_hip, f_ref)


def _bits(t):
    return t.cpu().numpy().view(np.int32 if t.dtype == torch.float32 else np.int64)


# ---- 1. the op
def _chunk_rows(F):
    return int(_lib.lib().ctrlsim_ffn_block_grad_chunk_rows(1 << 24, F))


@functools.lru_cache(maxsize=None)
def _trained_like():
    d = spec.Dims(spec.make_cfg())
    w = weights.generate_trained_like(d, 0)
    return [np.asarray(w[k], np.float32) for k in fgr.names(d)]


@functools.lru_cache(maxsize=None)
def _op_case(rows, F):
    """Seeded inputs of one op shape."""
    return fgr.make_case(rows, F, 7 + rows % 11, _trained_like())


_REFS = {}


def _refs(key, U, dY, T, db1_seen):
    """The float64 / float32 references of the function the device differentiated (ffn_grad_ref.resolve_kinks: the ReLU's side at
    the hidden elements that are zero to float32 rounding is read off the device's db1).  key: cache key (the device is deterministic)."""
    if key is None or key not in _REFS:
        relu_on, n = fgr.resolve_kinks(U, dY, T, np.asarray(db1_seen, np.float64))
        print(f"   ({n} of {relu_on.size} hidden elements are zero to float32 rounding)")
        out = fgr.grads(U, dY, T, relu_on=relu_on), fgr.grads(U, dY, T, dtype=torch.float32, relu_on=relu_on)
        if key is None:
            return out
        _REFS[key] = out
    return _REFS[key]


def _run_op(U, dY, T, ldu=256, lddy=256, lddu=256, want_dU=True, fill=0, alias=False):
    """ctrlsim_ffn_block_grad on host arrays -> ([six gradient tensors], dU or None) as device tensors."""
    lib, st = _lib.lib(), _lib.stream_ptr()
    rows, F = U.shape[0], T[0].shape[0]

    def padded(a, ld):
        t = torch.full((rows, ld), 7.0, device=DEV)
        t[:, :256] = torch.from_numpy(a).to(DEV)
        return t

    Ud, dYd = padded(U, ldu), padded(dY, lddy)
    Td = [torch.from_numpy(t).to(DEV) for t in T]
    n = int(lib.ctrlsim_ffn_block_grad_workspace_bytes(rows, F))
    assert n > 0
    ws = torch.full((n,), fill, dtype=torch.uint8, device=DEV)
    grads = torch.full((2 * F * 256 + F + 3 * 256,), float("nan"), device=DEV)
    dUd = dYd if alias else torch.full((rows, lddu), 7.0, device=DEV) if want_dU else None
    _lib.check(lib.ctrlsim_ffn_block_grad(Ud.data_ptr(), ldu, dYd.data_ptr(), lddy, *(t.data_ptr() for t in Td), rows, F, ws.data_ptr(),
                                          grads.data_ptr(), dUd.data_ptr() if dUd is not None else None, lddy if alias else lddu, st),
               "ffn_block_grad")
    torch.cuda.synchronize()
    if not alias:
        assert torch.equal(dYd[:, :256].cpu(), torch.from_numpy(dY)) and torch.equal(Ud[:, :256].cpu(), torch.from_numpy(U))     # inputs intact
    if dUd is not None and dUd.shape[1] > 256:
        assert (dUd[:, 256:] == 7.0).all()                                 # nothing beyond the 256 columns of a row
    out, o = [], 0
    for t in T:
        out.append(grads[o:o + t.size].view(t.shape))
        o += t.size
    return out, (dUd[:, :256].contiguous() if dUd is not None else None)


def _check_op(tag, got, dU, r64, r32):
    if tag:
        print(tag)
    for name, g, a, b in zip(fgr.PARTS, got, r64[0], r32[0]):
        _check(name, g.cpu().numpy(), a, b)
    if dU is not None:
        _check("dU", dU.cpu().numpy(), r64[1], r32[1])


@pytest.mark.parametrize("shape", ["small", "blocks", "chunk"])
def test_block_grad_matches_float64_autograd(shape):
    """(40, 96): under one tile, a partly filled wave, F no multiple of 64 or 32; (1536, 1024): several row blocks and K slabs;
    (chunk_rows + 48, 1024): crosses a chunk — the accumulation onto the gradient buffer.  All six tensors and dU against float64
    autograd of the same fp32 inputs."""
    rows, F = {"small": (40, 96), "blocks": (1536, 1024), "chunk": (_chunk_rows(1024) + 48, 1024)}[shape]
    U, dY, T = _op_case(rows, F)
    got, dU = _run_op(U, dY, T)
    print(f"op rows {rows} F {F}")
    r64, r32 = _refs((rows, F), U, dY, T, got[1].cpu().numpy())
    _check_op("", got, dU, r64, r32)


def test_block_grad_leading_dimensions_null_du_and_aliased_du():
    """Leading dimensions 320 / 288 / 272 for U / dY / dU give the bits of the dense call; dU = NULL leaves the six tensors unchanged;
    dU = dY (same leading dimension) gives the same dU."""
    U, dY, T = _op_case(1536, 1024)
    dense, dU = _run_op(U, dY, T)
    got, dU2 = _run_op(U, dY, T, ldu=320, lddy=288, lddu=272)
    print("op rows 1536 F 1024, leading dimensions 320 / 288 / 272")
    r64, r32 = _refs((1536, 1024), U, dY, T, got[1].cpu().numpy())
    _check_op("", got, dU2, r64, r32)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(dense, got)) and np.array_equal(_bits(dU), _bits(dU2))
    got, none = _run_op(U, dY, T, want_dU=False)
    assert none is None and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(dense, got))
    got, dU3 = _run_op(U, dY, T, lddy=288, alias=True)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(dense, got)) and np.array_equal(_bits(dU), _bits(dU3))


def test_block_grad_refuses_bad_arguments():
    lib = _lib.lib()
    x = torch.zeros(4096, device=DEV)
    p = x.data_ptr()
    ok = [p, 256, p, 256, p, p, p, p, p, p, 4, 4, p, p, None, 256, None]
    for i, v in ((10, 0), (11, 0), (0, None), (2, None), (4, None), (9, None), (12, None), (13, None)):
        a = list(ok)
        a[i] = v
        assert lib.ctrlsim_ffn_block_grad(*a) == -22, i        # CTRLSIM_EINVAL
    assert lib.ctrlsim_ffn_block_grad_workspace_bytes(0, 4) < 0 and lib.ctrlsim_ffn_block_grad_workspace_bytes(4, 0) < 0


# ---- 2. determinism, no stale state
def test_block_grad_identical_bits_whatever_the_workspace_held():
    U, dY, T = _op_case(1536, 1024)
    a, dUa = _run_op(U, dY, T, fill=0xFF)              # NaN bit patterns
    b, dUb = _run_op(U, dY, T, fill=0x5A)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b)) and np.array_equal(_bits(dUa), _bits(dUb))
    assert all(torch.isfinite(x).all() for x in a) and torch.isfinite(dUa).all()


# ---- 3. through the model, 4. against the reference's recorded backward
def _head_kinks(X, w, variant):
    """Number of head hidden elements relu(LayerNorm(X_k W0^T + b0)) whose LayerNorm output y (float64, from the decoder output X) is
    zero to float32 rounding, |y| <= 2^-24 sqrt(257) (1 + |beta|) — about 1e-6, for the O(1) values a LayerNorm gives.  There the
    ReLU's side, and with it a whole row of dX, belongs to the evaluation (module docstring)."""
    n = 0
    Xt = np.asarray(X, np.float64).reshape(-1, 3, X.shape[-1])
    for h, k in ((hgr.HEADS[0], hgr.action_type(variant)), (hgr.HEADS[1], 0), (hgr.HEADS[2], 2)):
        if h + hgr.PARTS[0] not in w:
            continue
        W0, b0, g, be = (np.asarray(w[h + p], np.float64) for p in hgr.PARTS[:4])
        Z = Xt[:, k] @ W0.T + b0
        mu = Z.mean(1, keepdims=True)
        y = (Z - mu) / np.sqrt(((Z - mu) ** 2).mean(1, keepdims=True) + 1e-5) * g + be
        n += int((np.abs(y) <= fgr.KINK_TOL * (1.0 + np.abs(be))).sum())
    return n


@functools.lru_cache(maxsize=None)
def _model_case(case):
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    return cfg, d, loss_ref.case_weights(case, d), loss_ref.case_inputs(case, d)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("case", MODEL_CASES)
def test_forward_loss_grad_ffn_through_the_model(case, split):
    """ctrlsim_forward_loss_grads at scope 1 on fixture cases 0, 1 (tiny) and 7 (full dims, B = 2): the loss against float64 heads on the
    returned decoder output and against the reference's recorded loss; head gradients and dX against float64 autograd of the heads on
    that output; the block's six tensors and dU against the float64 block applied to the returned U with the returned dX as dY (the
    ReLU's side at float32-zero hidden elements as ffn_grad_ref.resolve_kinks reads it off the device's db1); the
    six tensors against the reference's own recorded backward."""
    lib = _lib.lib()
    cfg, d, w, inp = _model_case(case)
    _split(lib, split)
    try:
        model = CtRLSim(cfg, w, device=DEV)
        assert model.train_grad_layout("heads") == model.head_grad_layout()
        cb, moving, B = model._ctx_of(_data(inp))
        sums, grads, dX, dU, xo, uo = model.loss_and_train_grads_ctx(cb, moving, B, dX=True, dU=True, x_out=True, u_out=True)
        sums = sums.cpu().numpy()
        losses = model.losses_from_sums(sums)
        X, Uh, dXh = xo.cpu().numpy(), uo.cpu().numpy(), dX.cpu().numpy()
        ctx = hgr.ctx_from_inputs(inp)
        r64 = hgr.loss_and_grads(X, w, ctx, **_kw(cfg, d))
        r32 = hgr.loss_and_grads(X, w, ctx, dtype=torch.float32, **_kw(cfg, d))
        print(f"case {case} {split}")
        for k, v in r64[0].items():
            print(f"   {k}: {losses[k]:.9g} float64 heads {v:.9g} rel {abs(losses[k] - v) / abs(v):.3e}")
            assert abs(losses[k] - v) <= LOSS_REL * abs(v), (k, losses[k], v)
        g = golden("loss")                        # the two-kernel last layer against the reference: ctrlsim_forward_loss's own bounds
        keys = [str(k) for k in g[f"c{case}_keys"]]
        assert model.loss_keys() == keys
        for j, k in enumerate(keys):
            want, cnt = float(g[f"c{case}_loss"][j]), float(g[f"c{case}_count"][j])
            assert sums[loss_ref.KEYS.index(k), 1] == cnt, k
            assert abs(losses[k] - want) / abs(want) <= 4 * (EXISTING_STATE if k == "loss_state" else EXISTING_CE), (k, losses[k], want)
        heads = hgr.head_names(w)
        new = fgr.names(d)
        assert list(grads) == heads + new
        got = {k: v.cpu().numpy() for k, v in grads.items()}
        for k in heads:
            _check(k, got[k], r64[2][k], r32[2][k], K_HEADS)
        _check("dX", dXh, r64[3], r32[3], K_HEADS)
        T = [np.asarray(w[k], np.float32) for k in new]
        f64, f32 = _refs(None, Uh, dXh, T, got[new[1]])
        for k, a, b in zip(new, f64[0], f32[0]):
            _check(k, got[k], a, b)
        _check("dU", dU.cpu().numpy(), f64[1], f32[1])
        # the reference's own numbers (its trunk, its float32): sampled rows, column sums, norms
        gf = golden("ffn_grads")
        P = f"c{case}_"
        worst = 0.0
        print(f"   cancellation in dbe = sum of dX's rows: sum |dX| / |sum dX| = {np.abs(dXh).sum(0).max() / np.abs(got[new[5]]).max():.1f}")
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
        nk = _head_kinks(X, w, d.VARIANT)
        bound = FIXTURE_CAP if nk else FIXTURE_BOUND
        print(f"   worst {worst:.3e} (bound {bound:.3e}: {nk} head hidden elements on a ReLU kink)")
        assert worst <= bound
    finally:
        _split(lib, "f16x3")


# ---- 5. HipModel.update
@pytest.mark.parametrize("split", SPLITS)
def test_update_of_the_block_equals_a_fresh_model_bit_for_bit(split):
    lib = _lib.lib()
    _split(lib, split)
    try:
        cfg, d, w, inp = _model_case(1)
        data = _data(inp)
        model = CtRLSim(cfg, dict(w), device=DEV)
        before = model.hip.flat.clone()
        rs = np.random.RandomState(4)
        names = fgr.names(d)
        new = {k: (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32) for k in names}
        model.hip.update(new)
        fresh = CtRLSim(cfg, {**w, **new}, device=DEV)
        assert torch.equal(model.hip.flat.view(torch.int32), fresh.hip.flat.view(torch.int32))          # every image re-derived in place
        a, b = model.loss_sums(data)[0].cpu().numpy(), fresh.loss_sums(data)[0].cpu().numpy()
        assert np.array_equal(a.view(np.int64), b.view(np.int64))
        touched = torch.zeros(before.numel(), dtype=torch.bool, device=DEV)
        off = model.hip._offset
        order = sorted(off.values()) + [before.numel()]
        pre = fgr.layer_prefix(d)
        for name, o in off.items():
            if name.split("#")[0] in new or name.startswith(pre + ".ffn#"):
                touched[o:order[order.index(o) + 1]] = True
        assert torch.equal(before.view(torch.int32)[~touched], model.hip.flat.view(torch.int32)[~touched])   # unrelated tensors unchanged
        assert not torch.equal(before.view(torch.int32)[touched], model.hip.flat.view(torch.int32)[touched])
        snap = model.hip.flat.clone()
        with pytest.raises(FloatingPointError):
            model.hip.update({names[2]: np.full_like(new[names[2]], 1.0e6)})
        assert torch.equal(snap.view(torch.int32), model.hip.flat.view(torch.int32))                    # nothing written
        with pytest.raises(KeyError):
            model.hip.update({"encoder.embed_ln.weight": np.ones(256, np.float32)})
        with pytest.raises(KeyError):
            model.hip.update({f"decoder.transformer_decoder.layers.{d.ND - 1}.norm2.weight": np.ones(256, np.float32)})
    finally:
        _split(lib, "f16x3")


# ---- 6. training loop
def _twin(cfg, d, w, U, ctx, kw, steps):
    """torch float64: the heads and the block on the same (constant) block input U, the same AdamW groups, clip and schedule."""
    heads, new = hgr.head_names(w), fgr.names(d)
    params = {k: torch.nn.Parameter(torch.tensor(np.asarray(w[k]), dtype=torch.float64)) for k in heads + new}
    decay, no_decay = CtRLSim.param_groups(heads + new)
    tr = cfg.train
    opt = torch.optim.AdamW([{"params": [params[k] for k in decay], "weight_decay": tr["weight_decay"]},
                             {"params": [params[k] for k in no_decay], "weight_decay": 0.0}], lr=tr["lr"], weight_decay=tr["weight_decay"])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=CtRLSim.lr_lambda(tr))

    def evaluate():
        now = {k: p.detach().numpy() for k, p in params.items()}
        T = [now[k] for k in new]
        _, final, g, dX = hgr.loss_and_grads(fgr.forward(U, T), {k: now[k] for k in heads}, ctx, **kw)
        g.update(zip(new, fgr.grads(U, dX, T)[0]))
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


@pytest.mark.parametrize("case", [0, 7])
def test_five_training_steps_in_scope_heads_ffn_follow_the_float64_twin(case):
    """training_step / optimizer_step five times on one fixed batch with set_trainable("heads+ffn").  Everything upstream of the block
    is frozen, so its input U is constant (asserted bit for bit) and a float64 twin can train the heads and the block on it.  Loss per
    step within STEP_LOSS_REL of the twin's; weights by the two-part criterion of tests/test_gpu_head_grads.py, recomputed here:
    (a) every element within 2 sum_t lr_t sqrt(t) + 5 x 2^-24 |w|, (b) all but 1e-3 of them within 1e-3 sum_t lr_t + 5 x 2^-24 |w|."""
    cfg, d, w, inp = _model_case(case)
    w0 = {k: np.array(v) for k, v in w.items()}
    model = CtRLSim(cfg, dict(w0), device=DEV).set_trainable("heads+ffn")
    data = _data(inp)
    u0 = model.loss_and_train_grads(data, u_out=True)[5]
    heads, new = hgr.head_names(w), fgr.names(d)
    assert list(model.trainable_parameters()) == heads + new
    assert all(model.trainable_parameters()[k] is model.head_parameters()[k] for k in heads)
    opt, sched = model.configure_optimizers()
    got = []
    for step in range(5):
        got.append(model.training_step(data, step))
        assert all(p.grad is not None for p in model.trainable_parameters().values())
        model.optimizer_step(opt, sched)
    out = model.loss_and_train_grads(data, u_out=True)
    got.append(model.final_loss(model.losses_from_sums(out[0].cpu().numpy())))
    assert torch.equal(u0, out[5])                                                 # everything in front of the block did not move
    want, w_twin = _twin(cfg, d, w0, u0.cpu().numpy(), hgr.ctx_from_inputs(inp), _kw(cfg, d), 5)
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
        have = (model.hip._heads if k in heads else model.hip._ffn)[k].astype(np.float64)
        assert np.array_equal(have, np.asarray(model.weights[k], np.float64))
        diff = np.abs(have - v)
        rnd = 5 * FLOOR * np.abs(v)
        assert (diff <= worst_case + rnd).all(), k
        n_all += diff.size
        n_off += int((diff > bulk + rnd).sum())
        drift = max(drift, float(diff.max()))
        assert np.abs(v - np.asarray(w0[k], np.float64)).max() > 0, k
    print(f"   weights after five steps: max |w - twin| {drift:.3e} (sum lr {sum(lrs):.1e}), {n_off} of {n_all} elements beyond the bulk tolerance")
    assert n_off <= 1e-3 * n_all


def test_default_scope_leaves_the_trunk_alone():
    """Scope "heads" (the default): training moves no decoder output — the assertion of the head training test, repeated here — and
    trainable_parameters() is head_parameters()."""
    cfg, d, w, inp = _model_case(0)
    model = CtRLSim(cfg, {k: np.array(v) for k, v in w.items()}, device=DEV)
    data = _data(inp)
    assert list(model.trainable_parameters()) == list(model.head_parameters())
    _, _, _, xo = model.loss_and_head_grads(data, x_out=True)
    opt, sched = model.configure_optimizers()
    for step in range(2):
        model.training_step(data, step)
        model.optimizer_step(opt, sched)
    _, _, _, xo2 = model.loss_and_head_grads(data, x_out=True)
    assert torch.equal(xo, xo2)
    with pytest.raises(ValueError):
        model.set_trainable("everything")
