"""GPU tests of the open-loop loss: ctrlsim_forward_loss (fused cross-entropy heads, csrc/loss.hip) against the from-memory route, the
float64 restatement of the reference's compute_loss (tests/loss_ref.py) and exact small-integer cases.

Bounds (profiles/loss_parity.md holds the measured figures), EPS = 2^-23:
  * PATHS — fused against from-memory, per row and softmax: |delta nll| <= 64 EPS (|lse| + |logit|).  Both routes evaluate the same
    logits in real arithmetic; they differ in the fp32 accumulation order of a K = 256 product (bias first / last, other MFMA chain:
    ~ sqrt(256) = 16 roundings of typical size), in two quantities (lse, target logit), and in the order of the exp sum (x 2).
  * HOST — from-memory route against a float64 log-sum-exp of the SAME fp32 logits: 16 EPS (|lse| + |logit|): fp32 exp / log within an
    ulp each, a 1000-term fp32 sum reduced in 64 lanes + a tree, and the final max + log rounding.
  * sums / means: the per-row bound times the count (sums) / as is (means); the state term sees identical fp32 predictions on every
    route and differs in float64 summation order only: 1e-12 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import cfg_of, golden  # noqa: E402
from ctrlsim_amd import spec, weights, _lib, pack  # noqa: E402
from ctrlsim_amd.models import CtRLSim  # noqa: E402
import synth_inputs  # noqa: E402
import loss_ref  # noqa: E402
from gpu_utils import DEV  # noqa: E402

EPS = 2.0 ** -23
K_PATHS, K_HOST = 64.0, 16.0


def _data(inp):
    return {"agent": {k: inp[k] for k in ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask")},
            "map": {k: inp[k] for k in ("road_points", "road_types")}}


def _inputs(d, seed, B):
    return loss_ref.make_inputs(d, seed, B)


def _row_bound(row, k):
    """k EPS (|lse| + |logit|) per row and softmax; rows the restatement does not define (NaN) get 0 weight through the caller's mask."""
    return k * EPS * (np.abs(row[..., 0]) + np.abs(row[..., 1]))


def _split(lib, name):
    _lib.check(lib.ctrlsim_bind(1 if name == "f16x3" else 0, None))


CASES = loss_ref.CASES


def _model(i):
    cfg = loss_ref.case_cfg(i)
    d = spec.Dims(cfg)
    return cfg, d, CtRLSim(cfg, loss_ref.case_weights(i, d), device=DEV)


def _ref(cfg, d, inp, preds):
    m = cfg.model
    p = {k: (v.cpu().numpy() if v is not None else None) for k, v in preds.items()}
    return loss_ref.loss_sums(inp, p, R=d.R, C=d.C, supervise_moving=bool(m.get("supervise_moving", True)),
                              local_frame=bool(m.get("local_frame_predictions", False)), trajeglish=d.VARIANT == 2)


@pytest.mark.parametrize("split", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_forward_loss_matches_float64_restatement_on_the_logits_route(case, split):
    """Every term of compute_loss: ctrlsim_forward_loss (fused where the split allows it) and compute_loss(data, preds) against the float64
    restatement applied to the logits of the shipped forward (ctrlsim_forward_all), per row, per context and in total; the reference's
    key set; compute_loss(data) == compute_loss(data, model(data)) within the bounds."""
    kind, variant, over, wkind, _ = CASES[case]
    lib = _lib.lib()
    lib.ctrlsim_nonfinite_count(1)
    _split(lib, split)
    try:
        cfg, d, model = _model(case)
        inp = loss_ref.case_inputs(case, d)
        data = _data(inp)
        preds = model(data)
        if not bool(cfg.model.get("predict_future_states", True)):
            preds.pop("state_preds", None)
        ref = _ref(cfg, d, inp, preds)
        keys = model.loss_keys()
        want_keys = ["loss_actions"] + (["loss_rtg_goal", "loss_rtg_veh", "loss_rtg_road"] if variant is None else []) + \
                    (["loss_state"] if variant is None else [])
        assert keys == want_keys
        coef = float(cfg.model.get("loss_action_coef", 1.0))
        want = loss_ref.losses(ref["sums"], keys, coef)
        assert all(ref["sums"][loss_ref.KEYS.index(k), 1] > 0 for k in keys)
        for tag, k_row, kw in (("fused", K_PATHS + K_HOST, dict()), ("memory", K_PATHS + K_HOST, dict(fused=False)), ("preds", K_HOST, dict(preds=preds))):
            sums, pc, rn = model.loss_sums(data, per_ctx=True, row_nll=True, **kw)
            sums, pc, rn = sums.cpu().numpy(), pc.cpu().numpy(), rn.cpu().numpy()
            nsm = 4 if "loss_rtg_goal" in keys else 1
            rr = ref["row"][..., :nsm, :]
            defined = np.isfinite(rr[..., 0])
            bound = _row_bound(rr, k_row)
            err = np.abs(rn[..., :nsm] - (rr[..., 0] - rr[..., 1]))
            print(f"case {case} {split} {tag}: max row err / bound = {np.nanmax(np.where(defined, err / bound, 0)):.3f}, max |err| = {np.nanmax(np.where(defined, err, 0)):.3e}")
            assert (err[defined] <= bound[defined]).all(), tag
            rb = float(bound[defined].max())
            for k in keys:
                i = loss_ref.KEYS.index(k)
                if i == 4:
                    np.testing.assert_allclose(pc[:, 4], ref["per_ctx"][:, 4], rtol=1e-12, atol=0, err_msg=tag)
                    np.testing.assert_allclose(sums[4], ref["sums"][4], rtol=1e-12, atol=0, err_msg=tag)
                else:
                    np.testing.assert_array_equal(pc[:, i, 1], ref["per_ctx"][:, i, 1])
                    assert (np.abs(pc[:, i, 0] - ref["per_ctx"][:, i, 0]) <= rb * np.maximum(ref["per_ctx"][:, i, 1], 1)).all(), (tag, k)
            got = model.losses_from_sums(sums)
            assert list(got) == keys
            for k in keys:
                tol = 1e-12 * abs(want[k]) if k == "loss_state" else rb * max(coef, 1.0)
                print(f"   {k}: got {got[k]:.9g} want {want[k]:.9g}")
                assert abs(got[k] - want[k]) <= tol, (tag, k, got[k], want[k])
            # per_ctx adds up to sums (same float64 values, another summation order)
            np.testing.assert_allclose(pc.sum(0), sums, rtol=1e-12, atol=0)
        a, b = model.compute_loss(data), model.compute_loss(data, model(data))
        assert list(a) == list(b) == keys
        val = model.validation_step(data)
        assert list(val) == [CtRLSim.VAL_NAMES[k] for k in keys] and val["val_loss"] == a["loss_actions"]
        for k in keys:
            assert abs(a[k] - b[k]) <= (1e-12 * abs(a[k]) if k == "loss_state" else K_PATHS * EPS * 2 * float(np.nanmax(np.abs(ref["row"]))) * max(coef, 1.0)), k
        assert lib.ctrlsim_nonfinite_count(0) % 65536 == 0
    finally:
        _split(lib, "f16x3")


# (i) bounds against the reference's own numbers (tests/golden/loss.npz).  Measured first on the EXISTING route — the logits of
# ctrlsim_forward_all reduced in float64 on the host — over every case (profiles/loss_parity.md): that error belongs to the shipped
# forward and to the reference's float32 evaluation of its loss, not to the new kernels; the bounds are 4 x those figures.
EXISTING_CE = 7.428e-07     # max |loss - reference| over the cross-entropy terms of every case, relative to the reference value
EXISTING_STATE = 2.978e-08  # the same for loss_state
EXISTING_ROW = 1.741e-04    # max |nll - reference| per row and softmax (tiny cases; the trained-like weights' logits reach +-60), absolute


def existing_route(case):
    """-> (model, data, losses of the existing route, its per-row nll) of one fixture case."""
    cfg, d, model = _model(case)
    inp = loss_ref.case_inputs(case, d)
    data = _data(inp)
    preds = model(data)
    if not bool(cfg.model.get("predict_future_states", True)):
        preds.pop("state_preds", None)
    ref = _ref(cfg, d, inp, preds)
    keys = model.loss_keys()
    return model, data, loss_ref.losses(ref["sums"], keys, float(cfg.model.get("loss_action_coef", 1.0))), ref["row"][..., 0] - ref["row"][..., 1]


@pytest.mark.parametrize("split", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_forward_loss_matches_reference_fixture(case, split):
    """(i) ctrlsim_forward_loss against the UNMODIFIED reference's compute_loss on its own forward (tests/golden/loss.npz): every case,
    both operand splits, every term; per-row nll where the fixture holds it (tiny cases)."""
    g = golden("loss")
    lib = _lib.lib()
    _split(lib, split)
    try:
        cfg, d, model = _model(case)
        data = _data(loss_ref.case_inputs(case, d))
        keys = [str(k) for k in g[f"c{case}_keys"]]
        assert model.loss_keys() == keys
        sums, _, rn = model.loss_sums(data, row_nll=True)
        sums = sums.cpu().numpy()
        got = model.losses_from_sums(sums)
        for j, k in enumerate(keys):
            want, cnt = float(g[f"c{case}_loss"][j]), float(g[f"c{case}_count"][j])
            rel = abs(got[k] - want) / abs(want)
            print(f"case {case} {split} {k}: got {got[k]:.9g} reference {want:.9g} rel {rel:.3e}")
            assert sums[loss_ref.KEYS.index(k), 1] == cnt, k
            assert rel <= 4 * (EXISTING_STATE if k == "loss_state" else EXISTING_CE), k
        if f"c{case}_row_nll" in g.files:
            want = g[f"c{case}_row_nll"]
            ok = np.isfinite(want)
            err = np.abs(rn.cpu().numpy() - want)[ok]
            print(f"case {case} {split} rows: max |nll - reference| = {err.max():.3e}")
            assert err.max() <= 4 * EXISTING_ROW
    finally:
        _split(lib, "f16x3")


def _full_batch(B, seed=5):
    cfg = cfg_of("full")
    d = spec.Dims(cfg)
    model = CtRLSim(cfg, weights.generate_trained_like(d, 0), device=DEV)
    inp = _inputs(d, seed, B=B)
    return cfg, d, model, inp


def test_fused_path_matches_memory_path_per_row_at_full_size():
    """(ii) one batch of 64 full-size windows, trained-like weights: per-row nll of the fused heads against the from-memory route."""
    lib = _lib.lib()
    lib.ctrlsim_nonfinite_count(1)
    cfg, d, model, inp = _full_batch(64)
    data = _data(inp)
    s_a, pc_a, rn_a = model.loss_sums(data, per_ctx=True, row_nll=True, fused=True)
    s_c, pc_c, rn_c = model.loss_sums(data, per_ctx=True, row_nll=True, fused=False)
    # the bound needs |lse| and |logit|: from the logits of the shipped forward, in float64 on the host, a few contexts at a time
    worst, worst_abs = 0.0, 0.0
    for b0 in range(0, 64, 8):
        sub = {k: v[b0:b0 + 8] for k, v in inp.items()}
        preds = model(_data(sub))
        ref = _ref(cfg, d, sub, preds)["row"]
        bound = _row_bound(ref, K_PATHS)
        err = np.abs(rn_a[b0:b0 + 8].cpu().numpy() - rn_c[b0:b0 + 8].cpu().numpy())
        worst = max(worst, float((err / bound).max()))
        worst_abs = max(worst_abs, float(err.max()))
        assert (err <= bound).all()
    print(f"fused vs memory, B = 64 full dims: max |delta nll| = {worst_abs:.3e}, max delta / bound(64 EPS) = {worst:.3f}")
    np.testing.assert_array_equal(s_a[:, 1].cpu().numpy(), s_c[:, 1].cpu().numpy())
    np.testing.assert_allclose(s_a[4].cpu().numpy(), s_c[4].cpu().numpy(), rtol=1e-12)
    assert lib.ctrlsim_nonfinite_count(0) == 0                                                   # (v) the guard pair stays 0


def test_batch_scored_whole_equals_two_calls_and_workspace_contents_do_not_matter():
    """(iii) B contexts in one call == the same contexts in two calls accumulated into the same sums (float64, another tree: 1e-12);
    (iv) a workspace full of 0xFF bytes gives identical bits (nothing is read before it is written); run to run identical bits."""
    cfg, d, model, inp = _full_batch(6, seed=9)
    from ctrlsim_amd.engine import ctx_from_reference_layout
    lib, st = _lib.lib(), _lib.stream_ptr()
    lcfg = model.loss_cfg(True)

    def run(lo, hi, sums, fill):
        sub = {k: v[lo:hi] for k, v in inp.items()}
        B = hi - lo
        cb = ctx_from_reference_layout(d, sub, d.T, DEV)
        mv = torch.from_numpy((sub["moving_agent_mask"] != 0).astype(np.uint8)).to(DEV)
        ws = torch.full((int(lib.ctrlsim_forward_loss_workspace_bytes(C.byref(model.hip.cdims), B, d.T)),), fill, dtype=torch.uint8, device=DEV)
        pc = torch.zeros(B, 5, 2, dtype=torch.float64, device=DEV)
        _lib.check(lib.ctrlsim_forward_loss(model.hip.handle, B, d.T, C.byref(cb.struct), mv.data_ptr(), C.byref(lcfg), ws.data_ptr(),
                                            sums.data_ptr(), pc.data_ptr(), None, st))
        torch.cuda.synchronize()
        return pc.cpu().numpy()

    z = lambda: torch.zeros(5, 2, dtype=torch.float64, device=DEV)
    whole, whole_ff, again, parts = z(), z(), z(), z()
    pc_w = run(0, 6, whole, 0)
    pc_f = run(0, 6, whole_ff, 0xFF)
    run(0, 6, again, 0)
    pc_1 = run(0, 4, parts, 0)
    pc_2 = run(4, 6, parts, 0xFF)
    assert np.array_equal(pc_w, pc_f) and np.array_equal(whole.cpu().numpy(), whole_ff.cpu().numpy())
    assert np.array_equal(whole.cpu().numpy(), again.cpu().numpy())
    assert np.array_equal(np.concatenate([pc_1, pc_2]), pc_w)                   # a context's numbers do not depend on its batch
    np.testing.assert_allclose(parts.cpu().numpy(), whole.cpu().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(pc_w.sum(0), whole.cpu().numpy(), rtol=1e-12, atol=0)


def test_zero_count_term_is_nan():
    """A term whose mask sums to zero is 0 / 0 in the reference: NaN here, with count 0 in the sums."""
    cfg, d, model = _model(0)
    inp = _inputs(d, 3, B=2)
    inp["moving_agent_mask"][:] = 0.0
    sums, _, _ = model.loss_sums(_data(inp))
    sums = sums.cpu().numpy()
    assert (sums[:, 1] == 0).all() and (sums[:, 0] == 0).all()
    assert all(np.isnan(v) for v in model.losses_from_sums(sums).values())


@pytest.mark.parametrize("n,nsm", [(1000, 1), (350, 3), (40, 2)])
def test_head_ce_pad_columns_and_block_edges_exact(n, nsm):
    """(vii) small-integer hidden rows, weights and biases: every logit is an exactly representable integer.  Targets at the last real
    column (999 / bin 349 of each component), at the first and last column of a block, and every real logit far BELOW the 0 a pad
    column would contribute if it were not masked by index."""
    lib, st = _lib.lib(), _lib.stream_ptr()
    rs = np.random.RandomState(n)
    M = 300                                                               # a full 256-row job and a partial one
    H = rs.randint(-3, 4, (M, 256)).astype(np.float32)
    W = rs.randint(-2, 3, (n * nsm, 256)).astype(np.float32)
    bias = rs.randint(-4, 5, n * nsm).astype(np.float32) - 3000.0       # real logits <= 256 * 6 + 4 - 3000 < 0 = an unmasked pad column
    tgt = rs.randint(0, n, (M, nsm)).astype(np.int32)
    edge = [n - 1, 0, 31, 32, min(63, n - 1), (n - 1) // 32 * 32]
    for i, e in enumerate(edge):
        tgt[i] = e
        tgt[256 + i] = e
    blk, bce = pack.head_ce_image(W, bias, nsm, 1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    Hd, Wd, bd, td = dev(H), dev(blk.reshape(-1).view(np.float32)), dev(bce), dev(tgt)
    lt = torch.full((M, 4, 2), float("nan"), device=DEV)
    rc = lib.ctrlsim_head_ce(Hd.data_ptr(), 256, Wd.data_ptr(), bd.data_ptr(), td.data_ptr(), M, n, nsm, lt.data_ptr(), st)
    assert rc == 0
    torch.cuda.synchronize()
    lt = lt.cpu().numpy().astype(np.float64)
    logits = (H.astype(np.float64) @ W.astype(np.float64).T + bias).reshape(M, n, nsm)
    for s in range(nsm):
        z = logits[:, :, s]
        mx = z.max(1)
        lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
        np.testing.assert_array_equal(lt[:, s, 1], z[np.arange(M), tgt[:, s]])                  # exact
        assert (np.abs(lt[:, s, 0] - lse) <= K_HOST * EPS * np.abs(lse)).all()
    assert np.isnan(lt[:, nsm:]).all()                                    # nothing written beyond the head's softmaxes


def test_open_loop_evaluator_chunks_add_up():
    """OpenLoopEvaluator over 5 full-size windows in chunks of 2 == the same windows scored in one call (counts exact, sums to float64
    summation order), the reference's keys, and a batch size from the workspace query that respects the budget."""
    from ctrlsim_amd.evaluators import OpenLoopEvaluator
    cfg, d, model, inp = _full_batch(5, seed=13)
    windows = [{k: v[i] for k, v in inp.items()} for i in range(5)]
    ev = OpenLoopEvaluator(cfg, model)
    out = ev.evaluate(windows, batch_size=2)
    whole, _, _ = model.loss_sums(_data(inp))
    whole = whole.cpu().numpy()
    np.testing.assert_array_equal(out["sums"][:, 1], whole[:, 1])
    np.testing.assert_allclose(out["sums"], whole, rtol=1e-12, atol=0)
    assert [k for k in out if k.startswith("loss_")] == model.loss_keys() and out["windows"] == 5 and out["windows_per_s"] > 0
    lib = _lib.lib()
    need = lambda b: int(lib.ctrlsim_forward_loss_workspace_bytes(C.byref(model.hip.cdims), b, d.T))
    small = OpenLoopEvaluator(cfg, model, workspace_bytes=need(3) + 1000)
    assert small.batch_size() == 3 and need(4) > need(3) + 1000
