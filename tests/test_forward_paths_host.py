"""Host checks of tests/forward_cases.py, without a GPU: the window writer against engine.ctx_from_reference_layout, the argument that one
oracle forward per context serves every step, and — per recipe of tests/test_gpu_forward_paths.py at tiny and loop dims — that each fault
those tests exist for (a cache row of RTG tokens or of action tokens left at its placeholder, the representative slot's keys missing)
moves the compared logits by more than 100 x the tolerance they are compared at."""
import numpy as np
import pytest
import torch

from helpers import cfg_of
from ctrlsim_amd import spec, weights
from ctrlsim_amd.engine import CtxBuffers, ctx_from_reference_layout
from ctrlsim_amd.spec import ZERO_ACTION_TOKEN, ZERO_RTG_BINS
import model_oracle as mo
import synth_inputs
import forward_cases as fc

TOL = 1e-4                                  # tests/test_gpu_forward_paths.py, tests/test_gpu_model.py
RECIPES = fc.HOST_RECIPES


def _fields(cb):
    return {f: getattr(cb, f).view(-1).numpy().copy() for f in CtxBuffers.FIELDS}


@pytest.mark.parametrize("kind,B", [("tiny", 3), ("loop", 2)])
def test_fill_window_equals_the_reference_layout_builder(kind, B):
    d = spec.Dims(cfg_of(kind))
    inp = synth_inputs.random_context(d, 31, B=B, n_agents=d.A - 1, n_polys=d.P - 1)
    gid = lambda A: np.broadcast_to(np.arange(A, dtype=np.int32), (B, A)).reshape(-1)
    for Tq in (d.T, 3, 1):
        want = _fields(ctx_from_reference_layout(d, inp, Tq, "cpu"))
        cb = CtxBuffers(d, B, "cpu")
        fc.fill_window(cb, d, inp, 0, Tq, [(B, d.A)])
        got = _fields(cb)
        for f in CtxBuffers.FIELDS:
            if f == "slot_gid":             # the builder leaves -1 and its callers write 0 .. A - 1; fill_window writes that itself
                np.testing.assert_array_equal(got[f], gid(d.A))
            else:
                np.testing.assert_array_equal(got[f], want[f], err_msg=f"{f} Tq={Tq}")
    # a compact class: the leading Actx slots, as _run_compact of tests/test_gpu_model.py hands them to the builder
    Actx = d.A - 1
    sub = {k: (v[:, :Actx] if k in fc.PER_SLOT else v) for k, v in inp.items()}
    want = _fields(ctx_from_reference_layout(d, sub, 3, "cpu"))
    cb = CtxBuffers(d, B, "cpu")
    fc.fill_window(cb, d, inp, 0, 3, [(B, Actx)])
    got = _fields(cb)
    for f in CtxBuffers.FIELDS:
        if f == "slot_gid":
            np.testing.assert_array_equal(got[f][:B * Actx], gid(Actx))
        else:
            np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    # a window that does not start at 0 holds what the builder makes of the inputs shifted by t0 steps
    t0, t1 = 2, 4
    shifted = {k: (np.roll(v, -t0, axis=2) if k in ("agent_states", "actions", "rtgs", "timesteps") else v) for k, v in inp.items()}
    want = _fields(ctx_from_reference_layout(d, shifted, t1 - t0, "cpu"))
    cb = CtxBuffers(d, B, "cpu")
    fc.fill_window(cb, d, inp, t0, t1, [(B, d.A)])
    got = _fields(cb)
    for f in CtxBuffers.FIELDS:
        if f != "slot_gid":
            np.testing.assert_array_equal(got[f], want[f], err_msg=f"{f} window [{t0},{t1})")


@pytest.mark.parametrize("t0,t1", [(0, 8), (3, 5), (0, 1)])
def test_fill_window_of_several_classes_is_the_single_class_fills_at_the_offsets_of_class_structs(t0, t1):
    d = spec.Dims(cfg_of("loop"))
    classes = [(2, 3), (1, 4), (2, 6)]
    rec = fc.teacher_forced(d, 3, classes, d.T)
    Tn = t1 - t0
    cb = CtxBuffers(d, sum(B for B, _ in classes), "cpu")
    fc.fill_window(cb, d, rec.data, t0, t1, classes)
    structs = cb.class_structs(classes, Tn)
    per_ctx = lambda A: dict(st12=Tn * A * 12, exist=Tn * A, goal5=A * 5, act_tok=Tn * A, rtg_bin=Tn * A * 3, tstep=Tn, slot_gid=A,
                             road_pts=d.P * d.NP * 3, road_types=d.P * 8)
    end = {f: 0 for f in CtxBuffers.FIELDS}
    for k, (B, A) in enumerate(classes):
        one = CtxBuffers(d, B, "cpu")
        fc.fill_window(one, d, rec.data[k], t0, t1, [(B, A)])
        for f in CtxBuffers.FIELDS:
            off = (getattr(structs[k], f) - getattr(cb, f).data_ptr()) // 4
            n = B * per_ctx(A)[f]
            assert off == end[f], (f, k)                       # back to back
            np.testing.assert_array_equal(getattr(cb, f).view(-1)[off:off + n].numpy(), getattr(one, f).view(-1)[:n].numpy(),
                                          err_msg=f"{f} class {k}")
            end[f] = off + n
    # separately allocated buffers hold each class from its own start
    sep = [CtxBuffers(d, B + 1, "cpu") for B, _ in classes]
    fc.fill_window(sep, d, rec.data, t0, t1, classes)
    for k, (B, A) in enumerate(classes):
        one = CtxBuffers(d, B + 1, "cpu")
        fc.fill_window(one, d, rec.data[k], t0, t1, [(B, A)])
        for f in CtxBuffers.FIELDS:
            np.testing.assert_array_equal(getattr(sep[k], f).numpy(), getattr(one, f).numpy(), err_msg=f"{f} class {k} (separate)")


def test_recipes_never_hold_a_placeholder_in_a_true_row():
    for name, (kind, wkind, wseed, seed, classes) in RECIPES.items():
        d = spec.Dims(cfg_of(kind))
        rec = fc.teacher_forced(d, seed, classes, d.T)
        for k, src in enumerate(rec.data):
            for c, z in enumerate(ZERO_RTG_BINS):
                assert not (src["rtgs"][..., c] == z).any(), (name, k, c)
            assert not (src["actions"] == ZERO_ACTION_TOKEN).any(), (name, k)
            at = rec.at_step(2)[k]
            assert (at["rtgs"][:, :, 2] == np.asarray(ZERO_RTG_BINS)).all() and (at["actions"][:, :, 2] == ZERO_ACTION_TOKEN).all()
            assert (at["rtgs"][:, :, :2] == src["rtgs"][:, :, :2]).all() and (at["actions"][:, :, :2] == src["actions"][:, :, :2]).all()


def _cut(x, T1):
    """The first T1 window steps of reference-layout inputs."""
    return {k: (v[:, :, :T1] if k in ("agent_states", "actions", "rtgs", "timesteps") else v) for k, v in x.items()}


def _fwd(tw, x, d, dtype=torch.float32):
    x = synth_inputs.to_torch(x)
    if dtype == torch.float64:
        x = {k: (v.double() if v.is_floating_point() else v) for k, v in x.items()}
    with torch.no_grad():
        o = fc._forward(tw, x, d, dtype)
    return o["rtg_preds"].numpy(), o["action_preds"].numpy()


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_one_full_window_oracle_forward_serves_every_step(name):
    """What the device computes at step t — the window cut after row t, placeholders where nothing is sampled yet — against row t of the
    forward over the whole true window, at the bound test_forward_matches_oracle uses for its placeholder argument.  Evaluated in float64:
    the statement is one about the mask, and a float32 forward over a shorter window sums its products in another order (the two float32
    forwards differ by up to 1.2e-6 at loop dims, round-off the 1e-4 of the GPU tests has room for)."""
    kind, wkind, wseed, seed, classes = RECIPES[name]
    d = spec.Dims(cfg_of(kind))
    f64 = torch.float64
    tw = {k: v.double() for k, v in mo.as_torch_weights(fc.make_weights(d, wkind, wseed)).items()}
    rec = fc.teacher_forced(d, seed, classes, d.T)
    rtg_full, act_full = fc.oracle_logits(tw, (wkind, wseed), rec, f64)
    rtg_32, act_32 = fc.oracle_logits(mo.as_torch_weights(fc.make_weights(d, wkind, wseed)), (wkind, wseed), rec)
    for k in range(len(classes)):           # (the float32 forward the GPU tests compare with leaves the device 3/4 of their tolerance)
        assert np.abs(rtg_32[k] - rtg_full[k]).max() < TOL / 4 and np.abs(act_32[k] - act_full[k]).max() < TOL / 4
    for t in range(d.T):
        for k, seen in enumerate(rec.at_step(t)):
            # the first pass: placeholder returns and action in row t
            rtg, _ = _fwd(tw, _cut(seen, t + 1), d, f64)
            assert np.abs(rtg[:, :, t] - rtg_full[k][:, :, t]).max() < 1e-6, (name, k, t, "rtg")
            # the second pass: the true returns of row t, the action still the placeholder
            seen = dict(seen, rtgs=seen["rtgs"].copy())
            seen["rtgs"][:, :, t] = rec.data[k]["rtgs"][:, :, t]
            rtg, act = _fwd(tw, _cut(seen, t + 1), d, f64)
            assert np.abs(rtg[:, :, t] - rtg_full[k][:, :, t]).max() < 1e-6, (name, k, t, "rtg")
            assert np.abs(act[:, :, t] - act_full[k][:, :, t]).max() < 1e-6, (name, k, t, "action")


def _moved(a, b, lv):
    """Per context: the largest change over the live slots."""
    return np.abs(a[:, :lv] - b[:, :lv]).reshape(a.shape[0], -1).max(1)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_the_seeded_faults_move_the_compared_logits(name):
    """A condition on the INPUTS of the GPU tests: each fault must be visible at 100 x the tolerance on at least one live slot of every
    context, or a test that compares at the tolerance could pass over it.  (Relative recipes: 100 x their relative bound x max |logit|.)"""
    kind, wkind, wseed, seed, classes = RECIPES[name]
    d = spec.Dims(cfg_of(kind))
    tw = mo.as_torch_weights(fc.make_weights(d, wkind, wseed))
    rec = fc.teacher_forced(d, seed, classes, d.T)
    rtg_full, act_full = fc.oracle_logits(tw, (wkind, wseed), rec)
    worst = {"stale rtg -> action": np.inf, "stale rtg -> next rtg": np.inf, "stale action -> next rtg": np.inf, "no representative": np.inf}
    for k, (B, A) in enumerate(classes):
        lv, src = fc.live(d, A), rec.data[k]
        need = lambda ref: 100 * TOL if wkind == "peaked" else 100 * 1e-5 * np.abs(ref).max()
        for t in range(d.T):
            # the RTG rows of step t left at the placeholder (the second pass did not refresh the cache)
            bad = dict(src, rtgs=src["rtgs"].copy())
            bad["rtgs"][:, :, t] = ZERO_RTG_BINS
            T1 = min(t + 2, d.T)
            rtg, act = _fwd(tw, _cut(bad, T1), d)
            m = _moved(act[:, :, t], act_full[k][:, :, t], lv) / need(act_full[k][:, :lv, t])
            worst["stale rtg -> action"] = min(worst["stale rtg -> action"], m.min())
            assert (m > 1).all(), (name, k, t, "stale rtg -> action", m)
            if t + 1 < d.T:
                m = _moved(rtg[:, :, t + 1], rtg_full[k][:, :, t + 1], lv) / need(rtg_full[k][:, :lv, t + 1])
                worst["stale rtg -> next rtg"] = min(worst["stale rtg -> next rtg"], m.min())
                assert (m > 1).all(), (name, k, t, "stale rtg -> next rtg", m)
                # the action rows of step t left at the placeholder (step t + 1 did not rewrite them)
                bad = dict(src, actions=src["actions"].copy())
                bad["actions"][:, :, t] = ZERO_ACTION_TOKEN
                rtg, _ = _fwd(tw, _cut(bad, T1), d)
                m = _moved(rtg[:, :, t + 1], rtg_full[k][:, :, t + 1], lv) / need(rtg_full[k][:, :lv, t + 1])
                worst["stale action -> next rtg"] = min(worst["stale action -> next rtg"], m.min())
                assert (m > 1).all(), (name, k, t, "stale action -> next rtg", m)
        # the representative slot's keys dropped: the live slots alone, no padded slot at all
        few = {f: (v[:, :lv] if f in fc.PER_SLOT else v) for f, v in src.items()}
        rtg, act = _fwd(tw, few, d)
        m = np.maximum(_moved(rtg.reshape(B, lv, -1), rtg_full[k][:, :lv].reshape(B, lv, -1), lv) / need(rtg_full[k][:, :lv]),
                       _moved(act.reshape(B, lv, -1), act_full[k][:, :lv].reshape(B, lv, -1), lv) / need(act_full[k][:, :lv]))
        worst["no representative"] = min(worst["no representative"], m.min())
        assert (m > 1).all(), (name, k, "no representative", m)
    print(name, {f: f"{v:.1f} x the need" for f, v in worst.items()})
