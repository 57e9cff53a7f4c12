"""CPU tests of the feed-forward-block gradient path's host side and of its checker:
  * tests/ffn_grad_ref.py (float64 autograd restatement of the block) against central finite differences;
  * ctrlsim_train_grad_layout against CtRLSim.head_grad_layout (scope 0) and the parameter table (scope 1);
  * pack.ffn_images against pack.pack, bit for bit;
  * the AdamW parameter groups with the new names;
  * the checker's handling of ReLU kinks (ffn_grad_ref.resolve_kinks)."""
import numpy as np
import pytest

from helpers import golden
from ctrlsim_amd import spec, weights, pack
from ctrlsim_amd.models import CtRLSim
import loss_ref
import head_grad_ref as hgr
import ffn_grad_ref as fgr


def test_restatement_matches_central_differences():
    """6 rows, F = 8, float64: d/dp sum(Y * dY) by central differences (step 1e-6) for every element of the six tensors and of U."""
    rs = np.random.RandomState(0)
    rows, Fh = 6, 8
    U = rs.standard_normal((rows, 256))
    dY = rs.standard_normal((rows, 256))
    T = [rs.standard_normal((Fh, 256)) / 16, rs.standard_normal(Fh), rs.standard_normal((256, Fh)) / 3, rs.standard_normal(256) * 0.1,
         1 + 0.1 * rs.standard_normal(256), 0.1 * rs.standard_normal(256)]
    g, dU = fgr.grads(U, dY, T)
    f = lambda U_, T_: float((fgr.forward(U_, T_) * dY).sum())
    h = 1e-6

    def fd(arr, idx, call):
        old = arr[idx]
        arr[idx] = old + h
        up = call()
        arr[idx] = old - h
        dn = call()
        arr[idx] = old
        return (up - dn) / (2 * h)

    for t, gt in zip(T, g):
        pick = [np.unravel_index(i, t.shape) for i in rs.permutation(t.size)[:48]]
        scale = np.abs(gt).max()
        for idx in pick:
            assert abs(fd(t, idx, lambda: f(U, T)) - gt[idx]) <= 1e-6 * scale + 1e-8, idx
    scale = np.abs(dU).max()
    for i in rs.permutation(U.size)[:48]:
        idx = np.unravel_index(i, U.shape)
        assert abs(fd(U, idx, lambda: f(U, T)) - dU[idx]) <= 1e-6 * scale + 1e-8, idx
    # relu'(0) = 0: a hidden unit that is exactly 0 passes nothing
    T0 = [np.zeros((Fh, 256)), np.zeros(Fh)] + T[2:]
    g0, dU0 = fgr.grads(U, dY, T0)
    assert not g0[0].any() and not g0[1].any() and not g0[2].any()


@pytest.mark.parametrize("case", [0, 4, 7])
def test_training_layout_extends_the_head_layout(case):
    """ctrlsim_train_grad_layout (needs the library, not a device): scope 0 is CtRLSim.head_grad_layout name by name and offset by
    offset; scope 1 appends the last decoder layer's six tensors, back to back, with the parameter table's shapes."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    w = loss_ref.case_weights(case, d)
    model = CtRLSim(cfg, w, device="cpu")
    heads, total = model.head_grad_layout()
    assert model.train_grad_layout("heads") == (heads, total)
    layout, total1 = model.train_grad_layout("heads+ffn")
    assert layout[:len(heads)] == heads
    table = {n: tuple(s) for n, s, _, _ in weights.param_table(d)}
    tail = layout[len(heads):]
    assert [n for n, _, _ in tail] == fgr.names(d)
    off = total
    for n, o, s in tail:
        assert o == off and s == table[n]
        off += int(np.prod(s))
    assert total1 == off
    assert table[fgr.names(d)[0]] == (d.F, d.D) and table[fgr.names(d)[2]] == (d.D, d.F)


@pytest.mark.parametrize("case", [0, 7])
def test_ffn_images_equal_a_fresh_pack(case):
    """pack.ffn_images on perturbed linear1 / linear2 weights: every image whose name derives from them, bit-equal to its slice of
    pack.pack of the perturbed state dict."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    w = dict(loss_ref.case_weights(case, d))
    pre = fgr.layer_prefix(d)
    rs = np.random.RandomState(5)
    for k in fgr.names(d):
        w[k] = (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32)
    flat, names, offsets = pack.pack(d, w)
    off = dict(zip(names, (int(o) for o in offsets)))
    layer = {k: w[k] for k in (pre + ".linear1.weight", pre + ".linear2.weight", pre + ".multihead_attn.out_proj.weight")}
    images = pack.ffn_images(d, layer, off)
    derived = {n for n in names if n.startswith((pre + ".linear1.weight#", pre + ".linear2.weight#", pre + ".ffn#"))}
    assert set(images) == derived and len(derived) == 10          # 2 x 2 planes, 2 x 2 fused images, w1q, wop
    for n, v in images.items():
        assert v.dtype == np.float32 and v.ndim == 1
        assert np.array_equal(flat[off[n]:off[n] + v.size].view(np.int32), v.view(np.int32)), n
    bad = dict(layer)
    bad[pre + ".linear2.weight"] = np.full_like(layer[pre + ".linear2.weight"], 1.0e6)
    with pytest.raises(FloatingPointError):
        pack.ffn_images(d, bad, off)


def test_param_groups_with_the_feed_forward_names():
    g = golden("head_grads")
    cfg = loss_ref.case_cfg(0)
    d = spec.Dims(cfg)
    heads = hgr.head_names(weights.generate(d, 0))
    decay, no_decay = CtRLSim.param_groups(heads)
    assert decay == [str(k) for k in g["decay"]] and no_decay == [str(k) for k in g["no_decay"]]      # head names alone: as recorded
    new = fgr.names(d)
    decay2, no_decay2 = CtRLSim.param_groups(heads + new)
    pre = fgr.layer_prefix(d)
    assert decay2 == sorted(decay + [pre + ".linear1.weight", pre + ".linear2.weight"])
    assert no_decay2 == sorted(no_decay + [pre + ".linear1.bias", pre + ".linear2.bias", pre + ".norm3.weight", pre + ".norm3.bias"])


def test_kink_resolution_follows_the_evaluation_under_test():
    """ffn_grad_ref.resolve_kinks: with the float64 mask the masked form of the block is the ReLU form, bit for bit; a hidden element
    planted at zero-to-float32-rounding is found, and its side is read off the db1 it is handed — either side."""
    rs = np.random.RandomState(1)
    rows, Fh = 12, 8
    U = rs.standard_normal((rows, 256))
    dY = rs.standard_normal((rows, 256))
    T = [rs.standard_normal((Fh, 256)) / 16, rs.standard_normal(Fh), rs.standard_normal((256, Fh)) / 3, rs.standard_normal(256) * 0.1,
         1 + 0.1 * rs.standard_normal(256), 0.1 * rs.standard_normal(256)]
    T[1][3] += 1e-9 - (U[5] @ T[0][3] + T[1][3])                    # Hp[5, 3] = +1e-9
    plain = fgr.grads(U, dY, T)
    on, n = fgr.resolve_kinks(U, dY, T, plain[0][1])
    assert n == 1 and on[5, 3]
    masked = fgr.grads(U, dY, T, relu_on=on)
    assert all(np.array_equal(a, b) for a, b in zip(plain[0], masked[0])) and np.array_equal(plain[1], masked[1])
    off = on.copy()
    off[5, 3] = False
    other = fgr.grads(U, dY, T, relu_on=off)
    assert other[0][1][3] != plain[0][1][3]
    on2, _ = fgr.resolve_kinks(U, dY, T, other[0][1])               # an evaluation that rounded Hp[5, 3] below zero
    assert np.array_equal(on2, off)
