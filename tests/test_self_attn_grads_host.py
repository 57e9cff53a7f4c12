"""CPU tests of the self-attention gradient path's host side and of its checker:
  * tests/self_attn_grad_ref.py: its mask against oracle/model_oracle.py:causal_mask_closed_form in both modes, every row with a visible
    key, and the restated sublayer against torch.nn.MultiheadAttention + LayerNorm with that mask, forward and backward;
  * ctrlsim_train_grad_layout: scope 3 against the parameter table, scopes 0 to 2 unchanged;
  * pack.self_images against pack.pack, image by image, bit for bit;
  * the names HipModel.update accepts under each flag combination (its master selection: no device needed);
  * the AdamW parameter groups with the new names."""
import numpy as np
import pytest
import torch

from ctrlsim_amd import spec, weights, pack
from ctrlsim_amd.models import CtRLSim
import loss_ref
import model_oracle
import head_grad_ref as hgr
import ffn_grad_ref as fgr
import attn_grad_ref as agr
import self_attn_grad_ref as sgr

OP_SHAPES = [(1, 1, 1), (2, 3, 4), (2, 5, 9), (1, 2, 64), (9, 10, 32), (1, 32, 24)]      # tests/test_gpu_self_attn_grads.py: SHAPES


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", OP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_equals_the_oracle_closed_form(shape, mode):
    _, T, A = shape
    m = sgr.mask(T, A, mode)
    want = model_oracle.causal_mask_closed_form(A, T, 3, 0, own_return=bool(mode)).numpy()
    assert m.dtype == bool and m.shape == (3 * T * A, 3 * T * A) and np.array_equal(m, want)
    assert m.diagonal().all() and m[:, 0].all()                   # every row sees itself and token 0
    if A > 1:
        assert np.triu(m, 1).any()                                # later agents' state tokens of the same timestep: not lower-triangular
    if mode == 1:
        assert not (m & ~sgr.mask(T, A, 0)).any()                 # mode 1 only hides


def test_restatement_matches_torch_multihead_attention():
    """B 2, T 2, A 3 (L 18), float64, both modes: output and every gradient equal those of nn.MultiheadAttention(256, 8, batch_first) with
    attn_mask = ~visible + residual + nn.LayerNorm to float64 rounding."""
    rs = np.random.RandomState(0)
    B, T, A = 2, 2, 3
    L = 3 * T * A
    X, dY = rs.standard_normal((B, L, 256)), rs.standard_normal((B, L, 256))
    W = [rs.standard_normal((768, 256)) / 16, 0.1 * rs.standard_normal(768), rs.standard_normal((256, 256)) / 16, 0.1 * rs.standard_normal(256),
         1 + 0.1 * rs.standard_normal(256), 0.1 * rs.standard_normal(256)]
    mha = torch.nn.MultiheadAttention(256, 8, batch_first=True).double()
    ln = torch.nn.LayerNorm(256, eps=1e-5).double()
    params = (mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias, ln.weight, ln.bias)
    with torch.no_grad():
        for p, t in zip(params, W):
            p.copy_(torch.from_numpy(t))
    for mode in (0, 1):
        for p in params:
            p.grad = None
        Xt = torch.tensor(X, requires_grad=True)
        Y = ln(Xt + mha(Xt, Xt, Xt, attn_mask=torch.from_numpy(~sgr.mask(T, A, mode)), need_weights=False)[0])
        Y.backward(torch.from_numpy(dY))
        assert np.abs(sgr.forward(X, T, A, mode, W) - Y.detach().numpy()).max() <= 1e-12
        g, dX = sgr.grads(X, dY, T, A, mode, W)
        for a, b in zip(g + [dX], [p.grad.numpy() for p in params] + [Xt.grad.numpy()]):
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    g0, g1 = sgr.grads(X, dY, T, A, 0, W), sgr.grads(X, dY, T, A, 1, W)
    assert np.abs(g0[1] - g1[1]).max() > 1e-6                     # the modes are different functions at A = 3, T = 2


def test_a_row_with_one_visible_key_has_no_query_gradient():
    """(B, T, A) = (1, 1, 1): row 0 sees one key, its softmax is the constant 1, so nothing reaches its query — in float64 and float32 the
    query rows of d in_proj_weight get nothing from it.  With dY on row 0 only: dWq = 0 and dbq = 0 exactly."""
    d = spec.Dims(spec.make_cfg())
    w = weights.generate_trained_like(d, 0)
    X, dY, W = sgr.make_case(1, 1, 1, 3, [np.asarray(w[k], np.float32) for k in sgr.names(d)])
    dY[0, 1:] = 0.0
    dY[0, 0] = 1e-3 * np.random.RandomState(1).standard_normal(256)
    for dtype in (torch.float64, torch.float32):
        g, dX = sgr.grads(X, dY, 1, 1, 0, W, dtype=dtype)
        assert not g[0][:256].any() and not g[1][:256].any() and g[0][512:].any()
        assert not dX[0, 1:].any() and dX[0, 0].any()             # rows 1 and 2 are invisible to row 0


@pytest.mark.parametrize("case", [0, 3, 7])
def test_training_layout_scope_3_extends_scope_2(case):
    """ctrlsim_train_grad_layout (needs the library, not a device): scopes 0 to 2 as tests/test_attn_grads_host.py has them; scope 3
    appends the last decoder layer's six self-attention tensors, back to back, with the parameter table's shapes."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    model = CtRLSim(cfg, loss_ref.case_weights(case, d), device="cpu")
    assert CtRLSim.SCOPES == ("heads", "heads+ffn", "heads+ffn+cross", "heads+last_layer")
    heads, total = model.head_grad_layout()
    assert model.train_grad_layout("heads") == (heads, total)
    l1, t1 = model.train_grad_layout("heads+ffn")
    assert l1[:len(heads)] == heads and [n for n, _, _ in l1[len(heads):]] == fgr.names(d)
    assert t1 == total + 2 * d.F * d.D + d.F + 3 * d.D
    l2, t2 = model.train_grad_layout("heads+ffn+cross")
    assert l2[:len(l1)] == l1 and [n for n, _, _ in l2[len(l1):]] == agr.names(d) and t2 == t1 + 4 * d.D * d.D + 6 * d.D
    l3, t3 = model.train_grad_layout("heads+last_layer")
    assert l3[:len(l2)] == l2
    table = {n: tuple(s) for n, s, _, _ in weights.param_table(d)}
    tail = l3[len(l2):]
    assert [n for n, _, _ in tail] == sgr.names(d)
    off = t2
    for n, o, s in tail:
        assert o == off and s == table[n]
        off += int(np.prod(s))
    assert t3 == off
    assert [table[n] for n in sgr.names(d)] == list(sgr.SHAPE_OF)
    for bad in ("heads+ffn+cross+self", "heads+self", "last_layer"):
        with pytest.raises(ValueError):
            model.train_grad_layout(bad)
        with pytest.raises(ValueError):
            model.set_trainable(bad)
    assert model.set_trainable("heads+last_layer")._scope == "heads+last_layer"


@pytest.mark.parametrize("case", [0, 7])
def test_self_images_equal_a_fresh_pack(case):
    """pack.self_images on perturbed self-attention weights: every image whose bits depend on them — found by comparing a fresh
    pack.pack of the perturbed state dict with the pack of the original one — is re-derived, bit-equal to its slice of the fresh pack;
    together with the six fp32 rows they are all that differs."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    w0 = dict(loss_ref.case_weights(case, d))
    w = dict(w0)
    pre = sgr.layer_prefix(d)
    rs = np.random.RandomState(8)
    for k in sgr.names(d):
        w[k] = (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32)
    flat0, names0, offsets0 = pack.pack(d, w0)
    flat, names, offsets = pack.pack(d, w)
    assert names == names0 and np.array_equal(offsets, offsets0)              # offsets fixed: a ctrlsim_model stays valid
    off = dict(zip(names, (int(o) for o in offsets)))
    end = dict(zip(names, [int(o) for o in offsets[1:]] + [flat.size]))
    changed = {n for n in names if not np.array_equal(flat[off[n]:end[n]].view(np.int32), flat0[off[n]:end[n]].view(np.int32))}
    layer = {k: w[k] for k in (pre + ".self_attn.in_proj_weight", pre + ".self_attn.out_proj.weight")}
    images = pack.self_images(d, layer, off)
    assert set(images) | set(sgr.names(d)) == changed
    assert {pre + ".self_attn.in_proj_weight#blk#pl1", pre + ".selfq#wop#pl1"} <= set(images) and len(images) == 6
    assert tuple(k[len(pre):] for k in sgr.names(d)) == pack.TRAINABLE_SELF_SUFFIXES
    for n, v in images.items():
        assert v.dtype == np.float32 and v.ndim == 1
        assert np.array_equal(flat[off[n]:off[n] + v.size].view(np.int32), v.view(np.int32)), n
    bad = dict(layer)
    bad[pre + ".self_attn.in_proj_weight"] = np.full_like(layer[pre + ".self_attn.in_proj_weight"], 1.0e6)
    with pytest.raises(FloatingPointError):
        pack.self_images(d, bad, off)


class _NoDevice:
    """HipModel.update's name and shape checks run before anything touches the device: an object with the host masters is enough to see
    which names a flag combination accepts (a refused name raises KeyError, an accepted one with a wrong shape ValueError)."""

    def __init__(self, d, w):
        from ctrlsim_amd.engine import HipModel
        self.update = HipModel.update.__get__(self)
        self.dims = d
        self._ffn_layer = sgr.layer_prefix(d)
        self._heads = {k: np.array(v, np.float32) for k, v in w.items() if k.startswith(pack.HEAD_PREFIXES)}
        for attr, sfx in (("_ffn", pack.TRAINABLE_FFN_SUFFIXES), ("_cross", pack.TRAINABLE_CROSS_SUFFIXES), ("_self", pack.TRAINABLE_SELF_SUFFIXES)):
            setattr(self, attr, {self._ffn_layer + s: np.array(w[self._ffn_layer + s], np.float32) for s in sfx})


def test_names_update_accepts_under_each_flag_combination():
    cfg = loss_ref.case_cfg(0)
    d = spec.Dims(cfg)
    w = loss_ref.case_weights(0, d)
    m = _NoDevice(d, w)
    groups = {"heads": hgr.head_names(w), "ffn": fgr.names(d), "cross": agr.names(d), "self": sgr.names(d),
              "other": [f"decoder.transformer_decoder.layers.{d.ND - 1}.norm9.weight", "encoder.embed_rtg.weight"]}
    if d.ND > 1:
        groups["other"].append("decoder.transformer_decoder.layers.0.self_attn.in_proj_weight")
    for cross in (False, True):
        for self_attn in (False, True):
            ok = {"heads", "ffn"} | ({"cross"} if cross else set()) | ({"self"} if self_attn else set())
            for g, ks in groups.items():
                for k in ks:
                    with pytest.raises(ValueError if g in ok else KeyError):
                        m.update({k: np.zeros((1, 2, 3), np.float32)}, cross=cross, self_attn=self_attn)


def test_param_groups_with_the_self_attention_names():
    d = spec.Dims(loss_ref.case_cfg(0))
    heads = hgr.head_names(weights.generate(d, 0))
    before = heads + fgr.names(d) + agr.names(d)
    decay2, no_decay2 = CtRLSim.param_groups(before)
    decay3, no_decay3 = CtRLSim.param_groups(before + sgr.names(d))
    pre = sgr.layer_prefix(d)
    assert decay3 == sorted(decay2 + [pre + ".self_attn.in_proj_weight", pre + ".self_attn.out_proj.weight"])
    assert no_decay3 == sorted(no_decay2 + [pre + ".self_attn.in_proj_bias", pre + ".self_attn.out_proj.bias", pre + ".norm1.weight",
                                            pre + ".norm1.bias"])
