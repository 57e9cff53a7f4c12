"""CPU tests of the cross-attention gradient path's host side and of its checker:
  * tests/attn_grad_ref.py (float64 autograd restatement of the sublayer) against torch.nn.MultiheadAttention + LayerNorm with a
    key_padding_mask — the reference's own module — forward and backward, and its float32 yardstick on the GPU tests' inputs;
  * ctrlsim_train_grad_layout: scope 2 against the parameter table, scopes 0 and 1 unchanged;
  * pack.cross_images against pack.pack, image by image, bit for bit;
  * the AdamW parameter groups with the new names."""
import numpy as np
import pytest
import torch

from ctrlsim_amd import spec, weights, pack
from ctrlsim_amd.models import CtRLSim
import loss_ref
import head_grad_ref as hgr
import ffn_grad_ref as fgr
import attn_grad_ref as agr


def test_restatement_matches_torch_multihead_attention():
    """B 3, Lq 5, Lk 7, float64, two contexts with padded keys (none of them fully padded: torch's module gives NaN there): output and
    every gradient equal those of nn.MultiheadAttention(256, 8, batch_first) + residual + nn.LayerNorm to float64 rounding."""
    rs = np.random.RandomState(0)
    B, Lq, Lk = 3, 5, 7
    X, Mem, dY = rs.standard_normal((B, Lq, 256)), rs.standard_normal((B, Lk, 256)), rs.standard_normal((B, Lq, 256))
    T = [rs.standard_normal((768, 256)) / 16, 0.1 * rs.standard_normal(768), rs.standard_normal((256, 256)) / 16, 0.1 * rs.standard_normal(256),
         1 + 0.1 * rs.standard_normal(256), 0.1 * rs.standard_normal(256)]
    kp = np.zeros((B, Lk), np.uint8)
    kp[0, 4:] = 1
    kp[2, [0, 3]] = 1
    mha = torch.nn.MultiheadAttention(256, 8, batch_first=True).double()
    ln = torch.nn.LayerNorm(256, eps=1e-5).double()
    with torch.no_grad():
        for p, t in zip((mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias, ln.weight, ln.bias), T):
            p.copy_(torch.from_numpy(t))
    Xt, Mt = torch.tensor(X, requires_grad=True), torch.tensor(Mem, requires_grad=True)
    Y = ln(Xt + mha(Xt, Mt, Mt, key_padding_mask=torch.from_numpy(kp.astype(bool)), need_weights=False)[0])
    Y.backward(torch.from_numpy(dY))
    assert np.abs(agr.forward(X, Mem, kp, T) - Y.detach().numpy()).max() <= 1e-12
    g, dX, dMem = agr.grads(X, Mem, kp, dY, T)
    want = [p.grad.numpy() for p in (mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias, ln.weight, ln.bias)]
    for a, b in zip(g + [dX, dMem], want + [Xt.grad.numpy(), Mt.grad.numpy()]):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert not dMem[kp.astype(bool)].any()                                     # a padded key's memory row feeds nothing
    # a context without keys: O = 0, so Y = LayerNorm(X + bo) and nothing reaches the in_proj or the memory
    kp[1] = 1
    g, dX, dMem = agr.grads(X, Mem, kp, dY, T)
    Y1 = agr.forward(X, Mem, kp, T)[1]
    S = X[1] + T[3]
    mu = S.mean(1, keepdims=True)
    assert np.abs(Y1 - ((S - mu) / np.sqrt(((S - mu) ** 2).mean(1, keepdims=True) + 1e-5) * T[4] + T[5])).max() <= 1e-12
    assert np.isfinite(dX).all() and not dMem[1].any()


@pytest.mark.parametrize("pad", agr.PADS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 33, 31), (2, 130, 65)])
def test_float32_yardstick_is_usable_on_the_op_inputs(shape, pad):
    """The inputs of tests/test_gpu_attn_grads.py: the float32 autograd's own error is finite for every tensor, and a tensor is
    identically zero in float64 only where that is documented — the in_proj gradients, the out-projection weight's (O = 0) and dMem of a
    batch whose every key is padded (B = 1, pattern "context") — and then in float32 too."""
    d = spec.Dims(spec.make_cfg())
    w = weights.generate_trained_like(d, 0)
    X, Mem, dY, T = agr.make_case(*shape, 11 + shape[1] % 13, [np.asarray(w[k], np.float32) for k in agr.names(d)])
    kp = agr.make_pad(shape[0], shape[2], pad, np.random.RandomState(shape[2]))
    r64, r32 = agr.grads(X, Mem, kp, dY, T), agr.grads(X, Mem, kp, dY, T, dtype=torch.float32)
    all_padded = kp is not None and kp.all()
    for i, (a, b) in enumerate(zip(list(r64[0]) + [r64[1], r64[2]], list(r32[0]) + [r32[1], r32[2]])):
        if not a.any():
            assert all_padded and i in (0, 1, 2, 7) and not b.any(), (i, pad)
            continue
        assert np.isfinite(hgr.errors(b, a)).all() and np.isfinite(b).all()
    if kp is not None:
        assert not r64[2][kp.astype(bool)].any() and not r32[2][kp.astype(bool)].any()


@pytest.mark.parametrize("case", [0, 4, 7])
def test_training_layout_scope_2_extends_scope_1(case):
    """ctrlsim_train_grad_layout (needs the library, not a device): scopes 0 and 1 as tests/test_ffn_grads_host.py has them; scope 2
    appends the last decoder layer's six cross-attention tensors, back to back, with the parameter table's shapes."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    model = CtRLSim(cfg, loss_ref.case_weights(case, d), device="cpu")
    heads, total = model.head_grad_layout()
    assert model.train_grad_layout("heads") == (heads, total)
    l1, t1 = model.train_grad_layout("heads+ffn")
    assert l1[:len(heads)] == heads and [n for n, _, _ in l1[len(heads):]] == fgr.names(d)
    assert t1 == total + 2 * d.F * d.D + d.F + 3 * d.D
    l2, t2 = model.train_grad_layout("heads+ffn+cross")
    assert l2[:len(l1)] == l1
    table = {n: tuple(s) for n, s, _, _ in weights.param_table(d)}
    tail = l2[len(l1):]
    assert [n for n, _, _ in tail] == agr.names(d)
    off = t1
    for n, o, s in tail:
        assert o == off and s == table[n]
        off += int(np.prod(s))
    assert t2 == off
    assert [table[n] for n in agr.names(d)] == [(3 * d.D, d.D), (3 * d.D,), (d.D, d.D), (d.D,), (d.D,), (d.D,)]
    with pytest.raises(ValueError):
        model.train_grad_layout("heads+ffn+cross+self")


@pytest.mark.parametrize("case", [0, 7])
def test_cross_images_equal_a_fresh_pack(case):
    """pack.cross_images on perturbed cross-attention weights: every image whose bits depend on them — found by comparing a fresh
    pack.pack of the perturbed state dict with the pack of the original one — is re-derived, bit-equal to its slice of the fresh pack;
    together with the six fp32 rows they are all that differs."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    w0 = dict(loss_ref.case_weights(case, d))
    w = dict(w0)
    pre = agr.layer_prefix(d)
    rs = np.random.RandomState(6)
    for k in agr.names(d):
        w[k] = (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32)
    flat0, names0, offsets0 = pack.pack(d, w0)
    flat, names, offsets = pack.pack(d, w)
    assert names == names0 and np.array_equal(offsets, offsets0)              # offsets fixed: a ctrlsim_model stays valid
    off = dict(zip(names, (int(o) for o in offsets)))
    end = dict(zip(names, [int(o) for o in offsets[1:]] + [flat.size]))
    changed = {n for n in names if not np.array_equal(flat[off[n]:end[n]].view(np.int32), flat0[off[n]:end[n]].view(np.int32))}
    layer = {k: w[k] for k in (pre + ".multihead_attn.in_proj_weight", pre + ".multihead_attn.out_proj.weight")}
    images = pack.cross_images(d, layer, off)
    assert set(images) | set(agr.names(d)) == changed
    assert {pre + ".multihead_attn.in_proj_weight#blk#pl1", pre + ".selfq#wqp#pl1", pre + ".ffn#wop#pl1"} <= set(images) and len(images) == 7
    for n, v in images.items():
        assert v.dtype == np.float32 and v.ndim == 1
        assert np.array_equal(flat[off[n]:off[n] + v.size].view(np.int32), v.view(np.int32)), n
    bad = dict(layer)
    bad[pre + ".multihead_attn.out_proj.weight"] = np.full_like(layer[pre + ".multihead_attn.out_proj.weight"], 1.0e6)
    with pytest.raises(FloatingPointError):
        pack.cross_images(d, bad, off)


def test_param_groups_with_the_cross_attention_names():
    d = spec.Dims(loss_ref.case_cfg(0))
    heads = hgr.head_names(weights.generate(d, 0))
    decay1, no_decay1 = CtRLSim.param_groups(heads + fgr.names(d))
    decay2, no_decay2 = CtRLSim.param_groups(heads + fgr.names(d) + agr.names(d))
    pre = agr.layer_prefix(d)
    assert decay2 == sorted(decay1 + [pre + ".multihead_attn.in_proj_weight", pre + ".multihead_attn.out_proj.weight"])
    assert no_decay2 == sorted(no_decay1 + [pre + ".multihead_attn.in_proj_bias", pre + ".multihead_attn.out_proj.bias",
                                            pre + ".norm2.weight", pre + ".norm2.bias"])
