"""CPU tests of the all-decoder-layers gradient path's host side and of its checker:
  * tests/layer_grad_ref.py: the composed layer against torch.nn.TransformerDecoderLayer in float64, outputs and gradients, and the
    stack against the layer applied twice;
  * ctrlsim_train_grad_layout at scope 4 through CtRLSim.train_grad_layout("heads+decoder"): the scope-3 layout as a prefix, then the earlier
    layers in descending order with the parameter table's names and shapes; SCOPES and the refused names unchanged;
  * pack.ffn_images / cross_images / self_images applied to EVERY decoder layer against a fresh pack.pack, bit for bit;
  * the names HipModel.update accepts with and without decoder=True;
  * the C symbols: declared, bound and exported, with the declared argument counts; the six entries folded into the scope-indexed ones
    absent from the header, the binding and the library;
  * the AdamW parameter groups with every layer's names."""
import os
import re

import numpy as np
import pytest
import torch

from ctrlsim_amd import spec, weights, pack
from ctrlsim_amd.models import CtRLSim
import loss_ref
import head_grad_ref as hgr
import ffn_grad_ref as fgr
import attn_grad_ref as agr
import self_attn_grad_ref as sgr
import layer_grad_ref as lgr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_layer(rs, F):
    att = lambda: [rs.standard_normal((768, 256)) / 16, 0.1 * rs.standard_normal(768), rs.standard_normal((256, 256)) / 16,
                   0.1 * rs.standard_normal(256), 1 + 0.1 * rs.standard_normal(256), 0.1 * rs.standard_normal(256)]
    ffn = [rs.standard_normal((F, 256)) / 16, 0.1 * rs.standard_normal(F), rs.standard_normal((256, F)) / 8, 0.1 * rs.standard_normal(256),
           1 + 0.1 * rs.standard_normal(256), 0.1 * rs.standard_normal(256)]
    return ffn + att() + att()


def test_composed_layer_matches_torch_transformer_decoder_layer():
    """B 2, T 2, A 3 (L 18), Lk 7 with a padded tail, F 40, float64, both mask modes: the output and every gradient (18 tensors, dX0,
    dMem) equal those of nn.TransformerDecoderLayer(256, 8, F, dropout 0, relu, batch_first, post-LN) in eval mode with tgt_mask =
    ~visible and memory_key_padding_mask = key_pad, to float64 rounding."""
    rs = np.random.RandomState(0)
    B, T, A, Lk, F = 2, 2, 3, 7, 40
    L = 3 * T * A
    X0, Mem, dY = rs.standard_normal((B, L, 256)), rs.standard_normal((B, Lk, 256)), rs.standard_normal((B, L, 256))
    W = _random_layer(rs, F)
    pad = agr.make_pad(B, Lk, "tail", rs)
    ref = torch.nn.TransformerDecoderLayer(256, 8, F, dropout=0.0, activation="relu", batch_first=True, norm_first=False).double().eval()
    params = dict(ref.named_parameters())
    order = [params[p[1:]] for p in lgr.PARTS]
    with torch.no_grad():
        for p, t in zip(order, W):
            p.copy_(torch.from_numpy(t))
    for mode in (0, 1):
        for p in order:
            p.grad = None
        Xt, Mt = torch.tensor(X0, requires_grad=True), torch.tensor(Mem, requires_grad=True)
        Y = ref(Xt, Mt, tgt_mask=torch.from_numpy(~sgr.mask(T, A, mode)), memory_key_padding_mask=torch.from_numpy(pad.astype(bool)))
        Y.backward(torch.from_numpy(dY))
        g, dX0, dMem, X1, U = lgr.grads(X0, Mem, pad, dY, T, A, mode, W)
        with torch.no_grad():
            mine = lgr.layer(torch.tensor(X0), torch.tensor(Mem), torch.from_numpy(pad.astype(bool)), torch.from_numpy(sgr.mask(T, A, mode)),
                             [torch.tensor(t) for t in W])[0].numpy()
        assert np.abs(mine - Y.detach().numpy()).max() <= 1e-12
        for a, b in zip(g + [dX0, dMem], [p.grad.numpy() for p in order] + [Xt.grad.numpy(), Mt.grad.numpy()]):
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
        assert not dMem[pad.astype(bool)].any()
        assert np.abs(X1 - sgr.forward(X0, T, A, mode, W[12:18])).max() <= 1e-12
        assert np.abs(U - agr.forward(X1, Mem, pad, W[6:12])).max() <= 1e-12
        on = (U.reshape(-1, 256) @ W[0].T + W[1]) > 0                      # the ReLU as its own on / off pattern: the same function
        g2 = lgr.grads(X0, Mem, pad, dY, T, A, mode, W, relu_on=on)
        assert all(np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()) for a, b in zip(g2[0] + [g2[1], g2[2]], g + [dX0, dMem]))


def test_stack_is_the_layer_applied_in_turn():
    """Two layers: the stack's gradients equal the layer reference chained by hand (layer 1 from dY, layer 0 from layer 1's dX0), and
    its dMem is the sum of the two layers' contributions."""
    rs = np.random.RandomState(1)
    B, T, A, Lk, F = 1, 2, 2, 5, 24
    L = 3 * T * A
    X0, Mem, dY = rs.standard_normal((B, L, 256)), rs.standard_normal((B, Lk, 256)), rs.standard_normal((B, L, 256))
    layers = [_random_layer(rs, F), _random_layer(rs, F)]
    g, dX, dMem = lgr.stack_grads(X0, Mem, None, dY, T, A, 0, layers)
    with torch.no_grad():
        Y0 = lgr.layer(torch.tensor(X0), torch.tensor(Mem), None, torch.from_numpy(sgr.mask(T, A, 0)), [torch.tensor(t) for t in layers[0]])[0]
    g1, d1, m1, _, _ = lgr.grads(Y0.numpy(), Mem, None, dY, T, A, 0, layers[1])
    g0, d0, m0, _, _ = lgr.grads(X0, Mem, None, d1, T, A, 0, layers[0])
    close = lambda a, b: np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max())
    assert all(close(a, b) for a, b in zip(g[1], g1)) and all(close(a, b) for a, b in zip(g[0], g0))
    assert close(dX[1], d1) and close(dX[0], d0) and close(dMem, m0 + m1)


@pytest.mark.parametrize("case", [0, 3, 7])
def test_decoder_layout_extends_the_last_layer_scope(case):
    """train_grad_layout("heads+decoder") (ctrlsim_train_grad_layout, scope 4; needs the library, not a device): "heads+last_layer" as a prefix,
    then for l = ND-2 .. 0 the 18 tensors of layer l, back to back, with the parameter table's shapes; the total is the sum."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    model = CtRLSim(cfg, loss_ref.case_weights(case, d), device="cpu")
    assert CtRLSim.SCOPES == ("heads", "heads+ffn", "heads+ffn+cross", "heads+last_layer") and CtRLSim.DECODER_SCOPE == "heads+decoder"
    l3, t3 = model.train_grad_layout("heads+last_layer")
    ld, td = model.train_grad_layout("heads+decoder")
    assert ld[:len(l3)] == l3 and len(ld) == len(l3) + 18 * (d.ND - 1)
    table = {n: tuple(s) for n, s, _, _ in weights.param_table(d)}
    want = [n for l in range(d.ND - 2, -1, -1) for n in lgr.names(l)]
    assert [n for n, _, _ in ld[len(l3):]] == want
    off = t3
    for n, o, s in ld[len(l3):]:
        assert o == off and s == table[n]
        off += int(np.prod(s))
    per_layer = 2 * d.F * d.D + d.F + 3 * d.D + 2 * (4 * d.D * d.D + 6 * d.D)
    assert td == off == t3 + (d.ND - 1) * per_layer
    assert [n for n, _, _ in l3[-18:]] == lgr.names(d.ND - 1)              # the last layer's 18: the same group order
    for bad in ("heads+ffn+cross+self", "heads+self", "last_layer"):
        with pytest.raises(ValueError):
            model.train_grad_layout(bad)
        with pytest.raises(ValueError):
            model.set_trainable(bad)
    assert model.set_trainable("heads+decoder")._scope == "heads+decoder"
    assert model.train_grad_layout() == (ld, td)


def test_decoder_layout_refuses_what_it_cannot_lay_out():
    import ctypes as C
    from ctrlsim_amd import _lib
    from ctrlsim_amd.engine import _dims_struct
    lib = _lib.lib()
    d = spec.Dims(loss_ref.case_cfg(0))
    cd = _dims_struct(d)
    n = lib.ctrlsim_train_grad_layout(C.byref(cd), 1, 4, 0, None, None)
    assert n > 0 and lib.ctrlsim_train_grad_layout(None, 1, 4, 0, None, None) == -22
    names, offs = (C.c_char_p * n)(), (C.c_int64 * (n + 1))()
    assert lib.ctrlsim_train_grad_layout(C.byref(cd), 1, 4, n - 1, names, offs) == -22         # too small a capacity
    assert lib.ctrlsim_train_grad_layout(C.byref(cd), 1, 4, n, names, offs) == n
    cd.ND = 9                                                              # more than CTRLSIM_MAX_DECODER_LAYERS
    assert lib.ctrlsim_train_grad_layout(C.byref(cd), 1, 4, 0, None, None) == -22
    assert lib.ctrlsim_train_grads_workspace_bytes(C.byref(cd), 1, 1, 4) == -22
    assert lib.ctrlsim_train_grads_workspace_bytes(None, 1, 1, 4) == -22
    assert lib.ctrlsim_forward_loss_grads(None, 1, 1, None, None, None, 1.0, 4, None, None, None, None, None, None) == -22
    for scope in (6, -1):                                                  # the scope-indexed entry ends at 5
        assert lib.ctrlsim_train_grad_layout(C.byref(_dims_struct(d)), 1, scope, 0, None, None) == -22
        assert lib.ctrlsim_train_grads_workspace_bytes(C.byref(_dims_struct(d)), 1, 1, scope) == -22


def _nd2_cfg():
    """A tiny configuration with two decoder layers (the tiny fixture cases have one)."""
    cfg = loss_ref.case_cfg(0)
    cfg.model.num_decoder_layers = 2
    return cfg


@pytest.mark.parametrize("case", ["nd2", 7])
def test_per_layer_images_equal_a_fresh_pack(case):
    """pack.ffn_images, cross_images and self_images on the perturbed 18 tensors of EVERY decoder layer, one layer at a time: every
    image whose bits depend on that layer's tensors — found by comparing a fresh pack.pack of the perturbed state dict with the pack
    of the original — is re-derived, bit-equal to its slice of the fresh pack; with the 18 fp32 rows they are all that differs."""
    cfg = _nd2_cfg() if case == "nd2" else loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    assert d.ND >= 2
    w0 = dict(weights.generate(d, 3) if case == "nd2" else loss_ref.case_weights(case, d))
    flat0, names0, offsets0 = pack.pack(d, w0)
    rs = np.random.RandomState(8)
    for l in range(d.ND):
        w = dict(w0)
        for k in lgr.names(l):
            w[k] = (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32)
        flat, names, offsets = pack.pack(d, w)
        assert names == names0 and np.array_equal(offsets, offsets0)          # offsets fixed: a ctrlsim_model stays valid
        off = dict(zip(names, (int(o) for o in offsets)))
        end = dict(zip(names, [int(o) for o in offsets[1:]] + [flat.size]))
        changed = {n for n in names if not np.array_equal(flat[off[n]:end[n]].view(np.int32), flat0[off[n]:end[n]].view(np.int32))}
        layer = {k: w[k] for k in lgr.names(l) if k.endswith("weight") and ".norm" not in k}
        images = {}
        for fn in (pack.ffn_images, pack.cross_images, pack.self_images):
            images.update(fn(d, layer, off))
        assert set(images) | set(lgr.names(l)) == changed, l
        pre = f"decoder.transformer_decoder.layers.{l}"
        assert all(n.startswith(pre + ".") for n in images) and len(images) >= 12
        for n, v in images.items():
            assert v.dtype == np.float32 and v.ndim == 1
            assert np.array_equal(flat[off[n]:off[n] + v.size].view(np.int32), v.view(np.int32)), n


class _NoDevice:
    """HipModel.update's name and shape checks run before anything touches the device (tests/test_self_attn_grads_host.py)."""

    def __init__(self, d, w):
        from ctrlsim_amd.engine import HipModel
        self.update = HipModel.update.__get__(self)
        self.dims = d
        self._ffn_layer = f"decoder.transformer_decoder.layers.{d.ND - 1}"
        self._heads = {k: np.array(v, np.float32) for k, v in w.items() if k.startswith(pack.HEAD_PREFIXES)}
        for attr, sfx in (("_ffn", pack.TRAINABLE_FFN_SUFFIXES), ("_cross", pack.TRAINABLE_CROSS_SUFFIXES), ("_self", pack.TRAINABLE_SELF_SUFFIXES)):
            setattr(self, attr, {self._ffn_layer + s: np.array(w[self._ffn_layer + s], np.float32) for s in sfx})
        self._early = {k: np.array(w[k], np.float32) for l in range(d.ND - 1) for k in lgr.names(l)}


def test_names_update_accepts_with_and_without_the_decoder_flag():
    cfg = _nd2_cfg()
    d = spec.Dims(cfg)
    w = weights.generate(d, 3)
    m = _NoDevice(d, w)
    early, last = lgr.names(0), lgr.names(1)
    other = ["decoder.transformer_decoder.layers.0.norm9.weight", "encoder.embed_rtg.weight",
             "encoder.transformer_encoder.layers.0.linear1.weight"]
    bad = np.zeros((1, 2, 3), np.float32)
    for k in hgr.head_names(w) + early + last:
        with pytest.raises(ValueError):
            m.update({k: bad}, decoder=True)
    for k in other:
        with pytest.raises(KeyError):
            m.update({k: bad}, decoder=True)
    for flags in ({}, {"cross": True}, {"self_attn": True}, {"cross": True, "self_attn": True}):
        for k in early + other:                                            # without the flag every earlier-layer name stays refused
            with pytest.raises(KeyError):
                m.update({k: bad}, **flags)


def test_new_symbols_are_declared_bound_and_exported_with_the_declared_argument_counts():
    from ctrlsim_amd import _lib
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "ctrlsim.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for sym, nargs in (("ctrlsim_decoder_layer_grad_workspace_bytes", 5), ("ctrlsim_decoder_layer_grad", 24),
                       ("ctrlsim_train_grad_layout", 6), ("ctrlsim_train_grads_workspace_bytes", 4), ("ctrlsim_forward_loss_grads", 14)):
        m = re.search(r"\b" + sym + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[sym][1]), sym
        assert hasattr(lib, sym)
    for sym in ("ctrlsim_decoder_grad_layout", "ctrlsim_decoder_grads_workspace_bytes", "ctrlsim_forward_loss_grads_decoder",
                "ctrlsim_encoder_grad_layout", "ctrlsim_encoder_grads_workspace_bytes", "ctrlsim_forward_loss_grads_encoder"):
        assert not re.search(r"\b" + sym + r"\b", hdr) and sym not in _lib.SIGNATURES and not hasattr(lib, sym), sym      # (dlsym finds none)
    assert "#define CTRLSIM_MAX_DECODER_LAYERS 8" in hdr and "#define CTRLSIM_TRAIN_SCOPES 6" in hdr
    import ctypes as C
    assert C.sizeof(_lib.TrainTaps) == (8 + 4 * 8) * C.sizeof(C.c_void_p)
    assert _lib.TrainTaps.dX0.offset == 8 * C.sizeof(C.c_void_p) and not hasattr(_lib, "DecoderTaps") and not hasattr(_lib, "EncoderTaps")
    assert lib.ctrlsim_decoder_layer_grad_workspace_bytes(1, 1, 1, 1, 0) == -22 and lib.ctrlsim_decoder_layer_grad_workspace_bytes(2, 3, 4, 7, 64) > 0
    # the workspace holds the four row buffers and the widest of the three ops' carves
    B, T, A, Lk, F = 9, 10, 32, 12, 1024
    rows = B * 3 * T * A
    ops = max(lib.ctrlsim_ffn_block_grad_workspace_bytes(rows, F), lib.ctrlsim_attn_block_grad_workspace_bytes(B, 3 * T * A, Lk),
              lib.ctrlsim_self_attn_block_grad_workspace_bytes(B, T, A))
    assert lib.ctrlsim_decoder_layer_grad_workspace_bytes(B, T, A, Lk, F) == 4 * rows * 1024 + ops


def test_param_groups_with_every_layer():
    d = spec.Dims(_nd2_cfg())
    names = hgr.head_names(weights.generate(d, 3)) + lgr.names(1) + lgr.names(0)
    decay, no_decay = CtRLSim.param_groups(names)
    assert sorted(decay + no_decay) == sorted(names) and not set(decay) & set(no_decay)
    for l in (0, 1):
        pre = f"decoder.transformer_decoder.layers.{l}"
        assert {pre + s for s in (".linear1.weight", ".linear2.weight", ".multihead_attn.in_proj_weight", ".multihead_attn.out_proj.weight",
                                  ".self_attn.in_proj_weight", ".self_attn.out_proj.weight")} <= set(decay)
        assert {k for k in lgr.names(l) if k.endswith("bias") or ".norm" in k} <= set(no_decay)
        assert len([k for k in decay if k.startswith(pre + ".")]) == 6 and len([k for k in no_decay if k.startswith(pre + ".")]) == 12
