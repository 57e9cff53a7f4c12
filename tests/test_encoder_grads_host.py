"""CPU tests of the scene-encoder gradient path's host side and of its checker:
  * tests/enc_layer_grad_ref.py: the composed layer against torch.nn.TransformerEncoderLayer (batch_first, src_key_padding_mask) in
    float64 on the non-padded rows, outputs and gradients, and the stack against the layer applied in turn;
  * ctrlsim_train_grad_layout at scope 5 through CtRLSim.train_grad_layout("heads+decoder+encoder"): the decoder layout as a prefix, then the
    encoder layers in descending order with the parameter table's names and shapes; SCOPES unchanged; refusals;
  * pack.encoder_images applied to EVERY encoder layer against a fresh pack.pack, bit for bit (both splits' images are in one pack);
  * the names HipModel.update accepts with and without encoder=True;
  * the C symbols: declared, bound and exported, with the declared argument counts; the six folded entries absent;
  * the AdamW parameter groups over the encoder names;
  * fixture self-consistency: the float64 twin of the encoder stack, run on the encoder input rows and the output gradient the tiny
    cases record, against every recorded gradient; and the fixture's structure in every case (each tensor of each layer, the rows of
    dE0 recorded as exactly zero where the case inputs pad a key)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from ctrlsim_amd import spec, weights, pack, _lib
from ctrlsim_amd.engine import _dims_struct
from ctrlsim_amd.models import CtRLSim
import loss_ref
import head_grad_ref as hgr
import attn_grad_ref as agr
import layer_grad_ref as lgr
import enc_layer_grad_ref as egr
from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENC = "heads+decoder+encoder"


def _random_layer(rs, F):
    att = [rs.standard_normal((768, 256)) / 16, 0.1 * rs.standard_normal(768), rs.standard_normal((256, 256)) / 16,
           0.1 * rs.standard_normal(256), 1 + 0.1 * rs.standard_normal(256), 0.1 * rs.standard_normal(256)]
    ffn = [rs.standard_normal((F, 256)) / 16, 0.1 * rs.standard_normal(F), rs.standard_normal((256, F)) / 8, 0.1 * rs.standard_normal(256),
           1 + 0.1 * rs.standard_normal(256), 0.1 * rs.standard_normal(256)]
    return ffn + att


@pytest.mark.parametrize("kind", ["none", "tail", "scattered"])
def test_composed_layer_matches_torch_transformer_encoder_layer(kind):
    """B 2, L 7, F 40, float64: the output on the non-padded rows and every gradient (12 tensors, dX0) equal those of
    nn.TransformerEncoderLayer(256, 8, F, dropout 0, relu, batch_first, post-LN) with src_key_padding_mask = key_pad, to float64
    rounding.  dY is zero on the padded rows (torch's layer may compute those rows differently: they are nobody's keys); the twin's dX0
    on them is then exactly zero."""
    rs = np.random.RandomState(0)
    B, L, F = 2, 7, 40
    X0, dY = rs.standard_normal((B, L, 256)), rs.standard_normal((B, L, 256))
    W = _random_layer(rs, F)
    pad = agr.make_pad(B, L, kind, rs)
    keep = np.ones((B, L), bool) if pad is None else ~pad.astype(bool)
    dY[~keep] = 0.0
    ref = torch.nn.TransformerEncoderLayer(256, 8, F, dropout=0.0, activation="relu", batch_first=True, norm_first=False).double()
    params = dict(ref.named_parameters())
    order = [params[p[1:]] for p in egr.PARTS]
    with torch.no_grad():
        for p, t in zip(order, W):
            p.copy_(torch.from_numpy(t))
    Xt = torch.tensor(X0, requires_grad=True)
    Y = ref(Xt, src_key_padding_mask=None if pad is None else torch.from_numpy(pad.astype(bool)))
    Y.backward(torch.from_numpy(dY))
    g, dX0, U = egr.grads(X0, pad, dY, W)
    with torch.no_grad():
        mine = egr.layer(torch.tensor(X0), None if pad is None else torch.from_numpy(pad.astype(bool)), [torch.tensor(t) for t in W])[0].numpy()
    assert np.abs(mine - Y.detach().numpy())[keep].max() <= 1e-12
    for a, b in zip(g + [dX0], [p.grad.numpy() for p in order] + [Xt.grad.numpy()]):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert not dX0[~keep].any()
    assert np.abs(U - agr.forward(X0, X0, pad, W[6:12])).max() <= 1e-12
    ga, dXa = egr.attn_grads(X0, pad, dY, W[6:12])                         # the sublayer alone = the cross reference with Mem = X, dX + dMem
    gc, dXc, dMc = agr.grads(X0, X0, pad, dY, W[6:12])
    assert all(np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()) for a, b in zip(ga + [dXa], gc + [dXc + dMc]))
    on = (U.reshape(-1, 256) @ W[0].T + W[1]) > 0                          # the ReLU as its own on / off pattern: the same function
    g2 = egr.grads(X0, pad, dY, W, relu_on=on)
    assert all(np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()) for a, b in zip(g2[0] + [g2[1]], g + [dX0]))


def test_stack_is_the_layer_applied_in_turn():
    rs = np.random.RandomState(1)
    B, L, F = 2, 5, 24
    X0, dY = rs.standard_normal((B, L, 256)), rs.standard_normal((B, L, 256))
    pad = agr.make_pad(B, L, "tail", rs)
    layers = [_random_layer(rs, F), _random_layer(rs, F)]
    g, dE = egr.stack_grads(X0, pad, dY, layers)
    with torch.no_grad():
        Y0 = egr.layer(torch.tensor(X0), torch.from_numpy(pad.astype(bool)), [torch.tensor(t) for t in layers[0]])[0]
    g1, d1, _ = egr.grads(Y0.numpy(), pad, dY, layers[1])
    g0, d0, _ = egr.grads(X0, pad, d1, layers[0])
    close = lambda a, b: np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max())
    assert all(close(a, b) for a, b in zip(g[1], g1)) and all(close(a, b) for a, b in zip(g[0], g0))
    assert close(dE[1], d1) and close(dE[0], d0)


@pytest.mark.parametrize("case", [0, 3, 7])
def test_encoder_layout_extends_the_decoder_scope(case):
    """train_grad_layout("heads+decoder+encoder") (ctrlsim_train_grad_layout, scope 5; needs the library, not a device): "heads+decoder" as a
    prefix, then for l = NE-1 .. 0 the 12 tensors of encoder layer l, back to back, with the parameter table's shapes."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    model = CtRLSim(cfg, loss_ref.case_weights(case, d), device="cpu")
    assert CtRLSim.SCOPES == ("heads", "heads+ffn", "heads+ffn+cross", "heads+last_layer") and CtRLSim.DECODER_SCOPE == "heads+decoder"
    assert CtRLSim.ENCODER_SCOPE == ENC and ENC not in CtRLSim.SCOPES
    ld, td = model.train_grad_layout("heads+decoder")
    le, te = model.train_grad_layout(ENC)
    assert d.NE >= 1 and le[:len(ld)] == ld and len(le) == len(ld) + 12 * d.NE
    table = {n: tuple(s) for n, s, _, _ in weights.param_table(d)}
    assert [n for n, _, _ in le[len(ld):]] == [n for l in range(d.NE - 1, -1, -1) for n in egr.names(l)]
    off = td
    for n, o, s in le[len(ld):]:
        assert o == off and s == table[n]
        off += int(np.prod(s))
    assert te == off == td + d.NE * (2 * d.F * d.D + d.F + 3 * d.D + 4 * d.D * d.D + 6 * d.D)
    for bad in ("heads+encoder", "encoder", "heads+decoder+encoder+map"):
        with pytest.raises(ValueError):
            model.train_grad_layout(bad)
        with pytest.raises(ValueError):
            model.set_trainable(bad)
    assert model.set_trainable(ENC)._scope == ENC
    assert model.train_grad_layout() == (le, te)
    with pytest.raises(ValueError):                                        # the encoder taps exist in the encoder scope only
        model.loss_and_train_grads_ctx(None, None, 1, dE0=True, scope="heads+decoder")
    with pytest.raises(ValueError):
        model.loss_and_train_grads_ctx(None, None, 1, dU=True, scope=ENC)


def test_encoder_layout_refuses_what_it_cannot_lay_out():
    lib = _lib.lib()
    d = spec.Dims(loss_ref.case_cfg(0))
    cd = _dims_struct(d)
    layout = lambda dims, scope, cap=0, names=None, offs=None: lib.ctrlsim_train_grad_layout(dims, 1, scope, cap, names, offs)
    ws = lib.ctrlsim_train_grads_workspace_bytes
    n = layout(C.byref(cd), 5)
    nd = layout(C.byref(cd), 4)
    assert n == nd + 12 * d.NE and layout(None, 5) == -22
    names, offs = (C.c_char_p * n)(), (C.c_int64 * (n + 1))()
    assert layout(C.byref(cd), 5, n - 1, names, offs) == -22               # too small a capacity
    assert layout(C.byref(cd), 5, n, names, offs) == n
    assert ws(C.byref(cd), 2, d.T, 5) > ws(C.byref(cd), 2, d.T, 4)
    cd.NE = 9                                                              # more than CTRLSIM_MAX_ENCODER_LAYERS
    assert layout(C.byref(cd), 5) == -22
    assert ws(C.byref(cd), 1, 1, 5) == -22
    cd.NE = 0                                                              # no encoder layer: the decoder scope's answers
    assert layout(C.byref(cd), 5) == nd
    assert ws(C.byref(cd), 2, d.T, 5) == ws(C.byref(cd), 2, d.T, 4)
    cd = _dims_struct(d)
    cd.ND = 9                                                              # what the decoder scope refuses
    assert layout(C.byref(cd), 5) == -22
    assert ws(C.byref(cd), 1, 1, 5) == -22
    assert ws(None, 1, 1, 5) == -22
    assert lib.ctrlsim_forward_loss_grads(None, 1, 1, None, None, None, 1.0, 5, None, None, None, None, None, None) == -22
    for scope in (6, -1):
        assert layout(C.byref(_dims_struct(d)), scope) == -22 and ws(C.byref(_dims_struct(d)), 1, 1, scope) == -22


def test_op_workspace_and_chunk_queries():
    lib = _lib.lib()
    for bad in ((0, 4), (4, 0), (-1, 4)):
        assert lib.ctrlsim_scene_attn_block_grad_workspace_bytes(*bad) == -22 and lib.ctrlsim_scene_attn_block_grad_chunk_contexts(*bad) == -22
        assert lib.ctrlsim_encoder_layer_grad_workspace_bytes(*bad, 8) == -22
    assert lib.ctrlsim_encoder_layer_grad_workspace_bytes(2, 7, 0) == -22
    assert 2796203 * 768 >= 2 ** 31 > 2796202 * 768                        # B * L * 768 against 2^31
    assert lib.ctrlsim_scene_attn_block_grad_workspace_bytes(2796203, 1) == -22 and lib.ctrlsim_scene_attn_block_grad_workspace_bytes(2796202, 1) > 0
    assert lib.ctrlsim_scene_attn_block_grad_workspace_bytes(1, 2796203) == -22
    assert lib.ctrlsim_encoder_layer_grad_workspace_bytes(2796203, 1, 8) == -22
    assert lib.ctrlsim_scene_attn_block_grad_chunk_contexts(37, 224) == 36 and lib.ctrlsim_scene_attn_block_grad_chunk_contexts(3, 64) == 3
    assert lib.ctrlsim_scene_attn_block_grad_chunk_contexts(2, 9000) == 1  # a context of more than 8192 rows: one per chunk
    # one source: no [B L, 512] K | V buffers of all contexts — with many contexts the op needs less than the cross op called with Mem = X
    assert lib.ctrlsim_scene_attn_block_grad_workspace_bytes(370, 224) < lib.ctrlsim_attn_block_grad_workspace_bytes(370, 224, 224)
    # the layer op holds U, dU and the wider of the two ops' carves
    B, L, F = 37, 224, 1024
    ops = max(lib.ctrlsim_ffn_block_grad_workspace_bytes(B * L, F), lib.ctrlsim_scene_attn_block_grad_workspace_bytes(B, L))
    assert lib.ctrlsim_encoder_layer_grad_workspace_bytes(B, L, F) == 2 * B * L * 1024 + ops


@pytest.mark.parametrize("case", [0, 7])
def test_encoder_images_equal_a_fresh_pack(case):
    """pack.encoder_images on the perturbed 12 tensors of EVERY encoder layer, one layer at a time: every image whose bits depend on
    that layer's tensors — found by comparing a fresh pack.pack of the perturbed state dict with the pack of the original — is
    re-derived, bit-equal to its slice of the fresh pack (a pack holds the images of both operand splits); with the 12 fp32 rows they
    are all that differs."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    w0 = dict(loss_ref.case_weights(case, d))
    flat0, names0, offsets0 = pack.pack(d, w0)
    rs = np.random.RandomState(8)
    assert pack.TRAINABLE_ENCODER_SUFFIXES == egr.PARTS
    for l in range(d.NE):
        w = dict(w0)
        for k in egr.names(l):
            w[k] = (np.asarray(w[k]) * (1 + 0.05 * rs.standard_normal(np.asarray(w[k]).shape))).astype(np.float32)
        flat, names, offsets = pack.pack(d, w)
        assert names == names0 and np.array_equal(offsets, offsets0)          # offsets fixed: a ctrlsim_model stays valid
        off = dict(zip(names, (int(o) for o in offsets)))
        end = dict(zip(names, [int(o) for o in offsets[1:]] + [flat.size]))
        changed = {n for n in names if not np.array_equal(flat[off[n]:end[n]].view(np.int32), flat0[off[n]:end[n]].view(np.int32))}
        layer = {k: w[k] for k in egr.names(l) if k.endswith("weight") and ".norm" not in k}
        images = pack.encoder_images(d, layer, off)
        assert set(images) | set(egr.names(l)) == changed, l
        pre = f"encoder.transformer_encoder.layers.{l}"
        assert all(n.startswith(pre + ".") for n in images)
        for sfx in ("#pl0", "#pl1"):                                       # the planes of both splits of the four matrices, and both w1p / w2p
            assert {pre + m + sfx for m in (".self_attn.in_proj_weight", ".self_attn.out_proj.weight", ".linear1.weight", ".linear2.weight",
                                            ".ffn#w1p", ".ffn#w2p")} <= set(images)
        assert {pre + ".self_attn.in_proj_weight#blk#pl1", pre + ".ffn#wop#pl1", pre + ".ffn#w1q#pl1"} <= set(images)
        for n, v in images.items():
            assert v.dtype == np.float32 and v.ndim == 1
            assert np.array_equal(flat[off[n]:off[n] + v.size].view(np.int32), v.view(np.int32)), n


class _NoDevice:
    """HipModel.update's name and shape checks run before anything touches the device (tests/test_decoder_grads_host.py)."""

    def __init__(self, d, w):
        from ctrlsim_amd.engine import HipModel
        self.update = HipModel.update.__get__(self)
        self.dims = d
        self._ffn_layer = f"decoder.transformer_decoder.layers.{d.ND - 1}"
        self._heads = {k: np.array(v, np.float32) for k, v in w.items() if k.startswith(pack.HEAD_PREFIXES)}
        for attr, sfx in (("_ffn", pack.TRAINABLE_FFN_SUFFIXES), ("_cross", pack.TRAINABLE_CROSS_SUFFIXES), ("_self", pack.TRAINABLE_SELF_SUFFIXES)):
            setattr(self, attr, {self._ffn_layer + s: np.array(w[self._ffn_layer + s], np.float32) for s in sfx})
        self._early = {k: np.array(w[k], np.float32) for l in range(d.ND - 1) for k in lgr.names(l)}
        self._enc = {k: np.array(w[k], np.float32) for l in range(d.NE) for k in egr.names(l)}


def test_names_update_accepts_with_and_without_the_encoder_flag():
    cfg = loss_ref.case_cfg(0)
    d = spec.Dims(cfg)
    w = loss_ref.case_weights(0, d)
    m = _NoDevice(d, w)
    enc = [n for l in range(d.NE) for n in egr.names(l)]
    dec = [n for l in range(d.ND) for n in lgr.names(l)]
    other = ["encoder.transformer_encoder.layers.0.norm3.weight", "encoder.embed_rtg.weight", f"encoder.transformer_encoder.layers.{d.NE}.linear1.weight",
             "encoder.map_encoder.norm1.weight"]
    bad = np.zeros((1, 2, 3), np.float32)
    for k in hgr.head_names(w) + dec + enc:                                # accepted by name (refused by shape): encoder implies decoder
        with pytest.raises(ValueError):
            m.update({k: bad}, encoder=True)
    for k in other:
        with pytest.raises(KeyError):
            m.update({k: bad}, encoder=True)
    for flags in ({}, {"cross": True}, {"self_attn": True}, {"cross": True, "self_attn": True}, {"decoder": True}):
        for k in enc + other:                                              # without the flag every encoder name stays refused
            with pytest.raises(KeyError):
                m.update({k: bad}, **flags)


def test_new_symbols_are_declared_bound_and_exported_with_the_declared_argument_counts():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "ctrlsim.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for sym, nargs in (("ctrlsim_scene_attn_block_grad_workspace_bytes", 2), ("ctrlsim_scene_attn_block_grad_chunk_contexts", 2),
                       ("ctrlsim_scene_attn_block_grad", 18), ("ctrlsim_encoder_layer_grad_workspace_bytes", 3),
                       ("ctrlsim_encoder_layer_grad", 15), ("ctrlsim_train_grad_layout", 6), ("ctrlsim_train_grads_workspace_bytes", 4),
                       ("ctrlsim_forward_loss_grads", 14)):
        m = re.search(r"\b" + sym + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
        assert m, sym
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[sym][1]), sym
        assert hasattr(lib, sym)
    assert "#define CTRLSIM_MAX_ENCODER_LAYERS 8" in hdr
    for sym in ("ctrlsim_decoder_grad_layout", "ctrlsim_decoder_grads_workspace_bytes", "ctrlsim_forward_loss_grads_decoder",
                "ctrlsim_encoder_grad_layout", "ctrlsim_encoder_grads_workspace_bytes", "ctrlsim_forward_loss_grads_encoder"):
        assert not re.search(r"\b" + sym + r"\b", hdr) and sym not in _lib.SIGNATURES and not hasattr(lib, sym), sym      # (dlsym finds none)
    assert C.sizeof(_lib.TrainTaps) == (8 + 4 * 8) * C.sizeof(C.c_void_p)
    assert _lib.TrainTaps.dE0.offset == (8 + 2 * 8) * C.sizeof(C.c_void_p)  # the encoder taps end the struct


def test_param_groups_over_the_encoder_names():
    """param_groups needs no change for the encoder: in_proj_weight, out_proj.weight, linear1 / linear2 weights decay; every bias and
    norm1 / norm2 do not; both lists sorted."""
    d = spec.Dims(loss_ref.case_cfg(0))
    w = loss_ref.case_weights(0, d)
    enc = [n for l in range(d.NE - 1, -1, -1) for n in egr.names(l)]
    names = hgr.head_names(w) + lgr.names(d.ND - 1) + enc
    decay, no_decay = CtRLSim.param_groups(names)
    assert sorted(decay + no_decay) == sorted(names) and not set(decay) & set(no_decay)
    assert decay == sorted(decay) and no_decay == sorted(no_decay)
    for l in range(d.NE):
        pre = f"encoder.transformer_encoder.layers.{l}"
        assert {pre + s for s in (".linear1.weight", ".linear2.weight", ".self_attn.in_proj_weight", ".self_attn.out_proj.weight")} <= set(decay)
        assert {k for k in egr.names(l) if k.endswith("bias") or ".norm" in k} <= set(no_decay)
        assert len([k for k in decay if k.startswith(pre + ".")]) == 4 and len([k for k in no_decay if k.startswith(pre + ".")]) == 8


def _key_pad(cfg, d, inp):
    """The scene rows' key-padding bytes (modules/encoder.py:155-170), [B, P + A] without the filler rows."""
    pad = np.ones((np.asarray(inp["agent_states"]).shape[0], d.P + d.A), bool)
    if bool(cfg.model.get("use_map", True)):
        pad[:, :d.P] = ~(np.asarray(inp["road_points"])[..., 2] != 0).any(-1)
    if bool(cfg.model.get("encode_initial_state", True)):
        pad[:, d.P:] = np.asarray(inp["agent_states"])[:, :, 0, 7] == 0
    return pad


@pytest.mark.parametrize("case", [0, 1, 7])
def test_fixture_holds_every_encoder_tensor_and_exercises_mask_and_filler(case):
    """tests/golden/encoder_grads.part*.npz (tools/gen_golden_encoder_grads.py): every one of the 12 tensors of every encoder layer in
    the recorded format, finite and non-zero; the sampled rows of a matrix agree with its recorded column sums and norm as far as 16
    rows can (|row| <= norm); dE0 [B (P + A), 256] with exactly the rows of the case inputs' padded keys recorded as zero — every
    context has a padded polyline and a non-existent initial agent, the tiny cases have M = 12 for 10 real rows (two filler rows), the
    full case M = 224 exactly."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    inp = loss_ref.case_inputs(case, d)
    gf = golden("encoder_grads")
    assert case in gf["cases"]
    P = f"c{case}_"
    table = {n: tuple(s) for n, s, _, _ in weights.param_table(d)}
    for l in range(d.NE):
        for k in egr.names(l):
            if len(table[k]) == 1:
                g = gf[P + "g_" + k]
                assert g.shape == table[k] and g.dtype == np.float32 and np.isfinite(g).all() and g.any()
                continue
            rows, s, nrm, cs = gf[P + "r_" + k], gf[P + "s_" + k], float(gf[P + "n_" + k]), gf[P + "c_" + k]
            assert s.shape == (len(rows), table[k][1]) and cs.shape == (table[k][1],) and rows[0] == 0 and rows[-1] == table[k][0] - 1
            assert np.isfinite(s).all() and s.any() and np.linalg.norm(s.astype(np.float64)) <= nrm * (1 + 1e-6)
            assert np.abs(cs).max() <= nrm * np.sqrt(table[k][0]) * (1 + 1e-6)
    pad = _key_pad(cfg, d, inp)
    B = pad.shape[0]
    assert pad[:, :d.P].any(1).all() and pad[:, d.P:].any(1).all() and not pad.all(1).any()
    M = (d.P + d.A + 3) & ~3
    assert M - (d.P + d.A) == (0 if case == 7 else 2)
    assert np.array_equal(gf[P + "z_dE0"], np.flatnonzero(pad.reshape(-1)))
    rows, s = gf[P + "r_dE0"], gf[P + "s_dE0"]
    assert rows[-1] == B * (d.P + d.A) - 1 and s.shape == (len(rows), 256)
    zero = np.isin(rows, gf[P + "z_dE0"])
    assert not s[zero].any() and s[~zero].any(axis=1).all()


TWIN_BOUND = 1e-4               # tests/test_gpu_self_attn_grads.py: FIXTURE_BOUND, the existing form for a float32 recording against float64


def fixture_errors(gf, P, k, got):
    """The deviation measure of tests/test_gpu_decoder_grads.py for one tensor against its recording, relative to max |T|: a vector in
    full; a matrix by its sampled rows, column sums and Frobenius norm."""
    got = np.asarray(got)
    scale = np.abs(got).max()
    if got.ndim == 1:
        return np.abs(got - gf[P + "g_" + k]).max() / scale
    rows = gf[P + "r_" + k]
    err = np.abs(got[rows] - gf[P + "s_" + k]).max() / scale
    nrm = abs(np.linalg.norm(got.astype(np.float64)) - float(gf[P + "n_" + k])) / float(gf[P + "n_" + k])
    if P + "c_" + k in gf:
        err = max(err, np.abs(got.astype(np.float64).sum(0) - gf[P + "c_" + k]).max() / (scale * got.shape[0]))
    return max(err, nrm)


@pytest.mark.parametrize("case", [0, 1])
def test_float64_twin_reproduces_the_recorded_reference_gradients(case):
    """The tiny cases record the reference's encoder input rows e0 and the gradient dOut at its encoder output.  The float64 twin of
    the NE layers on (e0, the case inputs' key padding, dOut) gives every recorded gradient — 12 tensors per layer and dE0 — within
    TWIN_BOUND of the tensor's largest element: the twin, the tensor order, the padding convention and the fixture agree."""
    cfg = loss_ref.case_cfg(case)
    d = spec.Dims(cfg)
    w, inp = loss_ref.case_weights(case, d), loss_ref.case_inputs(case, d)
    gf = golden("encoder_grads")
    P = f"c{case}_"
    pad = _key_pad(cfg, d, inp)
    B = pad.shape[0]
    e0, dOut = (gf[P + k].astype(np.float64).reshape(B, d.P + d.A, 256) for k in ("e0", "dOut"))
    layers = [[np.asarray(w[k], np.float64) for k in egr.names(l)] for l in range(d.NE)]
    g, dE = egr.stack_grads(e0, pad, dOut, layers)
    worst = 0.0
    for l in range(d.NE):
        for k, t in zip(egr.names(l), g[l]):
            err = fixture_errors(gf, P, k, t)
            print(f"   {k}: {err:.3e} of max |T|")
            worst = max(worst, err)
    err = fixture_errors(gf, P, "dE0", dE[0].reshape(-1, 256))
    print(f"   dE0: {err:.3e}; worst tensor {worst:.3e}")
    assert max(worst, err) <= TWIN_BOUND
    assert not dE[0].reshape(-1, 256)[gf[P + "z_dE0"]].any()
