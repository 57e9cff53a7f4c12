"""TEST INFRASTRUCTURE — one whole post-LN scene-encoder layer and a stack of them, composed from the sublayer references
    U = attn_grad_ref.block(X0, X0, key_pad)   (one source: queries, keys and values are the context's own rows),  Y = ffn_grad_ref.block(U)
and their backward from a given dY by torch autograd on the CPU.  Shares no code with the library.  dtype float64: the checker; dtype
float32: what torch computes on the CPU in fp32, the yardstick of the accuracy bound.

TENSOR ORDER of a layer (W12, and the gradients returned): the decoder layer's convention (tests/layer_grad_ref.py) — the six
feed-forward tensors (with norm2), then the six attention tensors (with norm1), each group in state-dict order.

RELU KINKS: as tests/layer_grad_ref.py — relu_on (bool [rows, F]) fixes the ReLU's on / off pattern to the one the evaluation under test
used; where it equals (Hp > 0) it is the same function."""
import numpy as np
import torch

import attn_grad_ref as agr
import ffn_grad_ref as fgr
import self_attn_grad_ref as sgr

FFN_PARTS = fgr.PARTS[:4] + (".norm2.weight", ".norm2.bias")
ATTN_PARTS = sgr.PARTS                     # self_attn.in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, norm1.weight, norm1.bias
PARTS = FFN_PARTS + ATTN_PARTS


def relu_pattern(U_seen, dY_ffn, W6, db1_seen):
    """layer_grad_ref.relu_pattern: the on / off pattern of the ReLU the evaluation under test used -> (relu_on, number of kinks)."""
    return fgr.resolve_kinks(np.asarray(U_seen).reshape(-1, 256), np.asarray(dY_ffn).reshape(-1, 256), W6, np.asarray(db1_seen, np.float64))


def sizes(F):
    return (F * 256, F, 256 * F, 256, 256, 256) + sgr.SIZES


def shapes(F):
    return ((F, 256), (F,), (256, F), (256,), (256,), (256,)) + sgr.SHAPE_OF


def names(layer):
    """State-dict names of scene-encoder layer `layer`'s 12 tensors, in gradient-layout order."""
    return [f"encoder.transformer_encoder.layers.{layer}{p}" for p in PARTS]


def layer(X0, key_pad, W12, relu_on=None):
    """X0 [B, L, 256], key_pad bool [B, L] or None -> (Y, U)."""
    U = agr.block(X0, X0, key_pad, W12[6:12])
    Y = fgr.block(U.reshape(-1, 256), W12[0:6], relu_on).view(U.shape)
    return Y, U


def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def _pad(key_pad):
    return None if key_pad is None else torch.tensor(np.asarray(key_pad).astype(bool))


def _on(relu_on, dtype):
    return None if relu_on is None else torch.tensor(np.asarray(relu_on), dtype=dtype)


def attn_grads(X, key_pad, dY, W6, dtype=torch.float64):
    """The attention sublayer alone -> ([six gradients], dX) as float64 ndarrays (dX through the residual, Q, K and V)."""
    W = [_t(t, dtype, True) for t in W6]
    Xt = _t(X, dtype, True)
    agr.block(Xt, Xt, _pad(key_pad), W).backward(_t(dY, dtype))
    return [w.grad.double().numpy() for w in W], Xt.grad.double().numpy()


def grads(X0, key_pad, dY, W12, dtype=torch.float64, relu_on=None):
    """-> ([12 gradients], dX0, U) as float64 ndarrays: the vector-Jacobian product of the layer with dY, and the intermediate rows."""
    W = [_t(t, dtype, True) for t in W12]
    Xt = _t(X0, dtype, True)
    Y, U = layer(Xt, _pad(key_pad), W, _on(relu_on, dtype))
    Y.backward(_t(dY, dtype))
    f8 = lambda t: t.detach().double().numpy()
    return [f8(w.grad) for w in W], f8(Xt.grad), f8(U)


def stack(X0, key_pad, layers, relu_on=None):
    """layers: a list of W12, first layer first -> (Y, [the rows that enter each layer])."""
    X, entered = X0, []
    for i, W12 in enumerate(layers):
        entered.append(X)
        X = layer(X, key_pad, W12, None if relu_on is None else relu_on[i])[0]
    return X, entered


def stack_grads(X0, key_pad, dY, layers, dtype=torch.float64, relu_on=None):
    """The stack's backward from dY at its output -> ([[12 gradients] per layer], [dE0 per layer]) as float64 ndarrays."""
    Ws = [[_t(t, dtype, True) for t in W12] for W12 in layers]
    Xt = _t(X0, dtype, True)
    on = None if relu_on is None else [_on(m, dtype) for m in relu_on]
    Y, entered = stack(Xt, _pad(key_pad), Ws, on)
    for x in entered[1:]:
        x.retain_grad()
    Y.backward(_t(dY, dtype))
    f8 = lambda t: t.detach().double().numpy()
    return [[f8(w.grad) for w in W] for W in Ws], [f8(x.grad) for x in entered]


def make_case(B, L, F, seed, w_trained_like):
    """Seeded op inputs in the sublayer references' conventions: X0 of trained-like magnitude, dY with a per-row scale spread over four
    decades around 1e-4 and a quarter of the rows exactly zero; the 12 tensors from trained-like weights (PARTS order, hidden width
    >= F), cut to hidden width F."""
    rs = np.random.RandomState(seed)
    X0 = (rs.standard_normal((B, L, 256)) * np.exp(rs.uniform(-1, 1, (B, L, 1)))).astype(np.float32)
    dY = (rs.standard_normal((B, L, 256)) * 1e-4 * np.exp(rs.uniform(-4.6, 4.6, (B, L, 1)))).astype(np.float32)
    zero = rs.rand(B, L) < 0.25
    zero[0, 0] &= not zero.all()
    dY[zero] = 0.0
    W = [np.asarray(t, np.float32) for t in w_trained_like]
    W[0], W[1], W[2] = W[0][:F], W[1][:F], W[2][:, :F]
    return X0, dY, [np.ascontiguousarray(t) for t in W]
