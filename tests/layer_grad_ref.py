"""TEST INFRASTRUCTURE — one whole post-LN decoder layer and a stack of them, composed from the three sublayer references
    X1 = self_attn_grad_ref.block(X0),  U = attn_grad_ref.block(X1, Mem),  Y = ffn_grad_ref.block(U)
and their backward from a given dY by torch autograd on the CPU.  Shares no code with the library.  dtype float64: the checker; dtype
float32: what torch computes on the CPU in fp32, the yardstick of the accuracy bound.

TENSOR ORDER of a layer (W18, and the gradients returned): the order a training scope appends them — the six feed-forward tensors, the
six cross-attention tensors, the six self-attention tensors, each group in state-dict order.

RELU KINKS (ffn_grad_ref.resolve_kinks): the layer op recomputes U in float32, so a hidden pre-activation within rounding of zero can
sit on the other side of the ReLU than in float64.  relu_on (bool [rows, F]) fixes the ReLU's on / off pattern to the one the evaluation
under test used; the twin then differentiates that function.  Where relu_on equals (Hp > 0) it is the same function."""
import numpy as np
import torch

import attn_grad_ref as agr
import ffn_grad_ref as fgr
import self_attn_grad_ref as sgr

PARTS = fgr.PARTS + agr.PARTS + sgr.PARTS


def sizes(F):
    return (F * 256, F, 256 * F, 256, 256, 256) + 2 * sgr.SIZES


def shapes(F):
    return ((F, 256), (F,), (256, F), (256,), (256,), (256,)) + 2 * sgr.SHAPE_OF


def names(layer):
    """State-dict names of decoder layer `layer`'s 18 tensors, in gradient-layout order."""
    return [f"decoder.transformer_decoder.layers.{layer}{p}" for p in PARTS]


def layer(X0, Mem, key_pad, vis, W18, relu_on=None):
    """X0 [B, L, 256], Mem [B, Lk, 256], key_pad bool [B, Lk] or None, vis bool [L, L] -> (Y, X1, U)."""
    X1 = sgr.block(X0, vis, W18[12:18])
    U = agr.block(X1, Mem, key_pad, W18[6:12])
    Y = fgr.block(U.reshape(-1, 256), W18[0:6], relu_on).view(U.shape)
    return Y, X1, U


def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def _pad(key_pad):
    return None if key_pad is None else torch.tensor(np.asarray(key_pad).astype(bool))


def _on(relu_on, dtype):
    return None if relu_on is None else torch.tensor(np.asarray(relu_on), dtype=dtype)


def grads(X0, Mem, key_pad, dY, T, A, mode, W18, dtype=torch.float64, relu_on=None):
    """-> ([18 gradients], dX0, dMem, X1, U) as float64 ndarrays: the vector-Jacobian product of the layer with dY, and the two
    intermediate rows."""
    W = [_t(t, dtype, True) for t in W18]
    Xt, Mt = _t(X0, dtype, True), _t(Mem, dtype, True)
    Y, X1, U = layer(Xt, Mt, _pad(key_pad), torch.from_numpy(sgr.mask(T, A, mode)), W, _on(relu_on, dtype))
    Y.backward(_t(dY, dtype))
    f8 = lambda t: t.detach().double().numpy()
    return [f8(w.grad) for w in W], f8(Xt.grad), f8(Mt.grad), f8(X1), f8(U)


def stack(X0, Mem, key_pad, vis, layers, relu_on=None):
    """layers: a list of W18, first layer first; relu_on: None or one mask (or None) per layer -> (Y, [the rows that enter each layer])."""
    X, entered = X0, []
    for i, W18 in enumerate(layers):
        entered.append(X)
        X = layer(X, Mem, key_pad, vis, W18, None if relu_on is None else relu_on[i])[0]
    return X, entered


def stack_grads(X0, Mem, key_pad, dY, T, A, mode, layers, dtype=torch.float64, relu_on=None):
    """The stack's backward from dY at its output -> ([[18 gradients] per layer], [dX0 per layer], dMem) as float64 ndarrays."""
    Ws = [[_t(t, dtype, True) for t in W18] for W18 in layers]
    Xt, Mt = _t(X0, dtype, True), _t(Mem, dtype, True)
    on = None if relu_on is None else [_on(m, dtype) for m in relu_on]
    Y, entered = stack(Xt, Mt, _pad(key_pad), torch.from_numpy(sgr.mask(T, A, mode)), Ws, on)
    for x in entered[1:]:
        x.retain_grad()
    Y.backward(_t(dY, dtype))
    f8 = lambda t: t.detach().double().numpy()
    return [[f8(w.grad) for w in W] for W in Ws], [f8(x.grad) for x in entered], f8(Mt.grad)


def relu_pattern(U_seen, dY_ffn, W6, db1_seen):
    """The on / off pattern of the ReLU the evaluation under test used: from the U it computed (U_seen [rows, 256], float32), with the
    elements within rounding of zero resolved by ffn_grad_ref.resolve_kinks from the db1 it produced.  -> (relu_on, number of kinks)."""
    return fgr.resolve_kinks(np.asarray(U_seen).reshape(-1, 256), np.asarray(dY_ffn).reshape(-1, 256), W6, np.asarray(db1_seen, np.float64))


def make_case(B, T, A, Lk, F, seed, w_trained_like):
    """Seeded op inputs in the conventions of the three sublayer references: X0 and Mem of trained-like magnitude, dY with a per-row scale
    spread over four decades around 1e-4 and a quarter of the rows exactly zero; the 18 tensors from trained-like weights
    (w_trained_like: 18 arrays in PARTS order with hidden width >= F), cut to hidden width F."""
    rs = np.random.RandomState(seed)
    L = 3 * T * A
    X0 = (rs.standard_normal((B, L, 256)) * np.exp(rs.uniform(-1, 1, (B, L, 1)))).astype(np.float32)
    Mem = (rs.standard_normal((B, Lk, 256)) * np.exp(rs.uniform(-1, 1, (B, Lk, 1)))).astype(np.float32)
    dY = (rs.standard_normal((B, L, 256)) * 1e-4 * np.exp(rs.uniform(-4.6, 4.6, (B, L, 1)))).astype(np.float32)
    zero = rs.rand(B, L) < 0.25
    zero[0, 0] &= not zero.all()
    dY[zero] = 0.0
    W = [np.asarray(t, np.float32) for t in w_trained_like]
    W[0], W[1], W[2] = W[0][:F], W[1][:F], W[2][:, :F]
    return X0, Mem, dY, [np.ascontiguousarray(t) for t in W]
