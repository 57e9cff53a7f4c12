"""TEST INFRASTRUCTURE — the post-LN feed-forward block of a transformer layer, Y = LayerNorm(U + linear2(relu(linear1(U)))) (width 256,
LayerNorm eps 1e-5, relu'(0) = 0 as torch has it), and its backward from a given dY, restated with torch autograd on the CPU from the
definitions.  Shares no code with the library.  dtype float64: the checker; dtype float32: what torch computes on the CPU in fp32, the
yardstick of the accuracy bound (as tests/head_grad_ref.py is for the heads)."""
import numpy as np
import torch
import torch.nn.functional as F

PARTS = (".linear1.weight", ".linear1.bias", ".linear2.weight", ".linear2.bias", ".norm3.weight", ".norm3.bias")


def layer_prefix(d):
    return f"decoder.transformer_decoder.layers.{d.ND - 1}"


def names(d):
    """State-dict names of the last decoder layer's feed-forward tensors, in gradient-layout order."""
    return [layer_prefix(d) + p for p in PARTS]


def block(U, W, relu_on=None):
    """W: the six tensors in PARTS order.  relu_on (bool [rows, F], optional): the ReLU as a multiplication by this constant mask —
    the same function and the same derivative wherever relu_on == (Hp > 0); see resolve_kinks."""
    W1, b1, W2, b2, g, be = W
    Hp = F.linear(U, W1, b1)
    H = F.relu(Hp) if relu_on is None else Hp * relu_on
    S = U + F.linear(H, W2, b2)
    return F.layer_norm(S, (S.shape[-1],), g, be, 1e-5)


def forward(U, tensors, dtype=torch.float64):
    with torch.no_grad():
        return block(torch.tensor(np.asarray(U), dtype=dtype), [torch.tensor(np.asarray(t), dtype=dtype) for t in tensors]).double().numpy()


def grads(U, dY, tensors, dtype=torch.float64, relu_on=None):
    """-> ([dW1, db1, dW2, db2, dg, dbe], dU) as float64 ndarrays: the vector-Jacobian product of the block with dY."""
    W = [torch.tensor(np.asarray(t), dtype=dtype, requires_grad=True) for t in tensors]
    U = torch.tensor(np.asarray(U), dtype=dtype, requires_grad=True)
    mask = None if relu_on is None else torch.tensor(np.asarray(relu_on), dtype=dtype)
    block(U, W, mask).backward(torch.tensor(np.asarray(dY), dtype=dtype))
    return [w.grad.double().numpy() for w in W], U.grad.double().numpy()


def make_case(rows, Fh, seed, w_trained_like):
    """Seeded op inputs: U of trained-like magnitude (head_grad_ref's recipe for X: unit normal rows times exp(uniform(-1, 1))), dY with a
    per-row scale spread over four decades around 1e-4 (a loss gradient: most rows small, a few large, some exactly zero), and the six
    tensors cut from trained-like weights `w_trained_like` = (W1 [>=Fh, 256], b1, W2 [256, >=Fh], b2, g, be)."""
    rs = np.random.RandomState(seed)
    U = (rs.standard_normal((rows, 256)) * np.exp(rs.uniform(-1, 1, (rows, 1)))).astype(np.float32)
    dY = (rs.standard_normal((rows, 256)) * 1e-4 * np.exp(rs.uniform(-4.6, 4.6, (rows, 1)))).astype(np.float32)
    dY[rs.rand(rows) < 0.25] = 0.0
    W1, b1, W2, b2, g, be = (np.asarray(t, np.float32) for t in w_trained_like)
    return U, dY, [np.ascontiguousarray(W1[:Fh]), np.ascontiguousarray(b1[:Fh]), np.ascontiguousarray(W2[:, :Fh]), b2.copy(), g.copy(), be.copy()]


KINK_TOL = 2.0 ** -24 * np.sqrt(257.0)


def resolve_kinks(U, dY, tensors, db1_seen):
    """The ReLU's derivative jumps where a hidden pre-activation Hp = u . w1 + b1 is zero, and a float32 evaluation of Hp — 257 rounded
    terms, in whatever order — differs from the exact value by about 2^-24 sqrt(257) (sum |u_k w1_k| + |b1|): below that size the SIGN
    of Hp, and with it relu'(Hp), is the evaluation's own, not the function's (seen on the device: full-size fixture case, one element
    of 4.7 million with Hp = 1.6e-8 in float64 and -3.0e-8 in torch's CPU float32; the whole of dW1's row and dU's row hang on it).
    Such elements are KINKS.  A gradient is checked against the float64 backward of the function the evaluation under test actually
    differentiated: for every hidden unit with kinks, the on / off choice of its kink elements that comes closest to the db1 element the
    evaluation produced (db1_seen [F]; db1[j] = sum over rows of relu' x dH, so the choice shows there).  Everywhere else the mask is the
    float64 one.  -> (relu_on bool [rows, F], number of kinks).  float64 NumPy from the formulas; the kinks' own H is ~ 0 either way."""
    f8 = lambda a: np.asarray(a, np.float64)
    U, dY = f8(U), f8(dY)
    W1, b1, W2, b2, g, _ = (f8(t) for t in tensors)
    Hp = U @ W1.T + b1
    kink = np.abs(Hp) <= KINK_TOL * (np.abs(U) @ np.abs(W1).T + np.abs(b1))
    on = Hp > 0
    if not kink.any():
        return on, 0
    S = U + np.maximum(Hp, 0.0) @ W2.T + b2
    mu = S.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((S - mu) ** 2).mean(1, keepdims=True) + 1e-5)
    xh = (S - mu) * rstd
    dxh = dY * g
    dS = rstd * (dxh - dxh.mean(1, keepdims=True) - xh * (dxh * xh).mean(1, keepdims=True))
    dH = dS @ W2
    for j in np.nonzero(kink.any(0))[0]:
        rows = np.nonzero(kink[:, j])[0][:12]
        base = (dH[:, j] * (on[:, j] & ~kink[:, j])).sum()
        best = min(range(1 << len(rows)), key=lambda c: abs(base + sum(dH[r, j] for i, r in enumerate(rows) if c >> i & 1) - db1_seen[j]))
        for i, r in enumerate(rows):
            on[r, j] = bool(best >> i & 1)
    return on, int(kink.sum())
