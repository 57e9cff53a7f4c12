"""TEST INFRASTRUCTURE — the first sublayer of a decoder layer: self-attention under the structured multi-agent causal mask, then norm1,
    Q | K | V = X Win^T + bin, O = concat_h softmax_{visible j}(Q_h K_h^T / sqrt(32)) V_h, Y = LayerNorm(X + O Wo^T + bo)
(width 256, 8 heads x 32, LayerNorm eps 1e-5) over contexts of L = 3 T A token rows, token i = (t, a, k) = (i // 3A, (i // 3) % A, i % 3),
and its backward from a given dY, restated with torch autograd on the CPU from the definitions: an explicit per-head softmax and the mask
closed form written out, no torch attention module.  Shares no code with the library.  dtype float64: the checker; dtype float32: what
torch computes on the CPU in fp32, the yardstick of the accuracy bound (as tests/attn_grad_ref.py is for the cross-attention sublayer).

mode 0: visible(i, j) <=> t_j < t_i or (t_j == t_i and ((a_j == a_i and k_j <= k_i) or k_j == 0)); mode 1 (attend_own_return_action):
the t_j < t_i term holds only where a_j == a_i or k_j == 0."""
import numpy as np
import torch
import torch.nn.functional as F

PARTS = (".self_attn.in_proj_weight", ".self_attn.in_proj_bias", ".self_attn.out_proj.weight", ".self_attn.out_proj.bias",
         ".norm1.weight", ".norm1.bias")
SIZES = (768 * 256, 768, 256 * 256, 256, 256, 256)
SHAPE_OF = ((768, 256), (768,), (256, 256), (256,), (256,), (256,))
NHEAD, HD = 8, 32


def layer_prefix(d):
    return f"decoder.transformer_decoder.layers.{d.ND - 1}"


def names(d):
    """State-dict names of the last decoder layer's self-attention tensors, in gradient-layout order."""
    return [layer_prefix(d) + p for p in PARTS]


def triples(T, A):
    """(t, a, k) of the L = 3 T A token rows, as int64 ndarrays."""
    i = np.arange(3 * T * A)
    return i // (3 * A), (i // 3) % A, i % 3


def mask(T, A, mode):
    """bool [L, L] ndarray, True = visible, written out pair by pair from the definition."""
    t, a, k = triples(T, A)
    ti, tj, ai, aj, ki, kj = t[:, None], t[None, :], a[:, None], a[None, :], k[:, None], k[None, :]
    own, state = ai == aj, kj == 0
    earlier = tj < ti
    if mode == 1:
        earlier = earlier & (own | state)
    elif mode != 0:
        raise ValueError(mode)
    return earlier | ((tj == ti) & ((own & (kj <= ki)) | state))


def block(X, vis, W):
    """X [B, L, 256], vis bool [L, L], W: the six tensors in PARTS order."""
    Win, bin_, Wo, bo, g, be = W
    B, L, D = X.shape
    QKV = F.linear(X, Win, bin_)
    Q, K, V = (QKV[..., i * D:(i + 1) * D].reshape(B, L, NHEAD, HD) for i in range(3))
    heads = []
    for h in range(NHEAD):
        s = torch.einsum("bqd,bkd->bqk", Q[:, :, h], K[:, :, h]) / np.sqrt(HD)
        p = torch.softmax(s.masked_fill(~vis[None], float("-inf")), dim=-1)      # every row sees itself: no empty row
        heads.append(torch.einsum("bqk,bkd->bqd", p, V[:, :, h]))
    S = X + F.linear(torch.cat(heads, dim=-1), Wo, bo)
    return F.layer_norm(S, (D,), g, be, 1e-5)


def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def forward(X, T, A, mode, tensors, dtype=torch.float64):
    with torch.no_grad():
        return block(_t(X, dtype), torch.from_numpy(mask(T, A, mode)), [_t(t, dtype) for t in tensors]).double().numpy()


def grads(X, dY, T, A, mode, tensors, dtype=torch.float64):
    """-> ([d in_proj_weight, d in_proj_bias, d out_proj.weight, d out_proj.bias, dg, dbe], dX) as float64 ndarrays: the vector-Jacobian
    product of the block with dY.  X, dY [B, 3 T A, 256]."""
    W = [_t(t, dtype, True) for t in tensors]
    Xt = _t(X, dtype, True)
    block(Xt, torch.from_numpy(mask(T, A, mode)), W).backward(_t(dY, dtype))
    return [w.grad.double().numpy() for w in W], Xt.grad.double().numpy()


def make_case(B, T, A, seed, w_trained_like):
    """Seeded op inputs, attn_grad_ref.make_case's conventions: X of trained-like magnitude (unit normal rows times exp(uniform(-1, 1))),
    dY with a per-row scale spread over four decades around 1e-4 and a quarter of the rows exactly zero, and the six tensors from
    trained-like weights (PARTS order)."""
    rs = np.random.RandomState(seed)
    L = 3 * T * A
    X = (rs.standard_normal((B, L, 256)) * np.exp(rs.uniform(-1, 1, (B, L, 1)))).astype(np.float32)
    dY = (rs.standard_normal((B, L, 256)) * 1e-4 * np.exp(rs.uniform(-4.6, 4.6, (B, L, 1)))).astype(np.float32)
    zero = rs.rand(B, L) < 0.25
    zero[0, 0] &= not zero.all()
    dY[zero] = 0.0
    return X, dY, [np.ascontiguousarray(np.asarray(t, np.float32)) for t in w_trained_like]
