"""TEST INFRASTRUCTURE — the post-LN attention sublayer of a transformer layer with a key-padding mask,
    Q = X Wq^T + bq, K = Mem Wk^T + bk, V = Mem Wv^T + bv, O = concat_h softmax_keys(Q_h K_h^T / sqrt(32)) V_h, Y = LayerNorm(X + O Wo^T + bo)
(width 256, 8 heads x 32, LayerNorm eps 1e-5; a context whose keys are all padded has O = 0) and its backward from a given dY, restated
with torch autograd on the CPU from the definitions: an explicit per-head softmax, no torch attention module.  Shares no code with the
library.  dtype float64: the checker; dtype float32: what torch computes on the CPU in fp32, the yardstick of the accuracy bound (as
tests/ffn_grad_ref.py is for the feed-forward block)."""
import numpy as np
import torch
import torch.nn.functional as F

PARTS = (".multihead_attn.in_proj_weight", ".multihead_attn.in_proj_bias", ".multihead_attn.out_proj.weight",
         ".multihead_attn.out_proj.bias", ".norm2.weight", ".norm2.bias")
NHEAD, HD = 8, 32


def layer_prefix(d):
    return f"decoder.transformer_decoder.layers.{d.ND - 1}"


def names(d):
    """State-dict names of the last decoder layer's cross-attention tensors, in gradient-layout order."""
    return [layer_prefix(d) + p for p in PARTS]


def block(X, Mem, key_pad, W):
    """X [B, Lq, 256], Mem [B, Lk, 256], key_pad bool [B, Lk] or None, W: the six tensors in PARTS order."""
    Win, bin_, Wo, bo, g, be = W
    B, Lq, D = X.shape
    Lk = Mem.shape[1]
    Q = F.linear(X, Win[:D], bin_[:D]).view(B, Lq, NHEAD, HD)
    K = F.linear(Mem, Win[D:2 * D], bin_[D:2 * D]).view(B, Lk, NHEAD, HD)
    V = F.linear(Mem, Win[2 * D:], bin_[2 * D:]).view(B, Lk, NHEAD, HD)
    heads = []
    for h in range(NHEAD):
        s = torch.einsum("bqd,bkd->bqk", Q[:, :, h], K[:, :, h]) / np.sqrt(HD)
        if key_pad is not None:
            s = s.masked_fill(key_pad[:, None, :], float("-inf"))      # mask first ...
        p = torch.softmax(s, dim=-1)
        p = torch.where(torch.isnan(p), torch.zeros_like(p), p)        # ... then zero the rows of a context without keys
        heads.append(torch.einsum("bqk,bkd->bqd", p, V[:, :, h]))
    O = torch.cat(heads, dim=-1)
    S = X + F.linear(O, Wo, bo)
    return F.layer_norm(S, (D,), g, be, 1e-5)


def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def forward(X, Mem, key_pad, tensors, dtype=torch.float64):
    with torch.no_grad():
        kp = None if key_pad is None else torch.tensor(np.asarray(key_pad).astype(bool))
        return block(_t(X, dtype), _t(Mem, dtype), kp, [_t(t, dtype) for t in tensors]).double().numpy()


def grads(X, Mem, key_pad, dY, tensors, dtype=torch.float64):
    """-> ([d in_proj_weight, d in_proj_bias, d out_proj.weight, d out_proj.bias, dg, dbe], dX, dMem) as float64 ndarrays: the
    vector-Jacobian product of the block with dY.  X, dY [B, Lq, 256]; Mem [B, Lk, 256]."""
    W = [_t(t, dtype, True) for t in tensors]
    Xt, Mt = _t(X, dtype, True), _t(Mem, dtype, True)
    kp = None if key_pad is None else torch.tensor(np.asarray(key_pad).astype(bool))
    block(Xt, Mt, kp, W).backward(_t(dY, dtype))
    return [w.grad.double().numpy() for w in W], Xt.grad.double().numpy(), Mt.grad.double().numpy()


PADS = ("none", "tail", "scattered", "tile", "context")


def make_pad(B, Lk, kind, rs):
    """Key-padding patterns: none (NULL); the tail padded; scattered keys; a whole 64-key tile (the first; everything but the last key where
    Lk <= 64); one context with EVERY key padded beside neighbours with none."""
    if kind == "none":
        return None
    pad = np.zeros((B, Lk), np.uint8)
    if kind == "tail":
        for b in range(B):
            pad[b, Lk - 1 - (Lk // 3 + b) % Lk:] = 1
            pad[b, 0] = 0
    elif kind == "scattered":
        pad[:] = rs.rand(B, Lk) < 0.3
        pad[:, rs.randint(Lk)] = 0
    elif kind == "tile":
        pad[:, :min(64, Lk - 1)] = 1
    elif kind == "context":
        pad[B // 2] = 1
    else:
        raise ValueError(kind)
    return pad


def make_case(B, Lq, Lk, seed, w_trained_like):
    """Seeded op inputs, ffn_grad_ref.make_case's conventions: X and Mem of trained-like magnitude (unit normal rows times
    exp(uniform(-1, 1))), dY with a per-row scale spread over four decades around 1e-4 and a quarter of the rows exactly zero, and the
    six tensors from trained-like weights (PARTS order)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, Lq, 256)) * np.exp(rs.uniform(-1, 1, (B, Lq, 1)))).astype(np.float32)
    Mem = (rs.standard_normal((B, Lk, 256)) * np.exp(rs.uniform(-1, 1, (B, Lk, 1)))).astype(np.float32)
    dY = (rs.standard_normal((B, Lq, 256)) * 1e-4 * np.exp(rs.uniform(-4.6, 4.6, (B, Lq, 1)))).astype(np.float32)
    zero = rs.rand(B, Lq) < 0.25
    zero[0, 0] &= not zero.all()                                       # (a single row: keep it)
    dY[zero] = 0.0
    return X, Mem, dY, [np.ascontiguousarray(np.asarray(t, np.float32)) for t in w_trained_like]
