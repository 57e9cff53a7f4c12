"""Outputs of the three attention-backward ops (ctrlsim_attn_block_grad, ctrlsim_self_attn_block_grad, ctrlsim_decoder_layer_grad) on seeded
inputs, hashed per case — to compare two builds bit for bit (CTRLSIM_LIB=...).  Every output is hashed: grads, dX, dMem, x1_out, u_out; the
workspace is pre-filled with a non-zero pattern.  Prints one JSON line {case: sha256}.  usage: python tools/attn_grad_bits.py"""
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import ctrlsim_amd  # noqa: F401
from ctrlsim_amd import _lib

DEV = "cuda:0"
D = 256
lib, st = _lib.lib(), _lib.stream_ptr()

CROSS = [(1, 1, 1), (3, 33, 31), (2, 130, 65), (2, 300, 257)]             # (B, Lq, Lk), each under the four pad patterns
PADS = ("none", "tail", "scattered", "context")
CROSS_CHUNKS = (2, 4608, 224)                                              # two chunks of one context each; scattered pads
SELF = [(1, 1, 1), (2, 3, 4), (2, 5, 9), (1, 2, 64), (9, 10, 32), (4, 32, 24)]   # (B, T, A), both mask modes; the last spans two chunks
LAYER = [(2, 5, 9, 64, 33), (1, 2, 64, 65, 1024)]                          # (B, T, A, Lk, F), accumulate_dmem 0 and 1, mode 0


def rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def attn_tensors(g):
    """in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, norm weight, norm bias"""
    return [rnd(g, 3 * D, D, scale=0.06), rnd(g, 3 * D, scale=0.1), rnd(g, D, D, scale=0.06), rnd(g, D, scale=0.1),
            1.0 + rnd(g, D, scale=0.1), rnd(g, D, scale=0.1)]


def make_pad(g, B, Lk, kind):
    if kind == "none":
        return None
    pad = torch.zeros(B, Lk, dtype=torch.uint8)
    if kind == "tail":
        pad[:, Lk - (Lk + 2) // 3:] = 1
    else:
        pad = (torch.rand(B, Lk, generator=g) < 0.3).to(torch.uint8)
        if kind == "context":
            pad[B - 1] = 1
    return pad.to(DEV)


def workspace(n):
    return torch.full((int(n),), 0xA5, dtype=torch.uint8, device=DEV)


def digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        assert torch.isfinite(t).all()             # every element written, none a NaN of the pre-fill
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def p(t):
    return t.data_ptr() if t is not None else None


def cross(B, Lq, Lk, kind, seed):
    g = torch.Generator().manual_seed(seed)
    X, Mem, dY, W = rnd(g, B * Lq, D), rnd(g, B * Lk, D), rnd(g, B * Lq, D, scale=0.1), attn_tensors(g)
    pad = make_pad(g, B, Lk, kind)
    ws = workspace(lib.ctrlsim_attn_block_grad_workspace_bytes(B, Lq, Lk))
    grads = torch.full((4 * D * D + 6 * D,), float("nan"), device=DEV)
    dX, dMem = torch.full((B * Lq, D), 7.0, device=DEV), torch.full((B * Lk, D), 7.0, device=DEV)
    _lib.check(lib.ctrlsim_attn_block_grad(p(X), D, p(Mem), D, p(pad), p(dY), D, *map(p, W), B, Lq, Lk, p(ws), p(grads), p(dX), D, p(dMem), D,
                                           st), "attn_block_grad")
    return digest(grads, dX, dMem)


def self_attn(B, T, A, mode, seed):
    g = torch.Generator().manual_seed(seed)
    L = 3 * T * A
    X, dY, W = rnd(g, B * L, D), rnd(g, B * L, D, scale=0.1), attn_tensors(g)
    ws = workspace(lib.ctrlsim_self_attn_block_grad_workspace_bytes(B, T, A))
    grads = torch.full((4 * D * D + 6 * D,), float("nan"), device=DEV)
    dX = torch.full((B * L, D), 7.0, device=DEV)
    _lib.check(lib.ctrlsim_self_attn_block_grad(p(X), D, p(dY), D, *map(p, W), B, T, A, mode, p(ws), p(grads), p(dX), D, st),
               "self_attn_block_grad")
    return digest(grads, dX)


def layer(B, T, A, Lk, F, accumulate, seed):
    g = torch.Generator().manual_seed(seed)
    L = 3 * T * A
    X0, Mem, dY = rnd(g, B * L, D), rnd(g, B * Lk, D), rnd(g, B * L, D, scale=0.1)
    ffn = [rnd(g, F, D, scale=0.06), rnd(g, F, scale=0.1), rnd(g, D, F, scale=0.06), rnd(g, D, scale=0.1), 1.0 + rnd(g, D, scale=0.1),
           rnd(g, D, scale=0.1)]
    W = ffn + attn_tensors(g) + attn_tensors(g)
    ptrs = (ctypes.c_void_p * 18)(*(t.data_ptr() for t in W))
    pad = make_pad(g, B, Lk, "scattered")
    ws = workspace(lib.ctrlsim_decoder_layer_grad_workspace_bytes(B, T, A, Lk, F))
    grads = torch.full((2 * D * F + F + 3 * D + 2 * (4 * D * D + 6 * D),), float("nan"), device=DEV)
    dX0, dMem = torch.full((B * L, D), 7.0, device=DEV), rnd(g, B * Lk, D)
    x1, u = torch.full((B * L, D), float("nan"), device=DEV), torch.full((B * L, D), float("nan"), device=DEV)
    _lib.check(lib.ctrlsim_decoder_layer_grad(p(X0), D, p(Mem), D, p(pad), p(dY), D, ptrs, B, T, A, Lk, F, 0, p(ws), p(grads), p(dX0), D, p(dMem),
                                              D, accumulate, p(x1), p(u), st), "decoder_layer_grad")
    return digest(grads, dX0, dMem, x1, u)


def main():
    out, seed = {}, 100
    for shape in CROSS:
        for kind in PADS:
            out["attn-" + "x".join(map(str, shape)) + "-" + kind] = cross(*shape, kind, seed)
            seed += 1
    out["attn-" + "x".join(map(str, CROSS_CHUNKS)) + "-scattered"] = cross(*CROSS_CHUNKS, "scattered", seed)
    for shape in SELF:
        for mode in (0, 1):
            seed += 1
            out["self-" + "x".join(map(str, shape)) + f"-mode{mode}"] = self_attn(*shape, mode, seed)
    for shape in LAYER:
        for accumulate in (0, 1):
            seed += 1
            out["layer-" + "x".join(map(str, shape)) + f"-acc{accumulate}"] = layer(*shape, accumulate, seed)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
