"""Time of the training step's device part in scope "heads+ffn+cross" against what it extends: ctrlsim_forward_loss_grad_ffn (forward +
loss + head gradients + the last decoder layer's feed-forward block) and ctrlsim_forward_loss_grad_cross (+ that layer's cross-attention
sublayer: six tensors + dX1 + dMem) on the same batch of B full-size windows, trained-like weights.  Device events around `reps` calls
per measurement, both entries warmed and ALTERNATING in one process, three rounds; prints one JSON line per round and the medians.
Recorded in profiles/attn_grad_rate.md, not gated.  `trace` / `trace_ffn` as a third argument: `reps` calls of
ctrlsim_forward_loss_grad_cross / ctrlsim_forward_loss_grad_ffn only, nothing timed — the runs to put under a kernel trace (the
attention-core kernels have names of their own; the products and the row sums share theirs with the feed-forward block's, so the
difference of the two per-kernel tables is what the sublayer's backward adds).

    python tools/cross_grad_rate.py [B=64] [reps=10] [trace | trace_ffn]
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

from ctrlsim_amd import spec, weights, _lib  # noqa: E402
from ctrlsim_amd.models import CtRLSim  # noqa: E402
from ctrlsim_amd.engine import ctx_from_reference_layout  # noqa: E402
import synth_inputs  # noqa: E402


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    trace = sys.argv[3] if len(sys.argv) > 3 else ""
    cfg = spec.make_cfg()
    d = spec.Dims(cfg)
    dev = "cuda:0"
    model = CtRLSim(cfg, weights.generate_trained_like(d, 0), device=dev)
    lib, st = _lib.lib(), _lib.stream_ptr()
    base = synth_inputs.random_context(d, 1, B=min(B, 32))
    inp = {k: np.concatenate([v] * ((B + len(v) - 1) // len(v)))[:B] for k, v in base.items()}
    cb = ctx_from_reference_layout(d, inp, d.T, dev)
    sizes = {"forward_loss_grad_ffn": model.train_grad_workspace_bytes(B),
             "forward_loss_grad_cross": model.train_grad_workspace_bytes(B, "heads+ffn+cross")}
    ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
    sums = torch.zeros(5, 2, dtype=torch.float64, device=dev)
    lc = model.loss_cfg(True)
    grads = torch.empty(model.train_grad_layout("heads+ffn+cross")[1], device=dev)
    dX = torch.empty(B * d.T * d.A * 3, d.D, device=dev)
    dU = torch.empty_like(dX)
    dX1 = torch.empty_like(dX)
    dMem = torch.empty(B * ((d.P + d.A + 3) & ~3), d.D, device=dev)
    h, ctx = model.hip.handle, C.byref(cb.struct)

    def loss_grad_ffn():
        _lib.check(lib.ctrlsim_forward_loss_grad_ffn(h, B, d.T, ctx, None, C.byref(lc), 1.0, ws.data_ptr(), sums.data_ptr(), None,
                                                     grads.data_ptr(), dX.data_ptr(), None, dU.data_ptr(), None, st))

    def loss_grad_cross():
        _lib.check(lib.ctrlsim_forward_loss_grad_cross(h, B, d.T, ctx, None, C.byref(lc), 1.0, ws.data_ptr(), sums.data_ptr(), None,
                                                       grads.data_ptr(), dX.data_ptr(), None, dU.data_ptr(), None, dX1.data_ptr(),
                                                       dMem.data_ptr(), None, None, st))

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            sums.zero_()
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    if trace:
        for _ in range(reps):
            sums.zero_()
            (loss_grad_cross if trace == "trace" else loss_grad_ffn)()
        torch.cuda.synchronize()
        return
    routes = [("forward_loss_grad_ffn_ms", loss_grad_ffn), ("forward_loss_grad_cross_ms", loss_grad_cross)]
    for _, fn in routes:
        timed(fn, 2)
    torch.cuda.synchronize()
    rows = []
    for r in range(3):
        row = {"B": B, "rows": B * d.T * d.A * 3, "reps": reps, "round": r}
        for name, fn in routes:
            row[name] = timed(fn, reps)
        rows.append(row)
        print(json.dumps(row))
    med = {name: float(np.median([r[name] for r in rows])) for name, _ in routes}
    print(json.dumps({"B": B, "query_rows": B * d.T * d.A * 3, "memory_rows": B * ((d.P + d.A + 3) & ~3), "medians_ms": med,
                      "workspace_bytes": sizes,
                      "added_over_forward_loss_grad_ffn_ms": med["forward_loss_grad_cross_ms"] - med["forward_loss_grad_ffn_ms"]}))


if __name__ == "__main__":
    main()
