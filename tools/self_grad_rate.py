"""Time of the training step's device part in scope "heads+last_layer" against what it extends: ctrlsim_forward_loss_grad_cross (forward +
loss + head gradients + the last decoder layer's feed-forward block and cross-attention sublayer) and ctrlsim_forward_loss_grad_layer
(+ that layer's causal self-attention sublayer: six tensors + dX0) on the same batch of B full-size windows, trained-like weights, and
the op ctrlsim_self_attn_block_grad alone on rows of the same shape.  Device events around `reps` calls per measurement, all routes
warmed and ALTERNATING in one process, three rounds; prints one JSON line per round and the medians with the workspace bytes.  Recorded
in profiles/self_attn_grad_rate.md, not gated.  `trace` / `trace_cross` as a third argument: `reps` calls of
ctrlsim_forward_loss_grad_layer / ctrlsim_forward_loss_grad_cross only, nothing timed — the runs to put under a kernel trace (the
attention-core kernels sa_fwd / sa_dq / sa_dkv have names of their own; the products and the row sums share theirs with the other
sublayers', so the difference of the two per-kernel tables is what this sublayer's backward adds).

    python tools/self_grad_rate.py [B=64] [reps=10] [trace | trace_cross]
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
    w = weights.generate_trained_like(d, 0)
    model = CtRLSim(cfg, w, device=dev)
    lib, st = _lib.lib(), _lib.stream_ptr()
    base = synth_inputs.random_context(d, 1, B=min(B, 32))
    inp = {k: np.concatenate([v] * ((B + len(v) - 1) // len(v)))[:B] for k, v in base.items()}
    cb = ctx_from_reference_layout(d, inp, d.T, dev)
    sizes = {"forward_loss_grad_cross": model.train_grad_workspace_bytes(B, "heads+ffn+cross"),
             "forward_loss_grad_layer": model.train_grad_workspace_bytes(B, "heads+last_layer"),
             "self_attn_block_grad": int(lib.ctrlsim_self_attn_block_grad_workspace_bytes(B, d.T, d.A))}
    ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
    sums = torch.zeros(5, 2, dtype=torch.float64, device=dev)
    lc = model.loss_cfg(True)
    grads = torch.empty(model.train_grad_layout("heads+last_layer")[1], device=dev)
    rows3 = B * d.T * d.A * 3
    dX = torch.empty(rows3, d.D, device=dev)
    dU, dX1, dX0, x0 = (torch.empty_like(dX) for _ in range(4))
    dMem = torch.empty(B * ((d.P + d.A + 3) & ~3), d.D, device=dev)
    h, ctx = model.hip.handle, C.byref(cb.struct)
    pre = f"decoder.transformer_decoder.layers.{d.ND - 1}"
    six = [torch.from_numpy(np.ascontiguousarray(np.asarray(w[pre + s], np.float32))).to(dev)
           for s in (".self_attn.in_proj_weight", ".self_attn.in_proj_bias", ".self_attn.out_proj.weight", ".self_attn.out_proj.bias",
                     ".norm1.weight", ".norm1.bias")]
    gop = torch.empty(4 * d.D * d.D + 6 * d.D, device=dev)

    def loss_grad_cross():
        _lib.check(lib.ctrlsim_forward_loss_grad_cross(h, B, d.T, ctx, None, C.byref(lc), 1.0, ws.data_ptr(), sums.data_ptr(), None,
                                                       grads.data_ptr(), dX.data_ptr(), None, dU.data_ptr(), None, dX1.data_ptr(),
                                                       dMem.data_ptr(), None, None, st))

    def loss_grad_layer():
        _lib.check(lib.ctrlsim_forward_loss_grad_layer(h, B, d.T, ctx, None, C.byref(lc), 1.0, ws.data_ptr(), sums.data_ptr(), None,
                                                       grads.data_ptr(), dX.data_ptr(), None, dU.data_ptr(), None, dX1.data_ptr(),
                                                       dMem.data_ptr(), None, None, dX0.data_ptr(), x0.data_ptr(), st))

    def op_alone():               # on the layer's own input rows and dX1 of the last loss_grad_layer call
        _lib.check(lib.ctrlsim_self_attn_block_grad(x0.data_ptr(), d.D, dX1.data_ptr(), d.D, *(t.data_ptr() for t in six), B, d.T, d.A,
                                                    int(model.hip.cdims.variant == 4), ws.data_ptr(), gop.data_ptr(),
                                                    dX0.data_ptr(), d.D, st))

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
            (loss_grad_layer if trace == "trace" else loss_grad_cross)()
        torch.cuda.synchronize()
        return
    routes = [("forward_loss_grad_cross_ms", loss_grad_cross), ("forward_loss_grad_layer_ms", loss_grad_layer),
              ("self_attn_block_grad_ms", op_alone)]
    for _, fn in routes:
        timed(fn, 2)
    torch.cuda.synchronize()
    rows = []
    for r in range(3):
        row = {"B": B, "rows": rows3, "reps": reps, "round": r}
        for name, fn in routes:
            row[name] = timed(fn, reps)
        rows.append(row)
        print(json.dumps(row))
    med = {name: float(np.median([r[name] for r in rows])) for name, _ in routes}
    print(json.dumps({"B": B, "token_rows": rows3, "rows_per_context": d.T * d.A * 3,
                      "chunk_contexts": int(lib.ctrlsim_self_attn_block_grad_chunk_contexts(B, d.T, d.A)), "medians_ms": med,
                      "workspace_bytes": sizes,
                      "added_over_forward_loss_grad_cross_ms": med["forward_loss_grad_layer_ms"] - med["forward_loss_grad_cross_ms"]}))


if __name__ == "__main__":
    main()
