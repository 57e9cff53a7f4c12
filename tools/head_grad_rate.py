"""Time of the training step's device part against the open-loop loss it extends: ctrlsim_forward_loss (forward + loss) and
ctrlsim_forward_loss_grad (forward + loss + head gradients + dX) on the same batch of B full-size windows, trained-like weights.
Device events around `reps` calls per measurement, both entries warmed and ALTERNATING in one process, three rounds; prints one JSON
line per round and the medians.  Recorded in profiles/head_grad_rate.md, not gated.

    python tools/head_grad_rate.py [B=64] [reps=10]
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
    cfg = spec.make_cfg()
    d = spec.Dims(cfg)
    dev = "cuda:0"
    model = CtRLSim(cfg, weights.generate_trained_like(d, 0), device=dev)
    lib, st = _lib.lib(), _lib.stream_ptr()
    base = synth_inputs.random_context(d, 1, B=min(B, 32))
    inp = {k: np.concatenate([v] * ((B + len(v) - 1) // len(v)))[:B] for k, v in base.items()}
    cb = ctx_from_reference_layout(d, inp, d.T, dev)
    has_grad = hasattr(lib, "ctrlsim_forward_loss_grad")
    n_loss = int(lib.ctrlsim_forward_loss_workspace_bytes(C.byref(model.hip.cdims), B, d.T))
    n_grad = model.head_grad_workspace_bytes(B) if has_grad else n_loss
    ws = torch.empty(max(n_loss, n_grad), dtype=torch.uint8, device=dev)
    sums = torch.zeros(5, 2, dtype=torch.float64, device=dev)
    lc = model.loss_cfg(True)
    total = model.head_grad_layout()[1] if has_grad else 1
    grads = torch.empty(total, device=dev)
    dX = torch.empty(B * d.T * d.A * 3, d.D, device=dev)

    def loss_only(n):
        for _ in range(n):
            sums.zero_()
            _lib.check(lib.ctrlsim_forward_loss(model.hip.handle, B, d.T, C.byref(cb.struct), None, C.byref(lc), ws.data_ptr(),
                                                sums.data_ptr(), None, None, st))

    def loss_grad(n):
        for _ in range(n):
            sums.zero_()
            _lib.check(lib.ctrlsim_forward_loss_grad(model.hip.handle, B, d.T, C.byref(cb.struct), None, C.byref(lc), 1.0, ws.data_ptr(),
                                                     sums.data_ptr(), None, grads.data_ptr(), dX.data_ptr(), None, st))

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(n)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    routes = [("forward_loss_ms", loss_only)] + ([("forward_loss_grad_ms", loss_grad)] if has_grad else [])
    for _, fn in routes:
        fn(2)
    torch.cuda.synchronize()
    rows = []
    for r in range(3):
        row = {"B": B, "rows": B * d.T * d.A, "reps": reps, "round": r}
        for name, fn in routes:
            row[name] = timed(fn, reps)
        rows.append(row)
        print(json.dumps(row))
    med = {name: float(np.median([r[name] for r in rows])) for name, _ in routes}
    out = {"B": B, "medians_ms": med, "workspace_bytes": {"forward_loss": n_loss, "forward_loss_grad": n_grad}}
    if has_grad:
        out["added_ms"] = med["forward_loss_grad_ms"] - med["forward_loss_ms"]
        out["added_over_forward_loss"] = out["added_ms"] / med["forward_loss_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
