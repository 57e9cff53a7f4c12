"""Open-loop evaluation throughput: OpenLoopEvaluator on the fused route (cross-entropy epilogue, no logits) against the from-memory
route (generic Linear + row kernel), full dims, trained-like weights.  Device events around >= 1 s of work per measurement, both
routes warmed and ALTERNATING in one process; peak device memory per route.  Recorded in profiles/loss_bench.md, not gated.

    python tools/bench_loss.py [--batches 256,0] [--seconds 1.0] [--rounds 3]        (0 = the largest batch whose workspace fits 64 GB)
"""
import argparse
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
from ctrlsim_amd.evaluators import OpenLoopEvaluator  # noqa: E402
import synth_inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,0")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    cfg = spec.make_cfg()
    d = spec.Dims(cfg)
    dev = "cuda:0"
    model = CtRLSim(cfg, weights.generate_trained_like(d, 0), device=dev)
    lib, st = _lib.lib(), _lib.stream_ptr()
    rows = []
    for B in [int(b) for b in a.batches.split(",")]:
        if B == 0:
            B = OpenLoopEvaluator(cfg, model, workspace_bytes=64 << 30, max_batch=4096).batch_size()
        base = synth_inputs.random_context(d, 1, B=min(B, 32))
        inp = {k: np.concatenate([v] * ((B + len(v) - 1) // len(v)))[:B] for k, v in base.items()}
        cb = ctx_from_reference_layout(d, inp, d.T, dev)
        nbytes = int(lib.ctrlsim_forward_loss_workspace_bytes(C.byref(model.hip.cdims), B, d.T))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        sums = torch.zeros(5, 2, dtype=torch.float64, device=dev)

        def run(fused, n):
            lc = model.loss_cfg(fused)
            for _ in range(n):
                _lib.check(lib.ctrlsim_forward_loss(model.hip.handle, B, d.T, C.byref(cb.struct), None, C.byref(lc), ws.data_ptr(),
                                                    sums.data_ptr(), None, None, st))

        def timed(fused, n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(fused, n)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3

        for f in (True, False):                                         # every shape warmed on both routes
            run(f, 2)
        torch.cuda.synchronize()
        n = max(1, int(np.ceil(a.seconds / (timed(True, 2) / 2))))
        res = {True: [], False: []}
        for _ in range(a.rounds):                                       # the two routes alternate
            for f in (True, False):
                res[f].append(B * n / timed(f, n))
        # what the from-memory route would hold if the caller went through ctrlsim_forward_all: the logits of every token
        logits_bytes = B * d.T * d.A * (d.V + d.R * d.C) * 4
        rows.append({"B": B, "calls_per_measurement": n, "workspace_bytes": nbytes, "forward_all_logits_bytes": logits_bytes,
                     "fused_windows_per_s": res[True], "memory_windows_per_s": res[False],
                     "fused_median": float(np.median(res[True])), "memory_median": float(np.median(res[False])),
                     "peak_allocated_bytes": int(torch.cuda.max_memory_allocated())})
        print(json.dumps(rows[-1]))
        del ws, cb
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()


if __name__ == "__main__":
    main()
