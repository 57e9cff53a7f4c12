"""Time of the training step's device part, scope by scope: ctrlsim_forward_loss (forward + loss) and ctrlsim_forward_loss_grads at every
scope from 0 (+ head gradients) up to the one asked for (1: + the last decoder layer's feed-forward block, 2: + its cross-attention
sublayer, 3: + its self-attention sublayer) on the same batch of B full-size windows, trained-like weights.  Each scope takes the gradient
taps it adds (dX; dU; dX1, dMem; dX0 and x0_out), as the per-scope tools this one replaces did.  Device events around `reps` calls per
measurement, all routes warmed and ALTERNATING in one process, three rounds; prints one JSON line per round, then the medians, the
differences between neighbouring scopes and the workspace bytes.  Recorded in profiles/train_grad_rate.md, not gated.
Scope 4 is "heads+decoder" (scope 3, then every earlier decoder layer by recompute), with the taps
dX, dMem and dX0 / x0_out of every layer; its difference to scope 3, divided by ND - 1, is the added time per earlier layer.
Scope 5 is "heads+decoder+encoder" (scope 4, then every scene-encoder layer by recompute), with
scope 4's taps and dE0 / e0_out of every encoder layer; a run that reaches it also writes profiles/encoder_grad_rate.md: the call's time and
workspace against "heads+decoder" at the same B, from this run's medians.  A record, not a gate.
`trace SCOPE`: `reps` calls at that scope only, nothing timed — the run to put under a kernel trace (the difference of two scopes'
per-kernel tables is what the wider one's backward adds).

    python tools/train_grad_rate.py [B=64] [reps=10] [scope=4 | 5 | trace SCOPE]
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

TAPS = (("dX",), ("dU",), ("dX1", "dMem"), ("dX0", "x0_out"))          # added per scope 0..3


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    trace = len(sys.argv) > 3 and sys.argv[3] == "trace"
    top = int(sys.argv[4 if trace else 3]) if len(sys.argv) > (4 if trace else 3) else 4
    cfg = spec.make_cfg()
    d = spec.Dims(cfg)
    dev = "cuda:0"
    model = CtRLSim(cfg, weights.generate_trained_like(d, 0), device=dev)
    lib, st = _lib.lib(), _lib.stream_ptr()
    base = synth_inputs.random_context(d, 1, B=min(B, 32))
    inp = {k: np.concatenate([v] * ((B + len(v) - 1) // len(v)))[:B] for k, v in base.items()}
    cb = ctx_from_reference_layout(d, inp, d.T, dev)
    sizes = {"forward_loss": int(lib.ctrlsim_forward_loss_workspace_bytes(C.byref(model.hip.cdims), B, d.T))}
    names = model.SCOPES + (model.DECODER_SCOPE, model.ENCODER_SCOPE)
    sizes.update({f"scope{s}": model.train_grad_workspace_bytes(B, names[s]) for s in range(top + 1)})
    ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
    sums = torch.zeros(5, 2, dtype=torch.float64, device=dev)
    lc = model.loss_cfg(True)
    grads = torch.empty(model.train_grad_layout(names[top])[1], device=dev)
    rows3, rowsm = B * d.T * d.A * 3, B * ((d.P + d.A + 3) & ~3)
    bufs = {k: torch.empty(rowsm if k == "dMem" else rows3, d.D, device=dev) for ks in TAPS[:top + 1] for k in ks}
    layer_bufs = [torch.empty(rows3, d.D, device=dev) for _ in range(2 * (d.ND - 1) if top >= 4 else 0)]
    enc_bufs = [torch.empty(rowsm, d.D, device=dev) for _ in range(2 * d.NE if top == 5 else 0)]
    taps = []
    for s in range(top + 1):
        t = _lib.TrainTaps(**{k: bufs[k].data_ptr() for ks in TAPS[:min(s, 2) + 1] for k in ks if s < 4 or k in ("dX", "dMem")})
        for l in range(d.ND - 1 if s == 3 else 0 if s >= 4 else d.ND, d.ND):
            t.dX0[l] = (bufs["dX0"] if l == d.ND - 1 else layer_bufs[2 * l]).data_ptr()
            t.x0_out[l] = (bufs["x0_out"] if l == d.ND - 1 else layer_bufs[2 * l + 1]).data_ptr()
        for l in range(d.NE if s == 5 else 0):
            t.dE0[l], t.e0_out[l] = enc_bufs[2 * l].data_ptr(), enc_bufs[2 * l + 1].data_ptr()
        taps.append(t)
    h, ctx = model.hip.handle, C.byref(cb.struct)

    def loss_only():
        _lib.check(lib.ctrlsim_forward_loss(h, B, d.T, ctx, None, C.byref(lc), ws.data_ptr(), sums.data_ptr(), None, None, st))

    def loss_grads(s):
        return lambda: _lib.check(lib.ctrlsim_forward_loss_grads(h, B, d.T, ctx, None, C.byref(lc), 1.0, s, ws.data_ptr(), sums.data_ptr(),
                                                                 None, grads.data_ptr(), C.byref(taps[s]), st))

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
            loss_grads(top)()
        torch.cuda.synchronize()
        return
    routes = [("forward_loss_ms", loss_only)] + [(f"scope{s}_ms", loss_grads(s)) for s in range(top + 1)]
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
    order = [name for name, _ in routes]
    out = {"B": B, "token_rows": rows3, "memory_rows": rowsm, "medians_ms": med, "workspace_bytes": sizes,
           "added_ms": {f"{b[:-3]}_over_{a[:-3]}": med[b] - med[a] for a, b in zip(order, order[1:])}}
    if top >= 4 and d.ND > 1:
        out["added_ms_per_earlier_layer"] = (med["scope4_ms"] - med["scope3_ms"]) / (d.ND - 1)
    if top == 5:
        out["added_ms_per_encoder_layer"] = (med["scope5_ms"] - med["scope4_ms"]) / max(d.NE, 1)
        write_encoder_record(out, d, reps)
    print(json.dumps(out))


def write_encoder_record(out, d, reps):
    med, sz = out["medians_ms"], out["workspace_bytes"]
    lines = ["# Training (e): the encoder scope's call against \"heads+decoder\"", "",
             f"`python tools/train_grad_rate.py {out['B']} {reps} 5` on one MI355X: trained-like weights, full-size windows, B = {out['B']}",
             f"({out['token_rows']} token rows, {out['memory_rows']} scene rows, ND = {d.ND}, NE = {d.NE}).  Medians of three rounds of {reps} calls,",
             "all routes warmed and alternating in one process; both scopes measured in the same run.  A record, not a gate.", "",
             "| call | ms | workspace bytes |", "|---|---|---|",
             f"| ctrlsim_forward_loss_grads, scope 4 (\"heads+decoder\") | {med['scope4_ms']:.3f} | {sz['scope4']} |",
             f"| ctrlsim_forward_loss_grads, scope 5 (\"heads+decoder+encoder\") | {med['scope5_ms']:.3f} | {sz['scope5']} |", "",
             f"The encoder layers add {med['scope5_ms'] - med['scope4_ms']:.3f} ms ({out['added_ms_per_encoder_layer']:.3f} ms per layer, "
             f"{100 * (med['scope5_ms'] / med['scope4_ms'] - 1):.2f} % of the decoder scope's call) and "
             f"{sz['scope5'] - sz['scope4']} bytes of workspace ({100 * (sz['scope5'] / sz['scope4'] - 1):.2f} %).", "",
             "```", json.dumps(out), "```", ""]
    with open(os.path.join(ROOT, "profiles", "encoder_grad_rate.md"), "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
