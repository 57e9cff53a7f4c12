"""Open-loop windows per second, window build included, on synthetic full-dim scenes: the host route (ingest.training_window per window ->
OpenLoopEvaluator.collate -> CtRLSim.loss_sums, which uploads) against the device route (DeviceDataset.validate + windows.launch_windows: ctrlsim_window_build ->
CtRLSim.loss_sums_ctx) on the SAME triples of the SAME logged batch (LogReplayer -> dataset(); the device route wraps its tensors with
device_dataset(), the host route reads them back into dictionaries first — outside the timing).
usage: python tools/window_rate.py [S=8] [N=32] [steps=90] [B=256] [rounds=3] [polylines=512]
Both routes are warmed and alternate in one process; every round prints its own wall-clock rates (one synchronisation at the end of each
route's batch), and, for the device route's batch, the device-event time of the build alone next to the loss call's."""
import json
import sys
import time

sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np
import torch
import ctrlsim_amd  # noqa: F401
from ctrlsim_amd import spec, scenarios, datagen, ingest, weights
from ctrlsim_amd.evaluators import OpenLoopEvaluator
from ctrlsim_amd.models import CtRLSim
from ctrlsim_amd.engine import CtxBuffers
from ctrlsim_amd.windows import launch_windows

arg = lambda i, default: int(sys.argv[i]) if len(sys.argv) > i else default
S, N, STEPS, B, ROUNDS, POLYS = arg(1, 8), arg(2, 32), arg(3, 90), arg(4, 256), arg(5, 3), arg(6, 512)

cfg = spec.make_cfg(nocturne__steps=STEPS)
d = spec.Dims(cfg)
dev = "cuda:0"
t0 = time.perf_counter()
scns = [scenarios.make_scenario(17, k, n_agents=N, n_polylines=POLYS, n_points=d.NP, extent=60.0) for k in range(S)]
logs = [scenarios.standin_log(s, STEPS + 1) for s in scns]
rp = datagen.LogReplayer(cfg, dev).load(scns, logs, STEPS)
rp.run()
out = rp.dataset()
ds = rp.device_dataset(out, scns)
dicts = datagen.read_back(rp, out, scns)
print(f"{S} scenes x {N} vehicles x {STEPS} steps, {POLYS} polylines x {d.NP} points per scene; windows of T = {d.T}, A = {d.A}, "
      f"P = {d.P}; batches of {B}; dataset on the device in {time.perf_counter() - t0:.1f} s")
model = CtRLSim(cfg, weights.generate_trained_like(d, 0), device=dev)


def triples(seed):
    tr = [(k % S,) + ds.choices(k % S, seed * 100003 + k) for k in range(B)]
    return np.array(tr)


def host_route(tr):
    t0 = time.perf_counter()
    wins = [ingest.training_window(dicts[s], cfg, t, a) for s, t, a in tr]
    t1 = time.perf_counter()
    sums = model.loss_sums(OpenLoopEvaluator.collate(wins))[0]
    back = sums.cpu().numpy()
    t2 = time.perf_counter()
    return back, dict(windows_per_s=len(tr) / (t2 - t0), cut_s=t1 - t0, collate_upload_loss_s=t2 - t1)


CB = CtxBuffers(d, B, dev)                                              # reused, as OpenLoopEvaluator.evaluate_dataset reuses its own


def device_route(tr):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t0 = time.perf_counter()
    scn, t, a = ds.validate(tr[:, 0], tr[:, 1], tr[:, 2])
    up = lambda x: torch.from_numpy(x).to(dev)
    scn, t, a = up(scn), up(t), up(a)
    ev[0].record()                                                      # the launch alone: triples validated and uploaded
    cb, moving, status = launch_windows(ds, scn, t, a, len(tr), out=CB)
    ev[1].record()
    sums = model.loss_sums_ctx(cb, moving, len(tr))[0]
    ev[2].record()
    back = sums.cpu().numpy()
    t1 = time.perf_counter()
    assert int(status.abs().sum()) == 0
    return back, dict(windows_per_s=len(tr) / (t1 - t0), build_event_ms=ev[0].elapsed_time(ev[1]), loss_event_ms=ev[1].elapsed_time(ev[2]))


for route in (host_route, device_route):                                # warm: first launches, allocations, the model's handle
    route(triples(0)[:min(B, 8)])
    route(triples(0))
rows = []
for r in range(ROUNDS):
    tr = triples(r + 1)
    hs, h = host_route(tr)
    dsum, g = device_route(tr)
    assert np.array_equal(hs[:, 1], dsum[:, 1]), "the two routes scored different rows"
    rel = float(np.abs(hs[:, 0] - dsum[:, 0]).max() / np.abs(hs[:, 0]).max())
    rows.append(dict(round=r, host=h, device=g, largest_relative_difference_of_the_sums=rel))
    print(json.dumps(rows[-1]))
hm, dm = np.median([x["host"]["windows_per_s"] for x in rows]), np.median([x["device"]["windows_per_s"] for x in rows])
bm, lm = np.median([x["device"]["build_event_ms"] for x in rows]), np.median([x["device"]["loss_event_ms"] for x in rows])
print(f"medians: host route {hm:.0f} windows/s ({1e3 / hm:.3f} ms per window), device route {dm:.0f} windows/s; "
      f"build {bm:.3f} ms against loss {lm:.3f} ms per batch of {B} ({100 * bm / lm:.2f} %)")
