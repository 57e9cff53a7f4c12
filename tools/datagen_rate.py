"""Throughput of offline-RL dataset generation (ctrlsim_amd/datagen.py): scenes per second of the device route (generate: LogReplayer.run +
csrc/dataset.hip + one read-back) and of the host route (generate_host: host-driven stepping + the NumPy host forms per scene), on
synthetic scenes with stand-in logs, at the same shape in the same run.
usage: python tools/datagen_rate.py [scenes=64] [agents=16] [steps=90] [host | device | both] [repeats=2] [polylines=200]
The device route's split comes from HIP events around the replay loop, the edge-distance kernel and the other dataset kernels; read-back
and host assembly from the wall clock.  Every repeat prints its own rate."""
import sys
import time

sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np
import torch
import ctrlsim_amd  # noqa: F401
from ctrlsim_amd import spec, scenarios, datagen

S = int(sys.argv[1]) if len(sys.argv) > 1 else 64
N = int(sys.argv[2]) if len(sys.argv) > 2 else 16
T = int(sys.argv[3]) if len(sys.argv) > 3 else 90
MODE = sys.argv[4] if len(sys.argv) > 4 else "both"
assert MODE in ("host", "device", "both"), MODE
REPEATS = int(sys.argv[5]) if len(sys.argv) > 5 else 2
P = int(sys.argv[6]) if len(sys.argv) > 6 else 200

cfg = spec.make_cfg(nocturne__steps=T)
NP = int(cfg.dataset.waymo.max_num_road_pts_per_polyline)
t0 = time.perf_counter()
scns = [scenarios.make_scenario(7, k, n_agents=N, n_polylines=P, n_points=NP, extent=60.0) for k in range(S)]
logs = [scenarios.standin_log(s, T + 1) for s in scns]
segs = np.array([len(s.edge_segments) for s in scns])
print(f"{S} scenes x {N} vehicles x {T} steps, {P} polylines per scene ({segs.mean():.0f} road-edge segments on average, "
      f"{S * N * T * segs.mean():.3g} point-segment pairs), built in {time.perf_counter() - t0:.1f} s")
warm = [scns[:2], logs[:2], min(T, 4)]


def timed_generate():
    """datagen.generate() step by step with HIP events around its three device phases -> (dictionaries, seconds by phase)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t0 = time.perf_counter()
    rp = datagen.LogReplayer(cfg).load(scns, logs, T)
    t1 = time.perf_counter()
    ev[0].record(); rp.run()
    d = rp.dataset_buffers()
    ev[1].record(); rp.dataset_edge_distance(d)
    ev[2].record(); rp.dataset_rewards(d)
    ev[3].record()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out = datagen.read_back(rp, d, scns)
    t3 = time.perf_counter()
    ms = [a.elapsed_time(b) * 1e-3 for a, b in zip(ev[:-1], ev[1:])]
    return out, dict(upload=t1 - t0, replay_loop=ms[0], edge_distance=ms[1], rewards_rtgs=ms[2], device_total_wall=t2 - t1,
                     read_back_and_assembly=t3 - t2)


if MODE in ("device", "both"):
    datagen.generate(cfg, *warm)                                     # first launches, allocations
    for rep in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, timing = timed_generate()
        el = time.perf_counter() - t0
        print(f"device route: {el:.3f} s = {S / el:.1f} scenes/s ({S * N * T / el:.0f} vehicle-steps/s); seconds by phase: "
              + ", ".join(f"{k} {v:.4f}" for k, v in timing.items()))
        pairs = S * N * T * segs.mean()
        print(f"  edge-distance kernel: {pairs / timing['edge_distance'] / 1e9:.1f} G point-segment pairs/s")
if MODE in ("host", "both"):
    datagen.generate_host(cfg, *warm)
    for rep in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = datagen.generate_host(cfg, scns, logs, T)
        el = time.perf_counter() - t0
        print(f"host route: {el:.3f} s = {S / el:.1f} scenes/s ({S * N * T / el:.0f} vehicle-steps/s)")
