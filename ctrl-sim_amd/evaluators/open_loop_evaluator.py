"""Open-loop evaluation of a checkpoint on logged windows: the reference's validation loop (CtRLSim.validation_step over a
DataLoader, models/ctrl_sim.py:217-228: Lightning averages the per-batch values weighted by batch size) as ONE pass that accumulates
sums and counts on the device — exact for any batching and any sharding, which a mean of per-batch means is not when the masks differ."""
from __future__ import annotations

import time

import numpy as np
import torch

from ..dist import allreduce_loss_sums

AGENT_KEYS = ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask")
MAP_KEYS = ("road_points", "road_types")


class OpenLoopEvaluator:
    """OpenLoopEvaluator(cfg, model).evaluate(windows) -> dict.

    windows: a sequence of reference-layout windows WITHOUT the batch axis — mappings with agent_states [A,T,8], agent_types [A,5],
    goals [A,5], actions [A,T], rtgs [A,T,3], timesteps [A,T,1], moving_agent_mask [A], road_points [P,NP,3], road_types [P,8] (one
    sample of the reference's dataset, datasets/rl_waymo/dataset_ctrl_sim.py:140-160).  Rank r of a world of W scores windows r, r + W,
    ...; the ten doubles are all-reduced once at the end."""

    def __init__(self, cfg, model, fused=True, workspace_bytes=64 << 30, max_batch=1024):
        self.cfg, self.model, self.fused = cfg, model, fused
        self.workspace_bytes, self.max_batch = int(workspace_bytes), int(max_batch)
        self.device = model.device

    def batch_size(self):
        """The largest number of windows per call whose workspace (ctrlsim_forward_loss_workspace_bytes) fits the budget."""
        import ctypes as C
        from .. import _lib
        lib, hip = _lib.lib(), self.model.hip
        need = lambda b: int(lib.ctrlsim_forward_loss_workspace_bytes(C.byref(hip.cdims), b, self.model.dims.T))
        lo, hi = 1, self.max_batch
        if need(1) > self.workspace_bytes:
            raise MemoryError(f"one window needs {need(1)} bytes of workspace, the budget is {self.workspace_bytes}")
        while lo < hi:                       # the query is monotonic in B
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if need(mid) <= self.workspace_bytes else (lo, mid - 1)
        return lo

    @staticmethod
    def collate(windows):
        g = lambda k: np.stack([np.asarray(w[k]) for w in windows])
        return {"agent": {k: g(k) for k in AGENT_KEYS}, "map": {k: g(k) for k in MAP_KEYS}}

    def score(self, data):
        """[5, 2] float64 (sum, count) per term of one collated batch, on self.device."""
        return self.model.loss_sums(data, fused=self.fused)[0]

    def evaluate(self, windows, batch_size=None):
        import torch.distributed as dist
        on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
        mine = [windows[i] for i in range(rank, len(windows), world)]
        B = batch_size or self.batch_size()
        total = torch.zeros(5, 2, dtype=torch.float64, device=self.device)
        t0 = time.perf_counter()
        for i in range(0, len(mine), B):
            total += self.score(self.collate(mine[i:i + B]))
        dt = time.perf_counter() - t0
        allreduce_loss_sums(total)
        sums = total.cpu().numpy()                                   # the one copy
        out = dict(self.model.losses_from_sums(sums))
        out["counts"] = {k: float(sums[self.model.LOSS_KEYS.index(k), 1]) for k in self.model.loss_keys()}
        out["sums"] = sums
        out["windows"] = len(windows)
        out["windows_per_s"] = len(mine) / dt if dt > 0 else float("nan")       # this rank's rate
        return out

    def evaluate_dataset(self, ds, triples, batch_size=None):
        """evaluate() for windows named by (scene, first step, origin agent) triples of a windows.DeviceDataset: the windows are built
        on the device (windows.build_windows: ctrlsim_window_build) and scored where they lie, so `windows_per_s` includes the build.
        Every triple is validated on the host first (ValueError, the messages of ingest.training_window); rank r of a world of W takes
        triples r, r + W, ...; the ten doubles are all-reduced once and come back in the one copy, together with this rank's count of
        windows the kernel itself refused (a non-zero count raises)."""
        import torch.distributed as dist
        from ..engine import CtxBuffers
        from ..windows import launch_windows
        tr = np.asarray(triples, np.int64).reshape(-1, 3)
        scn, t0, agent = ds.validate(tr[:, 0], tr[:, 1], tr[:, 2])
        on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a[rank::world])).to(self.device)
        scn_d, t0_d, agent_d = up(scn), up(t0), up(agent)
        n_mine = int(scn_d.shape[0])
        B = batch_size or self.batch_size()
        total = torch.zeros(5, 2, dtype=torch.float64, device=self.device)
        refused = torch.zeros(1, dtype=torch.float64, device=self.device)
        cb = CtxBuffers(self.model.dims, max(1, min(B, n_mine)), self.device)
        t_start = time.perf_counter()
        for i in range(0, n_mine, B):
            n = min(B, n_mine - i)
            _, moving, status = launch_windows(ds, scn_d[i:i + n], t0_d[i:i + n], agent_d[i:i + n], n, out=cb)
            total += self.model.loss_sums_ctx(cb, moving, n, fused=self.fused)[0]
            refused += (status != 0).sum()
        allreduce_loss_sums(total)
        back = torch.cat([total.reshape(-1), refused]).cpu().numpy()             # the one copy (it waits for the queue)
        dt = time.perf_counter() - t_start
        if back[10] != 0:
            raise RuntimeError(f"{int(back[10])} windows were refused by ctrlsim_window_build after the host tables had accepted them")
        sums = back[:10].reshape(5, 2)
        out = dict(self.model.losses_from_sums(sums))
        out["counts"] = {k: float(sums[self.model.LOSS_KEYS.index(k), 1]) for k in self.model.loss_keys()}
        out["sums"] = sums
        out["windows"] = len(tr)
        out["windows_per_s"] = n_mine / dt if dt > 0 else float("nan")          # this rank's rate, window build included
        return out
