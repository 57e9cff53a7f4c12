"""Open-loop training windows built on the device: logged scenes -> dataset -> windows -> loss without the dataset leaving HBM.

`ingest.training_window` cuts one window at a time in NumPy (the reference's training-mode get_data, dataset_ctrl_sim.py:99-160),
`OpenLoopEvaluator.collate` stacks them and `engine.ctx_from_reference_layout` transposes, casts and uploads them.  Here a
`DeviceDataset` keeps the `*_physics.pkl` arrays of a batch of scenes (equal vehicle count N <= 64, equal step count Td) on the
device — packed from loaded dictionaries (`from_dicts`) or wrapped around the tensors `LogReplayer.dataset()` left there
(`LogReplayer.device_dataset`) — and `build_windows` cuts B windows per launch (csrc/window.hip: ctrlsim_window_build) straight into
the context tensors `ctrlsim_forward_loss` reads.  What stays on the host are the small tables the reference's two random draws and
its refusals need: existence per step, the moving mask, `max_t` and the filtered ids per scene.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ingest
from .spec import Dims

def window_cfg(cfg):
    """ctrlsim_window_cfg of a configuration (cfg.dataset.waymo; continuous returns for a Decision-Transformer model)."""
    w = cfg.dataset.waymo
    return _lib.WindowCfg(agent_dist_threshold=w.agent_dist_threshold, moving_threshold=w.moving_threshold,
                          rtg_lo=(C.c_double * 3)(w.min_rtg_pos, w.min_rtg_veh, w.min_rtg_road),
                          rtg_hi=(C.c_double * 3)(w.max_rtg_pos, w.max_rtg_veh, w.max_rtg_road),
                          min_accel=w.min_accel, max_accel=w.max_accel, min_steer=w.min_steer, max_steer=w.max_steer,
                          rtg_discretization=int(w.rtg_discretization), accel_discretization=int(w.accel_discretization),
                          steer_discretization=int(w.steer_discretization),
                          continuous_rtg=int(bool(cfg.model.get("decision_transformer", False))))


class DeviceDataset:
    """The dictionaries of S scenes as device tensors (float64, the dictionary's values): ag_data [S,N,Td,8], actions [S,N,Td,2],
    rtgs [S,N,Td,5], goals5 [S,N,5], types [S,N,5], road_points [S,Pmax,NP,3], road_types [S,Pmax,8], n_polys [S] i32; host tables:
    exist [S,N,Td] bool, moving [S,N] bool, last_exist [S,N], max_t [S], filtered [S] -> ascending ids of the agents that exist at
    step 0."""

    def __init__(self, cfg, ag_data, actions, rtgs, goals5, types, road_points, road_types, n_polys, exist, xy0, last_exist=None):
        self.cfg, self.w, self.dims = cfg, cfg.dataset.waymo, Dims(cfg)
        self.ag_data, self.actions, self.rtgs, self.goals5, self.types = ag_data, actions, rtgs, goals5, types
        self.road_points, self.road_types, self.n_polys = road_points, road_types, n_polys
        self.device = ag_data.device
        self.S, self.N, self.Td = (int(v) for v in ag_data.shape[:3])
        self.Pmax, self.NP = int(road_points.shape[1]), int(road_points.shape[2])
        T = int(self.w.train_context_length)
        if not (1 <= self.N <= 64 and self.Td >= T):
            raise ValueError(f"a batch holds scenes of equal vehicle count N <= 64 and step count >= {T}: got N = {self.N}, steps = {self.Td}")
        if self.NP != self.dims.NP:
            raise ValueError(f"polylines of {self.NP} points, the configuration says {self.dims.NP}")
        for name, t, shape in (("ag_data", ag_data, (self.S, self.N, self.Td, 8)), ("actions", actions, (self.S, self.N, self.Td, 2)),
                               ("rtgs", rtgs, (self.S, self.N, self.Td, 5)), ("goals5", goals5, (self.S, self.N, 5)),
                               ("types", types, (self.S, self.N, 5)), ("road_points", road_points, (self.S, self.Pmax, self.NP, 3)),
                               ("road_types", road_types, (self.S, self.Pmax, 8))):
            if tuple(t.shape) != shape or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError(f"{name}: expected a contiguous float64 tensor of shape {shape}, got {tuple(t.shape)} {t.dtype}")
        if tuple(n_polys.shape) != (self.S,) or n_polys.dtype != torch.int32:
            raise ValueError("n_polys: expected int32 [S]")
        # ---- the host tables (ingest._window_tables per scene)
        self.exist = np.asarray(exist) != 0                                                # [S,N,Td]
        self.exist_is_one = np.asarray(exist) == 1
        goals_h = goals5.cpu().numpy()[:, :, :2]
        self.moving = np.linalg.norm(np.asarray(xy0, np.float64) - goals_h, axis=2) > self.w.moving_threshold
        there = self.exist[:, :, 0]
        if last_exist is None:                                                             # datagen._scene_dict's rule
            last_exist = np.where(there, self.Td - 1 - np.argmax(self.exist_is_one[:, :, ::-1], axis=2), -1)
        self.last_exist = np.asarray(last_exist, np.int64)
        self.filtered = [np.where(there[s])[0] for s in range(self.S)]
        self.n_polys_h = n_polys.cpu().numpy()
        # a scene without a moving agent has no valid window (the host form's np.max raises there): max_t = -1
        self.max_t = np.array([max(0, int(self.last_exist[s][self.moving[s]].max()) - (T - 1)) if self.moving[s].any() else -1
                               for s in range(self.S)], np.int64)
        self.wcfg = window_cfg(cfg)

    @classmethod
    def from_dicts(cls, cfg, dicts, device="cuda:0"):
        """Pack loaded `*_physics.pkl` dictionaries (ingest.preprocess_scene / datagen.generate) of equal N and Td; polylines are
        padded to the largest count of the batch.  A dictionary without `rtgs` gets them from ingest.load_preprocessed."""
        w = cfg.dataset.waymo
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        ag = [f64(d["ag_data"]) for d in dicts]
        if len({a.shape for a in ag}) != 1:
            raise ValueError("one batch = dictionaries of equal vehicle and step count")
        for k, d in enumerate(dicts):
            if list(d["filtered_ag_ids"]) != list(np.where(ag[k][:, 0, 7] != 0)[0]):
                raise ValueError(f"dictionary {k}: filtered_ag_ids are not the agents that exist at step 0")
        rtgs = [f64(d["rtgs"]) if "rtgs" in d else f64(ingest.load_preprocessed(d, w)["rtgs"]) for d in dicts]
        rp = [f64(d["road_points"]) for d in dicts]
        rt = [f64(d["road_types"]) for d in dicts]
        NP = int(w.max_num_road_pts_per_polyline)
        Pmax = max(len(p) for p in rp)
        road_points, road_types = np.zeros((len(dicts), Pmax, NP, 3)), np.zeros((len(dicts), Pmax, 8))
        for k, (p, t) in enumerate(zip(rp, rt)):
            road_points[k, :len(p)] = p.reshape(len(p), NP, 3)
            road_types[k, :len(p)] = t
        dev = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)
        ag = np.stack(ag)
        return cls(cfg, dev(ag), dev(np.stack([f64(d["ag_actions"]) for d in dicts])), dev(np.stack(rtgs)),
                   dev(np.stack([f64(d["ag_goals"])[:, 0] for d in dicts])), dev(np.stack([f64(d["ag_types"]) for d in dicts])),
                   dev(road_points), dev(road_types), dev([len(p) for p in rp], np.int32), ag[..., 7], ag[:, :, 0, :2],
                   last_exist=np.stack([np.asarray(d["last_exist_timesteps"]) for d in dicts]))

    def scene_dict(self, s):
        """Scene s sliced back into the dictionary's arrays (a read-back: tests and tools)."""
        n = int(self.n_polys_h[s])
        h = lambda t: t[s].cpu().numpy()
        return dict(ag_data=h(self.ag_data), ag_actions=h(self.actions), rtgs=h(self.rtgs), ag_types=h(self.types),
                    ag_goals=np.repeat(h(self.goals5)[:, None], self.Td, 1), road_points=h(self.road_points)[:n],
                    road_types=h(self.road_types)[:n], filtered_ag_ids=[int(i) for i in self.filtered[s]],
                    last_exist_timesteps=self.last_exist[s].copy())

    # ------------------------------------------------------------------ the reference's two draws and its refusals
    def choices(self, scene, seed):
        """ingest.window_choices(dict, cfg, seed) of scene `scene`: (origin_t, origin_agent)."""
        rs = np.random.RandomState(seed)
        fil = self.filtered[scene]
        origin_t = int(rs.randint(0, int(self.max_t[scene]) + 1))
        valid = np.where(self.exist_is_one[scene, fil, origin_t] * self.moving[scene, fil])[0]
        return origin_t, int(valid[rs.choice(len(valid))])

    def validate(self, scn, t0, agent):
        """Raise ValueError for the first triple the host form refuses (its messages); -> the triples as int32 arrays."""
        scn, t0, agent = (np.atleast_1d(np.asarray(a)).astype(np.int64) for a in (scn, t0, agent))
        if not (scn.shape == t0.shape == agent.shape and scn.ndim == 1):
            raise ValueError("scn, t0 and agent are three sequences of one length")
        for s, t, a in zip(scn, t0, agent):
            if not 0 <= s < self.S:
                raise ValueError(f"scene {s} outside [0, {self.S - 1}]")
            if not 0 <= t <= self.max_t[s]:
                raise ValueError(f"origin_t {t} outside [0, {self.max_t[s]}]")
            fil = self.filtered[s]
            if not 0 <= a < len(fil):
                raise ValueError(f"origin_agent {a} outside [0, {len(fil) - 1}]")
            if not (self.exist_is_one[s, fil[a], t] and self.moving[s, fil[a]]):
                raise ValueError("the origin agent must move and exist at the window's first step")
        return scn.astype(np.int32), t0.astype(np.int32), agent.astype(np.int32)


def launch_windows(ds, scn_d, t0_d, agent_d, B, out=None):
    """ctrlsim_window_build for the first B triples of three int32 device tensors, queued on the current stream -> (CtxBuffers, moving
    [B,A] u8, status [B] i32).  No check of the triples: the kernel's status is the only defence here (build_windows validates first)."""
    from .engine import CtxBuffers
    d = ds.dims
    cb = out if out is not None else CtxBuffers(d, max(B, 1), ds.device)
    if cb.st12.shape[0] < B:
        raise ValueError(f"{B} windows do not fit context buffers of {cb.st12.shape[0]}")
    for t in (scn_d, t0_d, agent_d):
        if t.dtype != torch.int32 or t.dim() != 1 or t.shape[0] < B or t.device != ds.ag_data.device:
            raise ValueError(f"the triples are three int32 tensors of at least {B} entries on the dataset's device")
    moving = torch.empty(max(B, 1), d.A, dtype=torch.uint8, device=ds.device)
    status = torch.empty(max(B, 1), dtype=torch.int32, device=ds.device)
    p = _lib.ptr
    _lib.check(_lib.lib().ctrlsim_window_build(B, ds.S, ds.N, ds.Td, d.T, d.A, ds.Pmax, d.P, d.NP, p(ds.ag_data), p(ds.actions), p(ds.rtgs),
                                               p(ds.goals5), p(ds.types), p(ds.road_points), p(ds.road_types), p(ds.n_polys), p(scn_d),
                                               p(t0_d), p(agent_d), C.byref(ds.wcfg), C.byref(cb.struct), p(moving), p(status),
                                               _lib.stream_ptr()), "window_build")
    return cb, moving[:B], status[:B]


def build_windows(ds, scn, t0, agent, out=None):
    """The windows (scn[b], t0[b], agent[b]) of DeviceDataset ds -> (CtxBuffers, moving [B,A] u8), queued on the current stream.  The
    triples are validated from the host tables BEFORE the launch (ValueError with the host form's messages); the kernel's own verdict
    per window stays on the device in the buffers' `status` attribute ([B] i32, 0 = served)."""
    scn, t0, agent = ds.validate(scn, t0, agent)
    up = lambda a: torch.from_numpy(a).to(ds.device)
    cb, moving, status = launch_windows(ds, up(scn), up(t0), up(agent), len(scn), out)
    cb.status = status
    return cb, moving
