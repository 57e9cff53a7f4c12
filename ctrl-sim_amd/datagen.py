"""Offline-RL dataset generation: logged scenes -> the `*_physics.pkl` dictionaries CtRL-Sim is trained on and the evaluators read
back (cfg.eval.preprocessed_files), with their returns-to-go, for a whole batch of scenes on the device.

What the reference does in three places, one vehicle and one scene at a time:
  data/generate_offline_rl_dataset.py:17-144    every vehicle of a logged scene pushed through the simulator with inverse-bicycle
                                                actions; existence latched; position, velocity, heading, action and one compute_reward
                                                row per vehicle and step
  datasets/rl_waymo/dataset.py:111-275,
  dataset_ctrl_sim.py:54-97                     that export -> the pickled dictionary (ag_data, ag_actions, ag_rewards, the signed
                                                road-edge distance reward, the nearest-vehicle reward, goals)
  dataset.py:240-275, dataset_ctrl_sim.py:92-97 the dictionary -> five-component returns-to-go at load time

Two routes to the same dictionaries:
  generate        LogReplayer.run() — the replay kernels (csrc/replay.hip) and the simulator, all scenes per step, no model — then
                  csrc/dataset.hip (signed road-edge distance, reward rows, distance rewards, RTGs) and ONE read-back
  generate_host   the host forms: NumPy replay.latch / replay.actions around one simulator step per step, then
                  metrics.compute_rewards, ingest.preprocess_scene and ingest.load_preprocessed per scene (the tests' and the rate
                  tool's twin; no kernel of csrc/dataset.hip)
A batch holds scenes of equal vehicle count N <= 64 (as RolloutEngine.load_scenarios).  The dataset has T = steps rows per vehicle:
the generator records the state BEFORE each of its `steps` simulator steps.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import pickle

import numpy as np
import torch

from . import _lib, ingest, replay
from .scenarios import ROAD_TYPES

REWARD_KEYS = ("ag_rewards", "veh_edge_dist_rewards", "veh_veh_dist_rewards")


def dataset_existence(log, steps=None):
    """The generator's existence rule (generate_offline_rl_dataset.py:88-93) on log [..., rows, >= 5] (column 4 = the log's flag):
    e_t = log[t].exist and log[t + 1].exist and e_{t-1}, for t < rows - 1 (or the first `steps` of them) -> [..., T] float64.
    It equals the `alive` flag of replay.actions with nothing controlled: the `exists` output of ctrlsim_replay_actions per step."""
    flag = np.asarray(log)[..., 4] != 0
    T = flag.shape[-1] - 1 if steps is None else int(steps)
    assert 0 <= T <= flag.shape[-1] - 1, "step t looks at log row t + 1"
    out = np.zeros(flag.shape[:-1] + (T,))
    prev = np.ones(flag.shape[:-1], bool)
    for t in range(T):
        prev = flag[..., t] & flag[..., t + 1] & prev
        out[..., t] = prev
    return out


def substituted_goals(scn, log, steps):
    """goals4 [N,4] float64 = goal x, y, heading, speed of every vehicle after the generator's substitution
    (generate_offline_rl_dataset.py:48-58 = PolicyEvaluator.initialize_goal_dict): a vehicle that leaves its log aims at where it was
    last seen.  log = {vehicle: {"traj": rows x, y, heading, speed, exist, ...}}; the generator's log holds steps + 1 rows."""
    from .evaluators import PolicyEvaluator
    out = np.zeros((scn.N, 4))
    for v in range(scn.N):
        g = PolicyEvaluator.initialize_goal_dict(None, scn, v, np.asarray(log[v]["traj"], np.float64)[:steps + 1])
        out[v, :2], out[v, 2], out[v, 3] = g["pos"], g["heading"], g["speed"]
    return out


def road_data_of(scn):
    """get_road_data of a scene: scn.road_data where the loader kept it (ingest.load_nocturne_json), else one road per row of
    road_points (synthetic scenes: a row IS a polyline), stop signs as a single point."""
    rd = getattr(scn, "road_data", None)
    if rd is not None:
        return rd
    inv = {v: k for k, v in ROAD_TYPES.items()}
    out = []
    for pl, ty in zip(scn.road_points, scn.road_types):
        kind = inv[int(np.argmax(ty))]
        n = int(pl[:, 2].sum())
        if kind == "stop_sign":
            out.append({"geometry": {"x": float(pl[0, 0]), "y": float(pl[0, 1])}, "type": kind})
        else:
            out.append({"geometry": [{"x": float(q[0]), "y": float(q[1])} for q in pl[:n]], "type": kind})
    return out


def edge_polylines_of(scn):
    """The scene's road-edge polylines in the order of scn.edge_segments: scn.road_edge_polylines (unchunked, ingest.load_nocturne_json)
    or the existing points of the road-edge rows of road_points."""
    polys = getattr(scn, "road_edge_polylines", None)
    if polys is not None:
        return [np.asarray(p, np.float64).reshape(-1, 2) for p in polys]
    rows = np.where(np.argmax(scn.road_types, axis=1) == ROAD_TYPES["road_edge"])[0] if len(scn.road_types) else []
    return [np.asarray(scn.road_points[p][:int(scn.road_points[p][:, 2].sum()), :2], np.float64) for p in rows]


def polyline_offsets(polys_per_scene):
    """poly_off [S, PE + 1] int32 for ctrlsim_dataset_edge_distance: segments poly_off[s, p] .. poly_off[s, p + 1] - 1 of scene s's
    segment table belong to its polyline p (n points = n - 1 segments; a polyline of one or no point has none); PE = the largest
    polyline count of the batch, unused entries repeat the end."""
    S = len(polys_per_scene)
    PE = max([len(p) for p in polys_per_scene] + [0])
    off = np.zeros((S, PE + 1), np.int32)
    for s, polys in enumerate(polys_per_scene):
        n = np.array([max(len(p) - 1, 0) for p in polys], np.int64)
        off[s, 1:len(polys) + 1] = np.cumsum(n)
        off[s, len(polys) + 1:] = n.sum()
    return off


def dataset_cfg(cfg):
    """ctrlsim_dataset_cfg of a configuration: cfg.nocturne.rew_cfg and the reward constants of cfg.dataset.waymo."""
    w, r = cfg.dataset.waymo, cfg.nocturne.rew_cfg
    return _lib.DatasetCfg(pos_tol=r["position_target_tolerance"], heading_tol=r["heading_target_tolerance"],
                           speed_tol=r["speed_target_tolerance"], shaped_scaling=r.get("shaped_goal_distance_scaling", 1.0),
                           reward_scaling=r["reward_scaling"], goal_mult=w.pos_target_achieved_rew_multiplier,
                           shaped_min=w.pos_goal_shaped_min, shaped_max=w.pos_goal_shaped_max,
                           veh_mult=w.veh_veh_collision_rew_multiplier, max_veh_dist=w.max_veh_veh_distance,
                           edge_mult=w.veh_edge_collision_rew_multiplier, edge_scale=w.dist_to_road_edge_scaling_factor,
                           remove_shaped_goal=int(bool(w.remove_shaped_goal)), remove_shaped_veh=int(bool(w.remove_shaped_veh_reward)),
                           remove_shaped_edge=int(bool(w.remove_shaped_edge_reward)), pad_=0)


class LogReplayer:
    """Model-free batched driver of fully logged scenes: every vehicle replays its log through the inverse bicycle model and the
    simulator (contacts on), existence follows the log.  load(scenes, logs, steps), run(), then results() / dataset().
    Per step t < steps, all scenes at once on the current stream: ctrlsim_replay_actions with nothing controlled (its `exists` output
    is the dataset's existence of step t, recorded per step, and the applied pair), ctrlsim_sim_step, ctrlsim_replay_latch(t + 1).
    No HipModel, no forward workspace, no lanes."""

    def __init__(self, cfg, device="cuda:0"):
        self.cfg, self.w = cfg, cfg.dataset.waymo
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.lib = _lib.lib()
        self.dt = float(cfg.nocturne.dt)
        w = self.w
        self.disc6 = (C.c_double * 6)(w.min_accel, w.max_accel, w.min_steer, w.max_steer, w.accel_discretization, w.steer_discretization)
        self.dcfg = dataset_cfg(cfg)
        # the simulator counts contacts beyond its island solver's table in the bound guard pair's second word (include/ctrlsim.h:
        # ctrlsim_bind): this driver binds its own pair for its launches and puts back what was bound
        self.guard = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.S = 0

    def __del__(self):
        try:
            self.lib.ctrlsim_unbind(self.guard.data_ptr())
        except Exception:
            pass

    @contextlib.contextmanager
    def _bound(self):
        prev = self.lib.ctrlsim_bound_guard()
        _lib.check(self.lib.ctrlsim_bind(-1, self.guard.data_ptr()), "bind")
        try:
            yield
        finally:
            self.lib.ctrlsim_bind(-1, prev)

    # ------------------------------------------------------------------ upload (shapes of RolloutEngine.load_scenarios / set_log)
    def load(self, scenes, logs, steps=None):
        """scenes: Scenario objects of equal N; logs[k] = {vehicle: {"traj": rows x, y, heading, speed, exist, ..., length}} of scene k
        (>= steps + 1 rows, as get_ground_truth_states gives them; shorter logs end the vehicle)."""
        dev = self.device
        S, N = len(scenes), scenes[0].N
        assert len(logs) == S and all(s.N == N for s in scenes) and 1 <= N <= 64, "one batch = equal N <= 64 vehicles per scene"
        self.S, self.N = S, N
        self.steps = int(steps if steps is not None else self.cfg.nocturne.steps)
        T, T1 = self.steps, self.steps + 1
        assert T >= 1
        polys = [edge_polylines_of(s) for s in scenes]
        for k, (s, pl) in enumerate(zip(scenes, polys)):
            segs = [np.concatenate([p[:-1], p[1:]], 1) for p in pl if len(p) > 1]
            if not segs:
                raise ValueError(f"scene {k} has no road-edge polyline: the road-edge distance reward is undefined there "
                                 "(the reference's compute_distance_to_road_edge raises on it)")
            if not np.array_equal(np.concatenate(segs).astype(np.float32), np.asarray(s.edge_segments, np.float32)):
                raise ValueError(f"scene {k}: its road-edge polylines are not the polylines of its edge_segments table, in order")
        self.poly_off_h = polyline_offsets(polys)
        self.PE = self.poly_off_h.shape[1] - 1
        E = max(len(s.edge_segments) for s in scenes)
        edges = np.full((S, E, 4), 1e30, np.float32)
        for i, s in enumerate(scenes):
            edges[i, :len(s.edge_segments)] = s.edge_segments
        self.E = E
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=dev)
        self.init_pose = f32(np.stack([np.stack([s.x, s.y, s.heading, s.speed], 1) for s in scenes]))
        self.size = f32(np.stack([np.stack([s.length, s.width], 1) for s in scenes]))
        self.edges = f32(edges)
        self.poly_off = torch.from_numpy(self.poly_off_h).to(dev)
        self.goals4_h = np.stack([substituted_goals(s, lg, T) for s, lg in zip(scenes, logs)])
        self.goals4 = torch.from_numpy(self.goals4_h).to(dev)
        self.log_h = replay.log_array(logs, N, T1)                              # [S,N,T1+1,6]
        self.log = torch.from_numpy(self.log_h).to(dev)
        self.controlled = z(S, N, dt=torch.uint8)                                # nothing is handed to a policy
        self.act_now = z(S, N, dt=torch.int32)
        self.exists = torch.ones(S, N, dtype=torch.uint8, device=dev)
        self.phys = z(S, N, 20)
        self.contact_state = z(S, int(self.lib.ctrlsim_sim_contact_floats(N)))
        self.hist_states = z(S, N, T1, 8)
        self.coll = z(S, N, T1, 2, dt=torch.uint8)
        self.hist_tok = z(S, N, T, dt=torch.int32)
        self.exist_hist = z(S, N, T1, dt=torch.float64)
        self.act_f64 = z(S, N, 2, dt=torch.float64)
        self.applied_steps = z(T, S, N, 2, dt=torch.float64)                     # step-major: row t is what the simulator writes
        self.alive_steps = z(T, S, N, dt=torch.uint8)                            # `exists` of every step: the dataset's existence
        self.reset()
        return self

    def reset(self):
        p, st = _lib.ptr, _lib.stream_ptr()
        for a in (self.hist_states, self.coll, self.hist_tok, self.exist_hist, self.applied_steps, self.alive_steps, self.guard):
            a.zero_()
        self.exists.fill_(1)
        _lib.check(self.lib.ctrlsim_sim_init(self.S, self.N, self.E, p(self.init_pose), p(self.size), p(self.edges), p(self.exists),
                                             p(self.phys), p(self.hist_states), p(self.coll), self.steps + 1, p(self.contact_state), st),
                   "sim_init")

    def _sim_step(self, t, act, exists, applied, st):
        # (ctrlsim_sim_step itself cuts a batch above the compute-unit count into launches of that many scenes)
        p = _lib.ptr
        _lib.check(self.lib.ctrlsim_sim_step(self.S, self.N, self.E, None, p(act), self.disc6, p(self.size), p(self.edges), p(exists),
                                             p(self.phys), p(self.hist_states), p(self.coll), p(applied), t, self.steps + 1, self.dt, 0,
                                             p(self.contact_state), st), "sim_step")

    def run(self):
        """Roll the loaded scenes from step 0 on the device (queued on the current stream; nothing synchronises)."""
        lib, p, st = self.lib, _lib.ptr, _lib.stream_ptr()
        S, N, T, T1 = self.S, self.N, self.steps, self.steps + 1
        with self._bound():
            _lib.check(lib.ctrlsim_replay_latch(S, N, 0, T1, p(self.log), p(self.phys), p(self.exist_hist), p(self.hist_states), None, st),
                       "replay_latch")
            for t in range(T):
                alive = self.alive_steps[t]
                _lib.check(lib.ctrlsim_replay_actions(S, N, t, T1, T, 1, self.dt, p(self.log), p(self.controlled), p(self.exist_hist),
                                                      p(self.hist_states), p(self.phys), p(self.act_now), self.disc6, p(self.act_f64),
                                                      p(alive), p(self.hist_tok), st), "replay_actions")
                self._sim_step(t, self.act_f64, alive, self.applied_steps[t], st)
                _lib.check(lib.ctrlsim_replay_latch(S, N, t + 1, T1, p(self.log), p(self.phys), p(self.exist_hist), p(self.hist_states),
                                                    None, st), "replay_latch")
        return self

    def run_host(self):
        """The same rollout stepped from the host: replay.latch / replay.actions in NumPy around one simulator step per step
        (generate_host; the stepping the device-side replay is compared with)."""
        S, N, T, d = self.S, self.N, self.steps, self.device
        st = _lib.stream_ptr()
        ctrl = np.zeros((S, N), bool)
        none = np.full((S, N), -1, np.int32)
        exist = np.zeros((S, N, T + 1))
        with self._bound():
            for t in range(T):
                exist[:, :, t] = replay.latch(self.log_h, t, exist[:, :, t - 1] if t else None)
                self.hist_states[:, :, t, 7] = torch.from_numpy(exist[:, :, t].astype(np.float32)).to(d)
                row = self.hist_states[:, :, t].cpu().numpy()
                speed = self.phys[:, :, 16].cpu().numpy()
                act, alive, tok = replay.actions(self.log_h, ctrl, exist[:, :, t], t, 1, row[..., 4], speed, none, self.dt, self.w)
                self.hist_tok[:, :, t] = torch.from_numpy(tok.astype(np.int32)).to(d)
                self.alive_steps[t].copy_(torch.from_numpy(alive.astype(np.uint8)).to(d))
                self._sim_step(t, torch.from_numpy(np.ascontiguousarray(act)).to(d), self.alive_steps[t], self.applied_steps[t], st)
            exist[:, :, T] = replay.latch(self.log_h, T, exist[:, :, T - 1])
            self.hist_states[:, :, T, 7] = torch.from_numpy(exist[:, :, T].astype(np.float32)).to(d)
            self.exist_hist.copy_(torch.from_numpy(exist).to(d))
        return self

    def check(self):
        """Synchronise; raise if the simulator met contacts beyond its island solver's table during this driver's steps."""
        torch.cuda.synchronize(self.device)
        n = int(self.guard[1].item())
        if n:
            self.guard.zero_()
            raise FloatingPointError(f"{n} simulator contacts beyond the island solver's table (csrc/sim.hip: MAX_ISLAND_CONTACTS)")

    def results(self):
        """states [S,N,steps+1,8], coll, existence [S,N,steps+1] (the latched log flag, as RolloutEngine.results), alive [S,N,steps]
        (the dataset's existence), applied [S,N,steps,2], tokens [S,N,steps]."""
        self.check()
        return dict(states=self.hist_states.cpu().numpy(), coll=self.coll.cpu().numpy(), existence=self.exist_hist.cpu().numpy(),
                    alive=self.alive_steps.permute(1, 2, 0).contiguous().cpu().numpy().astype(np.float64),
                    applied=self.applied_steps.permute(1, 2, 0, 3).contiguous().cpu().numpy(), tokens=self.hist_tok.cpu().numpy())

    # ------------------------------------------------------------------ the dataset's rewards on the device (csrc/dataset.hip)
    def dataset(self):
        """Queue the two dataset entries behind the rollout -> device tensors exist [S,N,T] f64, edge_dist, ag_rewards, veh_veh, veh_edge,
        rtgs."""
        out = self.dataset_buffers()
        self.dataset_edge_distance(out)
        self.dataset_rewards(out)
        return out

    def dataset_buffers(self):
        S, N, T, dev = self.S, self.N, self.steps, self.device
        z = lambda *sh: torch.empty(*sh, dtype=torch.float64, device=dev)
        exist = self.alive_steps.permute(1, 2, 0).to(torch.float64).contiguous()
        return dict(exist=exist, edge_dist=z(S, N, T), ag_rewards=z(S, N, T, 8), veh_veh=z(S, N, T), veh_edge=z(S, N, T), rtgs=z(S, N, T, 5))

    def dataset_edge_distance(self, out):
        p = _lib.ptr
        _lib.check(self.lib.ctrlsim_dataset_edge_distance(self.S, self.N, self.steps, self.steps + 1, self.E, self.PE, p(self.hist_states),
                                                          p(out["exist"]), p(self.edges), p(self.poly_off), p(out["edge_dist"]),
                                                          _lib.stream_ptr()), "dataset_edge_distance")

    def dataset_rewards(self, out):
        p = _lib.ptr
        _lib.check(self.lib.ctrlsim_dataset_rewards(self.S, self.N, self.steps, self.steps + 1, p(self.hist_states), p(self.coll),
                                                    p(out["exist"]), p(self.goals4), p(out["edge_dist"]), C.byref(self.dcfg),
                                                    p(out["ag_rewards"]), p(out["veh_veh"]), p(out["veh_edge"]), p(out["rtgs"]),
                                                    _lib.stream_ptr()), "dataset_rewards")

    def device_dataset(self, out, scenes):
        """The tensors dataset() left on the device (`out`) as a windows.DeviceDataset: what read_back() would put into the scenes'
        dictionaries, without the read-back of the large arrays.  The states are the simulator's float32 rows, cast to the dictionary's
        float64 on the device (the cast _scene_dict does on the host); what travels to the host are the existence flags (one byte per
        vehicle and step) and the step-0 positions, for the tables of the two random draws.  scenes: the Scenario objects given to
        load() (their types and polylines; the polylines are uploaded, padded to the largest count)."""
        from .windows import DeviceDataset
        S, N, T, dev = self.S, self.N, self.steps, self.device
        assert len(scenes) == S
        self.check()
        ag_data = torch.cat([self.hist_states[:, :, :T, :7].to(torch.float64), out["exist"].unsqueeze(-1)], dim=-1).contiguous()
        actions = self.applied_steps.permute(1, 2, 0, 3).contiguous()
        NP = int(self.w.max_num_road_pts_per_polyline)
        roads = [ingest.roads_to_polylines(road_data_of(s), NP)[:2] for s in scenes]
        Pmax = max(len(p) for p, _ in roads)
        road_points, road_types = np.zeros((S, Pmax, NP, 3)), np.zeros((S, Pmax, 8))
        for k, (p, t) in enumerate(roads):
            road_points[k, :len(p)] = p
            road_types[k, :len(p)] = t
        up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        exist = self.alive_steps.permute(1, 2, 0).contiguous().cpu().numpy()
        xy0 = self.hist_states[:, :, 0, :2].to(torch.float64).cpu().numpy()
        return DeviceDataset(self.cfg, ag_data, actions, out["rtgs"], up(_goals5(self.goals4_h)),
                             up(np.stack([np.asarray(s.types, np.float64) for s in scenes])), up(road_points), up(road_types),
                             up([len(p) for p, _ in roads], np.int32), exist, xy0)


def _goals5(goals4):
    """Policy.update_state's goal row of the dictionary: x, y, speed * cos(heading), speed * sin(heading), heading."""
    gh, gs = goals4[..., 2], goals4[..., 3]
    return np.stack([goals4[..., 0], goals4[..., 1], gs * np.cos(gh), gs * np.sin(gh), gh], -1)


def _scene_dict(cfg, scn, idx, states, exist, applied, goals4, rewards, veh_edge, veh_veh, rtgs):
    """One scene's dictionary in the layout of ingest.preprocess_scene from arrays [N,T,...] (+ rtgs)."""
    w = cfg.dataset.waymo
    N, T = exist.shape
    road_points, road_types, _ = ingest.roads_to_polylines(road_data_of(scn), w.max_num_road_pts_per_polyline)
    ag_data = np.concatenate([states[:, :T, :7].astype(np.float64), exist[..., None]], -1)
    there = exist[:, 0] != 0
    last = np.where(there, T - 1 - np.argmax(exist[:, ::-1] == 1.0, axis=1), -1)
    types = np.asarray(scn.types, np.float64)
    return dict(idx=idx, num_agents=N, road_points=road_points, road_types=road_types, ag_data=ag_data,
                ag_actions=np.array(applied, np.float64), ag_types=types.copy(), last_exist_timesteps=last.astype(np.int64),
                veh_edge_dist_rewards=veh_edge, veh_veh_dist_rewards=veh_veh, ag_rewards=rewards,
                filtered_ag_ids=[int(i) for i in np.where(there)[0]], ag_goals=np.repeat(_goals5(goals4)[:, None], T, 1), rtgs=rtgs)


def read_back(rp, d, scenes):
    """The one read-back of generate(): replayer rp and its dataset tensors d -> the scenes' dictionaries."""
    rp.check()
    states = rp.hist_states.cpu().numpy()
    applied = rp.applied_steps.permute(1, 2, 0, 3).contiguous().cpu().numpy()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    return [_scene_dict(rp.cfg, scn, k, states[k], h["exist"][k], applied[k], rp.goals4_h[k], h["ag_rewards"][k], h["veh_edge"][k],
                        h["veh_veh"][k], h["rtgs"][k]) for k, scn in enumerate(scenes)]


def generate(cfg, scenes, logs, steps=None, device="cuda:0"):
    """-> one dictionary per scene: the keys, shapes and dtypes of ingest.preprocess_scene, plus `rtgs` [N,T,5] (what
    ingest.load_preprocessed makes of it).  Everything preprocess_scene derives from positions comes from the device."""
    rp = LogReplayer(cfg, device).load(scenes, logs, steps)
    rp.run()
    return read_back(rp, rp.dataset(), scenes)


def export_json(name, scn, d, goals4=None, rewards=None):
    """The generator's export {"name", "objects", "roads"} (generate_offline_rl_dataset.py:60-74,124-139) of one scene from its
    dictionary d.  goals4 [N,4] = goal x, y, heading, speed (substituted_goals; None: heading from the dictionary, speed = the norm of
    its goal velocity, which need not give the last bit back); rewards [N,T,8] = the compute_reward rows (None: d["ag_rewards"], which
    are already multiplied by the existence — the dataset code multiplies again, to the same values)."""
    ag, act = np.asarray(d["ag_data"]), np.asarray(d["ag_actions"])
    rew = np.asarray(d["ag_rewards"] if rewards is None else rewards)
    N, T = ag.shape[:2]
    if goals4 is None:
        g5 = np.asarray(d["ag_goals"])[:, 0]
        goals4 = np.stack([g5[:, 0], g5[:, 1], g5[:, 4], np.hypot(g5[:, 2], g5[:, 3])], 1)
    types = np.asarray(d["ag_types"])
    objs = [{"position": [{"x": float(ag[v, t, 0]), "y": float(ag[v, t, 1])} for t in range(T)],
             "velocity": [{"x": float(ag[v, t, 2]), "y": float(ag[v, t, 3])} for t in range(T)],
             "heading": [float(x) for x in ag[v, :, 4]], "existence": [float(x) for x in ag[v, :, 7]],
             "acceleration": [float(x) for x in act[v, :, 0]], "steering": [float(x) for x in act[v, :, 1]],
             "reward": [[float(x) for x in rew[v, t]] for t in range(T)],
             "goal_position": {"x": float(goals4[v, 0]), "y": float(goals4[v, 1])}, "goal_heading": float(goals4[v, 2]),
             "goal_speed": float(goals4[v, 3]), "width": float(ag[v, 0, 6]), "length": float(ag[v, 0, 5]),
             "type": ingest.OBJECT_TYPES[int(np.argmax(types[v]))]} for v in range(N)]
    return {"name": name, "objects": objs, "roads": road_data_of(scn)}


def generate_host(cfg, scenes, logs, steps=None, device="cuda:0"):
    """The host-route twin of generate(): host-driven stepping (LogReplayer.run_host), then per scene metrics.compute_rewards,
    ingest.preprocess_scene on the generator's export and ingest.load_preprocessed."""
    from .metrics import compute_rewards
    w = cfg.dataset.waymo
    rp = LogReplayer(cfg, device).load(scenes, logs, steps)
    r = rp.run_host().results()
    T = rp.steps
    out = []
    for k, scn in enumerate(scenes):
        g4 = rp.goals4_h[k]
        states = r["states"][k][:, :T].astype(np.float64)
        rew = compute_rewards(states, r["coll"][k][:, :T].astype(np.float64), g4[:, :2], g4[:, 2], g4[:, 3], cfg.nocturne.rew_cfg)
        proto = dict(ag_data=np.concatenate([states[..., :7], r["alive"][k][..., None]], -1), ag_actions=r["applied"][k],
                     ag_rewards=rew, ag_types=np.asarray(scn.types, np.float64), ag_goals=None)
        pk = ingest.preprocess_scene(export_json(f"scene_{k}", scn, proto, goals4=g4), w, idx=k)
        pk["rtgs"] = ingest.load_preprocessed(pk, w)["rtgs"]
        out.append(pk)
    return out


def write_dataset(out_dir, names, dicts):
    """{out_dir}/{name}_physics.pkl per scene, without `rtgs`: the files Evaluator.load_preprocessed_data / ingest.load_preprocessed
    expect under cfg.eval.preprocessed_files.  -> the paths."""
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for name, d in zip(names, dicts):
        path = os.path.join(out_dir, f"{name}_physics.pkl")
        with open(path, "wb") as fh:
            pickle.dump({k: v for k, v in d.items() if k != "rtgs"}, fh)
        paths.append(path)
    return paths
