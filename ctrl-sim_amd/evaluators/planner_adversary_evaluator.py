"""`PlannerAdversaryEvaluator(cfg, planner, adversary).evaluate_planner_adversary() -> (metrics_dict, [str])` — the second
in-repo caller of the policy plugin surface (reference: evaluators/planner_adversary_evaluator.py:26-593, driver
eval_planner.py:16-137).

Two policies share one simulated scene: the planner (cfgs/policy/ctrl_sim_planner.yaml: tilts +10/+10/+10) drives the ego
vehicle, the adversary (ctrl_sim_adversary.yaml: vehicle-vehicle tilt -10) drives one other vehicle, everybody else — and
those two before `history_steps - 1` — replays the log through the inverse bicycle model.  Each policy keeps its own
history buffers, key names (`next_planner_acceleration`, `planner_rtgs`, ...) and device session, exactly as in the
reference loop (:497-546); an adversary named "cat" is not a policy but a fixed trajectory (`apply_adv_traj`, :163-199).

Forced by the environment (as in PolicyEvaluator): scenes come from `cfg.eval_planner_adversary.synthetic`, the log is the
stand-in of scenarios.standin_log, and — there being no CAT dictionary (cfg.cat.dict_path) — the ego is
vehicle 0 and the adversary the vehicle nearest to it at t = 0.  Pinned by tests/golden/planner_adversary.npz (two
unmodified reference policies + the real FreeCar/Box2D)."""
from __future__ import annotations

import random
from types import SimpleNamespace as _NS

import numpy as np
import torch
from scipy.spatial import distance

from .. import scenarios as _scn
from ..kinematics import bicycle_backward
from ..simulation import Simulation
from .policy_evaluator import PolicyEvaluator

PLANNER_KEYS = {"next_acceleration": "next_planner_acceleration", "next_steering": "next_planner_steering",
                "rtgs": "planner_rtgs"}                                       # eval_planner.py:19-23
ADVERSARY_KEYS = {"next_acceleration": "next_adversary_acceleration", "next_steering": "next_adversary_steering",
                  "rtgs": "adversary_rtgs"}                                   # eval_planner.py:76-80


def pick_ego_adversary(scn):
    """Stand-in of the CAT dictionary lookup (planner_adversary_evaluator.py:431-456)."""
    d = np.hypot(scn.x - scn.x[0], scn.y - scn.y[0])
    d[0] = np.inf
    return 0, int(np.argmin(d))


class PlannerAdversaryEvaluator(PolicyEvaluator):
    def __init__(self, cfg, planner, adversary):
        self.planner = planner
        self.adversary = adversary
        self.cfg_pa = cfg.eval_planner_adversary
        super().__init__(cfg, planner)
        self.history_steps = self.cfg_pa.history_steps
        syn = self.cfg_pa.get("synthetic") or dict(num_scenarios=1, n_agents=8, n_polylines=12, seed=0, extent=25.0)
        self.synthetic = dict(syn)
        self.ego_vehicle = None
        self.adversary_vehicle = None

    # ---- planner_adversary_evaluator.py:48-76
    def reset(self):
        seed = self.cfg.eval_planner_adversary.seed
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        self.ades_all, self.fdes_all, self.goal_achieved_all, self.progress_all = [], [], [], []
        self.collision_rate_scenario, self.collision_rate_w_adv_scenario, self.offroad_rate_scenario = [], [], []
        self.ego_jerk_all, self.ego_steering_rate_all, self.ego_accel_all = [], [], []
        self.lin_speed_sim_all, self.lin_speed_gt_all, self.ang_speed_sim_all, self.ang_speed_gt_all = [], [], [], []
        self.accel_sim_all, self.accel_gt_all, self.nearest_dist_sim_all, self.nearest_dist_gt_all = [], [], [], []
        self.collision_speed_with_ego = []

    # ---- :79-108
    def initialize_vehicle_data_dict(self, veh, goal_dict):
        d = super().initialize_vehicle_data_dict(veh, goal_dict)
        for k in ("rtgs", "next_acceleration", "next_steering"):
            d.pop(k)
        d.update({"planner_rtgs": [], "next_planner_acceleration": 0., "next_planner_steering": 0., "adversary_rtgs": [],
                  "next_adversary_acceleration": 0., "next_adversary_steering": 0.})
        return d

    # ---- :163-199
    def apply_adv_traj(self, veh, t, gt_data_dict, vdd, adv_traj):
        v = veh.getID()
        traj = gt_data_dict[v]["traj"]
        exists = traj[t][4] and traj[t + 1][4]
        if t > 0 and vdd[v]["existence"][-1] == 0:
            exists = 0
        if not exists:
            a, s = 0.0, 0.0
            veh.setPosition(-1000000, -1000000)
        else:
            nxt = np.array([[adv_traj[t + 1, 0], adv_traj[t + 1, 1], adv_traj[t + 1, 4],
                             np.sqrt(adv_traj[t + 1, 2] ** 2 + adv_traj[t + 1, 3] ** 2), traj[t + 1][-1]]])
            prev = np.array([[veh.getPosition().x, veh.getPosition().y, veh.getHeading(), veh.getSpeed()]])
            a, s = bicycle_backward(nxt, prev, self.dt)
            a, s = float(a[0]), float(s[0])
        if a > 0.0:
            veh.acceleration = a
        else:
            veh.brake(np.abs(a))
        veh.steering = s
        return veh, [a, s]

    # ---- :458-546
    def evaluate_planner_adversary(self, adv_traj_fn=None):
        """adv_traj_fn(scn, gt_data_dict, ego, adv) -> [steps+1, 5] (x, y, vx, vy, yaw): the fixed adversarial trajectory used
        when adversary.name == 'cat' (the reference reads it from the CAT dictionary).

        cfg.eval_planner_adversary.device_replay = True (default False) rolls the scenes on ONE RolloutEngine with policy roles per
        vehicle (_evaluate_on_device) where that route applies; anything else runs the loop below."""
        if self._device_route_applies():
            return self._evaluate_on_device(adv_traj_fn)
        self.reset()
        syn = self.synthetic
        d_model = self.planner.model.dims
        n_eval = 0
        for k in range(int(syn["num_scenarios"])):
            if n_eval == self.cfg_pa.num_files_to_evaluate:
                break
            scn = _scn.make_scenario(int(syn.get("seed", 0)), k, n_agents=int(syn["n_agents"]),
                                     n_polylines=int(syn["n_polylines"]), n_points=d_model.NP,
                                     extent=float(syn.get("extent", 100.0)))
            self.planner.scenario_index = self.adversary.scenario_index = scn.index
            gt_data_dict = self._ground_truth(scn)
            sim = Simulation(scn, device=self.planner.model.device, steps=self.steps, dt=self.dt)
            vehicles = sim.getScenario().vehicles()
            for veh in vehicles:
                veh.expert_control = False
                veh.physics_simulated = True
            self.ego_vehicle, self.adversary_vehicle = pick_ego_adversary(scn)
            cat = self.adversary.name == "cat"
            adv_traj = adv_traj_fn(scn, gt_data_dict, self.ego_vehicle, self.adversary_vehicle) if cat else None
            n_eval += 1
            preproc_data = {"road_points": scn.road_points.astype(np.float64), "road_types": scn.road_types.copy()}
            vdd, goal_dict, goal_norm = {}, {}, {}
            for veh in vehicles:
                v = veh.getID()
                goal_dict[v] = {"pos": scn.goal_pos[v].astype(np.float64), "heading": float(scn.goal_heading[v]),
                                "speed": float(scn.goal_speed[v])}
                vdd[v] = self.initialize_vehicle_data_dict(veh, goal_dict[v])
                goal_norm[v] = np.linalg.norm(np.array([veh.getPosition().x, veh.getPosition().y]) - goal_dict[v]["pos"])
            self.planner.reset(vdd)
            if not cat:
                self.adversary.reset(vdd)
            for t in range(self.steps):
                vdd = self.update_vehicle_data_dict(t, vehicles, vdd, goal_dict, goal_norm, gt_data_dict)
                self.planner.update_state(vdd, [self.ego_vehicle], t)
                if not cat:
                    self.adversary.update_state(vdd, [self.adversary_vehicle], t)
                vdd = self.planner.predict(vdd, gt_data_dict, preproc_data, None, [self.ego_vehicle], t)
                if not cat:
                    vdd = self.adversary.predict(vdd, gt_data_dict, preproc_data, None, [self.adversary_vehicle], t)
                for veh in vehicles:
                    v = veh.getID()
                    if t >= self.history_steps - 1 and v == self.ego_vehicle:
                        veh, act = self.planner.act(veh, t, vdd)
                    elif t >= self.history_steps - 1 and v == self.adversary_vehicle:
                        if cat:
                            veh, act = self.apply_adv_traj(veh, t, gt_data_dict, vdd, adv_traj)
                        else:
                            veh, act = self.adversary.act(veh, t, vdd)
                    else:
                        veh, act = self.apply_gt_action(veh, t, gt_data_dict, vdd)
                    vdd[v]["acceleration"].append(act[0])
                    vdd[v]["steering"].append(act[1])
                sim.step(self.dt)
            vdd = self.update_vehicle_data_dict(self.steps, vehicles, vdd, goal_dict, goal_norm, gt_data_dict)
            for veh in vehicles:
                vdd[veh.getID()]["acceleration"].append(0)
                vdd[veh.getID()]["steering"].append(0)
            self.last_vehicle_data_dict = vdd
            self.update_running_statistics(vdd)
        return self.compute_metrics()

    # ---- the same evaluation on the engine: policy roles per vehicle
    def _device_route_applies(self):
        """cfg.eval_planner_adversary.device_replay, for two of this repo's AutoregressivePolicy objects on the SAME model object with equal
        sampling and RTG settings (temperature, nucleus, use_rtg / predict_rtgs / discretize_rtgs, privileged / max / min return) and the policy's
        own RTGs (no real_time_rewards) — or such a planner against a fixed trajectory (adversary.name ==
        'cat').  Anything else keeps the stepwise loop."""
        from ..policies.autoregressive_policy import AutoregressivePolicy
        if not bool(self.cfg_pa.get("device_replay", False)):
            return False
        pl, ad = self.planner, self.adversary
        ok = lambda q: type(q) is AutoregressivePolicy and not q.real_time_rewards and hasattr(q.model, "hip")
        if not ok(pl):
            return False
        if getattr(ad, "name", None) == "cat":
            return True
        # one engine samples for both roles: everything but the tilts and the key names must be common to the two policies
        common = lambda q: (float(q.action_temperature), bool(q.nucleus_sampling), float(q.nucleus_threshold) if q.nucleus_sampling else 0.0,
                            bool(q.use_rtg), bool(q.predict_rtgs), bool(q.discretize_rtgs), bool(q.privileged_return),
                            bool(q.max_return), bool(q.min_return))
        return ok(ad) and ad.model is pl.model and common(ad) == common(pl)

    def _evaluate_on_device(self, adv_traj_fn=None):
        """evaluate_planner_adversary with the scenario loop turned inside out (as PolicyEvaluator._evaluate_policy_batched): scenes, ego
        and adversary are chosen exactly as the loop chooses them, then all scenes of equal shape roll in one RolloutEngine batch —
        the log attached (set_log), role 0 = the ego under the planner's tilts, role 1 = the adversary under the adversary's
        (set_roles: one policy view per role and scene, csrc/replay.hip), everybody else and the history steps replayed from the log
        on the device.  One run(), one check_finite(), one read-back per batch; every scene's vehicle_data_dict is then built from the
        arrays in this class's schema and fed to the unchanged update_running_statistics.  A 'cat' adversary needs no role: its log
        rows from history_steps on are the fixed trajectory (replay.merge_cat_log), which the replay branch follows exactly as
        apply_adv_traj does; the statistics keep the unmodified log.  The policy OBJECTS are not driven (no reset / update_state /
        predict calls)."""
        self.reset()
        syn = self.synthetic
        d_model = self.planner.model.dims
        cat = self.adversary.name == "cat"
        chosen, n_eval = [], 0
        for k in range(int(syn["num_scenarios"])):
            if n_eval == self.cfg_pa.num_files_to_evaluate:
                break
            scn = _scn.make_scenario(int(syn.get("seed", 0)), k, n_agents=int(syn["n_agents"]),
                                     n_polylines=int(syn["n_polylines"]), n_points=d_model.NP,
                                     extent=float(syn.get("extent", 100.0)))
            gt_data_dict = self._ground_truth(scn)
            ego, adv = pick_ego_adversary(scn)
            adv_traj = adv_traj_fn(scn, gt_data_dict, ego, adv) if cat else None
            n_eval += 1
            chosen.append((scn, gt_data_dict, ego, adv, adv_traj))
        eng = self._engine_of(self.planner, lanes=1)
        self.device_replay_scenes = 0
        for items in self._batches(chosen, int(self.cfg_pa.get("batch_scenarios", 256))):
            self._roll_on_device(eng, items, cat)
        return self.compute_metrics()

    def _roll_on_device(self, eng, items, cat):
        from .. import discretize as dz
        from .. import replay
        from ..metrics import nearest_vehicle_distance
        w, T, hs = self.cfg_rl_waymo, self.steps, self.history_steps
        S, N, T1 = len(items), items[0][0].N, T + 1
        gt = replay.log_array([it[1] for it in items], N, T1)
        role = -np.ones((S, N), np.int32)
        for k, (scn, gtd, ego, adv, adv_traj) in enumerate(items):
            role[k, ego] = 0
            if not cat:
                role[k, adv] = 1
        log = gt
        if cat:
            log = np.stack([replay.merge_cat_log(gt[k], it[3], it[4], hs) for k, it in enumerate(items)])
        eng.load_scenarios([it[0] for it in items], steps=T)
        eng.set_log(log, role >= 0, hs)
        eng.set_roles(role, [self._tilt_of(self.planner)] + ([] if cat else [self._tilt_of(self.adversary)]))
        eng.run()
        try:
            eng.check_finite()
        except FloatingPointError as e:
            raise FloatingPointError(f"{e} — batch of scenes {[int(it[0].index) for it in items]}") from None
        r = eng.results()                                      # the one read-back
        speeds = eng.speed_hist.cpu().numpy()
        states, coll, exist, applied = r["states"], r["coll"], r["existence"], r["applied"]
        cont = dz.undiscretize_rtgs(r["rtg_bins_roles"], w)    # [S,R,N,T,3]
        own, sampled = r["own_ctx"], r["sampled_roles"]
        keys = [PLANNER_KEYS] + ([] if cat else [ADVERSARY_KEYS])
        for k, (scn, gtd, ego, adv, adv_traj) in enumerate(items):
            self.ego_vehicle, self.adversary_vehicle = ego, adv
            ex_k = exist[k].astype(float)
            goals = {v: {"pos": scn.goal_pos[v].astype(np.float64), "heading": float(scn.goal_heading[v]), "speed": float(scn.goal_speed[v])}
                     for v in range(N)}
            # (the applied actions as Python floats, as the stepwise loop appends them)
            one = _NS(states=states[k], coll=coll[k], speeds=speeds[k], exist=exist[k], accel=applied[k, :, :, 0].tolist(),
                      steer=applied[k, :, :, 1].tolist(), gt=gt[k], rtg=cont[k], own=own[k], keys=keys,
                      nearest=nearest_vehicle_distance(states[k, :, :, :2].astype(np.float64), ex_k),
                      gt_nearest=nearest_vehicle_distance(gt[k, :, :T1, :2], ex_k))
            vdd = self._vehicle_data_dict_of(scn, goals, one)
            for rr, (kd, v) in enumerate(zip(keys, (ego, adv))):   # what the last predict() left for act()
                tok = int(sampled[k, rr, v, T - 1])
                a, s_ = dz.undiscretize_actions(np.array([tok]), w)[0] if tok >= 0 else (0.0, 0.0)
                vdd[v][kd["next_acceleration"]], vdd[v][kd["next_steering"]] = a, s_
            self.last_vehicle_data_dict = vdd
            self.update_running_statistics(vdd)
            self.device_replay_scenes += 1

    def _append_step_extras(self, d, r, v, t):
        """What update_vehicle_data_dict adds for this evaluator's statistics, and one RTG row per policy, vehicle and step
        (r.rtg [R,N,T,3], r.own [R,N,T], r.keys = the roles' key names)."""
        d["gt_acceleration"].append((r.gt[v, t + 1, 3] - r.gt[v, t - 1, 3]) / (2 * self.dt) if 0 < t < self.steps - 1 else 0)
        d["nearest_dist"].append(r.nearest[v, t])
        d["gt_nearest_dist"].append(r.gt_nearest[v, t])
        if t < self.steps and self.planner.predict_rtgs:
            for rr, kd in enumerate(r.keys):
                if r.own[rr, v, t] >= 0:
                    d["next_rtg_goal"], d["next_rtg_veh"], d["next_rtg_road"] = r.rtg[rr, v, t]
                    d[kd["rtgs"]].append(np.array(r.rtg[rr, v, t]))
                else:
                    d[kd["rtgs"]].append(np.array([0] * self.planner.cfg_model.num_reward_components))

    # ---- :202-365
    def update_running_statistics(self, data_dict):
        T1, hs = self.steps + 1, self.history_steps
        future = np.zeros(T1, bool)
        future[hs:] = True
        xy = lambda v, key: np.array([[p["x"], p["y"]] for p in data_dict[v][key]])
        collisions, collisions_w_adv, offroads = [], [], []
        has_adv_ego_collision = False

        v = self.ego_vehicle
        ego_mask = np.array(data_dict[v]["existence"]).astype(bool) * future
        if ego_mask.sum() != 0:
            rew = np.array(data_dict[v]["reward"])[ego_mask]
            goal_achieved = np.any(np.sum(rew[:, :1], axis=1) == 1)
            self.goal_achieved_all.append(float(goal_achieved))
            collisions.append(float(np.any(rew[:, 6] == 1)))
            offroads.append(float(np.any(rew[:, 7] == 1)))
            sim_pos, gt_pos = xy(v, "position"), xy(v, "gt_position")
            self.ades_all.append(np.linalg.norm(sim_pos[ego_mask] - gt_pos[ego_mask], axis=1).mean())
            last = np.where(ego_mask == 1)[-1][-1]
            self.fdes_all.append(np.linalg.norm(sim_pos[last] - gt_pos[last]))
            seg = sim_pos[hs:last + 1]
            step_len = np.linalg.norm(np.diff(seg, axis=0), axis=-1)
            if goal_achieved:
                progress = step_len.sum()
            else:                                                      # only the steps that bring the ego closer to its goal
                dist_to_goal = np.linalg.norm(seg - gt_pos[last][None], axis=-1)
                progress = step_len[np.diff(dist_to_goal) < 0].sum()
            self.progress_all.append(progress)
            acc = np.array(data_dict[v]["acceleration"])[ego_mask]
            self.ego_jerk_all.append(np.abs(np.diff(acc)) / self.dt)
            self.ego_accel_all.append(np.abs(acc))
            self.ego_steering_rate_all.append(np.abs(np.diff(np.array(data_dict[v]["steering"])[ego_mask])) / self.dt)

        v = self.adversary_vehicle
        adv_mask = np.array(data_dict[v]["existence"]).astype(bool) * future
        if adv_mask.sum() != 0:
            vel = xy(v, "velocity")[adv_mask]
            self.lin_speed_sim_all.append(np.linalg.norm(vel, axis=1)[:, None])
            self.lin_speed_gt_all.append(np.array(data_dict[v]["gt_speed"])[adv_mask][:, None])
            self.ang_speed_sim_all.append((np.array(data_dict[v]["heading"])[adv_mask] / self.dt)[:, None])
            self.ang_speed_gt_all.append((np.array(data_dict[v]["gt_heading"])[adv_mask] / self.dt)[:, None])
            gt_acc = np.array(data_dict[v]["gt_acceleration"])[adv_mask]
            sim_acc = np.array(data_dict[v]["acceleration"])[adv_mask]
            inner = np.ones(gt_acc.shape, bool)                        # central differences exist only inside the window
            inner[0] = inner[-1] = False
            self.accel_sim_all.append(sim_acc[inner][:, None])
            self.accel_gt_all.append(gt_acc[inner][:, None])
            self.nearest_dist_gt_all.append(np.array(data_dict[v]["gt_nearest_dist"])[adv_mask][:, None])
            self.nearest_dist_sim_all.append(np.array(data_dict[v]["nearest_dist"])[adv_mask][:, None])

        e, a = self.ego_vehicle, self.adversary_vehicle
        if ego_mask.sum() != 0 and adv_mask.sum() != 0:
            ego_coll = np.array(data_dict[e]["reward"])[ego_mask, 6]
            adv_coll = np.array(data_dict[a]["reward"])[adv_mask, 6]
            n = min(len(ego_coll), len(adv_coll))
            ego_coll, adv_coll = ego_coll[:n], adv_coll[:n]
            both = ((ego_coll == adv_coll).astype(float) * ego_coll).astype(bool)
            has = float(np.any(both))
            if has == 1.:                                              # both flagged: is it each other?  (distance test)
                ego_pos, adv_pos = xy(e, "position")[ego_mask][:n], xy(a, "position")[adv_mask][:n]
                adv_v = xy(a, "velocity")
                valid = False
                for c in np.where(both)[0]:
                    if np.linalg.norm(ego_pos[c] - adv_pos[c]) < data_dict[e]["length"] + data_dict[a]["length"]:
                        valid = True
                        # the reference appends sqrt(vx[c]^2 + vy^2) with vy the WHOLE array (:345); its mean is what
                        # compute_metrics reports, so the same array is kept
                        self.collision_speed_with_ego.append(np.sqrt(adv_v[c, 0] ** 2 + adv_v[:, 1] ** 2))
                        break
                if not valid:
                    has = 0.
            collisions_w_adv.append(has)
            has_adv_ego_collision = bool(has)
        if len(collisions) > 0:
            self.collision_rate_scenario.append(np.array(collisions).mean())
            if len(collisions_w_adv) == 0:
                collisions_w_adv.append(0.)
            self.collision_rate_w_adv_scenario.append(np.array(collisions_w_adv).mean())
            self.offroad_rate_scenario.append(np.array(offroads).mean())
        return has_adv_ego_collision

    # ---- :368-428
    def compute_metrics(self):
        w = self.cfg_rl_waymo
        m = {}
        m["ego_goal"] = np.array(self.goal_achieved_all).mean()
        m["ego_prog"] = np.array(self.progress_all).mean()
        m["ego_cr"] = np.array(self.collision_rate_scenario).mean()
        m["ego_cr_w_adv"] = np.array(self.collision_rate_w_adv_scenario).mean()
        m["ego_or"] = np.array(self.offroad_rate_scenario).mean()
        m["ego_fde"] = np.array(self.fdes_all).mean()
        m["ego_ade"] = np.array(self.ades_all).mean()
        m["ego_accel"] = np.concatenate(self.ego_accel_all, axis=0).mean()
        m["ego_jerk"] = np.concatenate(self.ego_jerk_all, axis=0).mean()
        m["ego_steer_rate"] = np.concatenate(self.ego_steering_rate_all, axis=0).mean()
        m["adv_coll_speed"] = np.array(self.collision_speed_with_ego).mean() if self.collision_speed_with_ego else float("nan")

        def jsd(sim, gt, lo, hi, edges):
            sim = np.clip(np.concatenate(sim, axis=0), lo, hi) if lo is not None else np.concatenate(sim, axis=0)
            gt = np.clip(np.concatenate(gt, axis=0), lo, hi) if lo is not None else np.concatenate(gt, axis=0)
            P = np.histogram(sim, bins=edges)[0] / len(sim)
            Q = np.histogram(gt, bins=edges)[0] / len(gt)
            return distance.jensenshannon(P, Q)
        m["adv_lin_jsd"] = jsd(self.lin_speed_sim_all, self.lin_speed_gt_all, 0, 30, np.arange(201) * 0.5 * (100 / 30))
        m["adv_ang_jsd"] = jsd(self.ang_speed_sim_all, self.ang_speed_gt_all, -50, 50, np.arange(201) * 0.5 - 50)
        gt_acc = np.concatenate(self.accel_gt_all, axis=0)              # discretise / undiscretise the log's accelerations
        gt_acc = (np.clip(gt_acc, a_min=w.min_accel, a_max=w.max_accel) - w.min_accel) / (w.max_accel - w.min_accel)
        gt_acc = np.round(gt_acc * (w.accel_discretization - 1)) / (w.accel_discretization - 1)
        gt_acc = gt_acc * (w.max_accel - w.min_accel) + w.min_accel
        m["adv_acc_jsd"] = jsd(self.accel_sim_all, [gt_acc], None, None,
                               np.arange(w.accel_discretization + 1) * 2 - w.accel_discretization)
        m["nearest_dist_jsd"] = jsd(self.nearest_dist_sim_all, self.nearest_dist_gt_all, 0, 40,
                                    np.arange(201) * 0.5 * (100 / 40))
        return m, ["{}: {:.6f}".format(k, v) for (k, v) in m.items()]
