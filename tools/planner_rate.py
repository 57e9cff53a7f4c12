"""Throughput of the planner-vs-adversary evaluation (eval_planner.py's flow): PlannerAdversaryEvaluator.evaluate_planner_adversary()
through both of its routes, at the full model size.
usage: python tools/planner_rate.py [scenarios=16] [agents=12] [steps=90] [stepwise | device] [repeats=1] [history_steps=10]
  stepwise  the per-scenario, per-step loop: two AutoregressivePolicy objects, each with a one-scene device session and a host round trip
            per policy and step (cfg.eval_planner_adversary.device_replay absent / False)
  device    all scenes in one RolloutEngine batch with policy roles per vehicle (RolloutEngine.set_roles, csrc/replay.hip's _views
            kernels): one run(), one check_finite(), one read-back (cfg.eval_planner_adversary.device_replay = True)
Every repeat is a complete evaluation and prints its own rate (profiles/planner_adversary_rate.md records them)."""
import sys
import time

sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import ctrlsim_amd  # noqa: F401
from ctrlsim_amd import spec
from ctrlsim_amd.models import CtRLSim
from ctrlsim_amd.policies import AutoregressivePolicy
from ctrlsim_amd.evaluators import PlannerAdversaryEvaluator
from ctrlsim_amd.evaluators.planner_adversary_evaluator import PLANNER_KEYS, ADVERSARY_KEYS

S = int(sys.argv[1]) if len(sys.argv) > 1 else 16
N = int(sys.argv[2]) if len(sys.argv) > 2 else 12
T = int(sys.argv[3]) if len(sys.argv) > 3 else 90
MODE = sys.argv[4] if len(sys.argv) > 4 else "stepwise"
assert MODE in ("stepwise", "device"), MODE
REPEATS = int(sys.argv[5]) if len(sys.argv) > 5 else 1
HS = int(sys.argv[6]) if len(sys.argv) > 6 else 10


def make_cfg(n_scn):
    cfg = spec.make_cfg(nocturne__steps=T)
    pa = cfg.eval_planner_adversary
    pa.history_steps = HS
    pa["synthetic"] = dict(num_scenarios=n_scn, n_agents=N, n_polylines=200, seed=7, extent=60.0)
    pa["device_replay"] = MODE == "device"
    return cfg


def role_policy(cfg, model, pol, key_dict):
    return AutoregressivePolicy(cfg=cfg, model_path="", model=model, use_rtg=pol.use_rtg, predict_rtgs=pol.predict_rtgs,
                                discretize_rtgs=pol.discretize_rtgs, real_time_rewards=pol.real_time_rewards,
                                privileged_return=pol.privileged_return, max_return=pol.max_return, min_return=pol.min_return, key_dict=key_dict,
                                tilt_dict={"tilt": True, "goal_tilt": pol.goal_tilt, "veh_veh_tilt": pol.veh_veh_tilt, "veh_edge_tilt": pol.veh_edge_tilt},
                                name=pol.model, action_temperature=pol.action_temperature, nucleus_sampling=pol.nucleus_sampling,
                                nucleus_threshold=pol.nucleus_threshold)


def evaluator(cfg, model):
    pa = cfg.eval_planner_adversary
    return PlannerAdversaryEvaluator(cfg, role_policy(cfg, model, pa.planner, PLANNER_KEYS), role_policy(cfg, model, pa.adversary, ADVERSARY_KEYS))


cfg = make_cfg(S)
model = CtRLSim(cfg, seed=0, device="cuda:0")
evaluator(make_cfg(1), model).evaluate_planner_adversary()              # warm-up: first launches, allocations
route = {"stepwise": "stepwise loop, two policy sessions per scene", "device": "one RolloutEngine.run() with policy roles"}[MODE]
for rep in range(REPEATS):
    t0 = time.perf_counter()
    ev = evaluator(cfg, model)
    m, _ = ev.evaluate_planner_adversary()
    el = time.perf_counter() - t0
    assert (MODE == "device") == hasattr(ev, "device_replay_scenes")
    print(f"planner vs adversary ({route}): {S} scenarios x {N} vehicles x {T} steps, history_steps {HS}, full model, in {el:.3f} s = "
          f"{S * T / el:.1f} scenario-steps/s ({el / (S * T) * 1e3:.2f} ms per scenario-step)")
