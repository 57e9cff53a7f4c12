"""CPU: offline-RL dataset generation (ctrlsim_amd/datagen.py, csrc/dataset.hip) — the C ABI of the new entries, the generator's
existence rule, the polyline offset table of the road-edge distance kernel, and the host forms on the issue's hand checks."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from helpers import cfg_of
from ctrlsim_amd import datagen, replay, scenarios, ingest
from ctrlsim_amd.rewards import signed_distance_to_road_edges

ENTRIES = ("ctrlsim_dataset_edge_distance", "ctrlsim_dataset_edge_distance_f64", "ctrlsim_dataset_rewards", "ctrlsim_dataset_rtgs")


def _declared_args(hdr, name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/ctrlsim.h"
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_dataset_entries_are_declared_bound_and_exported():
    from ctrlsim_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ctrlsim.h")).read()
    l = _lib.lib()
    for name in ENTRIES:
        args = _declared_args(hdr, name)
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
        res, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == len(args), (name, len(argtypes), len(args))
        assert res is _lib.I and argtypes[-1] is _lib.P and "hipStream_t" in args[-1]
        assert hasattr(l, name), f"{name} is not exported by the built library"
    # the struct the two reward entries take by pointer: one C double per float field, in the header's order
    body = re.search(r"typedef struct ctrlsim_dataset_cfg \{(.*?)\} ctrlsim_dataset_cfg;", hdr, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
    assert fields == [k for k, _ in _lib.DatasetCfg._fields_]
    # invalid arguments come back as status codes, nothing is launched (no GPU here)
    assert l.ctrlsim_dataset_edge_distance(1, 65, 4, 5, 0, 0, *([None] * 6)) == -22
    assert l.ctrlsim_dataset_edge_distance_f64(1, 0, 0, 0, *([None] * 6)) == -22
    assert l.ctrlsim_dataset_rewards(1, 4, 4, 5, *([None] * 11)) == -22
    assert l.ctrlsim_dataset_rtgs(1, 4, 4, *([None] * 7)) == -22
    assert l.ctrlsim_dataset_rtgs(0, 4, 4, *([None] * 7)) == -22                 # (null arrays are refused before the empty batch)


def test_dataset_file_is_built_like_the_other_float64_files():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ctrlsim_build", os.path.join(ROOT, "ctrl-sim_amd", "csrc", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.SRCS.get("dataset") == "-ffp-contract=off"
    assert "#pragma clang fp contract(off)" in open(os.path.join(b.HERE, "dataset.hip")).read()


def _generator_rule(flags):
    """generate_offline_rl_dataset.py:88-93 for one vehicle, as written there: flags [rows] of the log, steps = rows - 1."""
    existence = []
    for t in range(len(flags) - 1):
        veh_exists = flags[t] and flags[t + 1]
        if t > 0 and existence[-1] == 0:
            veh_exists = 0
        existence.append(float(bool(veh_exists)))
    return existence


def test_dataset_existence_is_the_generators_rule_and_the_replay_alive_flag():
    rs = np.random.RandomState(5)
    S, N, rows = 6, 12, 25
    flag = (rs.uniform(size=(S, N, rows)) < 0.9).astype(np.float64)              # flicker
    flag[0, :4, 0] = 0.0                                                         # not there at the start
    flag[1, :4, :3] = 1.0
    flag[1, :4, 3:] = 0.0                                                        # early drop-out
    flag[2, :4, :rows - 2] = 1.0
    flag[2, :4, rows - 2:] = 0.0                                                 # late drop-out: the last step has no next row
    flag[3] = 1.0                                                                # logged throughout
    log = np.zeros((S, N, rows, 6))
    log[..., 4] = flag
    log[..., 3] = 5.0
    log[..., 5] = 4.5
    ex = datagen.dataset_existence(log)
    assert ex.shape == (S, N, rows - 1) and ex.dtype == np.float64
    ref = np.array([[_generator_rule(flag[s, v]) for v in range(N)] for s in range(S)])
    assert np.array_equal(ex, ref)
    assert ex[3].all() and not ex[0, :4].any() and ex[1, :4].sum() == 4 * 2 and ex[2, :4, -1].sum() == 0
    assert np.array_equal(datagen.dataset_existence(log, steps=7), ref[..., :7])
    # ... which is the `alive` flag of the replay step with nothing controlled, the latched existence carried along
    w = cfg_of("loop").dataset.waymo
    ctrl, none = np.zeros((S, N), bool), np.full((S, N), -1, np.int32)
    latched = None
    for t in range(rows - 1):
        latched = replay.latch(log, t, latched)
        _, alive, _ = replay.actions(log, ctrl, latched, t, 1, np.zeros((S, N)), np.full((S, N), 5.0), none, 0.1, w)
        assert np.array_equal(alive, ex[..., t] != 0), t


def test_polyline_offsets():
    pts = lambda n: np.arange(2 * n, dtype=np.float64).reshape(n, 2)
    scenes = [[pts(12), pts(1), pts(2), pts(31)],                                # a one-point polyline: no segment
              [pts(9)],
              [pts(0), pts(3), pts(1), pts(1), pts(100), pts(2)],                # an empty one, two one-point ones in a row
              []]
    off = datagen.polyline_offsets(scenes)
    assert off.dtype == np.int32 and off.shape == (4, 7)
    assert off[0].tolist() == [0, 11, 11, 12, 42, 42, 42]
    assert off[1].tolist() == [0, 8, 8, 8, 8, 8, 8]
    assert off[2].tolist() == [0, 0, 2, 2, 2, 101, 102]
    assert off[3].tolist() == [0] * 7
    for s, polys in enumerate(scenes):                                           # a partition of the scene's segment table, in order
        segs = [np.concatenate([p[:-1], p[1:]], 1) for p in polys if len(p) > 1]
        assert off[s, -1] == sum(len(x) for x in segs)
        assert (np.diff(off[s]) >= 0).all()
        for p, poly in enumerate(polys):
            assert off[s, p + 1] - off[s, p] == max(len(poly) - 1, 0)


def test_edge_polylines_of_a_scene_are_those_of_its_segment_table():
    d = cfg_of("loop")
    # synthetic scene: a road-edge row of road_points is a polyline
    scn = scenarios.make_scenario(3, 1, n_agents=4, n_polylines=9, n_points=10, extent=30.0)
    polys = datagen.edge_polylines_of(scn)
    segs = np.concatenate([np.concatenate([p[:-1], p[1:]], 1) for p in polys if len(p) > 1])
    assert np.array_equal(segs.astype(np.float32), scn.edge_segments)
    assert datagen.polyline_offsets([polys])[0, -1] == len(scn.edge_segments)
    # a scene from a scenario file: polylines longer than a chunk stay whole (25 points = chunks of 10, 10 and 5 in road_points), a
    # polyline of exactly two chunks leaves no remainder, a one-point road edge gives no segment
    log = scenarios.standin_log(scn, 6)
    data = ingest.scenario_to_nocturne_json(scn, log)
    line = lambda n, y: [{"x": float(i), "y": float(y)} for i in range(n)]
    data["roads"] = [{"geometry": line(25, 0), "type": "road_edge"}, {"geometry": line(7, 3), "type": "lane"},
                     {"geometry": line(1, 5), "type": "road_edge"}, {"geometry": line(20, 9), "type": "road_edge"}]
    scn2, info = ingest.load_nocturne_json(data, max_pts=10, steps=5)
    polys2 = datagen.edge_polylines_of(scn2)
    assert [len(p) for p in polys2] == [25, 1, 20]
    assert scn2.road_points.shape[0] == 3 + 1 + 1 + 2
    off = datagen.polyline_offsets([polys2])
    assert off[0].tolist() == [0, 24, 24, 43] and len(scn2.edge_segments) == 43
    assert datagen.road_data_of(scn2) is info["road_data"]
    # the roads of a synthetic scene, rebuilt from its rows, chunk back into the same rows
    rp, rt, ep = ingest.roads_to_polylines(datagen.road_data_of(scn), 10)
    assert np.array_equal(rp.astype(np.float32), scn.road_points) and np.array_equal(rt, scn.road_types)
    assert all(np.array_equal(a, b) for a, b in zip(ep, polys))


def test_host_form_hand_checks_where_the_sign_is_zero():
    """A polyline whose sign comes out 0 wins with distance 0, as in the reference: the sign is taken per polyline before the
    comparison across polylines."""
    with np.errstate(all="ignore"):
        assert signed_distance_to_road_edges(np.array([[12.0, 0.0]]), [np.array([[0.0, 0.0], [10.0, 0.0]])])[0] == 0.0
        assert signed_distance_to_road_edges(np.array([[-1.0, 1.0]]), [np.array([[0.0, 0.0], [0.0, 0.0], [4.0, 0.0]])])[0] == 0.0
        far_first = [np.array([[0.0, 50.0], [10.0, 50.0]]), np.array([[0.0, 0.0], [10.0, 0.0]])]
        assert signed_distance_to_road_edges(np.array([[12.0, 0.0]]), far_first)[0] == 0.0


def test_goal_substitution_follows_the_generator():
    scn = scenarios.make_scenario(3, 2, n_agents=5, n_polylines=6, n_points=10, extent=30.0)
    log = scenarios.standin_log(scn, 9)
    log[1]["traj"][5:] = 0.0                                                     # leaves after row 4
    log[2]["traj"][0, 4] = 0.0                                                   # not there at the start: row -1, as the generator reads it
    g = datagen.substituted_goals(scn, log, 8)
    assert np.array_equal(g[0], [scn.goal_pos[0, 0], scn.goal_pos[0, 1], scn.goal_heading[0], scn.goal_speed[0]])
    assert np.array_equal(g[1], log[1]["traj"][4, :4])
    assert np.array_equal(g[2], log[2]["traj"][8, :4])
    cfg = cfg_of("loop")
    c = datagen.dataset_cfg(cfg)
    assert c.pos_tol == 1.0 and c.shaped_scaling == 0.2 and c.edge_scale == 15.0 and c.remove_shaped_goal == 1 and c.remove_shaped_veh == 0
