"""CPU: the host side of the device window build (ctrlsim_amd/windows.py) — packing, the two seeded draws, the refusals — and the ABI
entry's presence in the built library.  The kernel itself: tests/test_gpu_windows.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from helpers import cfg_of, golden
from ctrlsim_amd import _lib, ingest
from ctrlsim_amd.windows import DeviceDataset, window_cfg


def pre_of(tag):
    gp = golden("preprocessed")
    pre = {k[len(tag) + 5:]: gp[k] for k in gp.files if k.startswith(f"{tag}_pkl_")}
    pre["filtered_ag_ids"] = [int(i) for i in pre["filtered_ag_ids"]]
    return pre


@pytest.fixture(scope="module")
def packed():
    cfg = cfg_of("loop")
    pres = [pre_of("b"), pre_of("c")]
    return cfg, pres, DeviceDataset.from_dicts(cfg, pres, device="cpu")


def test_from_dicts_packs_so_that_slicing_back_reproduces_every_array(packed):
    cfg, pres, ds = packed
    w = cfg.dataset.waymo
    assert (ds.S, ds.N, ds.Td, ds.NP) == (2, 10, 21, 10) and ds.Pmax == 12 and list(ds.n_polys_h) == [9, 12]
    for s, pre in enumerate(pres):
        back = ds.scene_dict(s)
        for k in ("ag_data", "ag_actions", "ag_types", "ag_goals", "road_points", "road_types", "last_exist_timesteps"):
            assert np.array_equal(back[k], np.asarray(pre[k], np.float64)), k
        assert back["filtered_ag_ids"] == pre["filtered_ag_ids"]
        assert np.array_equal(back["rtgs"], ingest.load_preprocessed(pre, w)["rtgs"])
        # rows beyond a scene's polyline count are padding
        assert (ds.road_points[s, len(pre["road_points"]):] == 0).all()
        # the host tables are ingest._window_tables'
        _, ag_data, _, moving_ids, max_t = ingest._window_tables(pre, cfg)
        assert np.array_equal(np.where(ds.moving[s])[0], moving_ids) and ds.max_t[s] == max_t
        assert np.array_equal(ds.exist[s], ag_data[..., 7] != 0)
    # a single scene with more polylines than the model keeps
    one = DeviceDataset.from_dicts(cfg, [pre_of("a")], device="cpu")
    assert (one.S, one.N, one.Pmax) == (1, 8, 20)


def test_from_dicts_refuses_unequal_scenes_and_foreign_filters():
    cfg = cfg_of("loop")
    with pytest.raises(ValueError, match="equal vehicle and step count"):
        DeviceDataset.from_dicts(cfg, [pre_of("a"), pre_of("b")], device="cpu")
    pre = pre_of("b")
    pre["filtered_ag_ids"] = pre["filtered_ag_ids"][1:]
    with pytest.raises(ValueError, match="filtered_ag_ids"):
        DeviceDataset.from_dicts(cfg, [pre], device="cpu")


@pytest.mark.parametrize("seed", [0, 1, 5, 11, 12345])
def test_choices_equal_window_choices(packed, seed):
    cfg, pres, ds = packed
    for s, pre in enumerate(pres):
        assert ds.choices(s, seed) == ingest.window_choices(pre, cfg, seed)


def test_validate_raises_what_the_host_form_raises(packed):
    cfg, pres, ds = packed
    t0, a0 = ds.choices(0, 3)
    scn, t, a = ds.validate([0, 1], [t0, 0], [a0, _valid_agent(ds, 1, 0)])
    assert scn.dtype == t.dtype == a.dtype == np.int32 and list(scn) == [0, 1]
    for s, pre in enumerate(pres):
        # the first step: the host form's message, word for word
        for bad in (-1, int(ds.max_t[s]) + 1, 10 ** 6):
            with pytest.raises(ValueError) as host:
                ingest.training_window(pre, cfg, bad, a0)
            with pytest.raises(ValueError) as mine:
                ds.validate(s, bad, a0)
            assert str(mine.value) == str(host.value)
        # an origin that is absent at the first step, or does not move
        fil = ds.filtered[s]
        for t in range(int(ds.max_t[s]) + 1):
            for a in range(len(fil)):
                ok = ds.exist_is_one[s, fil[a], t] and ds.moving[s, fil[a]]
                if ok:
                    ds.validate(s, t, a)
                    ingest.training_window(pre, cfg, t, a)
                else:
                    with pytest.raises(ValueError) as host:
                        ingest.training_window(pre, cfg, t, a)
                    with pytest.raises(ValueError) as mine:
                        ds.validate(s, t, a)
                    assert str(mine.value) == str(host.value) == "the origin agent must move and exist at the window's first step"
    assert any(not (ds.exist_is_one[s, ds.filtered[s][a], t] and ds.moving[s, ds.filtered[s][a]])
               for s in range(2) for t in range(int(ds.max_t[s]) + 1) for a in range(len(ds.filtered[s]))), "no refused pair in the fixtures"
    with pytest.raises(ValueError, match="scene 2 outside"):
        ds.validate(2, 0, 0)
    with pytest.raises(ValueError, match="scene -1 outside"):
        ds.validate(-1, 0, 0)
    with pytest.raises(ValueError, match="origin_agent 10 outside"):
        ds.validate(0, 0, 10)
    with pytest.raises(ValueError, match="origin_agent -1 outside"):
        ds.validate(0, 0, -1)
    with pytest.raises(ValueError, match="one length"):
        ds.validate([0, 1], [0], [0, 0])


def _valid_agent(ds, s, t):
    fil = ds.filtered[s]
    return int(np.where(ds.exist_is_one[s, fil, t] * ds.moving[s, fil])[0][0])


def test_window_cfg_holds_the_configuration():
    cfg = cfg_of("loop")
    w, c = cfg.dataset.waymo, window_cfg(cfg)
    assert (c.agent_dist_threshold, c.moving_threshold) == (w.agent_dist_threshold, w.moving_threshold)
    assert list(c.rtg_lo) == [w.min_rtg_pos, w.min_rtg_veh, w.min_rtg_road] and list(c.rtg_hi) == [w.max_rtg_pos, w.max_rtg_veh, w.max_rtg_road]
    assert (c.min_accel, c.max_accel, c.min_steer, c.max_steer) == (w.min_accel, w.max_accel, w.min_steer, w.max_steer)
    assert (c.rtg_discretization, c.accel_discretization, c.steer_discretization) == (w.rtg_discretization, w.accel_discretization, w.steer_discretization)
    assert c.continuous_rtg == 0
    # the struct's layout is the header's: 12 doubles, 4 ints
    assert C.sizeof(_lib.WindowCfg) == 12 * 8 + 4 * 4


def test_window_build_is_exported_with_the_declared_signature():
    """The built library exports ctrlsim_window_build, and the loader's argtypes follow the parameter list of include/ctrlsim.h:
    int -> c_int, every pointer (hipStream_t included) -> a pointer type."""
    lib = _lib.lib()
    fn = lib.ctrlsim_window_build
    res, args = _lib.SIGNATURES["ctrlsim_window_build"]
    assert fn.restype is res is C.c_int and list(fn.argtypes) == list(args)
    src = open(os.path.join(ROOT, "include", "ctrlsim.h")).read()
    m = re.search(r"int ctrlsim_window_build\((.*?)\);", src, re.S)
    assert m, "no declaration in include/ctrlsim.h"
    params = [q.strip() for q in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == len(args) == 25 and params[-1] == "hipStream_t stream"
    for q, a in zip(params, args):
        if "*" in q or q.startswith("hipStream_t"):
            assert a is C.c_void_p or issubclass(a, C._Pointer), q
        else:
            assert q.startswith("int ") and a is C.c_int, q
    assert issubclass(args[20], C._Pointer) and args[20]._type_ is _lib.WindowCfg and args[21]._type_ is _lib.Ctx
    # the launcher is declared once in the internal header and the source is part of the build
    assert "launch_window_build" in open(os.path.join(ROOT, "ctrl-sim_amd", "csrc", "launchers.h")).read()
    import importlib.util
    spec = importlib.util.spec_from_file_location("ctrlsim_build_mod", os.path.join(ROOT, "ctrl-sim_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.SRCS["window"] == "-ffp-contract=off"
