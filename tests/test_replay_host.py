"""CPU: the device-side log replay (csrc/replay.hip) — its C ABI, its generated code and its host form ctrlsim_amd/replay.py."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from helpers import cfg_of, golden
from ctrlsim_amd import replay, discretize as dz

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ENTRIES = ("ctrlsim_replay_latch", "ctrlsim_replay_actions")


def _build_module():
    spec = importlib.util.spec_from_file_location("ctrlsim_build", os.path.join(ROOT, "ctrl-sim_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _declared_args(hdr, name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/ctrlsim.h"
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_replay_entries_are_declared_bound_and_exported():
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
    # header, bindings and exports still agree as a whole (tests/test_host_logic.py)
    declared = set(re.findall(r"\b(ctrlsim_[a-z0-9_]+)\s*\(", hdr)) - {"ctrlsim_dims", "ctrlsim_ctx", "ctrlsim_model"}
    assert set(_lib.SIGNATURES) == declared
    assert all(hasattr(l, s) for s in declared)
    # invalid arguments come back as status codes, nothing is launched (no GPU here)
    assert l.ctrlsim_replay_latch(1, 0, 0, 2, None, None, None, None, None, None) == -22
    assert l.ctrlsim_replay_actions(1, 4, 0, 2, 1, 1, 0.1, *([None] * 11)) == -22
    assert l.ctrlsim_replay_latch(0, 4, 0, 2, None, None, None, None, None, None) == 0          # nothing to do


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_replay_kernels_use_no_scratch_and_pass_the_isa_guard(tmp_path):
    b = _build_module()
    assert b.SRCS.get("replay") == "-ffp-contract=off"
    src = open(os.path.join(b.HERE, "replay.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    obj = str(tmp_path / "replay.o")
    cmd = b.compile_cmd("replay", b.SRCS["replay"], obj)
    assert "-ffp-contract=off" in cmd and "-fno-slp-vectorize" in cmd
    r = subprocess.run(cmd + ["-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    sizes = [int(line.rsplit(":", 1)[1].split()[0]) for line in r.stderr.splitlines() if "ScratchSize [bytes/lane]" in line]
    assert len(sizes) >= 2 and all(v == 0 for v in sizes), sizes
    assert b.isa_guard(obj) == (0, 0)                      # no packed-fp32 arithmetic at all in a float64 file
    isa = b.device_isa(obj)
    assert "v_fma_f64" in isa or "v_mul_f64" in isa       # (the disassembly is the float64 code we think it is)


def _rows_as_log(nxt, prev):
    """The rows of a (next, previous) table as a two-step log of n uncontrolled vehicles: row 1 = next state, row 0 exists."""
    n = len(nxt)
    log = np.zeros((n, 3, 6))
    log[:, 0, 4] = 1.0
    log[:, 1, :4] = nxt[:, :4]
    log[:, 1, 4] = 1.0
    log[:, 1, 5] = nxt[:, 4]
    return log


def test_replay_branch_reproduces_the_reference_inverse_bicycle_fixture():
    g = golden("bicycle_backward")
    w = cfg_of("loop").dataset.waymo
    nxt, prev = g["nxt"], g["prev"]
    n = len(nxt)
    log = _rows_as_log(nxt, prev)
    act, alive, tok = replay.actions(log, np.zeros(n, bool), replay.latch(log, 0), 0, 1, prev[:, 2], prev[:, 3],
                                     np.full(n, -1, np.int32), 0.1, w)
    np.testing.assert_allclose(act, g["accel_steer"], rtol=0, atol=1e-12)
    assert alive.all() and np.array_equal(tok, dz.discretize_actions(act, w).astype(np.int32))
    # a controlled vehicle in its history steps replays the log too
    act2, alive2, _ = replay.actions(log, np.ones(n, bool), replay.latch(log, 0), 0, 4, prev[:, 2], prev[:, 3],
                                     np.full(n, 7, np.int32), 0.1, w)
    assert np.array_equal(act2, act) and alive2.all()


def _hand_case():
    """Five vehicles, T1 = 6 (steps = 5), log rows 0 .. 6:
    0 controlled, logged throughout; 1 controlled, its log ends after row 2; 2 uncontrolled, logged throughout;
    3 uncontrolled, dead at t = 0 although rows 1.. are logged (latched out); 4 uncontrolled, log ends after row 3."""
    T1 = 6
    log = np.zeros((5, T1 + 1, 6))
    for v in range(5):
        for t in range(T1 + 1):
            log[v, t] = (1.0 * t + 10 * v, 0.5 * v, 0.05 * t, 1.0 + 0.1 * t, 1.0, 4.5)
    log[1, 3:] = 0.0
    log[3, 0, 4] = 0.0
    log[4, 4:] = 0.0
    ctrl = np.array([1, 1, 0, 0, 0], bool)
    return log, ctrl, T1


def test_existence_latch_on_a_hand_made_case():
    log, ctrl, T1 = _hand_case()
    ex = replay.latch_all(log, T1)
    assert ex.shape == (5, T1)
    assert np.array_equal(ex[0], np.ones(T1)) and np.array_equal(ex[2], np.ones(T1))
    assert np.array_equal(ex[1], [1, 1, 1, 0, 0, 0])
    assert np.array_equal(ex[3], np.zeros(T1))             # dead at t = 0 stays dead whatever the log says later
    assert np.array_equal(ex[4], [1, 1, 1, 1, 0, 0])
    log2 = log.copy()
    log2[4, 5, 4] = 1.0                                    # a flag that comes back does not revive the vehicle
    assert np.array_equal(replay.latch_all(log2, T1)[4], [1, 1, 1, 1, 0, 0])
    # the loop of the step-by-step route (policy_evaluator.py: exist[t] = gt[t, 4] * (exist[t - 1] != 0))
    ref = np.zeros((5, T1))
    for t in range(T1):
        ref[:, t] = log[:, t, 4] if t == 0 else log[:, t, 4] * (ref[:, t - 1] != 0)
    assert np.array_equal(ex, ref)


@pytest.mark.parametrize("history_steps", [1, 4])
def test_the_three_branches_on_a_hand_made_case(history_steps):
    log, ctrl, T1 = _hand_case()
    w = cfg_of("loop").dataset.waymo
    ex = replay.latch_all(log, T1)
    zero_tok = int(dz.discretize_actions(np.zeros((1, 2)), w)[0])
    for t in range(T1 - 1):
        heading = log[:, t, 2].astype(np.float32)
        speed = log[:, t, 3].astype(np.float32)
        toks = np.array([100 + t, 37, 5, 5, 5], np.int32)
        if t == 3:
            toks[0] = -1                                   # no context answers for vehicle 0 at this step
        act, alive, tok = replay.actions(log, ctrl, ex[:, t], t, history_steps, heading, speed, toks, 0.1, w)
        by_policy = t >= history_steps - 1
        # ---- vehicle 0: controlled, exists
        if by_policy:
            if toks[0] >= 0:
                assert np.array_equal(act[0], dz.undiscretize_actions(toks[:1], w)[0]) and tok[0] == toks[0]
            else:
                assert np.array_equal(act[0], [0.0, 0.0]) and tok[0] == zero_tok
            assert alive[0]
        else:                                              # history steps: the log drives it
            a, s = replay.bicycle_backward(np.r_[log[0, t + 1, :4], log[0, t + 1, 5]][None],
                                           np.array([[0, 0, np.float64(heading[0]), np.float64(speed[0])]]), 0.1)
            assert np.array_equal(act[0], [a[0], s[0]]) and alive[0]
        # ---- vehicle 1: controlled, its log ends after row 2
        if by_policy:
            if ex[1, t] != 0:
                assert alive[1] and tok[1] == 37
            else:
                assert not alive[1] and np.array_equal(act[1], [0.0, 0.0]) and tok[1] == zero_tok
        else:
            assert alive[1] == (t + 1 <= 2)
        # ---- vehicle 2: log replay throughout
        assert alive[2] and abs(act[2, 0] - (log[2, t + 1, 3] - np.float64(speed[2])) / 0.1) == 0.0
        assert abs(act[2, 1]) <= 0.7
        # ---- vehicle 3: dead at t = 0.  At t = 0 the log row itself says so; later the latch does
        assert not alive[3] and np.array_equal(act[3], [0.0, 0.0]) and tok[3] == zero_tok
        # ---- vehicle 4: valid while rows t and t + 1 are logged
        assert alive[4] == (t + 1 <= 3)
        if not alive[4]:
            assert np.array_equal(act[4], [0.0, 0.0])


def test_replay_edge_rows_follow_the_numpy_expressions():
    """speeds summing to -1e-10 (division by zero), |C| > 2 (NaN -> 0), |C| = 2 (atan(inf) clipped), a heading wrap across +-pi."""
    w = cfg_of("loop").dataset.waymo
    nxt = np.array([[0, 0, 0.3, -1e-10, 4.0],              # n_v + p_v + 1e-10 == 0, heading changes: C = inf -> NaN -> 0
                    [0, 0, 1.0, 0.5, 5.0],                 # huge turn at low speed: |C| > 2 -> sqrt of a negative -> 0
                    [0, 0, -3.1, 10.0, 4.0],               # 3.1 -> -3.1: the short way round (+0.083), not -6.2
                    [0, 0, 0.5, 10.0, 4.0]])               # a turn beyond the steering clip
    prev = np.array([[0, 0, 0.0, 0.0], [0, 0, 0.0, 0.5], [0, 0, 3.1, 10.0], [0, 0, 0.0, 10.0]])
    log = _rows_as_log(nxt, prev)
    act, alive, _ = replay.actions(log, np.zeros(4, bool), replay.latch(log, 0), 0, 1, prev[:, 2], prev[:, 3], np.zeros(4, np.int32), 0.1, w)
    assert alive.all() and np.isfinite(act).all()
    assert act[0, 1] == 0.0 and act[1, 1] == 0.0
    assert 0.0 < act[2, 1] < 0.7
    assert act[3, 1] == 0.7
    assert (replay.token_margin(act, w) <= 0.5).all()
