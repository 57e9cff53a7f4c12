"""CPU: policy roles per vehicle — the C ABI of the two _views entry points of csrc/replay.hip, their host form in
ctrlsim_amd/replay.py against the single-policy host form, and the log merge of a fixed-trajectory ("cat") adversary."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from helpers import cfg_of
from ctrlsim_amd import replay

ENTRIES = ("ctrlsim_replay_latch_views", "ctrlsim_replay_actions_views")


def _declared_args(hdr, name):
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert m, f"{name} is not declared in include/ctrlsim.h"
    return [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]


def test_views_entries_are_declared_bound_and_exported():
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
    launchers = open(os.path.join(ROOT, "ctrl-sim_amd", "csrc", "launchers.h")).read()
    assert "launch_replay_latch_views(" in launchers and "launch_replay_actions_views(" in launchers
    declared = set(re.findall(r"\b(ctrlsim_[a-z0-9_]+)\s*\(", hdr)) - {"ctrlsim_dims", "ctrlsim_ctx", "ctrlsim_model"}
    assert set(_lib.SIGNATURES) == declared
    # the existing entry points keep their signatures
    assert len(_lib.SIGNATURES["ctrlsim_replay_latch"][1]) == 10 and len(_lib.SIGNATURES["ctrlsim_replay_actions"][1]) == 18
    # invalid arguments come back as status codes, nothing is launched (no GPU here): no vehicles, more roles than supported,
    # several roles without view arrays
    m = re.search(r"#define\s+CTRLSIM_MAX_ROLES\s+(\d+)", hdr)
    assert m and int(m.group(1)) >= 4
    too_many = int(m.group(1)) + 1
    one = (l.ctrlsim_replay_latch_views, l.ctrlsim_replay_actions_views)
    assert one[0](1, 0, 1, 0, 2, *([None] * 7)) == -22
    assert one[0](1, 4, too_many, 0, 2, *([None] * 7)) == -22
    assert one[1](1, 4, 2, 0, 2, 1, 1, 0.1, *([None] * 12)) == -22
    assert one[1](1, 4, too_many, 0, 2, 1, 1, 0.1, *([None] * 12)) == -22
    assert one[0](0, 4, 2, 0, 2, *([None] * 7)) == 0 and one[1](0, 4, 2, 0, 2, 1, 1, 0.1, *([None] * 12)) == 0     # nothing to do


def _rows(S, N, T1, t, seed):
    rs = np.random.RandomState(seed)
    log = np.zeros((S, N, T1 + 1, 6))
    log[..., 0] = rs.uniform(-100, 100, (S, N, T1 + 1))
    log[..., 1] = rs.uniform(-100, 100, (S, N, T1 + 1))
    log[..., 2] = rs.uniform(-np.pi, np.pi, (S, N, 1)) + rs.uniform(-0.15, 0.15, (S, N, T1 + 1))
    log[..., 3] = rs.uniform(0.5, 25.0, (S, N, 1)) + rs.uniform(-0.4, 0.4, (S, N, T1 + 1))
    log[..., 4] = (rs.uniform(size=(S, N, T1 + 1)) < 0.9).astype(np.float64)
    log[..., 5] = rs.uniform(3.0, 7.0, (S, N, 1))
    exist_prev = (rs.uniform(size=(S, N)) < 0.9).astype(np.float64)
    heading = (log[:, :, t, 2] + rs.uniform(-0.02, 0.02, (S, N))).astype(np.float32)
    speed = (log[:, :, t, 3] + rs.uniform(-0.3, 0.3, (S, N))).astype(np.float32)
    return rs, log, exist_prev, heading, speed


def _views_step(log, role, R, exist_prev, t, T1, hsteps, heading, speed, toks_v, w, rs):
    """latch_views + actions_views on fresh view arrays -> (exist, scene row, view_states, act, alive, tok)."""
    S, N = role.shape
    row_in = rs.uniform(-5, 5, (S, N, 8)).astype(np.float32)
    row_in[..., 4] = heading
    vs = np.full((S, R, N, T1, 8), -3.0, np.float32)
    ex, row = replay.latch_views(log, t, exist_prev, row_in, vs)
    act, alive, tok = replay.actions_views(log, role, ex, t, hsteps, heading, speed, toks_v, 0.1, w)
    return ex, row, row_in, vs, act, alive, tok


@pytest.mark.parametrize("t,hsteps", [(0, 1), (1, 3), (3, 2)])
def test_one_role_equals_the_single_policy_host_form(t, hsteps):
    w = cfg_of("loop").dataset.waymo
    S, N, T1 = 5, 17, 5
    rs, log, exist_prev, heading, speed = _rows(S, N, T1, t, 3 + t)
    ctrl = rs.uniform(size=(S, N)) < 0.5
    toks = rs.randint(0, 1000, (S, N)).astype(np.int32)
    toks[rs.uniform(size=(S, N)) < 0.1] = -1
    role = np.where(ctrl, 0, -1)
    ex, row, row_in, vs, act, alive, tok = _views_step(log, role, 1, exist_prev, t, T1, hsteps, heading, speed, toks[:, None], w, rs)
    ex0 = replay.latch(log, t, exist_prev)
    act0, alive0, tok0 = replay.actions(log, ctrl, ex0, t, hsteps, heading, speed, toks, 0.1, w)
    assert np.array_equal(ex, ex0) and np.array_equal(act.view(np.int64), act0.view(np.int64))
    assert np.array_equal(alive, alive0) and np.array_equal(tok, tok0) and tok.dtype == np.int32
    # the view's row t = the scene's row with the latched existence; no other row of the view is touched
    assert np.array_equal(row[..., :7], row_in[..., :7]) and np.array_equal(row[..., 7], ex0.astype(np.float32))
    assert np.array_equal(vs[:, 0, :, t], row) and (np.delete(vs, t, axis=3) == -3.0).all()


@pytest.mark.parametrize("t,hsteps", [(0, 1), (2, 3), (4, 2)])
def test_three_roles_take_their_own_views_token(t, hsteps):
    w = cfg_of("loop").dataset.waymo
    S, N, T1, R = 6, 23, 6, 3
    rs, log, exist_prev, heading, speed = _rows(S, N, T1, t, 40 + t)
    role = rs.randint(-1, R, (S, N))
    role[0] = -1                                           # a scene nobody drives
    role[1][role[1] == 2] = 0                              # a scene with an unused role
    toks_v = rs.randint(0, 1000, (S, R, N)).astype(np.int32)
    toks_v[rs.uniform(size=(S, R, N)) < 0.15] = -1
    ex, row, row_in, vs, act, alive, tok = _views_step(log, role, R, exist_prev, t, T1, hsteps, heading, speed, toks_v, w, rs)
    for r in range(R):                                     # every view holds the scene's row
        assert np.array_equal(vs[:, r, :, t], row)
    # role -1 rows: the uncontrolled branch, whatever the views sampled
    act_u, alive_u, tok_u = replay.actions(log, np.zeros((S, N), bool), ex, t, hsteps, heading, speed, np.full((S, N), 7, np.int32), 0.1, w)
    free = role < 0
    assert free.sum() > N and np.array_equal(act[free].view(np.int64), act_u[free].view(np.int64))
    assert np.array_equal(alive[free], alive_u[free]) and np.array_equal(tok[free], tok_u[free])
    # role rows: the token of their own view — the single-policy form fed with that view's tokens, row by row
    by_policy = t >= hsteps - 1
    seen = {"token": 0, "nobody": 0}
    for r in range(R):
        mine = role == r
        act_r, alive_r, tok_r = replay.actions(log, mine, ex, t, hsteps, heading, speed, toks_v[:, r], 0.1, w)
        assert np.array_equal(act[mine].view(np.int64), act_r[mine].view(np.int64)) and np.array_equal(alive[mine], alive_r[mine])
        assert np.array_equal(tok[mine], tok_r[mine])
        if by_policy:
            live = mine & (ex != 0)
            ok = live & (toks_v[:, r] >= 0)
            assert np.array_equal(tok[ok], toks_v[:, r][ok])                      # discretise(undiscretise(token)) = token
            none = live & (toks_v[:, r] < 0)
            assert (act[none] == 0).all() and alive[none].all()                   # (0, 0) where the view has no answer
            seen["token"] += int(ok.sum()); seen["nobody"] += int(none.sum())
            # another view's token is NOT what drives the vehicle
            other = toks_v[:, (r + 1) % R]
            differs = ok & (other != toks_v[:, r]) & (other >= 0)
            assert differs.any() and (tok[differs] != other[differs]).all()
    if by_policy:
        assert seen["token"] > 20 and seen["nobody"] > 3
    # a role index the views do not hold answers like a missing token
    act_x, alive_x, _ = replay.actions_views(log, np.full((S, N), R), ex, t, hsteps, heading, speed, toks_v, 0.1, w)
    if by_policy:
        assert (act_x == 0).all() and np.array_equal(alive_x, ex != 0)


def test_cat_log_merge():
    rs = np.random.RandomState(5)
    N, T1, hs, adv = 4, 9, 3, 2
    log = rs.uniform(1, 2, (N, T1 + 1, 6))
    log[..., 4] = 1.0
    log[adv, 7:, :] = 0.0                                  # the adversary's log ends after row 6
    traj = rs.uniform(-3, 3, (T1, 5))                      # x, y, vx, vy, yaw — one row shorter than the log
    out = replay.merge_cat_log(log, adv, traj, hs)
    assert out is not log and out.shape == log.shape
    others = [v for v in range(N) if v != adv]
    assert np.array_equal(out[others], log[others])
    assert np.array_equal(out[adv, :hs], log[adv, :hs])                            # the history comes from the log
    assert np.array_equal(out[adv, hs:T1, 0], traj[hs:, 0]) and np.array_equal(out[adv, hs:T1, 1], traj[hs:, 1])
    assert np.array_equal(out[adv, hs:T1, 2], traj[hs:, 4])                        # heading = yaw
    assert np.array_equal(out[adv, hs:T1, 3], np.sqrt(traj[hs:, 2] ** 2 + traj[hs:, 3] ** 2))
    assert np.array_equal(out[adv, :, 4], log[adv, :, 4]) and np.array_equal(out[adv, :, 5], log[adv, :, 5])   # existence, length
    assert np.array_equal(out[adv, T1], log[adv, T1])                              # past the trajectory: the log's row
    # what the replay branch then does at step t >= hs - 1: Evaluator-style validity from the LOG's flags, target = the trajectory
    w = cfg_of("loop").dataset.waymo
    from ctrlsim_amd.kinematics import bicycle_backward
    ex = replay.latch_all(out, T1)
    assert np.array_equal(ex, replay.latch_all(log, T1))
    for t in (hs - 1, 4, 6):
        heading, speed = rs.uniform(-1, 1, N), rs.uniform(1, 2, N)
        act, alive, _ = replay.actions(out, np.zeros(N, bool), ex[:, t], t, hs, heading, speed, np.zeros(N, np.int32), 0.1, w)
        assert alive[adv] == (t + 1 <= 6)
        if alive[adv]:
            nxt = np.array([[traj[t + 1, 0], traj[t + 1, 1], traj[t + 1, 4], np.sqrt(traj[t + 1, 2] ** 2 + traj[t + 1, 3] ** 2), log[adv, t + 1, 5]]])
            a, s = bicycle_backward(nxt, np.array([[0, 0, heading[adv], speed[adv]]]), 0.1)
            assert act[adv, 0] == a[0] and act[adv, 1] == s[0]
        else:
            assert (act[adv] == 0).all()
