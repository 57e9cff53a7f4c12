"""Shared by tests/test_gpu_replay.py and tests/test_gpu_roles.py: the float64 comparison helpers, the log cuts, the engine of an
evaluator's policy, the host-driven stepping both files compare RolloutEngine.run() with, and the agreement the two owe each other."""
import ctypes as C

import numpy as np
import torch

from ctrlsim_amd import replay

ULP = 8          # steer: device atan within OpenCL's 5 ulp of the true value, glibc's within 1; every operation before it is identical


def _ulps(a, b):
    """|a - b| in units of the spacing of float64 at max(|a|, |b|) (0 where both are equal, signed zeros included)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return np.where(a == b, 0.0, np.abs(a - b) / sp)


def _disc6(w):
    return (C.c_double * 6)(w.min_accel, w.max_accel, w.min_steer, w.max_steer, w.accel_discretization, w.steer_discretization)


def _cut_logs(k, v, tr):
    """Vehicles that leave: in every scene vehicle 1's log ends after row 6 (+ k % 5) — at k % 5 == 0 inside the K/V-cached steps
    (t < 8), else after them —, vehicle 2's after row 11, vehicle 3 is not there at t = 0 (its later rows are logged: latched out),
    vehicle 4's flag drops at rows 8-9 and comes back (stays out)."""
    if v == 1:
        tr[7 + k % 5:] = 0.0
    elif v == 2:
        tr[12:] = 0.0
    elif v == 3:
        tr[0, 4] = 0.0
    elif v == 4:
        tr[8:10, 4] = 0.0
    return tr


def engine_of(ev, **kw):
    """The engine PolicyEvaluator._roll_batch rolls its batches on (lanes and the other engine options: kw)."""
    return ev._engine_of(ev.policy, tilt=ev._tilt_of(ev.policy), **kw)


def host_driven(engs, log, role, hsteps, dt, w, noise=None, after_policy_step=None):
    """R ordinary single-policy engines with the same scenes loaded (engine r = role r; one engine and role = 0 / -1: a plain logged
    batch), stepped by the host as PolicyEvaluator._roll_batch steps one: every step, the latched existence into each, policy_step on
    each, the tokens merged by role, the replay actions in NumPy (replay.latch / replay.actions), one sim_step on engine 0, the new state
    row and the token column copied into the others.  No code of set_log / set_roles is used.
    noise(t) -> (noise_rtg [S*R,N,3,bins], noise_act [S*R,N,V]): explicit sampling noise per view row; engine r takes rows r::R.
    after_policy_step(t, engs): called once every engine has sampled step t."""
    S, N = role.shape
    R, T, d = len(engs), engs[0].steps, engs[0].device
    exist = np.zeros((S, N, T + 1)); accel = np.zeros((S, N, T)); steer = np.zeros((S, N, T))
    sampled = np.zeros((S, R, N, T), np.int32)
    own = np.zeros((S, R, N, T), np.int32)
    ctrl = role >= 0
    for t in range(T):
        exist[:, :, t] = replay.latch(log, t, exist[:, :, t - 1] if t else None)
        col = torch.from_numpy(exist[:, :, t].astype(np.float32)).to(d)
        toks = np.zeros((S, R, N), np.int32)
        for r, e in enumerate(engs):
            e.hist_states[:, :, t, 7] = col
            if noise is None:
                e.policy_step(t)
            else:
                e.policy_step(t, *(a[r::R].contiguous() for a in noise(t)))
            toks[:, r] = e.act_now.cpu().numpy()
            own[:, r, :, t] = e.own_ctx.cpu().numpy()
            assert e.nonfinite() == 0
        sampled[..., t] = toks
        if after_policy_step is not None:
            after_policy_step(t, engs)
        row = engs[0].hist_states[:, :, t].cpu().numpy()
        speed = engs[0].phys[:, :, 16].cpu().numpy()
        merged = np.where(ctrl, np.take_along_axis(toks, np.clip(role, 0, R - 1)[:, None, :], 1)[:, 0], -1)
        act, alive, tok = replay.actions(log, ctrl, exist[:, :, t], t, hsteps, row[..., 4], speed, merged, dt, w)
        accel[:, :, t], steer[:, :, t] = act[..., 0], act[..., 1]
        tok_d = torch.from_numpy(tok.astype(np.int32)).to(d)
        for e in engs:
            e.hist_tok[:, :, t] = tok_d
        engs[0].exists.copy_(torch.from_numpy(alive.astype(np.uint8)).to(d))
        engs[0].sim_step(t, torch.from_numpy(act).to(d))
        for e in engs[1:]:
            e.hist_states[:, :, t + 1].copy_(engs[0].hist_states[:, :, t + 1])
    exist[:, :, T] = replay.latch(log, T, exist[:, :, T - 1])
    engs[0].hist_states[:, :, T, 7] = torch.from_numpy(exist[:, :, T].astype(np.float32)).to(d)
    return dict(tokens=engs[0].hist_tok.cpu().numpy(), states=engs[0].hist_states.cpu().numpy(), coll=engs[0].coll.cpu().numpy(),
                existence=exist, applied=np.stack([accel, steer], -1), sampled_roles=sampled, own_ctx=own,
                rtg_bins_roles=np.stack([e.hist_rtg.cpu().numpy() for e in engs], 1))


def assert_rollouts_agree(host, devr, what, equal_keys):
    """The agreement the host-driven and the device-side replay owe each other, once the sampled tokens are known to be equal."""
    for k in equal_keys:
        assert np.array_equal(host[k], devr[k]), (what, k)
    assert np.array_equal(host["states"][..., 7], devr["states"][..., 7])
    identical = np.array_equal(host["states"], devr["states"])
    print(f"{what}: states bit-identical: {identical}; largest difference {np.abs(host['states'] - devr['states']).max():.3g}")
    np.testing.assert_allclose(devr["states"], host["states"], rtol=0, atol=1e-4)
    assert np.array_equal(host["applied"][..., 0].view(np.int64), devr["applied"][..., 0].view(np.int64)), f"{what}: applied accel"
    u = _ulps(host["applied"][..., 1], devr["applied"][..., 1])
    print(f"{what}: largest applied-steer distance {u.max():.1f} ulp ({int((u > 0).sum())} of {u.size} differ)")
    assert u.max() <= ULP
