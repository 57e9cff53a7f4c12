"""GPU: the simulator step (csrc/sim.hip) against the CPU oracle on batches of DIFFERENT scenes and at its edges — the recipes of
tests/sim_cases.py (mixed float64 actions, action tokens, vehicles that come and go, 1..64 vehicles x 0..1000 road-edge segments,
more scenes than compute units, set-position requests and expert rows in some scenes only).  Per recipe: x, y, heading, vx, vy
within 1e-4 at every (scene, vehicle, row); length / width / existence exact; both collision flags equal everywhere; the applied
actions bit for bit; rows beyond the run still hold their fill; the guard pair stays 0.  tests/test_sim_cases_host.py shows on the
CPU that the recipes are well conditioned and see the errors they are meant to catch."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sim_cases as sc  # noqa: E402
import sim_libs  # noqa: E402
from ctrlsim_amd import _lib  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402

NAMES = ["mixed", "tokens", "existence", "chunked", "requests"] + [f"sizes_{n}_{e}" for n, e in sc.SIZES]


@pytest.fixture(scope="module")
def cases():
    sim_libs.build_oracle()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return {c["name"]: c for c in sc.all_cases(S_chunked=n_cu + 37)}


@pytest.fixture(scope="module")
def oracle(cases):
    """The oracle's run of every recipe: computed once, shared, never written to."""
    out = {k: sc.run_oracle(c) for k, c in cases.items()}
    for r in out.values():
        for a in r:
            a.setflags(write=False)
    return out


def _compare(case, got, want, tag):
    hist, coll, applied, info = got
    states, flags, applied_ref = want
    err = sc.state_errors(case, hist, states)
    print(f"{tag}: max |GPU - oracle| x {err[0]:.3g} y {err[1]:.3g} heading {err[2]:.3g} vx {err[3]:.3g} vy {err[4]:.3g}; "
          f"vehicle flags {int(flags[..., 0].sum())} edge flags {int(flags[..., 1].sum())}; "
          f"flag mismatches {int((coll != flags).sum())}; guard {info['guard']}")
    assert (err <= sc.ATOL).all(), (tag, err)
    assert np.array_equal(coll, flags), (tag, np.argwhere(coll != flags)[:8])


@pytest.mark.parametrize("name", NAMES)
def test_recipe_matches_oracle(cases, oracle, name):
    case, want = cases[name], oracle[name]
    states, flags, applied_ref = want
    f = case["facts"]
    if name == "chunked":
        S = case["pose"].shape[0]
        assert S == torch.cuda.get_device_properties(0).multi_processor_count + 37      # the launch is cut in two: s_base > 0
    got = sc.run_gpu(case)
    hist, coll, applied, info = got
    _compare(case, got, want, name)
    assert np.array_equal(hist[..., 5:8], sc.expected_history_tail(case))
    assert np.array_equal(applied.view(np.int64), applied_ref.view(np.int64))
    assert info["fill_ok"] and info["guard"] == 0
    assert flags[..., 1].sum() >= f["min_edge_flags"] and flags[..., 0].sum() >= f["min_veh_flags"]
    if name.startswith("sizes"):
        # the contact-free scene also through the step without a contact-state buffer (vehicles that never touch need none)
        k = f["contact_free_scene"]
        assert flags[k, ..., 0].sum() == 0
        got0 = sc.run_gpu(case, contacts=False, scenes=[k])
        _compare(case, got0, tuple(a[k:k + 1] for a in want), name + " (no contact buffer)")
        assert got0[3]["fill_ok"] and got0[3]["guard"] == 0


def test_mixed_without_a_contact_buffer_is_told_apart(cases, oracle):
    """Without the contact-state buffer the cars drive through each other: the recipe must tell the two apart."""
    case = cases["mixed"]
    hist, _, _, info = sc.run_gpu(case, contacts=False)
    err = sc.state_errors(case, hist, oracle["mixed"][0])
    print("mixed without contacts: max |GPU - oracle| per column", err)
    assert err[:2].max() > 1e-2 and info["fill_ok"]


def test_a_scene_runs_the_same_alone_and_in_the_batch(cases):
    case = cases["mixed"]
    hist, coll, applied, _ = sc.run_gpu(case)
    for k in range(case["pose"].shape[0]):
        h1, c1, a1, _ = sc.run_gpu(case, scenes=[k])
        assert np.array_equal(h1[0].view(np.int32), hist[k].view(np.int32)), k
        assert np.array_equal(c1[0], coll[k]) and np.array_equal(a1[0].view(np.int64), applied[k].view(np.int64)), k


def test_refusals_leave_the_buffers_alone(cases):
    """N = 0, N = 65, E < 0, t + 1 >= Tmax1, no action pointer at all, expert rows with the kinematic mode: nonzero, nothing written."""
    lib, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    S, N, E, T1 = 2, 65, 4, 4
    pose = torch.zeros(S, N, 4, device=DEV); size = torch.full((S, N, 2), 2.0, device=DEV)
    segs = torch.zeros(S, E, 4, device=DEV); exists = torch.ones(S, N, dtype=torch.uint8, device=DEV)
    act = torch.zeros(S, N, 2, dtype=torch.float64, device=DEV); tok = torch.zeros(S, N, dtype=torch.int32, device=DEV)
    expert = torch.zeros(S, N, 4, device=DEV); xy = torch.zeros(S, N, 2, device=DEV)
    disc = (C.c_double * 6)(*sc.DISC6)
    phys = torch.full((S, N, 20), float("nan"), device=DEV)
    hist = torch.full((S, N, T1, 8), float("nan"), device=DEV)
    coll = torch.full((S, N, T1, 2), 0xFF, dtype=torch.uint8, device=DEV)
    applied = torch.full((S, N, 2), float("nan"), dtype=torch.float64, device=DEV)
    cs = torch.full((S, int(lib.ctrlsim_sim_contact_floats(64)) + 2000), float("nan"), device=DEV)

    def init(n, e):
        return lib.ctrlsim_sim_init(S, n, e, p(pose), p(size), p(segs), p(exists), p(phys), p(hist), p(coll), T1, p(cs), st)

    def step(n, e, t, k_t, a_t, mode=0, t1=T1):
        return lib.ctrlsim_sim_step(S, n, e, k_t, a_t, disc, p(size), p(segs), p(exists), p(phys), p(hist), p(coll), p(applied), t, t1,
                                    sc.DT, mode, p(cs), st)
    assert init(0, E) != 0 and init(65, E) != 0 and init(4, -1) != 0
    assert step(0, E, 0, None, p(act)) != 0 and step(65, E, 0, None, p(act)) != 0 and step(4, -1, 0, None, p(act)) != 0
    assert step(4, E, T1 - 1, None, p(act)) != 0 and step(4, E, T1, p(tok), None) != 0 and step(4, E, 0, None, p(act), t1=1) != 0
    assert step(4, E, -1, None, p(act)) != 0
    assert step(4, E, 0, None, None) != 0
    assert lib.ctrlsim_sim_set_position(S, 0, p(xy), p(phys), st) != 0 and lib.ctrlsim_sim_set_position(S, 65, p(xy), p(phys), st) != 0
    assert lib.ctrlsim_sim_step_expert(S, 0, E, None, p(act), disc, p(size), p(segs), p(exists), p(phys), p(hist), p(coll), p(applied), 0,
                                       T1, sc.DT, p(cs), p(expert), st) != 0
    # expert rows are defined on the FreeCar / Box2D integrator only.  Neither C entry can ask for both (the expert entry has no mode,
    # the plain entry no expert pointer): the rule lives in the launcher both of them call, reached here by its C++ symbol
    launch = getattr(lib, "_Z15launch_sim_stepiiiPKiPKdS2_PKfS4_PKhPfS7_PhPdiifiS7_S4_P12ihipStream_t")
    launch.restype = C.c_int
    launch.argtypes = [C.c_int] * 3 + [C.c_void_p] * 10 + [C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    largs = lambda mode, ex: (S, 4, E, None, p(act), disc, p(size), p(segs), p(exists), p(phys), p(hist), p(coll), p(applied), 0, T1,
                              sc.DT, mode, p(cs), ex, st)
    assert launch(*largs(1, p(expert))) != 0
    torch.cuda.synchronize()
    assert torch.isnan(phys).all() and torch.isnan(hist).all() and (coll == 0xFF).all() and torch.isnan(applied).all()
    assert torch.isnan(cs).all()
