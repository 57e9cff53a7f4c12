"""CPU: the recipes of tests/sim_cases.py are fit for their purpose before a GPU sees them — every one is well conditioned (one float32
ulp on the initial headings moves no state column by more than a tenth of the 1e-4 bound and flips no flag), produces the flags and
events it promises, and tells a wrong simulator from a right one (three wrong-on-purpose oracle variants)."""
import numpy as np
import pytest

import sim_cases as sc


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in sc.all_cases()}


@pytest.fixture(scope="module")
def runs(cases):
    return {k: sc.run_oracle(c) for k, c in cases.items()}


NAMES = ["mixed", "tokens", "existence", "chunked", "requests"] + [f"sizes_{n}_{e}" for n, e in sc.SIZES]


@pytest.mark.parametrize("name", NAMES)
def test_recipe_is_well_conditioned(cases, name):
    diff, same_flags = sc.conditioning(cases[name])
    print(name, "largest change per state column for one ulp on the headings:", diff)
    assert diff.max() <= sc.COND, diff
    assert same_flags


@pytest.mark.parametrize("name", NAMES)
def test_recipe_produces_the_flags_it_promises(cases, runs, name):
    c, (states, flags, applied) = cases[name], runs[name]
    f = c["facts"]
    print(name, "vehicle flags", int(flags[..., 0].sum()), "edge flags", int(flags[..., 1].sum()))
    assert flags[..., 0].sum() >= f["min_veh_flags"] and flags[..., 1].sum() >= f["min_edge_flags"]
    if name.startswith("sizes"):
        assert flags[f["contact_free_scene"], ..., 0].sum() == 0
        if c["pose"].shape[1] >= 2:
            assert flags[1, ..., 0].sum() >= 2
    # every scene of a batch is a different scene
    S = c["pose"].shape[0]
    assert len({c["pose"][s].tobytes() + c["size"][s].tobytes() + c["segs"][s].tobytes() for s in range(S)}) == S


def test_mixed_has_a_sleeper_that_is_hit_and_a_clamped_vehicle(cases, runs):
    c, (states, flags, _) = cases["mixed"], runs["mixed"]
    s, v = c["facts"]["sleeper"]
    assert (c["act"][:, s, v] == 0).all()
    first_hit = int(np.argmax(flags[s, v, :, 0]))
    assert flags[s, v, :, 0].any() and first_hit >= 9          # stood for >= 8 steps (B2_TIMETOSLEEP = 0.5 s = 5 steps) before the hit
    assert (states[s, v, :first_hit, 3] == 0).all() and (states[s, v, :first_hit, :2] == states[s, v, 0, :2]).all()
    assert states[s, v, -1, 3] > 0 and np.abs(states[s, v, -1, :2] - states[s, v, 0, :2]).max() > 1e-3      # woken and pushed
    s, v = c["facts"]["clamped"]
    step0 = np.hypot(*(states[s, v, 1, :2].astype(np.float64) - states[s, v, 0, :2]))
    assert states[s, v, 0, 3] * sc.DT > 5.5 and 4.99 < step0 < 5.001                                       # 6 m asked, 5 m moved
    # the float64 scripts reach the setters' branch values
    a, st = c["act"][..., 0], c["act"][..., 1]
    assert ((np.abs(a) < 0.001) & (a != 0)).any() and (a == 0).any() and (st == 0).any() and ((np.abs(st) <= 1e-7) & (st != 0)).any()
    assert a.min() == -10.0 and a.max() == 10.0 and st.min() == -0.7 and st.max() == 0.7


def test_tokens_reach_the_corners_of_the_id_grid(cases, runs):
    c, (_, _, applied) = cases["tokens"], runs["tokens"]
    for tk in (0, sc.N_STEER - 1, sc.N_STEER, sc.N_ACCEL * sc.N_STEER - 1, sc.ZERO_TOKEN):
        assert (c["tok"] == tk).any(), tk
    assert applied[..., 0].min() == -10.0 and applied[..., 0].max() == 10.0
    assert applied[..., 1].min() == -0.7 and applied[..., 1].max() == 0.7


def _only_segment(case, k):
    d = dict(case)
    d["segs"] = case["segs"][:, k:k + 1].copy()
    return d


def test_sizes_cover_the_broad_phase_edges(cases, runs):
    # the long segment covers more than 16 cells of the 16 x 16 grid over the vehicles and does hit vehicles
    c, (states, flags, _) = cases["sizes_64_1000"], runs["sizes_64_1000"]
    k = c["facts"]["long_segment"]
    for s in range(2):
        lo, hi = states[s, :, 0, :2].min(0) - 3.0, states[s, :, 0, :2].max(0) + 3.0      # at least the vehicles' bounding box
        sg = c["segs"][s, k]
        cells = np.floor((np.array([[sg[0], sg[1]], [sg[2], sg[3]]]) - lo) / (hi - lo) * 16).clip(0, 15)
        assert np.prod(np.abs(cells[1] - cells[0]) + 1) > 16
    assert sc.run_oracle(_only_segment(c, k))[1][..., 1].sum() > 0
    # vehicles 32..63 are the only ones with edge hits in scene 0 of (64, 257); vehicle 32 of N = 33 has edge hits
    f = runs["sizes_64_257"][1]
    assert f[0, 32:, :, 1].sum() >= 20 and f[0, :32, :, 1].sum() == 0
    assert runs["sizes_33_257"][1][:, 32, :, 1].sum() > 0 and runs["sizes_33_256"][1][:, 32, :, 1].sum() > 0
    # from 32 vehicles on, one vehicle per scene stops existing mid-run (never two awake on the parking spot)
    for name in ("sizes_32_257", "sizes_33_0", "sizes_64_1000"):
        gone = cases[name]["exists"] == 0
        assert gone.any(0).sum(1).tolist() == [1, 1] and not gone[0].any() and gone[-1].sum() == 2
    # a segment that ends exactly ON the bounding box of a standing axis-aligned vehicle is no hit, one ulp further it is
    for name in ("sizes_1_257", "sizes_33_257", "sizes_64_1000"):
        c = cases[name]
        v, on, inside = c["facts"]["on_box"]
        assert sc.run_oracle(_only_segment(c, on))[1][0, v, :, 1].sum() == 0
        assert sc.run_oracle(_only_segment(c, inside))[1][0, v, :, 1].all()
    # the zero-length segment lies inside vehicle 0 of scene 1 at the start
    c = cases["sizes_2_257"]
    assert (c["segs"][1, 1, :2] == c["segs"][1, 1, 2:]).all() and sc.run_oracle(_only_segment(c, 1))[1][1, 0, 0, 1] == 1
    assert {(n, e) for n, e in sc.SIZES} >= {(n, e) for n in (1, 2, 32, 33, 64) for e in (0, 257)} | {(64, 1000), (2, 1), (33, 256)}


def test_existence_events(cases, runs):
    c, (states, flags, applied) = cases["existence"], runs["existence"]
    f, ex = c["facts"], c["exists"]
    for s, v in f["absent_on_edge_row0"]:
        assert ex[0, s, v] == 0 and flags[s, v, 0, 1] == 1            # absent in step 0, on a road edge in row 0
    s, t0 = f["nobody"]
    assert not ex[t0:, s].any() and ex[:t0, s].all()
    assert (states[s, :, t0 + 1:, :2] == sc.PARK).all()               # asleep: exactly on the parking spot, nothing pushes them
    s, v, t0 = f["one_live"]
    assert ex[t0:, s].sum(1).tolist() == [1] * (c["steps"] - t0) and ex[t0:, s, v].all()
    assert (np.delete(states[s], v, 0)[:, t0 + 1:, :2] == sc.PARK).all() and np.abs(states[s, v, :, :2]).max() < 100
    s, v, t0, t1 = f["returns"]
    assert not ex[t0:t1, s, v].any() and ex[t1:, s, v].all() and states[s, v, -1, 0] < -9e5 and states[s, v, -1, 3] > 0
    assert (applied[ex.transpose(1, 2, 0) == 0] == 0).all()
    # never two awake vehicles on the parking spot at once (see the recipe's docstring): scenes 0 and 3 park one vehicle, once
    assert (ex[:, [0, 3]] == 0).sum(2).max() == 1 and ((ex[:, [0, 3]] == 0).any(0).sum(1) == 1).all()


def test_requests_events(cases, runs):
    c, (states, flags, _) = cases["requests"], runs["requests"]
    f = c["facts"]
    s, v, onto, t = f["teleport_onto"]
    np.testing.assert_allclose(states[s, v, t + 1, :2], c["setpos"][t][s, v], atol=1.5)      # it landed there (then moved one step)
    assert flags[s, v, t + 1, 0] == 1 and flags[s, onto, t + 1, 0] == 1 and flags[s, onto, t, 0] == 0
    s, v, t = f["dropped_request"]
    assert c["exists"][t, s, v] == 0 and c["exists"][t + 1, s, v] == 1 and not np.isnan(c["setpos"][t][s, v]).any()
    assert states[s, v, t + 2, 0] < -9e5                                                       # revived where it was parked
    s, v, hit = f["expert_hits"]
    on = np.array([e is not None and not np.isnan(e[s, v, 0]) for e in c["expert"]])
    assert on[:4].all() and not on[4:8].any() and on[8:].all()                                 # on, off, on again
    assert flags[s, hit, :, 0].any() and np.isnan(c["expert"][0][0]).all() and np.isnan(c["expert"][0][1]).all()
    assert all(np.isnan(q[0]).all() for q in c["setpos"] if q is not None)                    # scene 0 has no request at all


def _worst(case, ref, wrong):
    (s0, f0, a0), (s1, f1, a1) = ref, wrong
    cols = list(sc.STATE_COLS)
    return np.abs(s0[..., cols].astype(np.float64) - s1[..., cols]).max(), not np.array_equal(f0, f1)


def test_wrong_on_purpose_oracles_are_told_apart(cases, runs):
    """Each variant must move a compared quantity by at least 100 x 1e-4, or flip a flag: the recipes can see the errors they are
    meant to catch."""
    d, flipped = _worst(cases["existence"], runs["existence"], sc.run_oracle(cases["existence"], ignore_existence=True))
    print("existence ignored:", d, flipped)
    assert d >= 100 * sc.ATOL or flipped
    d, flipped = _worst(cases["mixed"], runs["mixed"], sc.run_oracle(cases["mixed"], shift_scene_data=True))
    print("sizes and edges of the next scene:", d, flipped)
    assert d >= 100 * sc.ATOL or flipped
    for name in ("chunked", "requests", "sizes_33_257"):
        d, flipped = _worst(cases[name], runs[name], sc.run_oracle(cases[name], shift_scene_data=True))
        assert d >= 100 * sc.ATOL or flipped, name
    wrong = sc.run_oracle(cases["tokens"], swap_token_grid=True)
    d, flipped = _worst(cases["tokens"], runs["tokens"], wrong)
    print("token grid transposed:", d, flipped)
    assert d >= 100 * sc.ATOL or flipped
    assert np.abs(wrong[2] - runs["tokens"][2]).max() >= 100 * sc.ATOL
