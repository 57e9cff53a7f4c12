"""TEST INFRASTRUCTURE — recipes for direct tests of the simulator step (csrc/sim.hip) on batches of DIFFERENT scenes, and the two
drivers that run a recipe through the CPU oracle (oracle/sim_oracle.c, pinned to the real FreeCar / Box2D by tests/test_oracle_pinned.py)
and through ctrlsim_sim_init / _set_position / _step / _step_expert.

A case is a dict of numpy arrays for S scenes:
  pose [S,N,4] float32 (x, y, heading, speed)   size [S,N,2] float32 (length, width)   segs [S,E,4] float32 road-edge segments
  exists [steps,S,N] uint8                      act [steps,S,N,2] float64 (accel, steer)  OR  tok [steps,S,N] int32
  setpos: None or a list of `steps` entries, each None or [S,N,2] float32 (NaN = no request), issued before that step
  expert: None or a list of `steps` entries, each None or [S,N,4] float32 (x = NaN = not an expert in that step)
Host-only facts the recipes promise (which vehicle sleeps, which segment is the long one, ...) are under case["facts"].

Used by tests/test_sim_cases_host.py (CPU: conditioning, promised events, wrong-on-purpose oracles) and tests/test_gpu_sim_step.py."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

import sim_libs
from ctrlsim_amd import spec
from ctrlsim_amd.discretize import undiscretize_actions

W = spec.make_cfg().dataset.waymo
N_ACCEL, N_STEER = int(W.accel_discretization), int(W.steer_discretization)
ZERO_TOKEN = 524
DISC6 = (float(W.min_accel), float(W.max_accel), float(W.min_steer), float(W.max_steer), float(N_ACCEL), float(N_STEER))
PARK = -1000000.0
DT = 0.1
ATOL = 1e-4                # the project's trajectory bound (tests/test_gpu_sim_ctx.py: "north-star: 1e-4 on trajectories")
COND = 1e-5                # a tenth of it: what one float32 ulp on every initial heading may move a state column
CU_NOMINAL = 256           # compute units of an MI355X: the host tests size the "chunked" recipe with it
STATE_COLS = (0, 1, 2, 4, 5)   # of the oracle's rows x, y, heading, speed, vx, vy: the ones the history row holds
HIST_COLS = (0, 1, 4, 2, 3)    # the same five in a history row x, y, vx, vy, heading, length, width, existence


# ------------------------------------------------------------------------------------------------------------------ scene pieces
def _sizes(rs, n):
    return np.stack([rs.uniform(4.0, 5.5, n), rs.uniform(1.8, 2.3, n)], 1).astype(np.float32)


def _lattice(rs, n, spacing, jitter, speed_hi):
    """n vehicles on a square lattice (no two start overlapping for spacing >= 7), random headings and speeds."""
    k = int(np.ceil(np.sqrt(n)))
    ij = np.stack([np.arange(n) % k, np.arange(n) // k], 1).astype(np.float64)
    xy = (ij - (k - 1) / 2.0) * spacing + rs.uniform(-jitter, jitter, (n, 2))
    pose = np.zeros((n, 4), np.float32)
    pose[:, :2] = xy
    pose[:, 2] = rs.uniform(-np.pi, np.pi, n)
    pose[:, 3] = rs.uniform(0.0, speed_hi, n)
    return pose


def _segments(rs, e, lo, hi, max_len=6.0):
    """e random segments with one end in the box [lo, hi] and the other at most max_len away."""
    segs = np.zeros((e, 4), np.float32)
    if e:
        segs[:, :2] = rs.uniform(lo, hi, (e, 2))
        segs[:, 2:] = segs[:, :2] + rs.uniform(-max_len, max_len, (e, 2)).astype(np.float32)
    return segs


def _actions(rs, steps, n, a_hi=10.0, s_hi=0.7):
    """Float64 actions over the whole range, with the values at which the setters branch: |accel| < 0.001 (a brake request that is
    ignored), accel exactly 0, steer exactly 0 and |steer| <= 1e-7 (no steering radius)."""
    act = np.stack([rs.uniform(-a_hi, a_hi, (steps, n)), rs.uniform(-s_hi, s_hi, (steps, n))], -1)
    sp_a = np.array([0.0, 0.0005, -0.0005, -0.000999, 0.001, -0.001, -a_hi, a_hi])
    sp_s = np.array([0.0, 1e-7, -1e-7, 5e-8, 2e-7, -s_hi, s_hi])
    m = rs.rand(steps, n) < 0.25
    act[..., 0][m] = sp_a[rs.randint(0, len(sp_a), int(m.sum()))]
    m = rs.rand(steps, n) < 0.25
    act[..., 1][m] = sp_s[rs.randint(0, len(sp_s), int(m.sum()))]
    return act


def _stack(name, scenes, steps, **extra):
    case = dict(name=name, steps=steps, pose=np.stack([s["pose"] for s in scenes]).astype(np.float32),
                size=np.stack([s["size"] for s in scenes]).astype(np.float32),
                segs=np.stack([s["segs"] for s in scenes]).astype(np.float32).reshape(len(scenes), -1, 4),
                setpos=None, expert=None, facts={})
    S, N = case["pose"].shape[:2]
    case["exists"] = np.ones((steps, S, N), np.uint8)
    if all("act" in s for s in scenes):
        case["act"] = np.stack([s["act"] for s in scenes], 1).astype(np.float64)
    case.update(extra)
    return case


def dims(case):
    S, N = case["pose"].shape[:2]
    return S, N, case["segs"].shape[1], case["steps"]


# ------------------------------------------------------------------------------------------------------------------ (a) mixed
def _mixed_scenes(seed, steps=12, N=8, E=24):
    scenes = []
    # 0: open road — a column of cars driving east between two kerbs, some kerb pieces across their lanes
    rs = np.random.RandomState(seed * 100 + 0)
    pose = np.zeros((N, 4), np.float32)
    pose[:, 0] = rs.uniform(-3, 3, N); pose[:, 1] = (np.arange(N) - (N - 1) / 2) * 6.0
    pose[:, 2] = rs.uniform(-0.15, 0.15, N); pose[:, 3] = rs.uniform(3, 14, N)
    segs = _segments(rs, E, (-4, -24), (22, 24), 5.0)
    segs[0] = (-40, -27, 40, -27); segs[1] = (-40, 27, 40, 27)
    scenes.append(dict(pose=pose, size=_sizes(rs, N), segs=segs, act=_actions(rs, steps, N, 6.0, 0.3)))
    # 1: a two-car encounter (0 and 1 head-on, slightly offset), the rest spread out
    rs = np.random.RandomState(seed * 100 + 1)
    pose = _lattice(rs, N, 15.0, 2.0, 6.0)
    pose[0] = (-40.0, -40.0, 0.05, 7.0); pose[1] = (-29.0, -39.4, np.pi - 0.1, 6.0)
    act = _actions(rs, steps, N, 5.0, 0.4)
    act[:, :2, 0] = rs.uniform(0.5, 2.0, (steps, 2)); act[:, :2, 1] = rs.uniform(-0.05, 0.05, (steps, 2))
    scenes.append(dict(pose=pose, size=_sizes(rs, N), segs=_segments(rs, E, -28, 28), act=act))
    # 2: vehicle 0 stands with the zero action (asleep after B2_TIMETOSLEEP = 0.5 s), vehicle 1 coasts into it around step 9
    rs = np.random.RandomState(seed * 100 + 2)
    pose = _lattice(rs, N, 14.0, 2.0, 8.0)
    size = _sizes(rs, N)
    pose[0] = (50.0, 50.0, 0.0, 0.0)
    gap = 7.3                                          # front bumper of 1 to rear bumper of 0, covered at 0.8 m per step
    pose[1] = (50.0 - 0.5 * (size[0, 0] + size[1, 0]) - gap, 50.2, 0.0, 8.0)
    act = _actions(rs, steps, N, 8.0, 0.5)
    act[:, 0] = 0.0; act[:, 1] = 0.0
    scenes.append(dict(pose=pose, size=size, segs=_segments(rs, E, -26, 26), act=act))
    # 3: vehicle 0 starts at 60 m/s: 6 m per step, clamped to B2_MAXTRANSLATION = 5 m
    rs = np.random.RandomState(seed * 100 + 3)
    pose = _lattice(rs, N, 13.0, 3.0, 10.0)
    pose[0] = (-60.0, 40.0, 0.3, 60.0)
    act = _actions(rs, steps, N)
    act[0, 0] = (0.0, 0.0)
    scenes.append(dict(pose=pose, size=_sizes(rs, N), segs=_segments(rs, E, -24, 24), act=act))
    # 4: a tighter lot, full-range actions: several soft collisions
    rs = np.random.RandomState(seed * 100 + 4)
    scenes.append(dict(pose=_lattice(rs, N, 8.0, 1.0, 5.0), size=_sizes(rs, N), segs=_segments(rs, E, -14, 14),
                       act=_actions(rs, steps, N)))
    return scenes


def mixed(seed=None):
    seed = SEEDS["mixed"] if seed is None else seed
    c = _stack("mixed", _mixed_scenes(seed), 12)
    c["facts"] = dict(sleeper=(2, 0), clamped=(3, 0), min_veh_flags=24, min_edge_flags=70)
    return c


# ------------------------------------------------------------------------------------------------------------------ (b) tokens
def tokens(seed=None):
    """The scenes of `mixed`, driven by action tokens: uniformly drawn ids plus the corners of the id grid and the zero-action token."""
    seed = SEEDS["tokens"] if seed is None else seed
    scenes = _mixed_scenes(SEEDS["mixed"])
    c = _stack("tokens", scenes, 12)
    del c["act"]
    S, N, _, steps = dims(c)
    rs = np.random.RandomState(seed)
    tok = rs.randint(0, N_ACCEL * N_STEER, (steps, S, N)).astype(np.int32)
    # gentle ids (accel bins 8..12, steer bins 20..29) for most vehicles keep the runs well conditioned
    calm = rs.rand(steps, S, N) < 0.6
    tok[calm] = (rs.randint(8, 13, int(calm.sum())) * N_STEER + rs.randint(20, 30, int(calm.sum()))).astype(np.int32)
    special = [0, N_STEER - 1, N_STEER, N_ACCEL * N_STEER - 1, ZERO_TOKEN]
    for k, tk in enumerate(special):
        for s in range(S):
            tok[(k + s) % steps, s, (2 * k + s) % N] = tk
    c["tok"] = tok
    c["facts"] = dict(special=special, min_veh_flags=20, min_edge_flags=80)
    return c


# ------------------------------------------------------------------------------------------------------------------ (c) existence
def existence(seed=None):
    seed = SEEDS["existence"] if seed is None else seed
    """Every non-existing vehicle is moved to the SAME point (-1e6, -1e6) at every step.  Two awake boxes with one common centre are a
    centrally symmetric configuration: b2FindMaxSeparation's choice between an edge and the opposite edge is a tie that rounding
    decides, at coordinates whose float32 spacing is 0.0625 m — one ulp on a heading moves such a pair by 1e-3 after ONE step, in the
    oracle and in the real Box2D alike.  No bound of 1e-4 can hold there, so the recipe never has two AWAKE vehicles parked at once:
    scenes 0 and 3 park one vehicle at a time; in scenes 1 and 2 the vehicles that leave stood still long enough to be asleep (Box2D
    skips contacts between sleeping bodies, and b2Body::SetTransform does not wake)."""
    seed = SEEDS["existence"] if seed is None else seed
    steps, N, E = 10, 6, 16
    scenes = []
    for s in range(4):
        rs = np.random.RandomState(seed * 100 + s)
        pose = _lattice(rs, N, 9.0, 1.5, 7.0)
        act = _actions(rs, steps, N, 6.0, 0.4)
        if s in (1, 2):                                 # a car park: everybody stands with the zero action and is asleep by step 5
            pose[:, 3] = 0.0
            act[:] = 0.0
        segs = _segments(rs, E, -12, 12)
        for v in range(N):                              # a kerb piece through every start pose: an absent vehicle is ON an edge in row 0
            segs[v] = (pose[v, 0] - 1.0, pose[v, 1] - 0.2, pose[v, 0] + 1.0, pose[v, 1] + 0.3)
        scenes.append(dict(pose=pose, size=_sizes(rs, N), segs=segs, act=act))
    # scene 2: vehicle 3 is the one that stays and drives (its lattice place is a corner, it heads away from the others)
    scenes[2]["pose"][3, 2:] = (np.arctan2(scenes[2]["pose"][3, 1], scenes[2]["pose"][3, 0]), 6.0)
    scenes[2]["act"][:, 3] = _actions(np.random.RandomState(seed * 100 + 60), steps, 1, 4.0, 0.2)[:, 0]
    c = _stack("existence", scenes, steps)
    ex = c["exists"]
    # (a vehicle that comes back drives on from the parking spot and stays within a car's length of it for the rest of the run, so
    # no scene parks another one after a return)
    ex[:3, 0, 5] = 0                                   # scene 0: 5 is absent from step 0 and appears (at the parking spot) in step 3
    ex[7:, 1, :] = 0                                   # scene 1: from step 7 nobody exists (gany = 0 in rows 8..10)
    ex[7:, 2, :] = 0; ex[:, 2, 3] = 1                  # scene 2: from step 7 exactly one live vehicle (the grid is its own box)
    ex[4:7, 3, 2] = 0                                  # scene 3: 2 vanishes mid-run, is parked for three steps and comes back
    c["facts"] = dict(absent_on_edge_row0=((0, 5),), nobody=(1, 7), one_live=(2, 3, 7), returns=(3, 2, 4, 7),
                      min_veh_flags=20, min_edge_flags=100)
    return c


# ------------------------------------------------------------------------------------------------------------------ (d) sizes
SIZES = [(1, 0), (1, 257), (2, 0), (2, 1), (2, 257), (32, 0), (32, 257), (33, 0), (33, 256), (33, 257), (64, 0), (64, 257), (64, 1000)]


def sizes(N, E, seed=None):
    """Two scenes of N vehicles and E segments, 6 steps: scene 0 contact-free (a wide lattice, slow), scene 1 with contacts (a tight
    lattice).  With segments: segment 0 spans the whole scene, segment 1 has zero length and lies inside vehicle 0 of scene 1,
    segment 2 ends exactly ON the bounding box of the axis-aligned, standing last vehicle and segment 3 one ulp inside it; in scene 0 of
    (64, 257) only vehicles 32..63 have segments anywhere near them.  From 32 vehicles on, one vehicle per scene stops existing
    mid-run (vehicle 5 in scene 0, vehicle N - 2 in scene 1)."""
    seed = SEEDS["sizes"] if seed is None else seed
    steps = 6
    scenes = []
    for s, (spacing, speed_hi, a_hi) in enumerate(((16.0, 4.0, 3.0), (7.0, 6.0, 6.0))):
        rs = np.random.RandomState(seed * 10000 + N * 100 + (E % 97) * 2 + s)
        pose = _lattice(rs, N, spacing, 1.0, speed_hi)
        size = _sizes(rs, N)
        act = _actions(rs, steps, N, a_hi, 0.4)
        last = N - 1
        pose[last, 2:] = 0.0                            # axis-aligned and standing, zero action: its box never moves
        act[:, last] = 0.0
        if s == 1 and N >= 2:                           # vehicle 0 drives into vehicle 1 (which drives towards it when N > 2)
            pose[0] = (pose[1, 0] - 6.4, pose[1, 1] + 0.4, 0.05, 6.0)
            act[:, 0] = (1.0, 0.0)
            if N > 2:
                pose[1, 2:] = (np.pi - 0.05, 4.0)
        half = 0.5 * spacing * int(np.ceil(np.sqrt(N))) + 4.0
        lo, hi = (-half, -half), (half, half)
        if (N, E, s) == (64, 257, 0):                   # lattice rows 4..7 hold vehicles 32..63
            lo = (-half, 2.0)
        segs = _segments(rs, E, lo, hi)
        if E >= 4:
            segs[0] = (-half - 3.0, lo[1] + 1.0, half + 3.0, half - 2.0)
            segs[1] = (pose[0, 0], pose[0, 1], pose[0, 0], pose[0, 1]) if s == 1 else (half, half, half, half)
            right = np.float32(np.float32(size[last, 0] * np.float32(0.5)) + pose[last, 0])   # the kernel's corner expression at heading 0
            segs[2] = (right, pose[last, 1], right + np.float32(3.0), pose[last, 1] + np.float32(0.5))
            segs[3] = (np.nextafter(right, np.float32(-np.inf)), pose[last, 1], right + np.float32(3.0), pose[last, 1] - np.float32(0.5))
        elif E == 1:
            segs[0] = (pose[0, 0] - 1.0, pose[0, 1], pose[0, 0] + 30.0, pose[0, 1] + 2.0)
        scenes.append(dict(pose=pose, size=size, segs=segs, act=act))
    c = _stack(f"sizes_{N}_{E}", scenes, steps)
    if N >= 32:                                         # one vehicle per scene leaves mid-run: a hole in the grid's live mask
        c["exists"][3:, 0, 5] = 0
        c["exists"][2:, 1, N - 2] = 0
    c["facts"] = dict(contact_free_scene=0, long_segment=0 if E >= 4 else None, on_box=(N - 1, 2, 3) if E >= 4 else None,
                      min_veh_flags=(0 if N == 1 else 4 if N == 2 else 8),
                      min_edge_flags=(0 if E == 0 else 10 if E == 1 else 7 * min(N, 2) if N <= 2 else 150))
    return c


# ------------------------------------------------------------------------------------------------------------------ (e) chunked
def chunked(S=CU_NOMINAL + 37, seed=None):
    """More scenes than compute units, every scene different (scene s depends on (seed, s) only, so a prefix is a prefix)."""
    seed = SEEDS["chunked"] if seed is None else seed
    steps, N, E = 3, 4, 8
    scenes = []
    for s in range(S):
        rs = np.random.RandomState(seed * 100000 + s)
        pose = _lattice(rs, N, 6.5 if s % 3 == 0 else 10.0, 0.8, 8.0)
        scenes.append(dict(pose=pose, size=_sizes(rs, N), segs=_segments(rs, E, -9, 9), act=_actions(rs, steps, N)))
    c = _stack("chunked", scenes, steps)
    c["facts"] = dict(min_veh_flags=S // 8, min_edge_flags=4 * S)
    return c


# ------------------------------------------------------------------------------------------------------------------ (f) requests
def requests(seed=None):
    seed = SEEDS["requests"] if seed is None else seed
    steps, S, N, E = 12, 3, 6, 12
    scenes = []
    for s in range(S):
        rs = np.random.RandomState(seed * 100 + s)
        scenes.append(dict(pose=_lattice(rs, N, 10.0, 1.5, 6.0), size=_sizes(rs, N), segs=_segments(rs, E, -12, 12),
                           act=_actions(rs, steps, N, 5.0, 0.4)))
    # scene 2: vehicle 0 stands and brakes; vehicle 1's log drives over it
    scenes[2]["pose"][0, 2:] = (0.0, 0.0)
    scenes[2]["act"][:, 0] = (-3.0, 0.0)
    c = _stack("requests", scenes, steps)
    nan2, nan4 = np.full((S, N, 2), np.nan, np.float32), np.full((S, N, 4), np.nan, np.float32)
    setpos, expert = [None] * steps, [None] * steps
    p1 = c["pose"][1]
    setpos[3] = nan2.copy()
    setpos[3][1, 2] = (p1[0, 0] + 0.6, p1[0, 1] + 0.3)           # scene 1: vehicle 2 lands on top of vehicle 0's start area
    c["act"][:, 1, 0] = (0.0, 0.0); c["pose"][1, 0, 3] = 0.0      # ... which stands there
    setpos[5] = nan2.copy()
    setpos[5][1, 4] = (p1[3, 0] + 0.5, p1[3, 1])                 # scene 1: a request to vehicle 4, parked in this very step and
    c["exists"][5, 1, 4] = 0                                     # revived in the next: the request must not fire then
    setpos[8] = nan2.copy()
    setpos[8][1, 5] = (30.0, -30.0)                              # an ordinary move into the open
    p2 = c["pose"][2]
    for t in range(steps):                                       # scene 2: 1 is an expert except in steps 4..7, 3 only in steps 2..5
        row = nan4.copy()
        if not 4 <= t < 8:
            row[2, 1] = (p2[0, 0] - 7.0 + 0.8 * (t + 1), p2[0, 1] + 0.3, 0.04, 8.0)
        if 2 <= t < 6:
            row[2, 3] = (p2[3, 0] + 0.5 * (t + 1), p2[3, 1] + 0.2 * (t + 1), 0.4 + 0.02 * t, 5.0)
        expert[t] = row
    c["setpos"], c["expert"] = setpos, expert
    c["facts"] = dict(teleport_onto=(1, 2, 0, 3), dropped_request=(1, 4, 5), expert_hits=(2, 1, 0), min_veh_flags=20, min_edge_flags=40)
    return c


# the seeds: chosen on the CPU so that every promise in case["facts"] holds and the runs are well conditioned (conditioning());
# tests/test_sim_cases_host.py re-checks both for exactly these seeds
SEEDS = dict(mixed=2, tokens=5, existence=1, sizes=4, chunked=1, requests=4)


def all_cases(S_chunked=CU_NOMINAL + 37):
    out = [mixed(), tokens(), existence(), chunked(S_chunked), requests()]
    out += [sizes(n, e) for n, e in SIZES]
    return out


# ------------------------------------------------------------------------------------------------------------------ oracle driver
def decode_tokens(tok, n_accel=N_ACCEL, n_steer=N_STEER):
    w = SimpleNamespace(accel_discretization=n_accel, steer_discretization=n_steer, min_accel=W.min_accel, max_accel=W.max_accel,
                        min_steer=W.min_steer, max_steer=W.max_steer)
    return undiscretize_actions(tok, w)


def run_oracle(case, heading_ulps=0, ignore_existence=False, shift_scene_data=False, swap_token_grid=False):
    """One OracleSim per scene, driven as the rollout drives the reference (oracle/rollout_oracle.py: act()).
    -> states [S,N,steps+1,6] (x, y, heading, speed, vx, vy), flags [S,N,steps+1,2], applied [S,N,steps,2] float64.
    The keyword arguments are for the host tests: heading_ulps perturbs every initial heading; the other three are the
    wrong-on-purpose variants (existence ignored, scene s run with the sizes and edges of scene s + 1, token grid transposed)."""
    sim_libs.build_oracle()
    S, N, E, steps = dims(case)
    states = np.zeros((S, N, steps + 1, 6), np.float32)
    flags = np.zeros((S, N, steps + 1, 2), np.uint8)
    applied = np.zeros((S, N, steps, 2), np.float64)
    if "tok" in case:
        act = decode_tokens(case["tok"], *((N_STEER, N_ACCEL) if swap_token_grid else (N_ACCEL, N_STEER)))
    else:
        act = case["act"]
    for s in range(S):
        d = (s + 1) % S if shift_scene_data else s
        pose, size, segs = case["pose"][s], case["size"][d], case["segs"][d]
        h = pose[:, 2].copy()
        for _ in range(abs(heading_ulps)):
            h = np.nextafter(h, np.float32(np.inf if heading_ulps > 0 else -np.inf))
        o = sim_libs.OracleSim(size[:, 0], size[:, 1], pose[:, 0], pose[:, 1], h, pose[:, 3], segs)

        def read(t):
            st, cv, ce = o.state()
            states[s, :, t] = st
            flags[s, :, t, 0], flags[s, :, t, 1] = cv, ce
        read(0)
        for t in range(steps):
            sp = case["setpos"][t] if case["setpos"] is not None else None
            ex = case["expert"][t] if case["expert"] is not None else None
            for v in range(N):
                if sp is not None and not np.isnan(sp[s, v]).any():
                    o.set_position(v, sp[s, v, 0], sp[s, v, 1])
                if not case["exists"][t, s, v] and not ignore_existence:
                    o.set_position(v, PARK, PARK)
                    a, st_ = 0.0, 0.0
                else:
                    a, st_ = act[t, s, v]
                o.set_action(v, a, st_)
                applied[s, v, t] = (a, st_)
                if ex is not None and not np.isnan(ex[s, v, 0]):
                    o.set_expert(v, *[float(q) for q in ex[s, v]])
            o.step(DT)
            read(t + 1)
        o.close()
    return states, flags, applied


def conditioning(case):
    """Largest state difference between the oracle run and the run with every initial heading one float32 ulp up, per state column,
    and whether the flags are identical.  Rows of a parked vehicle (|x| ~ 1e6, float32 spacing 0.0625) are compared too."""
    a, fa, _ = run_oracle(case)
    b, fb, _ = run_oracle(case, heading_ulps=1)
    diff = np.abs(a.astype(np.float64) - b.astype(np.float64)).reshape(-1, 6).max(0)
    return diff, bool(np.array_equal(fa, fb))


# ------------------------------------------------------------------------------------------------------------------ GPU driver
def run_gpu(case, contacts=True, scenes=None):
    """The same case through the C ABI, whole batch per call.  phys / contact_state start as NaN, history rows as NaN, flags as 0xFF,
    applied as NaN; Tmax1 = steps + 3.  -> states [S,N,steps+1,8] (history rows), flags, applied, info dict (fill_ok, guard).
    scenes: a list of scene indices to run as a smaller batch of their own."""
    import torch
    from ctrlsim_amd import _lib
    lib, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    idx = list(range(case["pose"].shape[0])) if scenes is None else list(scenes)
    S, (_, N, E, steps) = len(idx), dims(case)
    T1 = steps + 3
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    pose, size = dev(case["pose"][idx]), dev(case["size"][idx])
    segs = dev(case["segs"][idx]) if E else torch.zeros(1, 4, device="cuda:0")
    exists = dev(case["exists"][:, idx])
    act = dev(case["act"][:, idx]) if "act" in case else None
    tok = dev(case["tok"][:, idx]) if "tok" in case else None
    phys = torch.full((S, N, 20), float("nan"), device="cuda:0")
    hist = torch.full((S, N, T1, 8), float("nan"), device="cuda:0")
    coll = torch.full((S, N, T1, 2), 0xFF, dtype=torch.uint8, device="cuda:0")
    applied = torch.full((steps, S, N, 2), float("nan"), dtype=torch.float64, device="cuda:0")
    cstate = torch.full((S, int(lib.ctrlsim_sim_contact_floats(N))), float("nan"), device="cuda:0") if contacts else None
    disc = (C.c_double * 6)(*DISC6)
    lib.ctrlsim_nonfinite_count(1)
    _lib.check(lib.ctrlsim_sim_init(S, N, E, p(pose), p(size), p(segs), p(exists[0]), p(phys), p(hist), p(coll), T1, p(cstate), st),
               "sim_init")
    keep = []
    for t in range(steps):
        sp = case["setpos"][t] if case["setpos"] is not None else None
        ex = case["expert"][t] if case["expert"] is not None else None
        if sp is not None:
            keep.append(dev(sp[idx]))
            _lib.check(lib.ctrlsim_sim_set_position(S, N, p(keep[-1]), p(phys), st), "sim_set_position")
        a_t, k_t = (p(act[t]) if act is not None else None), (p(tok[t]) if tok is not None else None)
        if ex is not None:
            keep.append(dev(ex[idx]))
            _lib.check(lib.ctrlsim_sim_step_expert(S, N, E, k_t, a_t, disc, p(size), p(segs), p(exists[t]), p(phys), p(hist), p(coll),
                                                   p(applied[t]), t, T1, DT, p(cstate), p(keep[-1]), st), "sim_step_expert")
        else:
            _lib.check(lib.ctrlsim_sim_step(S, N, E, k_t, a_t, disc, p(size), p(segs), p(exists[t]), p(phys), p(hist), p(coll),
                                            p(applied[t]), t, T1, DT, 0, p(cstate), st), "sim_step")
    torch.cuda.synchronize()
    h, c = hist.cpu().numpy(), coll.cpu().numpy()
    info = dict(fill_ok=bool(np.isnan(h[:, :, steps + 1:]).all() and (c[:, :, steps + 1:] == 0xFF).all()
                             and not np.isnan(h[:, :, :steps + 1]).any()),
                guard=int(lib.ctrlsim_nonfinite_count(0)))
    return h[:, :, :steps + 1], c[:, :, :steps + 1], applied.cpu().numpy().transpose(1, 2, 0, 3), info


def expected_history_tail(case):
    """Columns 5..7 of the history rows: length, width, and the existence byte the row was written with (row 0: step 0's)."""
    S, N, _, steps = dims(case)
    out = np.zeros((S, N, steps + 1, 3), np.float32)
    out[..., 0] = case["size"][:, :, None, 0]
    out[..., 1] = case["size"][:, :, None, 1]
    ex = case["exists"].astype(np.float32).transpose(1, 2, 0)
    out[:, :, 0, 2] = ex[:, :, 0]
    out[:, :, 1:, 2] = ex
    return out


def state_errors(case, hist, states):
    """max |GPU - oracle| per compared state column (x, y, heading, vx, vy)."""
    return np.array([np.abs(hist[..., hc].astype(np.float64) - states[..., sc].astype(np.float64)).max()
                     for hc, sc in zip(HIST_COLS, STATE_COLS)])
