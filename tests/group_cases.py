"""TEST INFRASTRUCTURE (no GPU, no library) for ctrlsim_group_build (csrc/context.hip: group_build_kernel).

group_ref      the focal grouping of ONE scenario at one step in plain Python loops and sets, written from the reference
               (policies/autoregressive_policy.py:86-137, datasets/rl_waymo/dataset.py:278-302) and the contract in include/ctrlsim.h.
               It shares no code with the kernel and none with oracle/features_oracle.py.
recipes        small scenes built so that the kernel's branches are reached on purpose: distances exactly at the threshold and one
               float32 ulp to either side, rank ties across the cut at A, the list-mutated-while-iterated quirk, persisted sets over
               several steps, window row w0 against row t, the sizes 1, 2, 63, 64 and 300 scenarios in one call.
twins          wrong-on-purpose variants of group_ref (one deviation each): tests/test_group_cases_host.py shows that every one of them
               changes a compared table on some recipe.
expected / compare_tables   the arrays the kernel leaves in pattern-filled buffers, and the comparison the GPU test makes.

Vehicle sets are Python ints used as 64-bit masks (bit v = vehicle v) where they stand for the kernel's tables."""
import math

import numpy as np

THR = 60.0                         # cfg.dataset.waymo.agent_dist_threshold
FILL = 0xA5                        # byte pattern of every output buffer before a call
TWINS = ("no_quirk", "le_threshold", "ties_high", "dist_at_t", "exist_at_w0", "readmit", "no_inherit", "tilt_all", "own_last",
         "late_empty")
TABLES = ("n_groups", "grp_focal", "grp_ids", "grp_members", "own_g", "mem_g", "tilted", "persist")
DTYPES = dict(n_groups=np.int32, grp_focal=np.int32, grp_ids=np.uint64, grp_members=np.uint64, own_g=np.int32, mem_g=np.int32,
              tilted=np.uint8, persist=np.uint64)


def bits(m):
    return [v for v in range(64) if (int(m) >> v) & 1]


def mask(vs):
    m = 0
    for v in vs:
        m |= 1 << int(v)
    return m


def distance(hs, f, row):
    """Distances of all vehicles to vehicle f at history row `row`: float32 positions widened to float64, sqrt(dx*dx + dy*dy)."""
    fx, fy = float(hs[f, row, 0]), float(hs[f, row, 1])
    out = []
    for v in range(hs.shape[0]):
        dx, dy = fx - float(hs[v, row, 0]), fy - float(hs[v, row, 1])
        out.append(math.sqrt(dx * dx + dy * dy))
    return out


def group_ref(hs, order, persist, A, T, t, thr, has_roads, twin=None):
    """hs [N,Tmax1,8] float32, order [N] (-1 padded), persist: N masks (0 = no set yet).  Returns a dict: n_groups, grp_focal / grp_ids /
    grp_members (lists of n_groups entries), persist / own_g / mem_g / tilted (lists of N entries), and `ev`, the events of this step
    (vehicles dropped from a persisted set because they left the disc; fresh selections at t > 0, the late-vehicle rule)."""
    assert twin is None or twin in TWINS
    N = hs.shape[0]
    w0 = 0 if t < T else t - (T - 1)
    pos_row = t if twin == "dist_at_t" else w0
    exist_row = w0 if twin == "exist_at_w0" else t
    exist = [hs[v, exist_row, 7] != 0 for v in range(N)]
    sets = [set(bits(m)) for m in persist]
    todo = [int(v) for v in order if v >= 0]
    focals, ids_of, members_of = [], [], []
    own_g, mem_g, tilted = [-1] * N, [-1] * N, [0] * N
    ev = dict(departures=0, late=0)
    while len(todo) > 0:
        f = todo.pop(0)
        if not exist[f] or not has_roads:
            continue                                          # dead_agent_veh_ids: no group, mem_g stays -1
        d = distance(hs, f, pos_row)
        valid = {v for v in range(N) if (d[v] <= thr if twin == "le_threshold" else d[v] < thr)}
        if t == 0 or len(sets[f]) == 0 or twin == "readmit":
            if t > 0 and len(sets[f]) == 0:
                ev["late"] += 1
                if twin == "late_empty":
                    continue
            ranked = sorted(range(N), key=(lambda v: (d[v], -v)) if twin == "ties_high" else (lambda v: (d[v], v)))
            ids = set(ranked[:A]) & valid
        else:
            ids = sets[f] & valid
            ev["departures"] += len(sets[f] - valid)
        members = [f]
        i = 0
        while i < len(todo):                                  # the list is mutated while it is iterated
            if todo[i] in ids:
                members.append(todo[i])
                del todo[i]
                if twin == "no_quirk":
                    continue
            i += 1
        g = len(focals)
        for m in ([f] if twin == "no_inherit" else members):
            sets[m] = set(ids)
        for m in members:
            mem_g[m] = g
        for v in ids:
            if own_g[v] < 0 or twin == "own_last":
                own_g[v] = g
                tilted[v] = 1 if (v in members or twin == "tilt_all") else 0
        focals.append(f); ids_of.append(mask(ids)); members_of.append(mask(members))
    return dict(n_groups=len(focals), grp_focal=focals, grp_ids=ids_of, grp_members=members_of, persist=[mask(s) for s in sets],
                own_g=own_g, mem_g=mem_g, tilted=tilted, ev=ev)


def run_recipe(rec, twin=None):
    """group_ref over the recipe's steps in sequence, persist carried from step to step (zero before the first).
    Returns out[k][s] = group_ref's dict of step rec["steps"][k], scenario s; its ev["inheritances"] counts the focals of that step
    that took the persisted branch with a set they last received as a folded member of another focal's group."""
    S, N = rec["order"].shape
    persist = [[0] * N for _ in range(S)]
    folded = [[False] * N for _ in range(S)]                  # the vehicle's set was last written while it was a folded member
    out = []
    for t in rec["steps"]:
        row = []
        for s in range(S):
            r = group_ref(rec["hs"][s], rec["order"][s], persist[s], rec["A"], rec["T"], t, rec["thr"], rec["has_roads"], twin)
            r["ev"]["inheritances"] = sum(1 for f in r["grp_focal"] if t > 0 and persist[s][f] != 0 and folded[s][f])
            for v in range(N):
                if r["mem_g"][v] >= 0:
                    folded[s][v] = r["grp_focal"][r["mem_g"][v]] != v
            persist[s] = r["persist"]
            row.append(r)
        out.append(row)
    return out


def filled(shape, dtype, fill=FILL):
    return np.full(tuple(shape) + (np.dtype(dtype).itemsize,), fill, np.uint8).view(dtype).reshape(shape)


def expected(step_out, N, guard=1, fill=FILL):
    """The tables as the kernel leaves them in buffers of S + guard scenarios filled with the byte pattern beforehand (of persist, which is
    in/out, only the guard rows): group entries at and beyond n_groups and all guard rows keep the pattern."""
    S = len(step_out)
    e = {k: filled((S + guard,) if k == "n_groups" else (S + guard, N), DTYPES[k], fill) for k in TABLES}
    for s, r in enumerate(step_out):
        G = r["n_groups"]
        e["n_groups"][s] = G
        for k in ("grp_focal", "grp_ids", "grp_members"):
            e[k][s, :G] = np.array(r[k], dtype=DTYPES[k])
        for k in ("own_g", "mem_g", "tilted", "persist"):
            e[k][s] = np.array(r[k], dtype=DTYPES[k])
    return e


def compare_tables(got, exp, where):
    """Exact equality of every table; the message names `where` (recipe, step), the table, the scenario and the index."""
    for k in TABLES:
        g, e = np.asarray(got[k]), exp[k]
        assert g.shape == e.shape and g.dtype == e.dtype, (where, k, g.shape, g.dtype, e.shape, e.dtype)
        if not np.array_equal(g, e):
            idx = tuple(int(i) for i in np.argwhere(g != e)[0])
            what = "guard row" if idx[0] >= e.shape[0] - 1 else f"scenario {idx[0]}"
            raise AssertionError(f"{where}: table {k}, {what}, index {idx[1:]}: got {g[idx]:#x}, expected {e[idx]:#x}")


def differing_tables(a, b):
    return [k for k in TABLES if not np.array_equal(a[k], b[k])]


# ------------------------------------------------------------------------------------------------ recipes
def _blank(S, N, Tmax1):
    """Every vehicle alone, more than 1 km from all others (at unequal spacings: no two equally far from a third), existing at every row."""
    hs = np.zeros((S, N, Tmax1, 8), np.float32)
    v = np.arange(N, dtype=np.float32)[None, :, None]
    hs[..., 0] = 5000.0 + 1000.0 * v + 37.0 * v * v
    hs[..., 1] = -7000.0 - 613.0 * v
    hs[..., 5], hs[..., 6], hs[..., 7] = 4.5, 2.0, 1.0
    return hs


def _put(hs, s, v, xy, rows=slice(None)):
    hs[s, v, rows, 0], hs[s, v, rows, 1] = np.float32(xy[0]), np.float32(xy[1])


def _order(S, N, lists):
    o = np.full((S, N), -1, np.int32)
    for s, l in enumerate(lists):
        o[s, :len(l)] = l
    return o


def _rec(name, hs, order, A, T, steps, has_roads=1, **facts):
    assert hs.dtype == np.float32 and order.dtype == np.int32 and max(steps) < hs.shape[2] and T <= hs.shape[2]
    for o in order:                                           # the contract of eval_order: packed, unique, in range
        n = int((o >= 0).sum())
        assert (o[:n] >= 0).all() and (o[n:] == -1).all() and len(set(o[:n])) == n and (o[:n] < hs.shape[1]).all()
    return dict(name=name, hs=hs, order=order, A=A, T=T, steps=list(steps), has_roads=has_roads, thr=THR, facts=facts)


def random_recipe():
    """5 scenes of 14 vehicles, 10 evaluated, 12 steps of a random walk large enough that vehicles leave discs; about 30 % of the
    vehicles stop existing at some step >= 1 (all exist at step 0: the reference defines every step).  Tie-free (asserted on the host)."""
    rs = np.random.RandomState(2024)
    S, N, Tmax1 = 5, 14, 12
    hs = _blank(S, N, Tmax1)
    hs[..., 0:2] = (rs.uniform(-70, 70, (S, N, 1, 2)) + rs.normal(0, 9, (S, N, Tmax1, 2)).cumsum(2)).astype(np.float32)
    for s in range(S):
        for v in range(N):
            if rs.uniform() < 0.3:
                hs[s, v, rs.randint(1, Tmax1):, 7] = 0
    order = _order(S, N, [rs.permutation(N)[:10] for _ in range(S)])
    return _rec("random", hs, order, 5, 4, range(12))


def threshold_recipe():
    """Integer 3-4-5 geometry.  Vehicles 1-4 exactly 60 m from focal 0 (excluded: strict <), 5-8 the same points one float32 ulp nearer
    (included), 9-12 one ulp beyond (excluded).  Scene 1: the same shifted by (-128, 256), exact in float32.  From history row 2 on (step
    5 reads it: w0 = 2) the near ones stand exactly at 60 (they leave the persisted set) and the far ones one ulp inside (not readmitted).
    Vehicles 1, 5 and 9 are evaluated too: 1 and 9 become focals of their own."""
    S, N, Tmax1 = 2, 13, 8
    hs = _blank(S, N, Tmax1)
    at60 = [(36, 48), (48, 36), (60, 0), (0, -60)]
    f32 = np.float32

    for s, off in enumerate([(0, 0), (-128, 256)]):
        _put(hs, s, 0, off)
        for k, p in enumerate(at60):
            exact = [f32(p[0] + off[0]), f32(p[1] + off[1])]  # small integers: exact
            c = 0 if abs(p[0]) >= abs(p[1]) else 1            # one float32 ulp on the larger offset, toward the focal or away from it
            near, far = list(exact), list(exact)
            near[c] = np.nextafter(exact[c], f32(off[c]))
            far[c] = np.nextafter(exact[c], f32(off[c] + 2 * p[c]))
            _put(hs, s, 1 + k, exact)
            _put(hs, s, 5 + k, near, slice(0, 2)); _put(hs, s, 5 + k, exact, slice(2, None))
            _put(hs, s, 9 + k, far, slice(0, 2)); _put(hs, s, 9 + k, near, slice(2, None))
    return _rec("threshold", hs, _order(S, N, [[0, 1, 5, 9], [0, 1, 5, 9]]), 13, 4, [0, 1, 5, 6], at60=[1, 2, 3, 4],
                near=[5, 6, 7, 8], far=[9, 10, 11, 12])


TIE_RING = [(3, 4), (4, 3), (5, 0), (0, -5), (-3, 4), (-4, 3), (-5, 0), (0, 5)]      # eight points at distance exactly 5


def ties_recipe():
    """N = 20, A = 8.  Scene 0: focal 0; vehicles 1-8 on TIE_RING, 9 at (1, 0), 10 at (0, 2), 11 and 12 both at (3, -4) (identical
    positions, distance 5), 13 on the focal's own position (distance 0, a tie with the focal itself).  Ranks 0-3 are 0, 13, 9, 10; the
    ten vehicles at distance 5 tie for ranks 4-13 and the cut at A = 8 takes the four lowest indices of them.  Scene 1: the mirror image
    v -> 19 - v (the focal is the highest index; the tied are 7, 8, 11-18 and the cut takes 7, 8, 11, 12).  Scene 2: focal 0 at (p, p), vehicle 5 at (a, b) and
    vehicle 3 at (b, a) with inexact squares: equal sums in either order of the same two products, but not under a fused multiply-add;
    six nearer vehicles put the pair on ranks 7 and 8, so A = 8 takes vehicle 3 only.  Evaluated vehicles on both sides of every cut."""
    S, N, Tmax1 = 3, 20, 8
    hs = _blank(S, N, Tmax1)
    pts = {0: (0, 0), 9: (1, 0), 10: (0, 2), 11: (3, -4), 12: (3, -4), 13: (0, 0)}
    pts.update({1 + k: p for k, p in enumerate(TIE_RING)})
    for v, p in pts.items():
        _put(hs, 0, v, (p[0] + 10, p[1] - 20))                # small integers: every difference and square is exact
        _put(hs, 1, 19 - v, (p[0] + 10, p[1] - 20))
    p, a, b = np.float32(0.001234), np.float32(31.4159), np.float32(17.2718)
    _put(hs, 2, 0, (p, p)); _put(hs, 2, 5, (a, b)); _put(hs, 2, 3, (b, a))
    for k, v in enumerate((1, 2, 4, 6, 7, 8)):
        _put(hs, 2, v, (np.float32(1.5 + 2.25 * k), np.float32(-0.75 * k)))
    order = _order(S, N, [[0, 2, 7, 12, 13], [19, 17, 12, 7, 6], [0, 5, 3]])
    return _rec("ties", hs, order, 8, 4, [0, 2, 5], tied0=[1, 2, 3, 4, 5, 6, 7, 8, 11, 12], mirror=(5, 3))


def quirk_recipe():
    """order = [f, a, b, c, d] = [2, 0, 4, 1, 5], all five inside f's context (N = 6, A = 5; vehicle 3 farther out): the fold loop takes a,
    skips b, takes c, skips d — members {f, a, c}; b is the next focal and folds d."""
    S, N, Tmax1 = 1, 6, 8
    hs = _blank(S, N, Tmax1)
    for v, p in {2: (0, 0), 0: (3.5, 1), 4: (-6, 2.25), 1: (9, -4), 5: (-2, -12.5), 3: (30, 31)}.items():
        _put(hs, 0, v, p)
    return _rec("quirk", hs, _order(S, N, [[2, 0, 4, 1, 5]]), 5, 4, [0, 1, 2, 5], f=2, a=0, b=4, c=1, d=5)


def persist_paths_recipe():
    """T = 4, A = 4, steps 0..9 (positions come from row w0 = 0 for t < 4, then row t - 3).
    Scene 0: vehicle 1 stands 10 m from focal 0, is 100 m away in rows 2-3 (read at t = 5, 6) and back at 10 m from row 4 on: it leaves the
      persisted set at t = 5 and stays out.  Vehicle 6, evaluated, is outside every step-0 group: a lone focal.
    Scene 1: focal 0 at the origin folds vehicle 1 at (40, 0); 0's set is {0, 2, 3, 1} with 3 at (-30, 0), 70 m from vehicle 1, and
      vehicle 4 at (45, 0) is not in it.  0 stops existing at row 2: from t = 2 vehicle 1 is the focal, with the inherited set cut by
      its own disc: {0, 1, 2} (the dead 0 stays in the set, as in the reference)."""
    S, N, Tmax1 = 2, 8, 12
    hs = _blank(S, N, Tmax1)
    _put(hs, 0, 0, (0, 0)); _put(hs, 0, 1, (10, 0)); _put(hs, 0, 1, (100, 0), slice(2, 4)); _put(hs, 0, 2, (0, -7.5))
    for v, p in {0: (0, 0), 2: (5, 0), 3: (-30, 0), 1: (40, 0), 4: (45, 0)}.items():
        _put(hs, 1, v, p)
    hs[1, 0, 2:, 7] = 0
    return _rec("persist_paths", hs, _order(S, N, [[0, 6], [0, 1]]), 4, 4, range(10), leaver=(0, 0, 1, 5, 7))


def persist_late_recipe():
    """OUTSIDE THE REFERENCE (self.relevant_agent_idxs[focal_id] raises KeyError there): vehicle 5, evaluated, does not exist at steps 0
    and 1 and stands far from focal 0's disc, so nobody folds it; it exists from step 2.  The project's rule (include/ctrlsim.h): with no
    set yet it makes the fresh nearest-A selection at t = 2 — {5, 6, 7} — and carries that set on; at t = 6 (row 3) vehicle 7 has left."""
    S, N, Tmax1 = 1, 8, 12
    hs = _blank(S, N, Tmax1)
    _put(hs, 0, 0, (0, 0)); _put(hs, 0, 1, (8, 1))
    _put(hs, 0, 5, (300, 300)); _put(hs, 0, 6, (310, 300)); _put(hs, 0, 7, (300, 320)); _put(hs, 0, 7, (300, 380), slice(3, None))
    hs[0, 5, :2, 7] = 0
    return _rec("persist_late", hs, _order(S, N, [[0, 5]]), 4, 4, range(8), late=5)


def window_recipe():
    """T = 4, steps 0, 3, 4, 6, 8, 9.  Focal 0 stands at the origin.  Around t = 6 (w0 = 3): vehicle 1 is inside the disc at row 3 and
    outside at row 6 (it stays in), vehicle 2 outside at row 3 and inside at row 6 (it leaves).  Vehicle 3, evaluated, exists at row 3 but
    not at row 6 (a dead focal at t = 6, alive again from row 7); vehicle 4, evaluated, exists at row 6 but not at row 3."""
    S, N, Tmax1 = 1, 8, 12
    hs = _blank(S, N, Tmax1)
    _put(hs, 0, 0, (0, 0))
    _put(hs, 0, 1, (10, 0)); _put(hs, 0, 1, (100, 0), slice(6, 7))
    _put(hs, 0, 2, (0, 12)); _put(hs, 0, 2, (0, 120), slice(3, 4))
    _put(hs, 0, 3, (200, 0)); _put(hs, 0, 5, (205, 3)); hs[0, 3, 6, 7] = 0
    _put(hs, 0, 4, (-200, 50)); _put(hs, 0, 6, (-190, 40)); hs[0, 4, 3, 7] = 0
    return _rec("window", hs, _order(S, N, [[0, 3, 4]]), 4, 4, [0, 3, 4, 6, 8, 9])


def _one_disc(name, N):
    """All N vehicles evaluated and inside one 40 m x 40 m box (diagonal < 60 m), A = 64: the first group folds every second entry of the
    full list and the leftovers form further groups."""
    rs = np.random.RandomState(N)
    hs = _blank(2, N, 6)
    hs[..., 0:2] = rs.uniform(-20, 20, (2, N, 1, 2)).astype(np.float32)
    return _rec(name, hs, _order(2, N, [np.arange(N), rs.permutation(N)]), 64, 4, [0, 1])


def shapes_recipes():
    rs = np.random.RandomState(7)
    out = []
    hs = _blank(2, 1, 6)
    out.append(_rec("shapes_n1", hs, _order(2, 1, [[0], []]), 1, 4, [0, 1, 4]))
    hs = _blank(2, 2, 6)
    _put(hs, 0, 0, (0, 0)); _put(hs, 0, 1, (3, 0)); _put(hs, 1, 0, (0, 0)); _put(hs, 1, 1, (3, 0))
    out.append(_rec("shapes_n2", hs, _order(2, 2, [[0, 1], [1]]), 1, 4, [0, 1, 4]))
    out.append(_one_disc("shapes_n63", 63))
    out.append(_one_disc("shapes_n64", 64))
    hs = _blank(2, 64, 8)
    hs[..., 0:2] = (rs.uniform(-200, 200, (2, 64, 1, 2)) + rs.normal(0, 6, (2, 64, 8, 2)).cumsum(2)).astype(np.float32)
    hs[..., 7] = rs.uniform(size=(2, 64, 8)) < 0.9
    hs[:, :, 0, 7] = 1
    out.append(_rec("shapes_wide", hs, _order(2, 64, [rs.permutation(64)[:48] for _ in range(2)]), 24, 4, [0, 1, 5, 7]))
    S, N, Tmax1 = 300, 9, 8
    hs = _blank(S, N, Tmax1)
    ext = (20.0 + 15.0 * (np.arange(S) % 11))[:, None, None, None]
    hs[..., 0:2] = (rs.uniform(-1, 1, (S, N, 1, 2)) * ext + rs.normal(0, 5, (S, N, Tmax1, 2)).cumsum(2)).astype(np.float32)
    hs[..., 7] = rs.uniform(size=(S, N, Tmax1)) < 0.8
    out.append(_rec("shapes_batch", hs, _order(S, N, [rs.permutation(N)[:s % 7] for s in range(S)]), 4, 4, [0, 1, 5, 7]))
    hs = _blank(2, 6, 6)
    hs[..., 0:2] = rs.uniform(-20, 20, (2, 6, 1, 2)).astype(np.float32)
    out.append(_rec("shapes_noroads", hs, _order(2, 6, [[3, 1, 0], [5]]), 4, 4, [0, 1, 4], has_roads=0))
    out.append(_rec("shapes_noorder", hs.copy(), _order(2, 6, [[], []]), 4, 4, [0, 1, 4]))
    return out


def all_recipes():
    return [random_recipe(), threshold_recipe(), ties_recipe(), quirk_recipe(), persist_paths_recipe(), persist_late_recipe(),
            window_recipe()] + shapes_recipes()


NAMES = ["random", "threshold", "ties", "quirk", "persist_paths", "persist_late", "window", "shapes_n1", "shapes_n2", "shapes_n63",
         "shapes_n64", "shapes_wide", "shapes_batch", "shapes_noroads", "shapes_noorder"]
