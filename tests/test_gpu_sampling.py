"""sample_rtg_kernel / sample_action_kernel (csrc/sample.hip) through both entry-point families — ctrlsim_sample_* with a uniform slot
count A, ctrlsim_sample_*_rows with a ctx_row0 of unequal strides, the one the engine uses — against the float64 races of
tests/sat_ref.py, at a batch shape where scenario, vehicle, context and slot are all different numbers: a wrong sv / N, a wrong row
base or a noise key that ignores the scenario id changes tokens here."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import _lib, weights  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402
import sat_ref  # noqa: E402

S, N, TMAX = 5, 7, 4
SN = S * N                                           # 35 waves: eight full blocks of four and a partial one
SIDS = np.array([0, 1, 2 ** 40 + 3, -1, 12345], np.int64)
ROWS = np.array([3, 7, 5, 4, 6, 2])                  # logits rows of the six contexts (the _rows family); slots stay below them
A_PLAIN = 8
TILT_SCN = np.array([[0.0, 0.0, 0.0], [10.0, -10.0, 5.0], [-20.0, 30.0, 0.0], [3.5, 0.25, -40.0], [-1.0, -2.0, -3.0]])
TILT3 = (7.0, -13.0, 21.0)
BIG_SEED = 0xDEADBEEFCAFEF00D                        # seed * 0x9E3779B97F4A7C15 wraps around 2^64
SENT = -7
MARGIN = 1e-9                                        # device log against libm: ulps; no reference draw may be this close


class Layout:
    """Which logits row every vehicle reads, for one family."""

    def __init__(self, family, seed):
        rs = np.random.RandomState(seed)
        self.family = family
        self.row0 = np.concatenate([[0], np.cumsum(ROWS)[:-1]]) if family == "rows" else np.arange(6) * A_PLAIN
        self.n_rows = int(ROWS.sum()) if family == "rows" else 6 * A_PLAIN
        self.ctx, self.slot = {}, {}
        for side in ("own", "mem"):
            ctx = rs.randint(0, 6, SN)
            ctx[rs.uniform(size=SN) < 0.25] = -1
            ctx[0] = 0
            slot = np.where(ctx >= 0, rs.randint(0, 10 ** 6, SN) % ROWS[np.maximum(ctx, 0)], -1)
            self.ctx[side], self.slot[side] = ctx, slot
            assert (ctx < 0).sum() >= 4 and (slot[ctx >= 0] != (np.arange(SN) % N)[ctx >= 0]).any()
        self.d_row0 = dev(self.row0.astype(np.int32))
        self.d = {(k, side): dev(getattr(self, k)[side].astype(np.int32)) for k in ("ctx", "slot") for side in ("own", "mem")}

    def row(self, side, sv):
        return int(self.row0[self.ctx[side][sv]] + self.slot[side][sv])


def sample_rtg(lay, logits, R, tilted, tilt3, tilt_scn, noise, seed, t, hist, sid=None):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    sid = dev(SIDS) if sid is None else sid
    t3 = (C.c_double * 3)(*tilt3)
    tail = (p(lay.d["ctx", "own"]), p(lay.d["slot", "own"]), p(tilted), t3, p(tilt_scn), p(noise), seed, p(sid), t, p(hist), S, N, TMAX, st)
    if lay.family == "rows":
        _lib.check(lib.ctrlsim_sample_rtg_rows(p(logits), p(lay.d_row0), R, *tail), "sample_rtg_rows")
    else:
        _lib.check(lib.ctrlsim_sample_rtg(p(logits), A_PLAIN, R, *tail), "sample_rtg")


def sample_action(lay, logits, V, temp, top_p, noise, seed, t, hist, now, zero_token, sid=None):
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    sid = dev(SIDS) if sid is None else sid
    tail = (p(lay.d["ctx", "mem"]), p(lay.d["slot", "mem"]), temp, top_p, p(noise), seed, p(sid), t, p(hist), p(now), S, N, TMAX,
            zero_token, st)
    if lay.family == "rows":
        _lib.check(lib.ctrlsim_sample_action_rows(p(logits), p(lay.d_row0), V, *tail), "sample_action_rows")
    else:
        _lib.check(lib.ctrlsim_sample_action(p(logits), A_PLAIN, V, *tail), "sample_action")


def host_noise(seed, t, head, n):
    """[SN, n] what the in-kernel generator draws for every (scenario id, vehicle) of the batch."""
    return np.stack([weights.exp_noise(seed, int(SIDS[sv // N]), t, sv % N, head, n) for sv in range(SN)])


def ref_rtg(lay, logits, tilted, tilt_of_scn, noise, t):
    """-> expected hist_rtg [S*N, TMAX, 3] over a sentinel-filled buffer, the smallest race margin."""
    want = np.full((SN, TMAX, 3), SENT, np.int64)
    worst = np.inf
    for sv in range(SN):
        if lay.ctx["own"][sv] < 0:
            continue
        bins, m = sat_ref.race_rtg(logits[lay.row("own", sv)], tilt_of_scn[sv // N], bool(tilted[sv]), noise[sv])
        want[sv, t], worst = bins, min(worst, m.min())
    return want, worst


def ref_action(lay, logits, temp, top_p, noise, t, zero_token):
    want = np.full((SN, TMAX), SENT, np.int64)
    now = np.full(SN, -1, np.int64)
    worst, worst_nuc = np.inf, np.inf
    for sv in range(SN):
        if lay.ctx["mem"][sv] < 0:
            want[sv, t] = zero_token
            continue
        tok, m, _ = sat_ref.race_action(logits[lay.row("mem", sv)], temp, top_p, noise[sv])
        want[sv, t] = now[sv] = tok
        nm = sat_ref.nucleus_margin_rounded(logits[lay.row("mem", sv)], temp, top_p) if top_p > 0 else np.inf
        worst, worst_nuc = min(worst, m), min(worst_nuc, nm)
    return want, now, worst, worst_nuc


def _exp1(rs, shape):
    return np.maximum(rs.exponential(size=shape), 1e-30).astype(np.float32)


@pytest.mark.parametrize("V,R", [(1000, 350), (65, 63), (64, 64), (5, 2)])
@pytest.mark.parametrize("family", ["plain", "rows"])
def test_batch_of_five_scenarios_matches_the_float64_races(family, V, R):
    """S = 5, N = 7, six contexts, a quarter of the vehicles in no context, mixed tilt flags, per-scenario and uniform tilts, steps 0
    and TMAX - 1, scenario ids up to 2^40 and -1, explicit and in-kernel noise (a seed whose product with the key constant wraps),
    temperatures 1.0 / 0.7 / 1.5.  Every bin and token equals the reference; vehicles in no context keep their RTG row and take the
    zero action; nothing else is written; no race is non-finite.  No draw is left out: the reference's smallest margin is asserted to
    be above 1e-9."""
    lib = _lib.lib()
    rs = np.random.RandomState(1000 * V + R + (family == "rows"))
    lay = Layout(family, 5 + V)
    rtg_logits = rs.normal(0, 2.0, (lay.n_rows, R * 3)).astype(np.float32)
    act_logits = rs.normal(0, 2.0, (lay.n_rows, V)).astype(np.float32)
    tilted = (rs.uniform(size=SN) < 0.5).astype(np.uint8)
    assert 0 < tilted.sum() < SN
    d_rtg, d_act, d_tilted, d_tscn = dev(rtg_logits), dev(act_logits), dev(tilted), dev(TILT_SCN)
    zero_token = V // 2
    lib.ctrlsim_nonfinite_count(1)
    left_out, smallest = 0, np.inf
    for t in (0, TMAX - 1):
        for mode in ("explicit", "in-kernel"):
            if mode == "explicit":
                nr, na, seed = _exp1(rs, (SN, 3, R)), _exp1(rs, (SN, V)), 0
                d_nr, d_na = dev(nr), dev(na)
            else:
                seed = BIG_SEED
                nr = np.stack([host_noise(seed, t, c, R) for c in range(3)], axis=1)
                na, d_nr, d_na = host_noise(seed, t, 3, V), None, None
            for per_scn in (True, False):
                hist = torch.full((S, N, TMAX, 3), SENT, dtype=torch.int32, device=DEV)
                sample_rtg(lay, d_rtg, R, d_tilted, TILT3, d_tscn if per_scn else None, d_nr, seed, t, hist)
                want, m = ref_rtg(lay, rtg_logits, tilted, TILT_SCN if per_scn else np.tile(TILT3, (S, 1)), nr, t)
                torch.cuda.synchronize()
                left_out, smallest = left_out + int(m < MARGIN), min(smallest, m)
                assert np.array_equal(hist.cpu().numpy().reshape(SN, TMAX, 3), want), (t, mode, per_scn)
            for temp in (1.0, 0.7, 1.5):
                hist = torch.full((S, N, TMAX), SENT, dtype=torch.int32, device=DEV)
                now = torch.full((S, N), SENT, dtype=torch.int32, device=DEV)
                sample_action(lay, d_act, V, temp, 0.0, d_na, seed, t, hist, now, zero_token)
                want, want_now, m, _ = ref_action(lay, act_logits, temp, 0.0, na, t, zero_token)
                torch.cuda.synchronize()
                left_out, smallest = left_out + int(m < MARGIN), min(smallest, m)
                assert np.array_equal(hist.cpu().numpy().reshape(SN, TMAX), want), (t, mode, temp)
                assert np.array_equal(now.cpu().numpy().reshape(SN), want_now), (t, mode, temp)
    print(f"{family} V={V} R={R}: smallest reference margin {smallest:.3e}, draws left out {left_out}")
    assert left_out == 0
    assert lib.ctrlsim_nonfinite_count(0) == 0


def _tie_row(V):
    """One loud token, a run of 40 exactly equal logits behind it and a floor of equal quiet ones: the nucleus cut falls inside the
    run.  The noise makes the score rise with the index inside the run and silences the loud token, so the winner is the LAST
    kept token of the run — one token more or less in the kept set changes the draw."""
    lg = np.full(V, -8.0, np.float32)
    lg[3] = np.log(9.3)
    lg[10:50] = 0.0
    q = np.ones(V, np.float32)
    q[3] = 1e6
    q[10:50] = np.exp(-0.1 * np.arange(40))
    return lg, q


@pytest.mark.parametrize("V", [1000, 65])
@pytest.mark.parametrize("family", ["plain", "rows"])
def test_nucleus_keeps_the_reference_set(family, V):
    """top_p in {1e-12, 0.5, 0.8, 1.0, 2.0}: the kept set is the tokens whose preceding mass is < top_p.  1e-12 leaves the arg-max of the
    logits whatever the noise, >= 1.0 is the plain race; inside a run of exactly equal logits the lower indices stay.  The
    reference's |before - top_p| stays above 1e-9 everywhere (asserted; the leading token's preceding mass, the empty sum, is exactly 0
    on both sides and no rounded quantity), so no row is left out."""
    rs = np.random.RandomState(77 + V)
    lay = Layout(family, 9 + V)
    logits = rs.normal(0, 1.5, (lay.n_rows, V)).astype(np.float32)
    noise = _exp1(rs, (SN, V))
    logits[lay.row("mem", 0)], noise[0] = _tie_row(V)
    d_logits, d_noise = dev(logits), dev(noise)
    zero_token, t = V // 2, 1
    lib = _lib.lib()
    lib.ctrlsim_nonfinite_count(1)

    def run(temp, top_p):
        hist = torch.full((S, N, TMAX), SENT, dtype=torch.int32, device=DEV)
        now = torch.full((S, N), SENT, dtype=torch.int32, device=DEV)
        sample_action(lay, d_logits, V, temp, top_p, d_noise, 0, t, hist, now, zero_token)
        torch.cuda.synchronize()
        return hist.cpu().numpy().reshape(SN, TMAX), now.cpu().numpy().reshape(SN)

    live = lay.ctx["mem"] >= 0
    for temp in (1.0, 0.7):
        plain, _ = run(temp, 0.0)
        for top_p in (1e-12, 0.5, 0.8, 1.0, 2.0):
            got, got_now = run(temp, top_p)
            want, want_now, m, nm = ref_action(lay, logits, temp, top_p, noise, t, zero_token)
            print(f"{family} V={V} T={temp} top_p={top_p}: race margin {m:.3e}, nucleus margin {nm:.3e}")
            assert nm > MARGIN and m > MARGIN
            assert np.array_equal(got, want) and np.array_equal(got_now, want_now), (temp, top_p)
            if top_p == 1e-12:
                scaled = (logits / np.float32(temp)).astype(np.float32)
                assert all(got[sv, t] == np.argmax(scaled[lay.row("mem", sv)]) for sv in np.where(live)[0])
            if top_p >= 1.0:
                assert np.array_equal(got, plain)
            if top_p in (0.5, 0.8) and temp == 1.0:
                assert 10 <= got[0, t] < 49, got[0, t]                     # the cut fell inside the run of ties
    assert lib.ctrlsim_nonfinite_count(0) == 0


@pytest.mark.parametrize("V,R", [(1000, 350), (65, 63)])
@pytest.mark.parametrize("family", ["plain", "rows"])
def test_ties_and_infinities(family, V, R):
    """With all noise equal: all logits equal -> token / bin 0 (the lowest index wins a tie); the leading k logits -inf -> the first
    finite one (k = 5, and k = 70 — past one sweep of the 64 lanes — where the vocabulary allows, else 40); one +inf logit wins.
    A row of nothing but -inf has no defined answer in the reference (its softmax is NaN and torch.multinomial raises); TODAY'S
    BEHAVIOUR IS THE CONTRACT: each head counts one non-finite race in ctrlsim_nonfinite_count and falls back to zero_token / bin 0."""
    lay = Layout(family, 3)
    k2 = 70 if V > 70 else 40
    inf = np.float32(np.inf)
    act = np.zeros((lay.n_rows, V), np.float32)
    rtg = np.zeros((lay.n_rows, R, 3), np.float32)
    tok_of_row, bin_of_row = np.zeros(lay.n_rows, np.int64), np.zeros((lay.n_rows, 3), np.int64)
    for r in range(lay.n_rows):                        # the case of a logits row: r % 5
        if r % 5 in (1, 2):
            k = 5 if r % 5 == 1 else k2
            act[r, :k], rtg[r, :min(k, R - 1)] = -inf, -inf
            tok_of_row[r], bin_of_row[r] = k, min(k, R - 1)
        elif r % 5 == 3:
            act[r, 37], rtg[r, [11, 12, 13], [0, 1, 2]] = inf, inf
            tok_of_row[r], bin_of_row[r] = 37, (11, 12, 13)
        elif r % 5 == 4:
            act[r], rtg[r] = -inf, -inf
            tok_of_row[r], bin_of_row[r] = V // 2, 0
    own_rows = np.array([lay.row("own", sv) if lay.ctx["own"][sv] >= 0 else -1 for sv in range(SN)])
    mem_rows = np.array([lay.row("mem", sv) if lay.ctx["mem"][sv] >= 0 else -1 for sv in range(SN)])
    for rows in (own_rows, mem_rows):
        assert set(rows[rows >= 0] % 5) == {0, 1, 2, 3, 4}                     # every case is read by some vehicle
    lib = _lib.lib()
    lib.ctrlsim_nonfinite_count(1)
    hist = torch.full((S, N, TMAX), SENT, dtype=torch.int32, device=DEV)
    now = torch.full((S, N), SENT, dtype=torch.int32, device=DEV)
    hr = torch.full((S, N, TMAX, 3), SENT, dtype=torch.int32, device=DEV)
    sample_action(lay, dev(act), V, 1.0, 0.0, dev(np.ones((SN, V), np.float32)), 0, 2, hist, now, V // 2)
    sample_rtg(lay, dev(rtg.reshape(lay.n_rows, R * 3)), R, dev(np.zeros(SN, np.uint8)), TILT3, None,
               dev(np.ones((SN, 3, R), np.float32)), 0, 2, hr)
    torch.cuda.synchronize()
    n_bad = int((mem_rows[mem_rows >= 0] % 5 == 4).sum()) + 3 * int((own_rows[own_rows >= 0] % 5 == 4).sum())
    assert lib.ctrlsim_nonfinite_count(0) == n_bad      # the all -inf rows: one action race, three RTG races per vehicle reading one
    tok, bins = hist.cpu().numpy().reshape(SN, TMAX)[:, 2], hr.cpu().numpy().reshape(SN, TMAX, 3)[:, 2]
    for sv in range(SN):
        if mem_rows[sv] >= 0:
            assert tok[sv] == tok_of_row[mem_rows[sv]], (sv, tok[sv])
        if own_rows[sv] >= 0:
            assert np.array_equal(bins[sv], bin_of_row[own_rows[sv]]), (sv, bins[sv])
    assert lib.ctrlsim_nonfinite_count(1) == n_bad and lib.ctrlsim_nonfinite_count(0) == 0


@pytest.mark.parametrize("family", ["plain", "rows"])
def test_in_kernel_noise_is_the_host_generator(family):
    """Five scenario ids x two steps x three seeds: the in-kernel draw of all four heads equals the draw with explicit noise from
    weights.exp_noise (the generator tests/test_sat_ref_cpu.py establishes as a fair Exp(1) source) — and the reference."""
    V, R = 1000, 350
    rs = np.random.RandomState(4)
    lay = Layout(family, 21)
    rtg_logits = rs.normal(0, 2.0, (lay.n_rows, R * 3)).astype(np.float32)
    act_logits = rs.normal(0, 2.0, (lay.n_rows, V)).astype(np.float32)
    tilted = np.ones(SN, np.uint8)
    d_rtg, d_act, d_tilted, d_tscn = dev(rtg_logits), dev(act_logits), dev(tilted), dev(TILT_SCN)
    left_out = 0
    for seed in (1, 9, BIG_SEED):
        for t in (0, TMAX - 1):
            nr = np.stack([host_noise(seed, t, c, R) for c in range(3)], axis=1)
            na = host_noise(seed, t, 3, V)
            out = []
            for d_nr, d_na in ((None, None), (dev(nr), dev(na))):
                hist = torch.full((S, N, TMAX), SENT, dtype=torch.int32, device=DEV)
                now = torch.full((S, N), SENT, dtype=torch.int32, device=DEV)
                hr = torch.full((S, N, TMAX, 3), SENT, dtype=torch.int32, device=DEV)
                sample_rtg(lay, d_rtg, R, d_tilted, TILT3, d_tscn, d_nr, seed, t, hr)
                sample_action(lay, d_act, V, 1.0, 0.0, d_na, seed, t, hist, now, 524)
                torch.cuda.synchronize()
                out.append((hr.cpu().numpy().reshape(SN, TMAX, 3), hist.cpu().numpy().reshape(SN, TMAX)))
            assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), (seed, t)
            want_r, m_r = ref_rtg(lay, rtg_logits, tilted, TILT_SCN, nr, t)
            want_a, _, m_a, _ = ref_action(lay, act_logits, 1.0, 0.0, na, t, 524)
            left_out += int(min(m_r, m_a) < MARGIN)
            assert np.array_equal(out[0][0], want_r) and np.array_equal(out[0][1], want_a), (seed, t)
    assert left_out == 0
