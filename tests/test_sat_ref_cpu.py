"""The plain references of tests/sat_ref.py pinned on the CPU: against the reference's own sampling code path (tests/golden/
sampling.npz), against the CPU oracle's races, against each other — and the counter-based noise source (ctrlsim_amd.weights.exp_noise,
the generator the HIP sampler evaluates in-kernel) as a fair Exp(1) source ACROSS keys, which the closed-loop tests take for granted:
they compare against an oracle fed by the same generator."""
import numpy as np
import torch

from helpers import golden
from ctrlsim_amd import rewards, spec, weights
import rollout_oracle
import sat_ref


def test_races_reproduce_the_reference_sampling_fixture():
    """Every RTG bin and every action token of tests/golden/sampling.npz (the reference's process_predicted_rtg / predict code path
    with the noise of seed 9, scenario 0, step 0).  An action token may differ only where the reference's own float32 race was a
    near-tie (act_margin_* < 1e-5: the admission rule of the GPU test)."""
    g = golden("sampling")
    n = g["rtg_logits"].shape[0]
    R, V = g["rtg_logits"].shape[1] // 3, g["act_logits"].shape[1]
    for ti, tl in enumerate(g["tilts"]):
        for i in range(n):
            q = np.stack([weights.exp_noise(9, 0, 0, i, c, R) for c in range(3)])
            bins, _ = sat_ref.race_rtg(g["rtg_logits"][i], tl, True, q)
            assert np.array_equal(bins, g[f"rtg_bins_tilt{ti}"][i]), (ti, i)
    for tag, temp, top_p in (("t1", 1.0, 0.0), ("t15", 1.5, 0.0), ("nuc", 1.0, 0.8), ("nuc_t07", 0.7, 0.8)):
        got = np.array([sat_ref.race_action(g["act_logits"][i], temp, top_p, weights.exp_noise(9, 0, 0, i, 3, V))[0] for i in range(n)])
        ok = got == g[f"act_tok_{tag}"]
        assert ok.all() or (g[f"act_margin_{tag}"][~ok] < 1e-5).all(), (tag, np.where(~ok))


def test_races_equal_the_cpu_oracle_on_random_rows():
    """sat_ref.race_rtg / race_action against oracle/rollout_oracle.py:sample_rtg / sample_action (softmax, sort, cumulative sum and
    the race in the reference's own precisions) on 200 random rows, seed 11.  A row may be left out only where the float64 nucleus
    margin is below 1e-6 — there the oracle's float32 cumulative sum decides the kept set —; the seed is chosen so that none is."""
    rs = np.random.RandomState(11)
    R, V, rows = 350, 1000, 200
    lin = np.linspace(0.0, 1.0, R)
    left_out = 0
    for i in range(rows):
        rtg = rs.normal(0, 2.0, R * 3).astype(np.float32)
        act = rs.normal(0, 2.0, V).astype(np.float32)
        tilts = rs.uniform(-30, 30, 3)
        tilted = bool(i % 3)
        q = np.stack([weights.exp_noise(5, i, i % 7, i % 11, c, R) for c in range(3)])
        qa = weights.exp_noise(5, i, i % 7, i % 11, 3, V)
        tilt_tab = (lin[:, None] * tilts[None, :]) * (1.0 if tilted else 0.0)
        bins, _ = sat_ref.race_rtg(rtg, tilts, tilted, q)
        assert list(bins) == rollout_oracle.sample_rtg(torch.from_numpy(rtg), tilt_tab, R, 3, lambda c, n: q[c]), i
        temp = (1.0, 0.7, 1.5)[i % 3]
        top_p = (0.0, 0.8, 0.5, 0.95)[i % 4]
        tok, _, nm = sat_ref.race_action(act, temp, top_p, qa)
        ref = rollout_oracle.sample_action(torch.from_numpy(act), temp, top_p > 0, top_p, lambda h, n: qa)
        if tok != ref:
            assert nm < 1e-6, (i, tok, ref, nm)
            left_out += 1
    print(f"rows left out (nucleus margin < 1e-6): {left_out} of {rows}")
    assert left_out == 0


def _keys():
    """1024 keys (scenario, step, agent, head): each axis varied alone, then all four together."""
    a = [(s, 0, 0, 3) for s in range(256)]
    b = [(7, t, 0, 3) for t in range(256)]
    c = [(7, 2, v, 3) for v in range(252)] + [(7, 2, 5, h) for h in range(4)]
    d = [(s, t, v, h) for s in (0, 1, 2 ** 40 + 3, -1) for t in range(4) for v in range(4) for h in range(4)]
    return a, b, c, d


def test_exp_noise_is_a_fair_exp1_source_across_keys():
    """weights.exp_noise over 1024 keys, seed 2024 (deterministic: a seed that passes always passes).  The tokens that win the race
    against fixed logits (V = 8, every expected count >= 5) follow the float64 softmax: chi-square with 7 degrees of freedom below
    24.32, the 99.9 % quantile.  The uniforms u = exp(-q) of neighbouring keys are uncorrelated along every key axis: |lag-1
    correlation| < 4 / sqrt(n)."""
    seed, V = 2024, 8
    logits = np.linspace(-1.2, 1.2, V)
    p = np.exp(logits) / np.exp(logits).sum()
    a, b, c, d = _keys()
    keys = a + b + c + d
    assert len(keys) == 1024 and (1024 * p).min() >= 5.0
    q = np.stack([weights.exp_noise(seed, *k, V) for k in keys]).astype(np.float64)
    assert (q > 0).all() and np.isfinite(q).all()
    wins = np.bincount(np.argmax(logits[None, :] - np.log(q), axis=1), minlength=V)
    chi2 = float(((wins - 1024 * p) ** 2 / (1024 * p)).sum())
    print(f"chi-square of the winning tokens over 1024 keys (7 dof, bound 24.32): {chi2:.3f}")
    assert chi2 < 24.32
    u = np.exp(-q)
    assert abs(u.mean() - 0.5) < 4 / np.sqrt(12 * u.size)                     # mean of 8192 uniforms
    axes = {"scenario": (u[0:256][:-1], u[0:256][1:]), "step": (u[256:512][:-1], u[256:512][1:]),
            "agent": (u[512:764][:-1], u[512:764][1:])}
    ud = u[768:].reshape(4, 4, 4, 4, V)
    axes["head"] = (ud[:, :, :, :-1], ud[:, :, :, 1:])
    axes["together"] = (ud.reshape(-1, V)[:-1], ud.reshape(-1, V)[1:])
    for name, (x, y) in axes.items():
        x, y = x.ravel(), y.ravel()
        r = float(np.corrcoef(x, y)[0, 1])
        print(f"lag-1 correlation of u along {name}: {r:+.4f} (n = {x.size}, bound {4 / np.sqrt(x.size):.4f})")
        assert abs(r) < 4 / np.sqrt(x.size), name


def _random_groups(rs, S, N):
    n_groups = rs.randint(0, N + 1, S)
    n_groups[:3] = (0, N, 1)
    grp_ids = np.zeros((S, N), np.uint64)
    for s in range(S):
        for g in range(N):
            k = rs.randint(1, N + 1)
            bits = rs.choice(N, k, replace=False)
            grp_ids[s, g] = np.uint64(sum(1 << int(b) for b in bits))
    own_g = np.array([[rs.randint(-1, n_groups[s]) if n_groups[s] else -1 for _ in range(N)] for s in range(S)])
    mem_g = np.array([[rs.randint(-1, n_groups[s]) if n_groups[s] else -1 for _ in range(N)] for s in range(S)])
    return n_groups, grp_ids, own_g, mem_g


def test_ctx_index_classes_with_one_class_is_ctx_index_and_classes_are_first_fit():
    rs = np.random.RandomState(3)
    for N in (3, 64):
        S, A = 40, 64
        n_groups, grp_ids, own_g, mem_g = _random_groups(rs, S, N)
        for s0, s1 in ((0, S), (5, 31)):
            one = sat_ref.ctx_index_classes(n_groups, grp_ids, own_g, mem_g, [A], A, s0, s1)
            flat = sat_ref.ctx_index(n_groups, grp_ids, own_g, mem_g, s0, s1)
            for k in ("ctx_scn", "ctx_grp", "own_ctx", "own_slot", "mem_ctx", "mem_slot"):
                assert np.array_equal(one[k], flat[k]), k
            assert np.array_equal(one["ctx_row0"], np.arange(len(one["ctx_scn"])) * A)
            assert np.array_equal(flat["ctx_base"][s0:s1], np.cumsum(np.r_[0, n_groups[s0:s1]])[:-1])
            sizes = [4, 8, 12, 24, 40, A]
            cls = sat_ref.ctx_index_classes(n_groups, grp_ids, own_g, mem_g, sizes, A, s0, s1)
            assert len(cls["ctx_scn"]) == n_groups[s0:s1].sum()
            bounds = np.cumsum(np.r_[0, cls["class_counts"]])
            row = 0
            for c, (s, g) in enumerate(zip(cls["ctx_scn"], cls["ctx_grp"])):
                k = int(np.searchsorted(bounds, c, side="right")) - 1
                need = sat_ref.popcount(grp_ids[s, g]) + 1
                first_fit = next((j for j, a in enumerate(sizes) if a >= need), len(sizes) - 1)
                assert k == first_fit and cls["ctx_row0"][c] == row
                row += sizes[k] - 1 if sizes[k] < A else A
            assert np.array_equal(sat_ref.group_size_hist(n_groups, grp_ids, sizes)[s0:s1].sum(0), cls["class_counts"])


def test_ledger_reference_is_the_host_form_and_where_it_is_not():
    """sat_ref.ledger_step is rewards.dense_reward on two-point polylines: on a table of regular rows its road-edge component is the
    host form's own.  A zero-length row is the stated exception: as a two-point polyline the host form zeroes the distance of the
    WHOLE scenario (the cross product that signs the distance is 0), which no segment table cut from real polylines means; the
    reference treats it as a point obstacle at its plain distance."""
    cfg = spec.make_cfg()
    w = sat_ref.reward_cfg(cfg.dataset.waymo, remove=(0, 0, 0))
    st = np.zeros((3, 8), np.float32)
    st[:, 0], st[:, 1], st[:, 7] = (0.0, 3.0, 9.0), (1.0, 2.0, -4.0), 1.0
    segs = np.array([[-5, 0, 5, 0], [8, -8, 8, 8]], np.float32)
    (led, rtg, nrm), carry = sat_ref.ledger_step(0, st, np.zeros((3, 2)), np.full((3, 2), 50.0), segs, w, cfg.nocturne.rew_cfg, None)
    np.testing.assert_allclose(led[:, 5], np.array([1.0, 2.0, 1.0]) / 5.0, rtol=1e-14)
    assert np.array_equal(rtg, np.tile([10.0, 90.0, 90.0], (3, 1))) and np.array_equal(nrm, np.ones((3, 3)))
    (led1, rtg1, _), _ = sat_ref.ledger_step(1, st, np.zeros((3, 2)), None, segs, w, cfg.nocturne.rew_cfg, carry)
    np.testing.assert_array_equal(rtg1, rtg - led[:, 3:6])
    point = np.array([[3.0, 0.5, 3.0, 0.5]], np.float32)
    xy = st[:, :2].astype(np.float64)
    assert (rewards.signed_distance_to_road_edges(xy, [point.reshape(2, 2).astype(np.float64)]) == 0).all()      # the host form
    (led2, _, _), _ = sat_ref.ledger_step(0, st, np.zeros((3, 2)), np.full((3, 2), 50.0), np.concatenate([segs, point]), w,
                                          cfg.nocturne.rew_cfg, None)
    np.testing.assert_allclose(led2[:, 5], np.array([1.0, 1.5, 1.0]) / 5.0, rtol=1e-14)                            # the point obstacle
