"""Host checks of tests/hidden_cases.py, without a GPU: the staged oracle is model_oracle.forward, the stage functions chain to it, each
recipe holds the edges it promises, the float32 yardstick of tests/test_gpu_hidden_rows.py is sane, and every wrong-on-purpose twin of the
staged oracle moves the tensor it first appears in by at least 100 x the largest bound that test could ever be granted (K = 8 times the
yardstick), on the tiny and the loop recipe under both kinds of weights.  profiles/hidden_state_parity.md records what is printed here."""
import numpy as np
import pytest
import torch

import hidden_cases as hc
import model_oracle as mo

HOST = ("tiny", "loop")
K_MAX = 8.0                 # the largest factor the project grants against a float32 evaluation
CATCH = 100.0


@pytest.mark.parametrize("kind,wkind,own", [(k, w, False) for k in HOST for w in hc.WEIGHTS] + [("tiny", "trained", True)])
def test_staged_oracle_is_model_oracle_bit_for_bit_in_float32(kind, wkind, own):
    d = hc.cfg_dims(kind, own)[1]
    tw = hc.torch_weights(hc.make_weights(kind, wkind, own), torch.float32)
    x = hc.torch_inputs(hc.recipe(kind), torch.float32)
    s = hc.staged(tw, x, d, torch.float32)
    with torch.no_grad():
        o = mo.forward(tw, x, d, return_hidden=True)
    for mine, theirs in (("tokens", "stacked_embeddings"), ("seg", "road_seg_emb"), ("mem", "encoder_embeddings"), ("x_out", "decoder_out"),
                         ("rtg_preds", "rtg_preds"), ("action_preds", "action_preds"), ("state_preds", "state_preds")):
        assert s[mine].dtype == torch.float32 and torch.equal(s[mine], o[theirs]), mine
    B, L = x["agent_states"].shape[0], 3 * d.T * d.A
    assert s["tokens"].shape == (B, L, 256) and s["seg"].shape == (B, d.P, 256) and s["mem"].shape == (B, d.P + d.A, 256)
    assert s["pad"].shape == (B, d.P + d.A) and len(s["x0"]) == d.ND and s["x0"][0] is s["tokens"]
    assert all(t.shape == (B, L, 256) for t in s["x0"] + [s["x1_last"], s["u_last"], s["x_out"]])
    assert not s["pad"].all(1).any()                                               # no context without a key: no NaN row by construction
    assert all(torch.isfinite(t).all() for t in s["x0"] + [s["seg"], s["mem"], s["x1_last"], s["u_last"], s["x_out"]])


@pytest.mark.parametrize("kind,wkind,own", [(k, w, False) for k in HOST for w in hc.WEIGHTS] + [("tiny", "init", True)])
def test_chained_stage_functions_reproduce_the_staged_oracle_exactly_in_float64(kind, wkind, own):
    """Each stage function on the previous stage's float64 rows: tokens, seg, mem, then layer_grad_ref.layer layer after layer — the form
    the GPU test feeds device rows into — gives staged()'s float64 tensors bit for bit."""
    f8 = torch.float64
    d = hc.cfg_dims(kind, own)[1]
    s = hc.staged_of(kind, wkind, f8, own)
    tw, x = hc.torch_weights(hc.make_weights(kind, wkind, own), f8), hc.torch_inputs(hc.recipe(kind), f8)
    same = lambda t, a: np.array_equal(t.numpy(), a)
    tokens, init_rows, init_exist = hc.stage_tokens(tw, x, d, f8)
    seg, valid = hc.stage_seg(tw, x["road_points"], x["road_types"], d, f8)
    pad = ~torch.cat([valid, init_exist], 1)
    assert tokens.dtype == f8 and same(tokens, s["tokens"]) and same(seg, s["seg"]) and same(pad, s["pad"]) and same(init_rows, s["init_rows"])
    mem = hc.stage_mem(tw, seg, init_rows, pad, d, f8)
    assert same(mem, s["mem"])
    xx = tokens
    for l in range(d.ND):
        assert same(xx, s["x0"][l]), l
        xx, x1, u = hc.stage_layer(tw, l, xx, mem, pad, d)
    assert same(x1, s["x1_last"]) and same(u, s["u_last"]) and same(xx, s["x_out"])


@pytest.mark.parametrize("kind", list(hc.PRESETS))
def test_recipe_holds_the_edges_it_promises(kind):
    d = hc.cfg_dims(kind)[1]
    inp = hc.recipe(kind)
    B = hc.PRESETS[kind][1]
    e = hc.edges(inp)
    ex = inp["agent_states"][..., 7] != 0
    npts = (inp["road_points"][..., 2] != 0).sum(-1)
    assert ex.shape == (B, d.A, d.T) and npts.shape == (B, d.P)
    flat = [np.concatenate([np.asarray(v[b], np.float64).reshape(-1) for v in inp.values()]) for b in range(B)]
    assert all(not np.array_equal(flat[i], flat[j]) for i in range(B) for j in range(i))          # every context differs
    assert min(e["live_polys"]) >= 1 and ex[:, :, 0].any(1).all()                                 # no fully masked attention row
    ctxs = lambda pairs: {b for b, _ in pairs}
    every = set(range(B))
    # an agent absent at window step 0 and present later: key-padded scene row, live tokens
    assert ctxs(e["late"]) == every and all(not ex[b, a, 0] and ex[b, a, 1:].any() for b, a in e["late"])
    # an agent present at step 0 that vanishes
    assert ctxs(e["gone"]) == every and all(ex[b, a, 0] and not ex[b, a, -1] for b, a in e["gone"])
    # a dead slot between two live slots
    assert ctxs(e["dead_between"]) == every
    for b, a in e["dead_between"]:
        assert not inp["agent_states"][b, a].any() and (inp["agent_types"][b, a] == -1).all()
        assert (inp["agent_types"][b, a - 1] != -1).any() and (inp["agent_types"][b, a + 1] != -1).any()
    # a live polyline with exactly one point, one with all NP points, a zero-point polyline in the middle of the list
    assert ctxs(e["one_point"]) == every and all(npts[b, p] == 1 and inp["road_points"][b, p, 0, 2] == 1 for b, p in e["one_point"])
    assert ctxs(e["all_points"]) == every and all(npts[b, p] == d.NP for b, p in e["all_points"])
    assert ctxs(e["zero_mid"]) == every
    for b, p in e["zero_mid"]:
        assert npts[b, p] == 0 and npts[b, :p].any() and npts[b, p + 1:].any() and not inp["road_points"][b, p].any()
    # each of the road types used; RTG bins 0 and R-1 and action tokens 0 and V-1 on rows that exist
    assert e["road_types"] == set(hc.ROAD_TYPES)
    assert {0, d.R - 1} <= e["rtg_bins"] and {0, d.V - 1} <= e["actions"]
    assert min(e["rtg_bins"]) >= 0 and max(e["rtg_bins"]) < d.R and min(e["actions"]) >= 0 and max(e["actions"]) < d.V
    # the smallest and the largest legal window start (a batch of one context: the largest)
    assert d.MAXT - d.T in e["starts"] and (B == 1 or 0 in e["starts"])
    assert 0 <= inp["timesteps"].min() and inp["timesteps"].max() == d.MAXT - 1
    assert (np.diff(inp["timesteps"][:, :, :, 0], axis=2) == 1).all()


@pytest.mark.parametrize("kind,wkind", [(k, w) for k in HOST for w in hc.WEIGHTS])
def test_yardstick_is_finite_nonzero_and_small(kind, wkind):
    s64 = hc.staged_of(kind, wkind, torch.float64)
    e = hc.yardstick(kind, wkind)
    big = {k: max(float(np.abs(t).max()) for t in v) for k, v in hc.compared(s64, s64["pad"]).items()}
    print(f"\n{kind} {wkind}: " + "  ".join(f"{k} e_ref {e[k]:.2e} (max {big[k]:.2f})" for k in hc.KINDS))
    assert set(e) == set(hc.KINDS)
    for k in hc.KINDS:
        assert np.isfinite(e[k]) and 0.0 < e[k] < 1e-4 * big[k], (k, e[k], big[k])


def _moved(fault, twin, s64):
    where = hc.FAULTS[fault]
    pad = s64["pad"]
    if where in ("tokens", "seg"):
        return where, hc.dist(twin[where], s64[where])
    if where == "mem":
        keep = ~pad
        return "mem", hc.dist(twin["mem"].numpy()[keep], s64["mem"][keep])
    if where == "u_last":
        return "u", hc.dist(twin["u_last"], s64["u_last"])
    assert where == "x0_1"
    return "layer", hc.dist(twin["x0"][1], s64["x0"][1])


@pytest.mark.parametrize("fault", list(hc.FAULTS))
@pytest.mark.parametrize("kind,wkind", [(k, w) for k in HOST for w in hc.WEIGHTS])
def test_wrong_on_purpose_twin_moves_its_tensor_a_hundred_bounds(kind, wkind, fault):
    """The twin is planted in the float64 staged oracle; the tensor where it first appears must move by CATCH x K_MAX x e_ref of that tensor
    kind.  Printed, not asserted: how far the logits of the queried (last) step move — what a logit-level test would have seen."""
    f8 = torch.float64
    d = hc.cfg_dims(kind)[1]
    s64 = hc.staged_of(kind, wkind, f8)
    twin = hc.staged(hc.torch_weights(hc.make_weights(kind, wkind), f8), hc.torch_inputs(hc.recipe(kind), f8), d, f8, fault=fault)
    tkind, moved = _moved(fault, twin, s64)
    need = CATCH * K_MAX * hc.yardstick(kind, wkind)[tkind]
    shift = max(hc.dist(twin[h][:, :, d.T - 1], s64[h][:, :, d.T - 1]) for h in ("rtg_preds", "action_preds"))
    print(f"\n{kind} {wkind} {fault}: {tkind} moves {moved:.3e} (needs {need:.3e}: {moved / need:.1f} x); logits of the last step move {shift:.3e}")
    assert np.isfinite(moved) and moved >= need, (fault, tkind, moved, need)
    # what the defect cannot reach is untouched: the tensor named is where it FIRST appears
    before = {"tokens": ["seg"], "seg": ["tokens"], "mem": ["tokens", "seg"], "u": ["tokens", "seg", "mem", "x1_last"], "layer": ["tokens", "seg", "mem"]}
    for k in before[tkind]:
        assert np.array_equal(twin[k].numpy(), s64[k]), (fault, k)
