"""CPU pins of the open-loop loss: the float64 restatement of compute_loss (tests/loss_ref.py) on the oracle's logits against the
UNMODIFIED reference's numbers (tests/golden/loss.npz, tools/gen_golden_loss.py); key sets per model variant; the head image of the
cross-entropy kernel; the evaluator's sharding on gloo."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import golden
from ctrlsim_amd import spec, pack
from ctrlsim_amd.models import CtRLSim
from ctrlsim_amd.evaluators import OpenLoopEvaluator
import model_oracle as mo
import synth_inputs
import loss_ref

EPS = 2.0 ** -23


def _oracle_sums(i):
    cfg = loss_ref.case_cfg(i)
    d = spec.Dims(cfg)
    w = loss_ref.case_weights(i, d)
    inp = loss_ref.case_inputs(i, d)
    with torch.no_grad():
        preds = {k: v.numpy() for k, v in mo.forward(mo.as_torch_weights(w), synth_inputs.to_torch(inp), d).items()}
    m = cfg.model
    if not m.predict_future_states:
        preds.pop("state_preds", None)
    scale = max(1.0, max(float(np.abs(preds[k]).max()) for k in ("action_preds", "rtg_preds") if k in preds))
    return cfg, d, w, scale, loss_ref.loss_sums(inp, preds, R=d.R, C=d.C, supervise_moving=bool(m.supervise_moving),
                                         local_frame=bool(m.local_frame_predictions), trajeglish=d.VARIANT == 2)


@pytest.mark.parametrize("case", range(len(loss_ref.CASES)))
def test_restatement_on_oracle_logits_matches_reference_compute_loss(case):
    """Bounds from the formats, not from the code under test: the oracle's logits are pinned to the reference's within 2e-5 at
    random-init weights, whose logits are of order 1 (tests/test_oracle_pinned.py); two float32 evaluations of one network differ in
    proportion to the logits' magnitude (the trained-like weights are the random ones with the heads' last Linear times 15: logits and
    their differences scale alike), so the logit bound is 2e-5 x max(1, max |logit|); a row's nll = lse - logit[target] moves by at most
    twice that, and the reference evaluates its means in float32 (8 EPS relative for sums of ~1e3 like-signed terms).  The state term: predictions within 2e-5 of targets ~1e2 apart, so
    1e-5 relative with the float32 evaluation included.  Counts are exact."""
    g = golden("loss")
    cfg, d, w, scale, r = _oracle_sums(case)
    model = CtRLSim(cfg, w)
    keys = [str(k) for k in g[f"c{case}_keys"]]
    assert model.loss_keys() == keys                                   # the reference's key set for this variant
    got = loss_ref.losses(r["sums"], keys, float(cfg.model.loss_action_coef))
    assert model.losses_from_sums(r["sums"]) == got                    # the library's sums -> means rule is the restatement's
    coef = float(cfg.model.loss_action_coef)
    for j, k in enumerate(keys):
        want = float(g[f"c{case}_loss"][j])
        assert r["sums"][loss_ref.KEYS.index(k), 1] == float(g[f"c{case}_count"][j]), k
        tol = 1e-5 * abs(want) if k == "loss_state" else max(coef, 1.0) * 4e-5 * scale + 8 * EPS * abs(want)
        assert abs(got[k] - want) <= tol, (k, got[k], want)
    if f"c{case}_row_nll" in g.files:
        want = g[f"c{case}_row_nll"]
        ok = np.isfinite(want)
        nll = r["row"][..., 0] - r["row"][..., 1]
        assert np.array_equal(np.isfinite(nll), ok)                    # the same rows are defined (Trajeglish: not the last step)
        assert np.abs(nll[ok] - want[ok]).max() <= 4e-5 * scale + 8 * EPS * np.abs(want[ok]).max()


def test_key_sets_and_logged_names_per_variant():
    want = {None: ["loss_actions", "loss_rtg_goal", "loss_rtg_veh", "loss_rtg_road", "loss_state"],
            "il": ["loss_actions"], "trajeglish": ["loss_actions"], "decision_transformer": ["loss_actions"]}
    for i, (size, variant, over, _, _) in enumerate(loss_ref.CASES):
        if size != "tiny":
            continue
        cfg = loss_ref.case_cfg(i)
        model = CtRLSim(cfg, loss_ref.case_weights(i, spec.Dims(cfg)))
        assert model.loss_keys() == want[variant]
        assert [CtRLSim.VAL_NAMES[k] for k in model.loss_keys()] == \
            ["val_loss", "val_rtg_goal_loss", "val_rtg_veh_loss", "val_rtg_road_loss", "val_state_loss"][:len(want[variant])] + []
    # sums -> means: loss_action_coef on the actions only, 100 * 2 * count under the state term, 0 / 0 = NaN
    cfg = spec.make_cfg(model__loss_action_coef=0.5, **loss_ref.TINY)
    model = CtRLSim(cfg)
    out = model.losses_from_sums(np.array([[8.0, 4.0], [6.0, 3.0], [0.0, 0.0], [1.0, 2.0], [400.0, 4.0]]))
    assert out["loss_actions"] == 1.0 and out["loss_rtg_goal"] == 2.0 and np.isnan(out["loss_rtg_veh"])
    assert out["loss_rtg_road"] == 0.5 and out["loss_state"] == 0.5


@pytest.mark.parametrize("n,nsm", [(1000, 1), (350, 3), (33, 2)])
def test_head_ce_image_is_softmax_major_and_zero_padded(n, nsm):
    """pack.head_ce_image: block cb of the image holds the columns of ONE softmax (component-major for the return head, whose rows are
    bin-major / component-minor in the checkpoint), pad rows and pad biases are zeros, and the planes add up to the weight."""
    rs = np.random.RandomState(n)
    W = rs.normal(0, 0.05, (n * nsm, 256)).astype(np.float32)
    b = rs.normal(0, 1, n * nsm).astype(np.float32)
    blk, bias = pack.head_ce_image(W, b, nsm, 1)
    bps = (n + 31) // 32
    assert blk.shape == (nsm * bps, 2, 16, 2, 32, 8) and bias.shape == (nsm * bps * 32,)
    planes = blk.view(np.float16).astype(np.float64)                                 # [cb][p][ks][half][col][e]
    Wimg = planes.sum(1).transpose(0, 3, 1, 2, 4).reshape(nsm, bps * 32, 256) / 256.0   # [cb][col][ks][half][e] -> rows of 256
    for s in range(nsm):
        np.testing.assert_allclose(Wimg[s, :n], W[s::nsm].astype(np.float64), rtol=0, atol=2.0 ** -22 * np.abs(W).max())
        assert not Wimg[s, n:].any()
        assert np.array_equal(bias.reshape(nsm, -1)[s, :n], b[s::nsm]) and not bias.reshape(nsm, -1)[s, n:].any()


class _OracleEvaluator(OpenLoopEvaluator):
    """The evaluator with its device call replaced by the CPU oracle + the float64 restatement: the sharding, the accumulation and the
    all-reduce are the shipped code."""

    def __init__(self, cfg, model):
        self.cfg, self.model, self.fused, self.device = cfg, model, True, "cpu"
        self.tw = mo.as_torch_weights(model.weights)

    def score(self, data):
        inp = dict(data["agent"], **data["map"])
        d, m = self.model.dims, self.cfg.model
        with torch.no_grad():
            preds = {k: v.numpy() for k, v in mo.forward(self.tw, synth_inputs.to_torch(inp), d).items()}
        r = loss_ref.loss_sums(inp, preds, R=d.R, C=d.C, supervise_moving=bool(m.supervise_moving),
                               local_frame=bool(m.local_frame_predictions))
        return torch.from_numpy(r["sums"])


def _windows(d, n):
    inp = loss_ref.make_inputs(d, 77, n)
    return [{k: v[i] for k, v in inp.items()} for i in range(n)]


def _evaluate():
    # (one window per call, one thread: the float32 CPU oracle standing in for the device is then the same function of a window in
    # every process, whatever its batch neighbours; the device path's own batch invariance is tests/test_gpu_loss.py's business)
    torch.set_num_threads(1)
    cfg = spec.make_cfg(**loss_ref.TINY)
    model = CtRLSim(cfg)
    return _OracleEvaluator(cfg, model).evaluate(_windows(model.dims, 7), batch_size=1)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = _evaluate()
    if rank == 0:
        q.put({k: out[k] for k in ("sums", "loss_actions", "loss_state", "windows")})
    dist.barrier()
    dist.destroy_process_group()


def test_evaluator_sharding_world_2_equals_world_1():
    """Seven windows (an odd count: the shards differ in size, and so do their masks) scored by two gloo ranks over interleaved shards
    give the sums, counts and means of one process — what per-shard means would not."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=180)
    for p in procs:
        p.join(timeout=90)
        assert p.exitcode == 0
    one = _evaluate()
    np.testing.assert_array_equal(got["sums"][:, 1], one["sums"][:, 1])
    np.testing.assert_allclose(got["sums"], one["sums"], rtol=1e-12, atol=0)
    assert got["windows"] == one["windows"] == 7
    for k in ("loss_actions", "loss_state"):
        assert abs(got[k] - one[k]) <= 1e-12 * abs(one[k])


@pytest.mark.parametrize("key", ["a0", "a1", "b0", "b1", "c0", "c1"])
def test_training_window_matches_reference_get_data(key):
    """ingest.training_window against the window the reference's training-mode get_data returned for the same preprocessed scene and
    the same two draws (tests/golden/loss.npz: win_*; validation split): integers exact, float64 arrays as tight as the other ingest
    pins (tests/test_ingest_pinned.py: 1e-12)."""
    from helpers import cfg_of
    from ctrlsim_amd import ingest
    g, gp = golden("loss"), golden("preprocessed")
    tag = key[0]
    cfg = cfg_of("loop")
    pre = {k[len(tag) + 5:]: gp[k] for k in gp.files if k.startswith(f"{tag}_pkl_")}
    pre["filtered_ag_ids"] = [int(i) for i in pre["filtered_ag_ids"]]
    origin_t, origin_agent = [int(v) for v in g[f"win_{key}_draws"]]
    win = ingest.training_window(pre, cfg, origin_t, origin_agent)
    assert set(win) == {"agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask", "road_points", "road_types"}
    for k in ("actions", "rtgs", "timesteps", "moving_agent_mask", "agent_types", "road_types"):
        assert np.array_equal(win[k], g[f"win_{key}_{k}"]), k
    for k in ("agent_states", "goals", "road_points"):
        np.testing.assert_allclose(win[k], g[f"win_{key}_{k}"], rtol=0, atol=1e-12, err_msg=k)
    # the seeded default draws a valid pair, and the same one for the same seed
    t0, a0 = ingest.window_choices(pre, cfg, 5)
    assert (t0, a0) == ingest.window_choices(pre, cfg, 5)
    w2 = ingest.training_window(pre, cfg, t0, a0)
    assert w2["timesteps"][0, 0, 0] == t0 and w2["moving_agent_mask"].sum() >= 1
    with pytest.raises(ValueError):
        ingest.training_window(pre, cfg, 10 ** 6, origin_agent)
