"""TEST INFRASTRUCTURE — a float64 NumPy restatement of the reference's `CtRLSim.compute_loss` (models/ctrl_sim.py:48-189), written
from its definition: masked cross-entropy of the action head and of the three interleaved return softmaxes, the shifted future-state
table with its `100 * 2 * mask.sum()` divisor, the local-frame form of the same, the Trajeglish shift.  It returns what the library
returns — sums and counts per term, per context, and the unmasked per-row nll — so that every layer of the new path has a checker
that shares no code with it."""
import numpy as np

KEYS = ("loss_actions", "loss_rtg_goal", "loss_rtg_veh", "loss_rtg_road", "loss_state")


def _lse_nll(logits, target):
    """logits [..., n] float64, target [...] int -> (lse, target logit)."""
    m = logits.max(-1)
    lse = m + np.log(np.exp(logits - m[..., None]).sum(-1))
    tl = np.take_along_axis(logits, target[..., None], -1)[..., 0]
    return lse, tl


def loss_sums(inp, preds, R=350, C=3, supervise_moving=True, local_frame=False, trajeglish=False):
    """inp: reference-layout arrays (agent_states [B,A,T,8], actions [B,A,T], rtgs [B,A,T,3], moving_agent_mask [B,A]);
    preds: {'action_preds' [B,A,T,V], 'rtg_preds' [B,A,T,R*C] or absent, 'state_preds' [B,A,T,2T] or absent} (any float dtype).
    -> dict(per_ctx [B,5,2] float64, sums [5,2], row [B,T,A,4,2] (lse, target logit) in the library's row order)."""
    st = np.asarray(inp["agent_states"], np.float32).astype(np.float64)         # the model sees float32 states
    B, A, T = st.shape[:3]
    ex = st[..., 7]
    mov = np.asarray(inp["moving_agent_mask"], np.float64)[:, :, None] if supervise_moving else np.ones((B, A, 1))
    mask = ex * mov
    per = np.zeros((B, 5, 2))
    row = np.full((B, A, T, 4, 2), np.nan)
    act = np.asarray(preds["action_preds"], np.float64)
    tok = np.asarray(inp["actions"]).astype(np.int64)
    if trajeglish:
        lse, tl = _lse_nll(act[:, :, :-1], tok[:, :, 1:])
        m = mask[:, :, 1:]
        row[:, :, :-1, 0, 0], row[:, :, :-1, 0, 1] = lse, tl
    else:
        lse, tl = _lse_nll(act, tok)
        m = mask
        row[:, :, :, 0, 0], row[:, :, :, 0, 1] = lse, tl
    per[:, 0, 0] = ((lse - tl) * m).sum((1, 2))
    per[:, 0, 1] = m.sum((1, 2))
    if preds.get("rtg_preds") is not None:
        rtg = np.asarray(preds["rtg_preds"], np.float64).reshape(B, A, T, R, C)
        bins = np.asarray(inp["rtgs"]).astype(np.int64)
        for c in range(C):
            lse, tl = _lse_nll(rtg[..., c], bins[..., c])
            row[:, :, :, 1 + c, 0], row[:, :, :, 1 + c, 1] = lse, tl
            per[:, 1 + c, 0] = ((lse - tl) * mask).sum((1, 2))
            per[:, 1 + c, 1] = mask.sum((1, 2))
    if preds.get("state_preds") is not None:
        sp = np.asarray(preds["state_preds"], np.float64).reshape(B, A, T, -1, 2)
        nslot = sp.shape[3]
        smask = ex if local_frame else mask                                        # (:152: the local-frame branch has no moving mask)
        for i in range(T):
            for j in range(min(nslot, T - i - 1)):
                tgt = st[:, :, i + 1 + j, :2]
                if local_frame:
                    d = tgt - st[:, :, i, :2]
                    yaw = st[:, :, i, 4]
                    c_, s_ = np.cos(-yaw), np.sin(-yaw)
                    tgt = np.stack([c_ * d[..., 0] - s_ * d[..., 1], s_ * d[..., 0] + c_ * d[..., 1]], -1)
                mk = smask[:, :, i + 1 + j]
                per[:, 4, 0] += (((sp[:, :, i, j] - tgt) ** 2).sum(-1) * mk).sum(1)
                per[:, 4, 1] += mk.sum(1)
    return dict(per_ctx=per, sums=per.sum(0), row=row.transpose(0, 2, 1, 3, 4))


def losses(sums, keys, loss_action_coef=1.0):
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in keys:
            i = KEYS.index(k)
            s, n = sums[i]
            out[k] = float((loss_action_coef * s if i == 0 else s) / (200.0 * n if i == 4 else n))
    return out


# ---- the cases of tests/golden/loss.npz (tools/gen_golden_loss.py writes them from the reference; the tests rebuild the inputs)
CASES = [
    # size, variant, model overrides, weights, batch
    ("tiny", None, {}, "random", 3),
    ("tiny", None, {"supervise_moving": False, "loss_action_coef": 0.5}, "trained", 3),
    ("tiny", None, {"local_frame_predictions": True}, "random", 3),
    ("tiny", None, {"attend_own_return_action": True}, "random", 3),
    ("tiny", "il", {}, "random", 3),
    ("tiny", "trajeglish", {}, "trained", 3),
    ("tiny", "decision_transformer", {}, "random", 3),
    ("full", None, {"loss_action_coef": 2.0}, "trained", 2),
    ("full", None, {"local_frame_predictions": True, "supervise_moving": False}, "random", 2),
    ("full", "trajeglish", {}, "random", 2),
]
TINY = dict(dataset__waymo__max_num_agents=4, dataset__waymo__train_context_length=4,
            dataset__waymo__max_num_road_polylines=6, dataset__waymo__max_num_road_pts_per_polyline=8)


def case_cfg(i):
    from ctrlsim_amd import spec
    size, variant, over, _, _ = CASES[i]
    base = dict(TINY if size == "tiny" else {})
    if variant:
        base.update({f"model__{variant}": True, "model__predict_rtg": False, "model__predict_future_states": False})
    base.update({"model__" + k: v for k, v in over.items()})
    return spec.make_cfg(**base)


def case_weights(i, d):
    from ctrlsim_amd import weights
    _, variant, _, wkind, _ = CASES[i]
    w = weights.generate(d, 0) if wkind == "random" else weights.generate_trained_like(d, 0)
    if variant in ("il", "trajeglish"):         # the reference modules of these cfgs have no such heads (cfgs/model/{il,trajeglish}.yaml)
        w = {k: v for k, v in w.items() if not k.startswith(("decoder.predict_rtg", "decoder.predict_future_states"))}
    return w


def make_inputs(d, seed, B, dt=False):
    """Windows with padded slots, agents that stop existing mid-window (synth_inputs.random_context) and a non-trivial moving mask."""
    import synth_inputs
    inp = synth_inputs.random_context(d, seed, B=B, n_agents=max(2, d.A - 1), n_polys=d.P - 1)
    mv = (np.random.RandomState(100 + seed).uniform(size=(B, d.A)) < 0.7).astype(np.float64)
    mv[:, 0] = 1.0
    inp["moving_agent_mask"] = mv
    if dt:
        inp["rtgs"] = synth_inputs.dt_rtgs(inp["rtgs"], seed)
    return inp


def case_inputs(i, d):
    return make_inputs(d, 20 + i, CASES[i][4], dt=CASES[i][1] == "decision_transformer")
