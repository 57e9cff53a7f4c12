"""TEST INFRASTRUCTURE — writes tests/golden/head_grads.part<k>.npz from the UNMODIFIED reference: its forward with autograd, its
compute_loss, final_loss summed as its training_step does (models/ctrl_sim.py:190-214), and backward — for the cases of
tests/loss_ref.py:CASES that the head-gradient tests use (tiny 0, 1, 2, 4, 5, 6 and full 7).  Runs only where the reference checkout
exists; nothing under tests/ -m gpu, smoke() or bench.py imports it.  The fixture holds arrays and name lists only.  Inputs are
recipes (tests/loss_ref.py:case_inputs), weights are generated (ctrlsim_amd/weights.py).  The model is in eval mode (no dropout, as
the library's forward) with gradients enabled.

    python tools/gen_golden_head_grads.py

Per case c<i>_:
  keys, loss            the reference's loss names and values; final = their sum as training_step forms it
  g_<name>              the full gradient of every head bias and LayerNorm parameter (float32, as autograd left it)
  r_<name>, s_<name>    for every head weight matrix: 16 sampled row indices (row 0, the last class — 999 / bin 349 component 2 —, a class
                        that is some row's target, the rest seeded) and those rows of the gradient
  n_<name>, c_<name>    its Frobenius norm and its column sums (float64 sums of the float32 gradient)
  X, X_types            tiny cases: the decoder output (the result of `transformer_decoder`) as [B*T*A, len(X_types), 256], the token
                        types, in the LIBRARY's three-slot numbering, that a head reads
  dx_rows, dx, dx_norm  32 sampled token rows of the gradient at the decoder output (library row numbering), and its norm
And once: decay / no_decay — the reference's AdamW groups restricted to decoder.predict_* (of the CtRL-Sim model); lr_steps,
lr_base, lr_finetuning — create_lambda_lr at those steps under cfgs/train/base.yaml and ctrl_sim_finetuning.yaml."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_loss as ggl  # noqa: E402  (the shims and the reference model constructor)
import synth_inputs  # noqa: E402
import loss_ref  # noqa: E402
from ctrlsim_amd import spec  # noqa: E402

CASES = (0, 1, 2, 4, 5, 6, 7)
LR_STEPS = (0, 1, 249, 250, 500, 1440, 200000)
PARTS = ((0, 1), (2, 4), (5, 6, 7))           # cases per file: every part stays below the largest fixture committed before it


def lib_types(variant):
    """reference token type -> the library's three-slot type (csrc/forward.hip), for the types a head reads."""
    if variant == "il":
        return {0: 0}
    if variant == "trajeglish":
        return {0: 2}
    if variant == "decision_transformer":
        return {1: 0}
    return {0: 0, 1: 1, 2: 2}


def run_case(i):
    import torch
    size, variant, over, wkind, B = loss_ref.CASES[i]
    cfg = loss_ref.case_cfg(i)
    d = spec.Dims(cfg)
    w = loss_ref.case_weights(i, d)
    ref = ggl.reference_model(cfg, w)
    inp = loss_ref.case_inputs(i, d)
    data = synth_inputs.to_motion_data(inp)
    seen = []

    def keep(module, args, result):            # (returns None: the result goes on unchanged)
        result.retain_grad()
        seen.append(result)

    hook = ref.decoder.transformer_decoder.register_forward_hook(keep)
    preds = ref(data, eval=True)
    hook.remove()
    ld = ref.compute_loss(data, preds)
    m = cfg.model
    final = ld["loss_actions"]                                  # training_step, models/ctrl_sim.py:207-214
    if m.predict_rtg:
        final = final + ld["loss_rtg_goal"] + ld["loss_rtg_veh"] + ld["loss_rtg_road"]
    if m.predict_future_states:
        final = final + ld["loss_state"]
    ref.zero_grad()
    final.backward()
    out = {}
    P = f"c{i}_"
    keys = list(ld)
    out[P + "keys"] = np.array(keys)
    out[P + "loss"] = np.array([float(ld[k].detach()) for k in keys], np.float64)
    out[P + "final"] = np.array(float(final.detach()))
    rs = np.random.RandomState(1000 + i)
    tok = np.asarray(inp["actions"]).reshape(-1)
    bins = np.asarray(inp["rtgs"]).reshape(-1, 3)
    for name, p in ref.named_parameters():
        if not name.startswith("decoder.predict_"):
            continue
        g = p.grad.detach().numpy()
        assert np.isfinite(g).all(), name
        if g.ndim == 1:
            out[P + "g_" + name] = g.astype(np.float32)
            continue
        n = g.shape[0]
        fixed = [0, n - 1]
        if name.endswith("mlp.3.weight") and "predict_action" in name:
            fixed.append(int(tok[0]))
        if name.endswith("mlp.3.weight") and "predict_rtg" in name:
            fixed.append(int(bins[0, 1]) * 3 + 1)
        rest = [r for r in rs.permutation(n) if r not in fixed][:16 - len(fixed)]
        rows = np.array(sorted(set(fixed)) + sorted(int(r) for r in rest))[:16]
        out[P + "r_" + name] = rows.astype(np.int32)
        out[P + "s_" + name] = g[rows].astype(np.float32)
        out[P + "n_" + name] = np.array(np.linalg.norm(g.astype(np.float64)))
        out[P + "c_" + name] = g.astype(np.float64).sum(0)
    o = seen[0]
    ntypes = o.shape[1] // (d.T * d.A)
    X = o.detach().numpy().reshape(B * d.T * d.A, ntypes, d.D)
    dX = o.grad.detach().numpy().reshape(B * d.T * d.A, ntypes, d.D)
    tmap = lib_types(variant)
    if size == "tiny":
        out[P + "X"] = np.ascontiguousarray(X[:, sorted(tmap)]).astype(np.float32)
        out[P + "X_types"] = np.array([tmap[k] for k in sorted(tmap)], np.int32)
    # the gradient at the decoder output: rows of the types a head reads, in the library's numbering (every other row is zero there)
    other = [k for k in range(ntypes) if k not in tmap]
    assert all(not dX[:, k].any() for k in other)
    cand = np.array([(r, k) for r in range(B * d.T * d.A) for k in sorted(tmap)])
    pick = cand[np.sort(rs.permutation(len(cand))[:32])]
    out[P + "dx_rows"] = np.array([r * 3 + tmap[k] for r, k in pick], np.int64)
    out[P + "dx"] = np.stack([dX[r, k] for r, k in pick]).astype(np.float32)
    out[P + "dx_norm"] = np.array(np.linalg.norm(dX.astype(np.float64)))
    print(i, size, variant, over, wkind, dict(zip(keys, out[P + "loss"])), "final", float(final.detach()), "|dX|", float(out[P + "dx_norm"]))
    return out


def optimizer_facts():
    """The reference's own parameter groups (configure_optimizers on its CtRL-Sim model) and learning-rate factors."""
    from utils.train_utils import create_lambda_lr
    cfg = loss_ref.case_cfg(0)
    d = spec.Dims(cfg)
    ref = ggl.reference_model(cfg, loss_ref.case_weights(0, d))
    ref.cfg["train"] = spec.Cfg(dict(spec.TRAIN))
    (opt,), _ = ref.configure_optimizers()
    name_of = {id(p): n for n, p in ref.named_parameters()}
    groups = [[name_of[id(p)] for p in g["params"]] for g in opt.param_groups]
    assert opt.param_groups[0]["weight_decay"] == spec.TRAIN["weight_decay"] and opt.param_groups[1]["weight_decay"] == 0.0
    out = {"decay": np.array([n for n in groups[0] if n.startswith("decoder.predict_")]),
           "no_decay": np.array([n for n in groups[1] if n.startswith("decoder.predict_")]),
           "lr_steps": np.array(LR_STEPS, np.int64)}
    for tag, tr in (("base", spec.TRAIN), ("finetuning", spec.TRAIN_FINETUNING)):
        lam = create_lambda_lr(spec.Cfg({"train": spec.Cfg(dict(tr))}))
        out["lr_" + tag] = np.array([lam(s) for s in LR_STEPS], np.float64)
    return out


def main():
    ggl.install()
    per_case = {i: run_case(i) for i in CASES}
    facts = optimizer_facts()
    for k, cases in enumerate(PARTS):
        out = {}
        for i in cases:
            out.update(per_case[i])
        if k == 0:
            out.update(facts)
            out["cases"] = np.array(CASES)
        path = os.path.join(ROOT, "tests", "golden", f"head_grads.part{k}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
