"""TEST INFRASTRUCTURE — writes tests/golden/loss.npz from the UNMODIFIED reference: its CtRLSim.compute_loss (models/ctrl_sim.py:48-189)
on its own forward, for the cases of tests/loss_ref.py:CASES.  Runs only where the reference checkout exists (the build container);
nothing under tests/ -m gpu, smoke() or bench.py imports it.  The fixture holds arrays only: per case the reference's loss values, the
mask counts behind them, and — tiny cases — F.cross_entropy(reduction='none') per row and softmax.  Inputs are recipes
(tests/loss_ref.py:case_inputs), weights are generated (ctrlsim_amd/weights.py).

    python tools/gen_golden_loss.py

Beyond oracle/ref_shims.py the reference's models/ctrl_sim.py needs: pytorch_lightning (absent: LightningModule = nn.Module with a
no-op save_hyperparameters, utilities.grad_norm), a namespace package `models`, cfg.train.finetuning.  Stubs without arithmetic."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_shims  # noqa: E402
import synth_inputs  # noqa: E402
import loss_ref  # noqa: E402
from ctrlsim_amd import spec  # noqa: E402


def install():
    import torch.nn as nn
    ref_shims.install()
    if "pytorch_lightning" not in sys.modules:
        class LightningModule(nn.Module):
            def save_hyperparameters(self, *a, **k):
                pass

            def log(self, *a, **k):
                pass

        pl = types.ModuleType("pytorch_lightning")
        pl.LightningModule = LightningModule
        ut = types.ModuleType("pytorch_lightning.utilities")
        ut.grad_norm = lambda *a, **k: {}
        pl.utilities = ut
        sys.modules["pytorch_lightning"], sys.modules["pytorch_lightning.utilities"] = pl, ut
    if "models" not in sys.modules:
        m = types.ModuleType("models")
        m.__path__ = [os.path.join(ref_shims.REF, "models")]
        sys.modules["models"] = m


def reference_model(cfg, w):
    import torch
    from models.ctrl_sim import CtRLSim
    cfg = cfg.copy()
    cfg["train"] = spec.Cfg({"finetuning": False})
    m = CtRLSim(cfg)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in w.items()}, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return m.eval()


def reference_windows():
    """The reference's training-mode get_data (datasets/rl_waymo/dataset_ctrl_sim.py:99-160, validation split: no agent shuffle) on the
    preprocessed scenes of tests/golden/preprocessed.npz under a seeded np.random: the window it returned and the two draws that
    reproduce it (origin step = timesteps[0, 0]; origin agent = what its select_random_origin_agent returned)."""
    import tempfile
    from datasets.rl_waymo.dataset_ctrl_sim import RLWaymoDatasetCtRLSim
    g = np.load(os.path.join(ROOT, "tests", "golden", "preprocessed.npz"))
    LOOP = dict(dataset__waymo__max_num_agents=6, dataset__waymo__train_context_length=8,
                dataset__waymo__max_num_road_polylines=12, dataset__waymo__max_num_road_pts_per_polyline=10, nocturne__steps=20)
    cfg = spec.make_cfg(**LOOP)
    cfg.dataset.waymo.preprocess_dir = tempfile.mkdtemp()
    cfg.dataset.waymo.preprocess = True
    ds = RLWaymoDatasetCtRLSim(cfg, split_name="val", mode="train")
    picked = []
    inner = ds.select_random_origin_agent
    ds.select_random_origin_agent = lambda *a: (picked.append(int(inner(*a))), picked[-1])[1]
    out = {}
    for tag in ("a", "b", "c"):
        pre = {k[len(tag) + 5:]: g[k] for k in g.files if k.startswith(f"{tag}_pkl_")}
        pre["filtered_ag_ids"] = [int(i) for i in pre["filtered_ag_ids"]]
        pre["idx"], pre["num_agents"] = 0, len(pre["ag_data"])
        for seed in (0, 1):
            np.random.seed(100 + seed)
            d, no_road = ds.get_data({k: (v.copy() if hasattr(v, "copy") else v) for k, v in pre.items()}, 0)
            assert not no_road
            key = f"win_{tag}{seed}"
            for k in ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps", "moving_agent_mask"):
                out[f"{key}_{k}"] = np.asarray(d["agent"][k])[0]
            for k in ("road_points", "road_types"):
                out[f"{key}_{k}"] = np.asarray(d["map"][k])[0]
            out[f"{key}_draws"] = np.array([int(out[f"{key}_timesteps"][0, 0, 0]), picked[-1]])
            print(key, "origin_t, origin agent", out[f"{key}_draws"], "agents", int((out[f"{key}_agent_types"][:, 0] != -1).sum()),
                  "moving", out[f"{key}_moving_agent_mask"])
    return out


def main():
    import torch
    import torch.nn.functional as F
    install()
    out = {"n_cases": np.array(len(loss_ref.CASES))}
    for i, (size, variant, over, wkind, B) in enumerate(loss_ref.CASES):
        cfg = loss_ref.case_cfg(i)
        d = spec.Dims(cfg)
        ref = reference_model(cfg, loss_ref.case_weights(i, d))
        inp = loss_ref.case_inputs(i, d)
        data = synth_inputs.to_motion_data(inp)
        with torch.no_grad():
            preds = ref(data, eval=True)
            ld = ref.compute_loss(data, preds)
        keys = list(ld)
        vals = np.array([float(ld[k]) for k in keys], np.float64)
        # the mask counts behind the means (data only): existence x moving; the shifted state table; Trajeglish: existence of the next step
        ex = inp["agent_states"][..., 7]
        mov = inp["moving_agent_mask"][:, :, None] if cfg.model.supervise_moving else np.ones_like(ex[:, :, :1])
        m = ex * mov
        cnt = {"loss_actions": (m[:, :, 1:] if variant == "trajeglish" else m).sum()}
        for k in ("loss_rtg_goal", "loss_rtg_veh", "loss_rtg_road"):
            cnt[k] = m.sum()
        ms = ex if cfg.model.local_frame_predictions else m
        cnt["loss_state"] = sum(ms[:, :, t + 1:].sum() for t in range(d.T))
        counts = np.array([cnt[k] for k in keys], np.float64)
        assert (counts > 0).all(), (i, keys, counts)
        assert np.isfinite(vals).all()
        out[f"c{i}_keys"] = np.array(keys)
        out[f"c{i}_loss"] = vals
        out[f"c{i}_count"] = counts
        out[f"c{i}_recipe"] = np.array([20 + i, B, d.A, d.T])
        if size == "tiny":
            row = np.full((B, d.A, d.T, 4), np.nan)
            ap, tok = preds["action_preds"].double(), data["agent"].actions.long()
            if variant == "trajeglish":
                row[:, :, :-1, 0] = F.cross_entropy(ap[:, :, :-1].reshape(-1, d.V), tok[:, :, 1:].reshape(-1), reduction="none").view(B, d.A, d.T - 1).numpy()
            else:
                row[..., 0] = F.cross_entropy(ap.reshape(-1, d.V), tok.reshape(-1), reduction="none").view(B, d.A, d.T).numpy()
            if "rtg_preds" in preds:
                rp = preds["rtg_preds"].double().reshape(-1, d.R, d.C)
                for c in range(d.C):
                    row[..., 1 + c] = F.cross_entropy(rp[:, :, c], data["agent"].rtgs[..., c].long().reshape(-1),
                                                      reduction="none").view(B, d.A, d.T).numpy()
            out[f"c{i}_row_nll"] = row.transpose(0, 2, 1, 3)                 # the library's row order [B,T,A,4]
        print(i, size, variant, over, wkind, dict(zip(keys, vals)), counts)
    out.update(reference_windows())
    path = os.path.join(ROOT, "tests", "golden", "loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
