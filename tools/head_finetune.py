"""Head-only fine-tuning over a frozen trunk, end to end on the device: logged scenes -> LogReplayer.dataset -> DeviceDataset ->
windows.launch_windows -> CtRLSim.training_step_ctx / optimizer_step for N steps on one generated batch, printing the loss per step
under the names the reference logs (models/ctrl_sim.py:190-214).  Synthetic scenes and trained-like weights; the schedule is
cfgs/train/ctrl_sim_finetuning.yaml's (250 warm-up steps), so the first steps run at a small fraction of the learning rate.

    python tools/head_finetune.py [steps=20] [B=32] [S=4] [N=16] [rollout_steps=60] [polylines=64]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctrlsim_amd  # noqa: E402,F401
from ctrlsim_amd import spec, scenarios, datagen, weights  # noqa: E402
from ctrlsim_amd.models import CtRLSim  # noqa: E402
from ctrlsim_amd.engine import CtxBuffers  # noqa: E402
from ctrlsim_amd.windows import launch_windows  # noqa: E402


def main(scope="heads"):
    """scope: what CtRLSim.set_trainable takes (tools/ffn_finetune.py runs this loop with "heads+ffn")."""
    arg = lambda i, default: int(sys.argv[i]) if len(sys.argv) > i else default
    steps, B, S, N, T1, polys = arg(1, 20), arg(2, 32), arg(3, 4), arg(4, 16), arg(5, 60), arg(6, 64)
    cfg = spec.make_cfg(nocturne__steps=T1, **{"train__" + k: v for k, v in spec.TRAIN_FINETUNING.items()})
    d = spec.Dims(cfg)
    dev = "cuda:0"
    scns = [scenarios.make_scenario(23, k, n_agents=N, n_polylines=polys, n_points=d.NP, extent=60.0) for k in range(S)]
    logs = [scenarios.standin_log(s, T1 + 1) for s in scns]
    rp = datagen.LogReplayer(cfg, dev).load(scns, logs, T1)
    rp.run()
    ds = rp.device_dataset(rp.dataset(), scns)
    tr = np.array([(k % S,) + ds.choices(k % S, 7 * 100003 + k) for k in range(B)])
    scn, t, a = ds.validate(tr[:, 0], tr[:, 1], tr[:, 2])
    up = lambda x: torch.from_numpy(x).to(dev)
    cb, moving, status = launch_windows(ds, up(scn), up(t), up(a), B, out=CtxBuffers(d, B, dev))
    assert int(status.abs().sum()) == 0
    model = CtRLSim(cfg, weights.generate_trained_like(d, 0), device=dev).set_trainable(scope)
    opt, sched = model.configure_optimizers()
    first = last = None
    for step in range(steps):
        lr = opt.param_groups[0]["lr"]
        loss = model.training_step_ctx(cb, moving, B)
        norm = model.optimizer_step(opt, sched)
        print(json.dumps({"step": step, "final_loss": loss, "lr": lr, "grad_norm": norm, **model.logged}))
        first = loss if first is None else first
        last = loss
    print(f"{B} windows of {S} scenes, scope {scope}, {steps} steps: final_loss {first:.6f} -> {last:.6f}")
    assert last < first, "the loss did not fall"


if __name__ == "__main__":
    main()
