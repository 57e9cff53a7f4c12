"""TEST INFRASTRUCTURE — writes tests/golden/self_grads.npz from the UNMODIFIED reference: its forward with autograd, its compute_loss,
final_loss summed as its training_step does (models/ctrl_sim.py:190-214), and backward — the gradients of the LAST decoder layer's
self-attention sublayer (self_attn.in_proj / out_proj, norm1) for the cases of tests/loss_ref.py:CASES that
tests/test_gpu_self_attn_grads.py runs through the model (tiny 0 and 1, full 7), in the format of tools/gen_golden_cross_grads.py.  Runs only where the reference checkout exists; nothing under tests/ -m gpu, smoke() or bench.py imports
it.  The fixture holds arrays only.  Inputs are recipes (tests/loss_ref.py:case_inputs), weights are generated (ctrlsim_amd/weights.py).
The model is in eval mode (no dropout, as the library's forward) with gradients enabled.

    python tools/gen_golden_self_grads.py

Per case c<i>_ and tensor <name> (state-dict name):
  g_<name>              the full gradient of every bias and LayerNorm parameter (float32, as autograd left it)
  r_<name>, s_<name>    for in_proj_weight / out_proj.weight: 16 sampled row indices (first, last, the rest seeded) and those rows
  n_<name>, c_<name>    its Frobenius norm and its column sums (float64 sums of the float32 gradient)"""
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

CASES = (0, 1, 7)


def run_case(i):
    cfg = loss_ref.case_cfg(i)
    d = spec.Dims(cfg)
    ref = ggl.reference_model(cfg, loss_ref.case_weights(i, d))
    data = synth_inputs.to_motion_data(loss_ref.case_inputs(i, d))
    ld = ref.compute_loss(data, ref(data, eval=True))
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
    rs = np.random.RandomState(3000 + i)
    pre = f"decoder.transformer_decoder.layers.{d.ND - 1}."
    grads = {n: p.grad.detach().numpy() for n, p in ref.named_parameters() if n.startswith((pre + "self_attn.", pre + "norm1"))}
    assert len(grads) == 6, sorted(grads)
    for name, g in grads.items():
        assert np.isfinite(g).all() and g.any(), name
        if g.ndim == 1:
            out[P + "g_" + name] = g.astype(np.float32)
            continue
        n = g.shape[0]
        rows = np.array(sorted({0, n - 1} | set(int(r) for r in rs.permutation(n)[:14])))[:16]
        out[P + "r_" + name] = rows.astype(np.int32)
        out[P + "s_" + name] = g[rows].astype(np.float32)
        out[P + "n_" + name] = np.array(np.linalg.norm(g.astype(np.float64)))
        out[P + "c_" + name] = g.astype(np.float64).sum(0)
    print(i, "final", float(final.detach()), {k.split(".")[-2] + "." + k.split(".")[-1]: float(np.abs(v).max()) for k, v in grads.items()})
    return out


def main():
    ggl.install()
    out = {"cases": np.array(CASES)}
    for i in CASES:
        out.update(run_case(i))
    path = os.path.join(ROOT, "tests", "golden", "self_grads.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
