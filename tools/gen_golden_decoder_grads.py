"""TEST INFRASTRUCTURE — writes tests/golden/decoder_grads.part*.npz from the UNMODIFIED reference: its forward with autograd, its
compute_loss, final_loss summed as its training_step does (models/ctrl_sim.py:190-214), and backward — the gradients of the decoder layers
0 .. ND-2 (all 18 tensors of each) and, by tensor hooks on the two inputs of its transformer decoder, the gradient at the scene encoder's
output and at the decoder's input rows, for the cases of tests/loss_ref.py:CASES that tests/test_gpu_decoder_grads.py runs through the model
(tiny 0 and 1, full 7), in the format of tools/gen_golden_self_grads.py, one part per case.  Runs only where the reference checkout exists;
nothing under tests/ -m gpu, smoke() or bench.py imports it.  The fixture holds arrays only.  Inputs are recipes
(tests/loss_ref.py:case_inputs), weights are generated (ctrlsim_amd/weights.py).  The model is in eval mode (no dropout, as the library's
forward) with gradients enabled.

    python tools/gen_golden_decoder_grads.py

Per case c<i>_ and tensor <name> (state-dict name):
  g_<name>              the full gradient of every bias and LayerNorm parameter (float32, as autograd left it)
  r_<name>, s_<name>    for the six matrices of a layer: 16 sampled row indices (first, last, the rest seeded) and those rows
  n_<name>, c_<name>    its Frobenius norm and its column sums (float64 sums of the float32 gradient)
and for <name> = dMem (the gradient at the encoder output, [B * (P + A), 256]: the reference has no filler rows) and dX0 (at the decoder
input, [B * 3 T A, 256]): r_, s_ and n_ as for a matrix."""
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


def sample(out, P, name, g, rs):
    n = g.shape[0]
    rows = np.array(sorted({0, n - 1} | set(int(r) for r in rs.permutation(n)[:14])))[:16]
    out[P + "r_" + name] = rows.astype(np.int32)
    out[P + "s_" + name] = g[rows].astype(np.float32)
    out[P + "n_" + name] = np.array(np.linalg.norm(g.astype(np.float64)))


def run_case(i):
    cfg = loss_ref.case_cfg(i)
    d = spec.Dims(cfg)
    ref = ggl.reference_model(cfg, loss_ref.case_weights(i, d))
    data = synth_inputs.to_motion_data(loss_ref.case_inputs(i, d))
    seen = {}

    def tap(module, args, kwargs):                              # transformer_decoder(stacked_embeddings, encoder_embeddings, ...)
        args[0].register_hook(lambda g: seen.__setitem__("dX0", g.detach().numpy().copy()))
        args[1].register_hook(lambda g: seen.__setitem__("dMem", g.detach().numpy().copy()))

    handle = ref.decoder.transformer_decoder.register_forward_pre_hook(tap, with_kwargs=True)
    ld = ref.compute_loss(data, ref(data, eval=True))
    handle.remove()
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
    rs = np.random.RandomState(4000 + i)
    pres = tuple(f"decoder.transformer_decoder.layers.{l}." for l in range(d.ND - 1))
    grads = {n: p.grad.detach().numpy() for n, p in ref.named_parameters() if n.startswith(pres)}
    assert len(grads) == 18 * (d.ND - 1), sorted(grads)
    for name, g in grads.items():
        assert np.isfinite(g).all() and g.any(), name
        if g.ndim == 1:
            out[P + "g_" + name] = g.astype(np.float32)
            continue
        sample(out, P, name, g, rs)
        out[P + "c_" + name] = g.astype(np.float64).sum(0)
    for key in ("dMem", "dX0"):
        g = seen[key].reshape(-1, seen[key].shape[-1])
        assert np.isfinite(g).all() and g.any(), key
        sample(out, P, key, g, rs)
    print(i, "final", float(final.detach()), "dMem", seen["dMem"].shape, "dX0", seen["dX0"].shape, len(out), "arrays")
    return out


def main():
    ggl.install()
    for part, i in enumerate(CASES):
        out = {"cases": np.array(CASES)}
        out.update(run_case(i))
        path = os.path.join(ROOT, "tests", "golden", f"decoder_grads.part{part}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
