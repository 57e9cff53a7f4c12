"""TEST INFRASTRUCTURE — writes tests/golden/encoder_grads.part*.npz from the UNMODIFIED reference: its forward with autograd, its
compute_loss, final_loss summed as its training_step does (models/ctrl_sim.py:190-214), and backward — the gradients of every scene-encoder
layer (all 12 tensors of each) and, by a forward pre-hook on its transformer encoder, the gradient at pre_encoder_embeddings, the rows
[polylines || initial states] that enter the encoder, for the cases of tests/loss_ref.py:CASES that tests/test_gpu_encoder_grads.py runs
through the model (tiny 0 and 1, full 7), in the format of tools/gen_golden_decoder_grads.py, one part per case.  Runs only where the
reference checkout exists; nothing under tests/ -m gpu, smoke() or bench.py imports it.  The fixture holds arrays only.  Inputs are
recipes (tests/loss_ref.py:case_inputs), weights are generated (ctrlsim_amd/weights.py).  The model is in eval mode (no dropout, as the
library's forward) with gradients enabled.

    python tools/gen_golden_encoder_grads.py

Per case c<i>_ and tensor <name> (state-dict name):
  g_<name>              the full gradient of every bias and LayerNorm parameter (float32, as autograd left it)
  r_<name>, s_<name>    for the four matrices of a layer: 16 sampled row indices (first, last, the rest seeded) and those rows
  n_<name>, c_<name>    its Frobenius norm and its column sums (float64 sums of the float32 gradient)
and for <name> = dE0 (the gradient at the encoder input, [B * (P + A), 256]: the reference has no filler rows): r_, s_ and n_ as for a
matrix, and z_dE0, the indices of its rows that are exactly zero (the rows of padded keys).  The tiny cases (at most 64 encoder rows) also
hold e0 and dOut, the encoder's input rows and the gradient at its output in full ([B * (P + A), 256] float32): with them a float64 twin of
the encoder stack reproduces every recorded gradient on the CPU (tests/test_encoder_grads_host.py)."""
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
from gen_golden_decoder_grads import sample  # noqa: E402

CASES = (0, 1, 7)


def run_case(i):
    cfg = loss_ref.case_cfg(i)
    d = spec.Dims(cfg)
    ref = ggl.reference_model(cfg, loss_ref.case_weights(i, d))
    data = synth_inputs.to_motion_data(loss_ref.case_inputs(i, d))
    seen = {}

    def tap(module, args, kwargs):                              # transformer_encoder(pre_encoder_embeddings, src_key_padding_mask=...)
        args[0].register_hook(lambda g: seen.__setitem__("dE0", g.detach().numpy().copy()))

    def tap_out(module, args, output):
        seen["e0"] = args[0].detach().numpy().copy()
        output.register_hook(lambda g: seen.__setitem__("dOut", g.detach().numpy().copy()))

    handle = ref.encoder.transformer_encoder.register_forward_pre_hook(tap, with_kwargs=True)
    handle_out = ref.encoder.transformer_encoder.register_forward_hook(tap_out)
    ld = ref.compute_loss(data, ref(data, eval=True))
    handle.remove()
    handle_out.remove()
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
    rs = np.random.RandomState(5000 + i)
    pres = tuple(f"encoder.transformer_encoder.layers.{l}." for l in range(d.NE))
    grads = {n: p.grad.detach().numpy() for n, p in ref.named_parameters() if n.startswith(pres)}
    assert len(grads) == 12 * d.NE, sorted(grads)
    for name, g in grads.items():
        assert np.isfinite(g).all() and g.any(), name
        if g.ndim == 1:
            out[P + "g_" + name] = g.astype(np.float32)
            continue
        sample(out, P, name, g, rs)
        out[P + "c_" + name] = g.astype(np.float64).sum(0)
    g = seen["dE0"].reshape(-1, seen["dE0"].shape[-1])
    assert g.shape[0] == np.asarray(loss_ref.case_inputs(i, d)["agent_states"]).shape[0] * (d.P + d.A)
    assert np.isfinite(g).all() and g.any()
    sample(out, P, "dE0", g, rs)
    out[P + "z_dE0"] = np.flatnonzero(~g.any(axis=1)).astype(np.int32)
    if g.shape[0] <= 64:                                        # the tiny cases: the encoder's input rows and the gradient at its output, whole
        out[P + "e0"] = seen["e0"].reshape(g.shape).astype(np.float32)
        out[P + "dOut"] = seen["dOut"].reshape(g.shape).astype(np.float32)
    print(i, "final", float(final.detach()), "dE0", seen["dE0"].shape, len(out[P + "z_dE0"]), "zero rows", len(out), "arrays")
    return out


def main():
    ggl.install()
    for part, i in enumerate(CASES):
        out = {"cases": np.array(CASES)}
        out.update(run_case(i))
        path = os.path.join(ROOT, "tests", "golden", f"encoder_grads.part{part}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
