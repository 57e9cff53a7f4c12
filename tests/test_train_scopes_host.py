"""CPU test of the one scope-indexed gradient layout (ctrlsim_train_grad_layout, scopes 0..5; needs the library, not a device): on the
tiny fixture configurations of the per-scope layout tests — cases 0, 3, 7 and the two-decoder-layer configuration — every scope's layout
has the scope before it as a prefix, the tensors lie back to back with the parameter table's shapes, and the extra offsets[n] is the
total."""
import numpy as np
import pytest

from ctrlsim_amd import spec, weights
from ctrlsim_amd.models import CtRLSim
import loss_ref

NAMES = CtRLSim.SCOPES + (CtRLSim.DECODER_SCOPE, CtRLSim.ENCODER_SCOPE)


def _model(case):
    cfg = loss_ref.case_cfg(0 if case == "nd2" else case)
    if case == "nd2":
        cfg.model.num_decoder_layers = 2
    d = spec.Dims(cfg)
    return d, CtRLSim(cfg, weights.generate(d, 3) if case == "nd2" else loss_ref.case_weights(case, d), device="cpu")


@pytest.mark.parametrize("case", [0, 3, 7, "nd2"])
def test_every_scope_extends_the_one_before_back_to_back(case):
    d, model = _model(case)
    assert len(NAMES) == 6 and CtRLSim._SCOPE_INDEX == {n: i for i, n in enumerate(NAMES)}
    table = {n: tuple(s) for n, s, _, _ in weights.param_table(d)}
    layouts = [model.train_grad_layout(n) for n in NAMES]
    added = [6, 6, 6, 18 * (d.ND - 1), 12 * d.NE]                          # tensors scope s appends to scope s - 1
    for s, (lay, total) in enumerate(layouts):
        off = 0
        for name, o, shape in lay:
            assert o == off and shape == table[name], (s, name)
            off += int(np.prod(shape))
        assert total == off                                                # offsets[n]: the total
        assert len({name for name, _, _ in lay}) == len(lay)
        if s:
            prev = layouts[s - 1]
            assert lay[:len(prev[0])] == prev[0] and len(lay) == len(prev[0]) + added[s - 1] and total >= prev[1]
    assert len(layouts[0][0]) in (6, 12, 18)                               # the heads the model has
