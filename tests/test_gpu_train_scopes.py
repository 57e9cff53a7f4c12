"""GPU test of the tap rules of the one scope-indexed training entry (ctrlsim_forward_loss_grads, scopes 0..5; include/ctrlsim.h:
ctrlsim_train_taps): a tap outside its scope range, or of a layer the scope does not differentiate, is refused with CTRLSIM_EINVAL before
anything is launched.  The two-decoder-layer tiny configuration, B = 2, through ctypes."""
import ctypes as C

import numpy as np
import pytest
import torch

from ctrlsim_amd import spec, weights, _lib
from ctrlsim_amd.models import CtRLSim
import loss_ref
from gpu_utils import DEV
from test_gpu_self_attn_grads import _data, _bits

pytestmark = pytest.mark.gpu


def test_taps_outside_their_scope_or_layers_are_refused_and_nothing_is_launched():
    cfg = loss_ref.case_cfg(0)
    cfg.model.num_decoder_layers = 2
    d = spec.Dims(cfg)
    assert d.ND == 2 and 1 <= d.NE < 8
    model = CtRLSim(cfg, weights.generate(d, 5), device=DEV)
    cb, moving, B = model._ctx_of(_data(loss_ref.make_inputs(d, 31, 2)))
    assert B == 2
    lib, st = _lib.lib(), _lib.stream_ptr()
    lc = model.loss_cfg()
    ws = torch.empty(model.train_grad_workspace_bytes(B, CtRLSim.ENCODER_SCOPE), dtype=torch.uint8, device=DEV)
    sums = torch.full((5, 2), 3.0, dtype=torch.float64, device=DEV)
    grads = torch.full((model.train_grad_layout(CtRLSim.ENCODER_SCOPE)[1],), 7.0, device=DEV)
    buf = torch.full((B * d.T * d.A * 3, 256), 7.0, device=DEV)          # (the scene-row taps are smaller: any tap fits)
    sums0, grads0, buf0 = _bits(sums).copy(), _bits(grads).copy(), _bits(buf).copy()

    def refused(scope, name, layer=None):
        t = _lib.TrainTaps()
        if layer is None:
            setattr(t, name, buf.data_ptr())
        else:
            getattr(t, name)[layer] = buf.data_ptr()
        rc = lib.ctrlsim_forward_loss_grads(model.hip.handle, B, d.T, C.byref(cb.struct), _lib.ptr(moving), C.byref(lc), 1.0, scope, ws.data_ptr(),
                                            sums.data_ptr(), None, grads.data_ptr(), C.byref(t), st)
        torch.cuda.synchronize()
        same = np.array_equal(_bits(sums), sums0) and np.array_equal(_bits(grads), grads0) and np.array_equal(_bits(buf), buf0)
        return rc == -22 and same

    assert refused(4, "dU")                            # the last layer's intermediate taps end at scope 3
    assert refused(5, "x1_out")
    assert refused(3, "dX0", 0)                        # scope 3 differentiates layer ND-1 = 1 alone
    assert refused(4, "dX0", d.ND)                     # a decoder layer the model does not have
    assert refused(5, "dE0", d.NE)                     # an encoder layer the model does not have
    assert refused(4, "dE0", 0)                        # the encoder taps exist at scope 5 only
    assert refused(1, "dMem")                          # dMem starts at scope 2
