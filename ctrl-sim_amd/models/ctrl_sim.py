"""`CtRLSim` — the model object of the plugin surface (reference: models/ctrl_sim.py:19-45).

The reference class is a LightningModule whose only rollout-relevant members are `.cfg`, `.eval()` and
`forward(data, eval) -> {'action_preds','rtg_preds','state_preds'}`; `load_from_checkpoint(path)` builds it from a
Lightning checkpoint whose `hyper_parameters` carry the cfg (eval_sim.py:52, policies/policy.py:28-29).
Here the object owns the packed device weights (`HipModel`); the HIP forward is driven by the policy/engine through
the C ABI; `forward` on reference-layout tensors is the reference's return contract ([B,A,T,.] logits of every head,
teacher-forced), or — with `token_index` — the two-pass logits of one timestep, the slice AutoregressivePolicy reads.
`compute_loss` / `validation_step` (models/ctrl_sim.py:48-189,217-228) score logged windows: ctrlsim_forward_loss, no logits tensor.
`training_step` / `configure_optimizers` / `optimizer_step` (models/ctrl_sim.py:190-214,242-282) train the three MLP heads over a frozen
trunk: ctrlsim_forward_loss_grads gives the loss and, at scope 0, the head gradients (csrc/head_grad.hip), torch's AdamW steps the fp32
masters, `HipModel.update` puts them back into the packed buffer.  `set_trainable("heads+ffn")` adds the last decoder layer's feed-forward
block (linear1, linear2, norm3): scope 1 (csrc/ffn_grad.hip) differentiates it too and returns `dU`, the gradient at that block's input;
`set_trainable("heads+ffn+cross")` adds that layer's cross-attention sublayer (multihead_attn, norm2): scope 2 (csrc/attn_grad.hip)
starts from `dU` and returns `dX1` and `dMem`, the gradients at the layer's norm1 output and at the scene encoder's output;
`set_trainable("heads+last_layer")` adds its self-attention sublayer (self_attn, norm1), so that the whole last decoder layer trains:
scope 3 (csrc/self_attn_grad.hip) starts from `dX1` and returns `dX0`, the gradient at the layer's input rows.
`set_trainable("heads+decoder")` (CtRLSim.DECODER_SCOPE) trains every decoder layer: scope 4 does what scope 3
does and then, for each earlier layer from the last but one down, recomputes the layer's inside from the rows that entered it and runs the
three backward ops (csrc/decoder_layer_grad.hip); it returns `dX0` of every layer and `dMem` summed over all of them, the gradients the
encoder's and the embeddings' backward start from.
`set_trainable("heads+decoder+encoder")` (CtRLSim.ENCODER_SCOPE) also trains every scene-encoder layer: scope 5
does what scope 4 does and then, from `dMem` back, recomputes each encoder layer's inside from the scene rows that entered it and
runs the two backward ops (csrc/encoder_layer_grad.hip); it returns `dE0` of every encoder layer — `dE0[0]` is the gradient at the rows
[polylines || initial states], where the map encoder's and the embeddings' backward — not built — would start."""
from __future__ import annotations

import numpy as np

from ..spec import Dims, check_supported
from .. import weights as _weights


class CtRLSim:
    def __init__(self, cfg, weights=None, seed=0, device="cuda:0"):
        self.cfg = cfg
        check_supported(cfg)                    # e.g. a checkpoint trained with use_map=False: another network
        self.dims = Dims(cfg)
        self.weights = weights if weights is not None else _weights.generate(self.dims, seed)
        self.device = device
        self._hip = None
        self.training = False
        self._scope = "heads"

    @classmethod
    def load_from_checkpoint(cls, path, cfg=None, device="cuda:0"):
        """Lightning checkpoint: {'state_dict': {...}, 'hyper_parameters': {'cfg': ...}} (models/ctrl_sim.py:23-25)."""
        import torch
        ck = torch.load(path, map_location="cpu", weights_only=False)
        if cfg is None:
            cfg = ck["hyper_parameters"]["cfg"]
        check_supported(cfg)
        d = Dims(cfg)
        return cls(cfg, _weights.from_state_dict(d, ck["state_dict"]), device=device)

    def eval(self):
        self.training = False
        return self

    def state_dict(self):
        return dict(self.weights)

    @property
    def hip(self):
        if self._hip is None:
            from ..engine import HipModel
            self._hip = HipModel(self.cfg, self.weights, self.device)
        return self._hip

    def __call__(self, data, eval=False, token_index=None):
        return self.forward(data, eval, token_index)

    def _arrays(self, data):
        ag, mp = data["agent"], data["map"]
        g = lambda o, k: (o[k] if isinstance(o, dict) else getattr(o, k))
        host = lambda v: np.asarray(v.cpu() if hasattr(v, "cpu") else v)
        arrs = {k: host(g(ag, k)) for k in ("agent_states", "agent_types", "goals", "actions", "rtgs", "timesteps")}
        arrs["road_points"], arrs["road_types"] = host(g(mp, "road_points")), host(g(mp, "road_types"))
        return arrs

    def forward(self, data, eval=False, token_index=None):
        """data: reference MotionData-like mapping (data['agent'].agent_states ...).
        token_index None (the reference's contract, models/ctrl_sim.py:41-45 + decoder.py:52-77): one teacher-forced forward,
        {'action_preds': [B,A,T,V], 'rtg_preds': [B,A,T,R*C], 'state_preds': [B,A,T,2T]} (the keys the model's heads provide).
        token_index given: the logits of that window step for every slot, {'rtg_preds': [B,A,R*C], 'action_preds': [B,A,V]},
        from the two-pass HIP forward with the rtg bins already present in data (what the reference's second call computes)."""
        import ctypes as C
        import torch
        from .. import _lib
        from ..engine import ctx_from_reference_layout
        d = self.dims
        arrs = self._arrays(data)
        B = arrs["agent_states"].shape[0]
        dev = self.device
        lib, st = _lib.lib(), _lib.stream_ptr()
        if token_index is None:
            cb = ctx_from_reference_layout(d, arrs, d.T, dev)
            cb.slot_gid.copy_(torch.arange(d.A, dtype=torch.int32, device=dev).expand(B, d.A))
            ws = torch.empty(self.hip.workspace_bytes(B, d.T), dtype=torch.uint8, device=dev)
            act = torch.empty(B, d.T, d.A, d.V, device=dev)
            rtg = torch.empty(B, d.T, d.A, d.R * d.C, device=dev) if d.VARIANT == 0 else None
            fut = torch.empty(B, d.T, d.A, d.FUT, device=dev) if "decoder.predict_future_states.mlp.0.weight" in self.weights else None
            _lib.check(lib.ctrlsim_forward_all(self.hip.handle, B, d.T, C.byref(cb.struct), ws.data_ptr(), act.data_ptr(),
                                               rtg.data_ptr() if rtg is not None else None,
                                               fut.data_ptr() if fut is not None else None, st), "forward_all")
            torch.cuda.synchronize()
            out = {"action_preds": act.permute(0, 2, 1, 3)}
            if fut is not None:
                out["state_preds"] = fut.permute(0, 2, 1, 3)
            if rtg is not None:
                out["rtg_preds"] = rtg.permute(0, 2, 1, 3)
            return out
        ti = token_index if token_index >= 0 else d.T + token_index
        Tq = ti + 1
        cb = ctx_from_reference_layout(d, arrs, Tq, dev)
        cb.slot_gid.copy_(torch.arange(d.A, dtype=torch.int32, device=dev).expand(B, d.A))
        ws = torch.empty(self.hip.workspace_bytes(B, Tq), dtype=torch.uint8, device=dev)
        rtg = torch.empty(B, d.A, d.R * d.C, device=dev)
        act = torch.empty(B, d.A, d.V, device=dev)
        hist = torch.zeros(B, d.A, 1, 3, dtype=torch.int32, device=dev)
        hist[:, :, 0] = torch.from_numpy(arrs["rtgs"][:, :, ti].astype(np.int32)).to(dev)
        scn = torch.arange(B, dtype=torch.int32, device=dev)
        _lib.check(lib.ctrlsim_dt_forward_pass1(self.hip.handle, B, Tq, C.byref(cb.struct), ws.data_ptr(), rtg.data_ptr(), None, st))
        _lib.check(lib.ctrlsim_dt_forward_pass2(self.hip.handle, B, Tq, 0, d.A, 1, C.byref(cb.struct), scn.data_ptr(),
                                                hist.data_ptr(), ws.data_ptr(), act.data_ptr(), 0, st))
        torch.cuda.synchronize()
        return {"rtg_preds": rtg, "action_preds": act}

    # ---- open-loop evaluation (reference: models/ctrl_sim.py:48-189, 217-228)
    LOSS_KEYS = ("loss_actions", "loss_rtg_goal", "loss_rtg_veh", "loss_rtg_road", "loss_state")
    VAL_NAMES = {"loss_actions": "val_loss", "loss_rtg_goal": "val_rtg_goal_loss", "loss_rtg_veh": "val_rtg_veh_loss",
                 "loss_rtg_road": "val_rtg_road_loss", "loss_state": "val_state_loss"}

    def loss_keys(self):
        """The terms this model's heads provide, in the order of the packed sums."""
        m = self.cfg.model
        keys = ["loss_actions"]
        if self.dims.VARIANT == 0 and bool(m.get("predict_rtg", True)):
            keys += ["loss_rtg_goal", "loss_rtg_veh", "loss_rtg_road"]
        if bool(m.get("predict_future_states", True)) and "decoder.predict_future_states.mlp.0.weight" in self.weights:
            keys.append("loss_state")
        return keys

    def loss_cfg(self, fused=True):
        from .. import _lib
        m = self.cfg.model
        return _lib.LossCfg(int(bool(m.get("supervise_moving", True))), int(bool(m.get("local_frame_predictions", False))), int(bool(fused)), 0)

    def losses_from_sums(self, sums):
        """[5,2] (sum, count) per term -> the reference's loss dictionary: sum / count, the actions times loss_action_coef, the state
        term over 100 * 2 * count (models/ctrl_sim.py:84,146).  A term whose count is 0 is NaN, as 0 / 0 is in the reference."""
        sums = np.asarray(sums, np.float64).reshape(5, 2)
        coef = float(self.cfg.model.get("loss_action_coef", 1.0))
        out = {}
        with np.errstate(invalid="ignore", divide="ignore"):
            for k in self.loss_keys():
                i = self.LOSS_KEYS.index(k)
                s, n = sums[i]
                out[k] = float(np.float64(coef * s if i == 0 else s) / np.float64(200.0 * n if i == 4 else n))
        return out

    def loss_sums(self, data, preds=None, fused=True, per_ctx=False, row_nll=False):
        """One teacher-forced forward over the reference-layout windows `data` -> device tensors (sums [5,2] float64, per_ctx [B,5,2] or
        None, row_nll [B,T,A,4] or None).  preds (the dictionary `forward` returns): the reduction over those logits instead."""
        import ctypes as C
        import torch
        from .. import _lib
        d, dev = self.dims, self.device
        lib, st = _lib.lib(), _lib.stream_ptr()
        cb, moving, B = self._ctx_of(data)
        if preds is None:
            return self.loss_sums_ctx(cb, moving, B, fused=fused, per_ctx=per_ctx, row_nll=row_nll)
        sums = torch.zeros(5, 2, dtype=torch.float64, device=dev)
        pc = torch.zeros(B, 5, 2, dtype=torch.float64, device=dev) if per_ctx else None
        rn = torch.zeros(B, d.T, d.A, 4, device=dev) if row_nll else None
        cfg = self.loss_cfg(fused)
        rows = lambda k: (preds[k].to(dev).float().permute(0, 2, 1, 3).contiguous() if preds.get(k) is not None else None)
        act, rtg, fut = rows("action_preds"), rows("rtg_preds"), rows("state_preds")
        scratch = torch.empty(int(lib.ctrlsim_loss_scratch_bytes(B, d.T, d.A)), dtype=torch.uint8, device=dev)
        _lib.check(lib.ctrlsim_loss_from_preds(C.byref(self.hip.cdims), B, d.T, C.byref(cb.struct), _lib.ptr(moving), C.byref(cfg),
                                               _lib.ptr(act), _lib.ptr(rtg), _lib.ptr(fut), scratch.data_ptr(), sums.data_ptr(),
                                               _lib.ptr(pc), _lib.ptr(rn), st), "loss_from_preds")
        return sums, pc, rn                 # enqueued on the current stream; reading the tensors waits for it

    def loss_sums_ctx(self, cb, moving, B, fused=True, per_ctx=False, row_nll=False):
        """loss_sums below the upload: one teacher-forced forward + loss over the first B contexts of `cb` (engine.CtxBuffers already on
        the device: ctx_from_reference_layout, or windows.build_windows) with moving [B,A] uint8 or None -> (sums, per_ctx, row_nll)."""
        import ctypes as C
        import torch
        from .. import _lib
        d, dev = self.dims, self.device
        lib, st = _lib.lib(), _lib.stream_ptr()
        sums = torch.zeros(5, 2, dtype=torch.float64, device=dev)
        pc = torch.zeros(B, 5, 2, dtype=torch.float64, device=dev) if per_ctx else None
        rn = torch.zeros(B, d.T, d.A, 4, device=dev) if row_nll else None
        cfg = self.loss_cfg(fused)
        n = lib.ctrlsim_forward_loss_workspace_bytes(C.byref(self.hip.cdims), B, d.T)
        if n < 0:
            raise RuntimeError(f"loss workspace query failed: {n}")
        ws = torch.empty(int(n), dtype=torch.uint8, device=dev)
        _lib.check(lib.ctrlsim_forward_loss(self.hip.handle, B, d.T, C.byref(cb.struct), _lib.ptr(moving), C.byref(cfg), ws.data_ptr(),
                                            sums.data_ptr(), _lib.ptr(pc), _lib.ptr(rn), st), "forward_loss")
        return sums, pc, rn                 # enqueued on the current stream; reading the tensors waits for it

    def compute_loss(self, data, preds=None):
        """The reference's loss dictionary (models/ctrl_sim.py:48-189) of the windows in `data`.  preds None: the fused forward + loss
        (no logits); preds = model(data): the reduction over those tensors, the reference's call shape."""
        sums, _, _ = self.loss_sums(data, preds)
        return self.losses_from_sums(sums.cpu().numpy())

    def validation_step(self, data, batch_idx=0):
        """The values the reference logs per validation batch (models/ctrl_sim.py:217-228), under its names."""
        return {self.VAL_NAMES[k]: v for k, v in self.compute_loss(data).items()}

    # ---- training, first stage: the heads over a frozen trunk (reference: models/ctrl_sim.py:190-214, 242-282)
    TRAIN_NAMES = {"loss_actions": "loss", "loss_rtg_goal": "loss_rtg_goal", "loss_rtg_veh": "loss_rtg_veh",
                   "loss_rtg_road": "loss_rtg_road", "loss_state": "loss_state"}

    def head_grad_layout(self):
        """[(state-dict name, offset in floats, shape)] of the flat gradient buffer, and its length (ctrlsim_train_grad_layout, scope 0)."""
        return self.train_grad_layout("heads")

    def _parameters(self, scope):
        """state-dict name -> torch.nn.Parameter over the fp32 master values of a scope's tensors, in layout order (each created once, in
        one name-keyed cache; the optimiser's state hangs on these objects)."""
        import torch
        cache = self.__dict__.setdefault("_params", {})
        make = lambda k: torch.nn.Parameter(torch.from_numpy(np.array(self.weights[k], np.float32)).to(self.device))
        return {k: cache[k] if k in cache else cache.setdefault(k, make(k)) for k, _, _ in self.train_grad_layout(scope)[0]}

    def head_parameters(self):
        """state-dict name -> torch.nn.Parameter over the fp32 master values of the heads this model has (created once; the
        optimiser's state hangs on these objects)."""
        return self._parameters("heads")

    def head_grad_workspace_bytes(self, B):
        return self.train_grad_workspace_bytes(B, "heads")

    # the optional outputs of ctrlsim_forward_loss_grads (ctrlsim_train_taps) in the order the result tuples list them: name -> (first
    # scope, last scope, rows: B*T*A*3 token rows or B*M scene rows, the Dims count of a per-layer tap: a list from scope 4 on, at
    # scope 3 the last layer's tensor alone)
    _TAPS = {"dX": (0, 5, "rows3", None), "dU": (1, 3, "rows3", None), "x_out": (0, 5, "rows3", None), "u_out": (1, 3, "rows3", None),
             "dX1": (2, 3, "rows3", None), "dMem": (2, 5, "rowsm", None), "x1_out": (2, 3, "rows3", None), "mem_out": (2, 5, "rowsm", None),
             "dX0": (3, 5, "rows3", "ND"), "x0_out": (3, 5, "rows3", "ND"), "dE0": (5, 5, "rowsm", "NE"), "e0_out": (5, 5, "rowsm", "NE")}

    def _forward_loss_grads(self, cb, moving, B, scope, want=(), fused=True, workspace=None, X=None):
        """The one call behind every loss_and_*_grads: forward + loss + the gradients of `scope` with the taps named in `want` ->
        (sums, {state-dict name: gradient tensor} — views of one flat buffer in train_grad_layout(scope) order —, {tap name: tensor}).
        X given (scope "heads" only): no forward, ctrlsim_heads_loss_grad on those decoder output rows."""
        import ctypes as C
        import torch
        from .. import _lib
        d, dev = self.dims, self.device
        lib, st = _lib.lib(), _lib.stream_ptr()
        layout, total = self.train_grad_layout(scope)
        sums = torch.zeros(5, 2, dtype=torch.float64, device=dev)
        grads = torch.empty(total, device=dev)
        sc = self._scope_index(scope)
        rows = {"rows3": B * d.T * d.A * 3, "rowsm": B * ((d.P + d.A + 3) & ~3)}
        ct, taps = _lib.TrainTaps(), {}
        for k in (k for k in self._TAPS if k in want):
            _, _, r, per = self._TAPS[k]
            if per is None:
                taps[k] = torch.empty(rows[r], d.D, device=dev)
                setattr(ct, k, taps[k].data_ptr())
                continue
            n = getattr(d, per)
            layers = range(n) if sc >= 4 else (n - 1,)
            ts = [torch.empty(rows[r], d.D, device=dev) for _ in layers]
            for l, t in zip(layers, ts):
                getattr(ct, k)[l] = t.data_ptr()
            taps[k] = ts if sc >= 4 else ts[0]
        cfg = self.loss_cfg(fused)
        coef = float(self.cfg.model.get("loss_action_coef", 1.0))
        n = self.train_grad_workspace_bytes(B, scope)
        ws = workspace if workspace is not None else torch.empty(n, dtype=torch.uint8, device=dev)
        assert ws.dtype == torch.uint8 and ws.numel() >= n
        head = (self.hip.handle, B, d.T, C.byref(cb.struct), _lib.ptr(moving), C.byref(cfg), coef)
        if X is None:
            _lib.check(lib.ctrlsim_forward_loss_grads(*head, sc, ws.data_ptr(), sums.data_ptr(), None, grads.data_ptr(), C.byref(ct), st),
                       "forward_loss_grads")
        else:
            assert sc == 0 and X.dtype == torch.float32 and tuple(X.shape) == (rows["rows3"], d.D)
            _lib.check(lib.ctrlsim_heads_loss_grad(*head, _lib.ptr(X), ws.data_ptr(), sums.data_ptr(), None, grads.data_ptr(),
                                                   _lib.ptr(taps.get("dX")), st), "heads_loss_grad")
        named = {k: grads[o:o + int(np.prod(shp))].view(shp) for k, o, shp in layout}
        return sums, named, taps            # enqueued on the current stream; reading the tensors waits for it

    def loss_and_head_grads_ctx(self, cb, moving, B, fused=True, dX=False, x_out=False, X=None, workspace=None):
        """One teacher-forced forward + loss + head gradients over the first B contexts of `cb` (engine.CtxBuffers on the device:
        ctx_from_reference_layout, or windows.build_windows) with moving [B,A] uint8 or None -> (sums [5,2] float64 on the device,
        {state-dict name: gradient tensor} — views of one flat buffer —, dX [B*T*A*3,256] or None, x_out likewise).  X given (decoder
        output rows, plain layout): no forward, loss and gradients from those rows (ctrlsim_heads_loss_grad).  workspace: a uint8
        device tensor of at least head_grad_workspace_bytes(B) to use instead of a fresh one."""
        want = [k for k, on in (("dX", dX), ("x_out", x_out and X is None)) if on]
        sums, named, taps = self._forward_loss_grads(cb, moving, B, "heads", want, fused, workspace, X)
        return sums, named, taps.get("dX"), taps.get("x_out")

    def _ctx_of(self, data):
        import torch
        from ..engine import ctx_from_reference_layout
        d, dev = self.dims, self.device
        arrs = self._arrays(data)
        B = arrs["agent_states"].shape[0]
        ag = data["agent"]
        mv = ag.get("moving_agent_mask") if isinstance(ag, dict) else getattr(ag, "moving_agent_mask", None)
        moving = None
        if mv is not None:
            mv = np.asarray(mv.cpu() if hasattr(mv, "cpu") else mv)
            moving = torch.from_numpy(np.ascontiguousarray(mv != 0).astype(np.uint8)).to(dev)
        cb = ctx_from_reference_layout(d, arrs, d.T, dev)
        cb.slot_gid.copy_(torch.arange(d.A, dtype=torch.int32, device=dev).expand(B, d.A))
        return cb, moving, B

    def loss_and_head_grads(self, data, fused=True, dX=False, x_out=False):
        """loss_and_head_grads_ctx over reference-layout windows `data`."""
        cb, moving, B = self._ctx_of(data)
        return self.loss_and_head_grads_ctx(cb, moving, B, fused=fused, dX=dX, x_out=x_out)

    def final_loss(self, losses):
        """models/ctrl_sim.py:207-214 over the terms this model has (loss_actions already carries loss_action_coef)."""
        return float(sum(np.float64(losses[k]) for k in self.loss_keys()))

    # ---- training, second stage (a): the heads and the last decoder layer's feed-forward block
    SCOPES = ("heads", "heads+ffn", "heads+ffn+cross", "heads+last_layer")
    # training (d): the heads and EVERY decoder layer (scope 4); accepted wherever a scope name is taken
    DECODER_SCOPE = "heads+decoder"
    # training (e): and EVERY scene-encoder layer (scope 5); accepted wherever a scope name is taken
    ENCODER_SCOPE = "heads+decoder+encoder"
    # scope name -> the scope index of ctrlsim_train_grad_layout, ctrlsim_train_grads_workspace_bytes and ctrlsim_forward_loss_grads
    _SCOPE_INDEX = {s: i for i, s in enumerate(SCOPES + (DECODER_SCOPE, ENCODER_SCOPE))}

    def _scope_index(self, scope):
        if scope not in self._SCOPE_INDEX:
            raise ValueError(f"trainable scope {scope!r}: one of {tuple(self._SCOPE_INDEX)}")
        return self._SCOPE_INDEX[scope]

    def set_trainable(self, scope="heads"):
        """What training_step / configure_optimizers / optimizer_step train: "heads" (the default: the three MLP heads), "heads+ffn"
        (the heads and linear1, linear2, norm3 of the last decoder layer), "heads+ffn+cross" (and that layer's cross-attention:
        multihead_attn.in_proj / out_proj and norm2) or "heads+last_layer" (and its self-attention: self_attn.in_proj / out_proj and
        norm1 — the whole last decoder layer) or "heads+decoder" (and the 18 tensors of every earlier decoder layer) or
        "heads+decoder+encoder" (and the 12 tensors of every scene-encoder layer).  Choose before configure_optimizers."""
        self._scope_index(scope)
        self._scope = scope
        return self

    def train_grad_layout(self, scope=None):
        """head_grad_layout for a scope (ctrlsim_train_grad_layout): "heads" gives exactly head_grad_layout's answer, "heads+ffn" appends
        the six tensors of the last decoder layer's feed-forward block, "heads+ffn+cross" the six of its cross-attention sublayer behind
        them, "heads+last_layer" the six of its self-attention sublayer behind those; "heads+decoder"
        behind those, for the layers ND-2 down to 0, each layer's 18 tensors in the same group order; "heads+decoder+encoder"
        behind those, for the encoder layers NE-1 down to 0, each layer's 12 tensors (the feed-forward
        six, then the attention six).  Needs no device."""
        import ctypes as C
        from .. import _lib
        from ..engine import _dims_struct
        lib = _lib.lib()
        scope = self._scope if scope is None else scope
        has_fut = int("decoder.predict_future_states.mlp.0.weight" in self.weights)
        cd = _dims_struct(self.dims)
        sc = self._scope_index(scope)
        query = lambda cap, names, offs: lib.ctrlsim_train_grad_layout(C.byref(cd), has_fut, sc, cap, names, offs)
        n = query(0, None, None)
        names, offs = (C.c_char_p * max(n, 1))(), (C.c_int64 * (max(n, 0) + 1))()
        if n < 0 or query(n + 1, names, offs) != n:
            raise RuntimeError("training gradient layout query failed")
        out = [(names[i].decode(), int(offs[i]), tuple(np.asarray(self.weights[names[i].decode()]).shape)) for i in range(n)]
        return out, int(offs[n])

    def trainable_parameters(self):
        """state-dict name -> torch.nn.Parameter of the selected scope, in layout order: head_parameters() (the same objects), then under
        "heads+ffn" the six tensors of the last decoder layer's feed-forward block, under "heads+ffn+cross" the six of its cross-attention
        sublayer too, under "heads+last_layer" the six of its self-attention sublayer as well, under "heads+decoder" the 18 tensors of
        every earlier decoder layer too, under "heads+decoder+encoder" the 12 tensors of every scene-encoder layer as well (each created
        once)."""
        return self._parameters(self._scope)

    def train_grad_workspace_bytes(self, B, scope="heads+ffn"):
        import ctypes as C
        from .. import _lib
        n = _lib.lib().ctrlsim_train_grads_workspace_bytes(C.byref(self.hip.cdims), B, self.dims.T, self._scope_index(scope))
        if n < 0:
            raise RuntimeError(f"training gradient workspace query failed: {n}")
        return int(n)

    def loss_and_train_grads_ctx(self, cb, moving, B, dX=False, dU=False, x_out=False, u_out=False, workspace=None, dX1=False, dMem=False,
                                 x1_out=False, mem_out=False, scope=None, dX0=False, x0_out=False, dE0=False, e0_out=False):
        """loss_and_head_grads_ctx for the scope "heads+ffn" (ctrlsim_forward_loss_grads, scope 1): one teacher-forced forward + loss + the
        gradients of the heads and of the last decoder layer's feed-forward block -> (sums, {state-dict name: gradient tensor} in
        train_grad_layout("heads+ffn") order, dX, dU, x_out, u_out), each of the last four [B*T*A*3, 256] or None: the gradient at the
        decoder output, the gradient at the block's input U, the decoder output and U itself.  The gradients are those of the function
        this call evaluated (the block applied to U as stored).
        scope (default: the trainable scope, "heads+ffn" under "heads"): under "heads+ffn+cross" (scope 2) the
        gradients continue with the six cross-attention tensors and the tuple with (dX1, dMem, x1_out, mem_out): the gradient at the
        layer's norm1 output [B*T*A*3, 256], this layer's share of the gradient at the scene encoder's output [B*M, 256], M = (P + A + 3)
        & ~3, and the two inputs themselves; everything the narrower scope returns is bit for bit what it returns.  Under
        "heads+last_layer" (scope 3) the gradients continue with the six self-attention tensors and the tuple
        with (dX0, x0_out): the gradient at the layer's input rows [B*T*A*3, 256] and those rows themselves.
        Under "heads+decoder" (scope 4) the gradients continue with the 18 tensors of each earlier layer and
        the tuple is (sums, gradients, dX, x_out, dMem, mem_out, dX0, x0_out): dMem summed over all ND layers; dX0 and x0_out LISTS of ND
        tensors, entry l the gradient at the rows that enter layer l and those rows (dX0[0]: the gradient at the assembled tokens).  The
        intermediate taps of the last layer (dU, u_out, dX1, x1_out) do not exist in that scope.
        Under "heads+decoder+encoder" (scope 5) the gradients continue with the 12 tensors of each encoder layer
        and the tuple is the decoder scope's followed by (dE0, e0_out): LISTS of NE tensors [B*M, 256], entry l the gradient at the scene
        rows that enter encoder layer l and those rows (dE0[0]: the gradient at [polylines || initial states]); they exist in that
        scope only."""
        if scope is None:
            scope = self._scope if self._scope != "heads" else "heads+ffn"
        if (dE0 or e0_out) and scope != self.ENCODER_SCOPE:
            raise ValueError("dE0 and e0_out exist under the scope \"heads+decoder+encoder\" only")
        if scope in (self.DECODER_SCOPE, self.ENCODER_SCOPE):
            if dU or u_out or dX1 or x1_out:
                raise ValueError(f"dU, u_out, dX1 and x1_out do not exist under the scope \"{scope}\"")
        elif scope not in self.SCOPES[1:]:
            raise ValueError(f"loss_and_train_grads scope {scope!r}: one of {self.SCOPES[1:]}")
        sc = self._scope_index(scope)
        if sc < 2 and (dX1 or dMem or x1_out or mem_out):
            raise ValueError("dX1, dMem, x1_out and mem_out exist from the scope \"heads+ffn+cross\" on only")
        if sc < 3 and (dX0 or x0_out):
            raise ValueError("dX0 and x0_out exist under the scope \"heads+last_layer\" only")
        asked = dict(dX=dX, dU=dU, x_out=x_out, u_out=u_out, dX1=dX1, dMem=dMem, x1_out=x1_out, mem_out=mem_out, dX0=dX0, x0_out=x0_out,
                     dE0=dE0, e0_out=e0_out)
        order = [k for k, (first, last, _, _) in self._TAPS.items() if first <= sc <= last]
        sums, named, taps = self._forward_loss_grads(cb, moving, B, scope, [k for k in order if asked[k]], workspace=workspace)
        return (sums, named) + tuple(taps.get(k) for k in order)

    def loss_and_train_grads(self, data, dX=False, dU=False, x_out=False, u_out=False, **more):
        """loss_and_train_grads_ctx over reference-layout windows `data` (more: dX1, dMem, x1_out, mem_out, dX0, x0_out, scope)."""
        cb, moving, B = self._ctx_of(data)
        return self.loss_and_train_grads_ctx(cb, moving, B, dX=dX, dU=dU, x_out=x_out, u_out=u_out, **more)

    def _train_backward(self, sums, grads):
        for k, p in self.trainable_parameters().items():
            p.grad = grads[k].clone()
        losses = self.losses_from_sums(sums.cpu().numpy())
        self.logged = {self.TRAIN_NAMES[k]: v for k, v in losses.items()}
        return self.final_loss(losses)

    def training_step(self, data, batch_idx=0):
        """The reference's training_step for the heads: final_loss of the batch; `.grad` of head_parameters() is filled with its gradient
        (the trunk is frozen: it has no parameters here), `self.logged` holds what the reference logs per step, under its names."""
        return self.training_step_ctx(*self._ctx_of(data))

    def training_step_ctx(self, cb, moving, B):
        """training_step on contexts that are already on the device (windows.build_windows)."""
        sums, grads, _ = self._forward_loss_grads(cb, moving, B, self._scope)
        return self._train_backward(sums, grads)

    @staticmethod
    def param_groups(names):
        """The reference's AdamW groups (models/ctrl_sim.py:242-268) restricted to `names`: the weight of a Linear decays; every bias
        and every LayerNorm weight (mlp.1 of an MLPLayer, utils/layers.py:6-19; norm1 / norm2 / norm3 of a transformer layer: the
        reference groups by module type) do not; an attention's in_proj_weight is a weight of a whitelisted module there and decays.
        Both lists sorted, as there."""
        import re
        ln = re.compile(r"\.(mlp\.1|norm\d*)\.weight$")
        decay = sorted(k for k in names if k.endswith((".weight", ".in_proj_weight")) and not ln.search(k))
        no_decay = sorted(k for k in names if k not in set(decay))
        return decay, no_decay

    @staticmethod
    def lr_lambda(train_cfg):
        """utils/train_utils.py:5-12 (create_lambda_lr): linear warm-up over warmup_steps, then linear decay to 0 at max_steps."""
        warm, total = train_cfg["warmup_steps"], train_cfg["max_steps"]
        return lambda step: step / warm if step < warm else max(0.0, (total - step) / (total - warm))

    def configure_optimizers(self):
        """(optimizer, scheduler): torch.optim.AdamW over trainable_parameters() in the reference's two groups with cfg.train.lr /
        weight_decay, LambdaLR with the reference's warm-up / decay, stepped once per optimiser step."""
        import torch
        tr = self.cfg.train
        params = self.trainable_parameters()
        decay, no_decay = self.param_groups(list(params))
        groups = [{"params": [params[k] for k in decay], "weight_decay": tr["weight_decay"]},
                  {"params": [params[k] for k in no_decay], "weight_decay": 0.0}]
        opt = torch.optim.AdamW(groups, lr=tr["lr"], weight_decay=tr["weight_decay"])
        return opt, torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=self.lr_lambda(tr))

    def optimizer_step(self, optimizer, scheduler=None):
        """Clip the global 2-norm of the trainable gradients at cfg.train.gradient_clip_val (Lightning clips the norm over the whole model;
        only trainable_parameters() have gradients here, so the norm is theirs alone), step, advance the schedule, and write the new values into
        the packed device weights (HipModel.update).  -> the gradient norm before clipping."""
        import torch
        params = self.trainable_parameters()
        clip = self.cfg.train.get("gradient_clip_val", None)
        if clip:
            norm = torch.nn.utils.clip_grad_norm_(list(params.values()), float(clip))
        else:
            norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params.values()]))
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
        optimizer.zero_grad(set_to_none=True)
        new = {k: p.detach().cpu().numpy() for k, p in params.items()}
        if self._scope in (self.DECODER_SCOPE, self.ENCODER_SCOPE):
            self.hip.update(new, decoder=True, encoder=self._scope == self.ENCODER_SCOPE)
        else:
            self.hip.update(new, cross=self._scope in self.SCOPES[2:], self_attn=self._scope == "heads+last_layer")
        self.weights.update({k: v.copy() for k, v in new.items()})
        return float(norm)
