"""What the hidden-row tests share (tests/test_hidden_cases_host.py, tests/test_gpu_hidden_rows.py): input recipes that hold the edges the
front end and the trunk can get wrong, a staged oracle that returns every hidden tensor a training entry can tap, one function per stage
that takes the stage's INPUT ROWS (so that a device tensor can be fed in), and the wrong-on-purpose twins of the staged oracle.

ROW ORDER (csrc/forward.hip: Shape, scene_side; csrc/embed.hip: assemble_tokens_kernel; include/ctrlsim.h), stated once:
  token row of context b     b L + ((t A + a) 3 + k),  L = 3 T A,  k = 0 state, 1 return, 2 action — model_oracle.embed_tokens' order;
  scene row of context b     b M + p for polyline p < P,  b M + P + a for the initial state of slot a,  M = (P + A + 3) & ~3; the rows
                             P + A .. M - 1 are filler: zero source rows, key-padded (the oracle has no such rows).
The taps x0_out[l], x1_out, u_out, x_out hold [B L, 256] in the first order, mem_out [B M, 256] in the second; dbg_seg_emb of
ctrlsim_dt_forward_pass1 holds [B P, 256], polyline after polyline.

RECIPES.  recipe(kind): synth_inputs.random_context with every slot and polyline live, then deterministic edits (the table in _edit);
edges(inp) finds the edges again from the arrays alone, and tests/test_hidden_cases_host.py asserts each of them.

STAGED ORACLE.  staged(tw, x, d, dtype): model_oracle's own functions (embed_tokens, map_encoder, _enc_layer, _mha, _ln, _linear,
causal_mask_closed_form), the decoder layer written out so that the last layer's norm1 and norm2 outputs can be returned; in float32 bit
for bit model_oracle.forward(return_hidden=True).  float64: forward_cases.widened.

STAGE FUNCTIONS.  stage_tokens, stage_seg, stage_mem take what the stage reads; stage_layer is layer_grad_ref.layer (the composition of
self_attn_grad_ref.block, attn_grad_ref.block and ffn_grad_ref.block: written from the definitions, no code shared with model_oracle)
on (x0, mem, pad) and returns (Y, X1, U): the rows that leave the layer and its norm1 and norm2 outputs.  oracle_layer is the same stage
in model_oracle's functions, the one staged() chains."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from helpers import TINY, LOOP
from ctrlsim_amd import spec, weights
import forward_cases as fc
import layer_grad_ref as lgr
import model_oracle as mo
import self_attn_grad_ref as sgr
import synth_inputs

# preset -> (size overrides, contexts, input seed).  tiny: 144 token rows and 36 scene rows (below one tile, no multiple of 128);
# full: ONE context, 2304 token rows, M = 224, NP = 100 — where the multi-tile paths of the map pooling and of the attention run
PRESETS = {"tiny": (TINY, 3, 51), "loop": (LOOP, 2, 52), "full": ({}, 1, 53)}
WEIGHTS = ("init", "trained")          # weights.generate(d, 0), weights.generate_trained_like(d, 1)
KINDS = ("tokens", "seg", "mem", "layer", "x1", "u", "x_out")
ROAD_TYPES = (1, 2, 3, 4, 5, 6)        # the one-hot columns synth_inputs.random_context uses


@functools.lru_cache(maxsize=None)
def cfg_dims(kind, own=False):
    """(cfg, dims) of a preset; own: the attend_own_return_action model (mask mode 1 of the causal attention)."""
    over = dict(PRESETS[kind][0])
    if own:
        over["model__attend_own_return_action"] = True
    cfg = spec.make_cfg(**over)
    return cfg, spec.Dims(cfg)


@functools.lru_cache(maxsize=None)
def make_weights(kind, wkind, own=False):
    d = cfg_dims(kind, own)[1]
    return weights.generate(d, 0) if wkind == "init" else weights.generate_trained_like(d, 1)


def torch_weights(w, dtype):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in w.items()}


# ---------------------------------------------------------------------------------------------------------------- recipes
def _edit(d, inp, seed):
    """Context b of the batch (A slots, P polylines, T steps):
      slot dead  = 1 + b % (A - 2)      padded like select_relevant_agents does (zeros, types -1): a dead slot between two live ones
      slot late  = (dead + 1) % A       absent at the steps below 1 + b % (T - 1), present from there on: key-padded scene row, live tokens
      slot gone  = (dead + 2) % A       present up to step 1 + (b + 1) % (T - 1), absent from there on
      slot head  = (dead + 3) % A       present throughout; RTG bins (0, 0, 0) and action 0 at step 0, (R-1, R-1, R-1) and V-1 at step 1
      every other slot                  as random_context drew it (some of them vanish part-way)
      polyline zero = 1 + b % (P - 2)   no point, type row -1: a padded polyline in the middle of the list
      polyline one  = zero + 1          exactly one point
      polyline all  = (zero + 2) % P    all NP points (a fresh random walk: random_context zeroes the coordinates of the points it drops)
      road type of polyline p           1 + (p + b) % 6
      window start                      context 0: 0; context 1: MAXT - T; the others as drawn.  A batch of one context: MAXT - T."""
    rs = np.random.RandomState(seed + 7)
    st, ty, go = inp["agent_states"], inp["agent_types"], inp["goals"]
    B, A, T, P, NP = st.shape[0], d.A, d.T, d.P, d.NP
    for b in range(B):
        dead = 1 + b % (A - 2)
        late, gone, head = (dead + 1) % A, (dead + 2) % A, (dead + 3) % A
        st[b, dead], ty[b, dead], go[b, dead] = 0.0, -1.0, 0.0
        st[b, late, :, 7] = 1.0
        st[b, late, :1 + b % (T - 1), 7] = 0.0
        st[b, gone, :, 7] = 1.0
        st[b, gone, 1 + (b + 1) % (T - 1):, 7] = 0.0
        st[b, head, :, 7] = 1.0
        inp["rtgs"][b, head, 0], inp["rtgs"][b, head, 1] = 0.0, d.R - 1.0
        inp["actions"][b, head, 0], inp["actions"][b, head, 1] = 0.0, d.V - 1.0
        rp, rt = inp["road_points"], inp["road_types"]
        zero = 1 + b % (P - 2)
        one, full = zero + 1, (zero + 2) % P
        rt[b] = 0.0
        rt[b, np.arange(P), 1 + (np.arange(P) + b) % 6] = 1.0
        rp[b, zero], rt[b, zero] = 0.0, -1.0
        rp[b, one, 1:] = 0.0
        rp[b, one, 0, 2] = 1.0
        if not rp[b, one, 0, :2].any():
            rp[b, one, 0, :2] = rs.uniform(-60, 60, 2)
        rp[b, full, :, :2] = rs.uniform(-60, 60, (1, 2)) + np.cumsum(rs.normal(0, 1.0, (NP, 2)), axis=0)
        rp[b, full, :, 2] = 1.0
        t0 = {0: 0, 1: d.MAXT - T}.get(b) if B > 1 else d.MAXT - T
        if t0 is not None:
            inp["timesteps"][b] = (t0 + np.arange(T))[None, :, None]
    return inp


@functools.lru_cache(maxsize=None)
def recipe(kind):
    """The inputs of a preset's batch in the reference's layout (read-only arrays: one recipe serves every test of the process)."""
    over, B, seed = PRESETS[kind]
    d = cfg_dims(kind)[1]
    inp = _edit(d, synth_inputs.random_context(d, seed, B=B), seed)
    for v in inp.values():
        v.setflags(write=False)
    return inp


def edges(inp):
    """The edges of a batch, found again from its arrays: lists of (context, slot) or (context, polyline), and the values seen."""
    ex = np.asarray(inp["agent_states"])[..., 7] != 0                       # [B, A, T]
    live_slot = (np.asarray(inp["agent_types"]) != -1).any(-1)              # [B, A]
    pe = np.asarray(inp["road_points"])[..., 2] != 0                        # [B, P, NP]
    npts = pe.sum(-1)
    B, A, _ = ex.shape
    P, NP = pe.shape[1:]
    last_live = [int(np.nonzero(npts[b])[0].max()) for b in range(B)]
    pairs = lambda m: [tuple(int(i) for i in ix) for ix in np.argwhere(m)]
    return dict(
        late=pairs(~ex[:, :, 0] & ex.any(-1)),
        gone=pairs(ex[:, :, 0] & ~ex[:, :, -1]),
        dead_between=[(b, a) for b in range(B) for a in range(1, A - 1)
                      if not live_slot[b, a] and not ex[b, a].any() and live_slot[b, a - 1] and live_slot[b, a + 1]],
        one_point=pairs(npts == 1), all_points=pairs(npts == NP),
        zero_mid=[(b, p) for b in range(B) for p in range(1, P) if npts[b, p] == 0 and p < last_live[b] and npts[b, :p].any()],
        live_polys=[int(n) for n in (npts > 0).sum(-1)],
        road_types={int(c) for c in np.argwhere(np.asarray(inp["road_types"])[npts > 0] == 1)[:, 1]},
        rtg_bins={int(v) for v in np.asarray(inp["rtgs"])[ex].reshape(-1)}, actions={int(v) for v in np.asarray(inp["actions"])[ex]},
        starts=sorted({int(v) for v in np.asarray(inp["timesteps"])[:, 0, 0, 0]}))


def torch_inputs(inp, dtype):
    x = {k: torch.from_numpy(np.array(v)) for k, v in inp.items()}             # (copies: a recipe's arrays are read-only)
    if dtype == torch.float64:
        x = {k: (v.double() if v.is_floating_point() else v) for k, v in x.items()}
    return x


# ---------------------------------------------------------------------------------------------------------------- stages
def _mode(d):
    return 1 if getattr(d, "MASK_OWN", False) else 0


def _patched(name, fn):
    """model_oracle.<name> replaced for the length of a with block (the twins' way into a function that has no hook)."""
    class _P:
        def __enter__(self):
            self.orig = getattr(mo, name)
            setattr(mo, name, fn(self.orig))

        def __exit__(self, *a):
            setattr(mo, name, self.orig)
    return _P()


def stage_tokens(tw, x, d, dtype, fault=None):
    """The inputs -> (token rows [B, 3 T A, 256], initial-state rows [B, A, 256] (before embed_ln), existence at step 0 [B, A])."""
    with fc.widened(dtype), torch.no_grad():
        if fault == "agent_id_next_slot":
            tw = dict(tw)
            tw["encoder.embed_agent_id.weight"] = torch.roll(tw["encoder.embed_agent_id.weight"], -1, 0)
        if fault == "timestep_is_window_position":
            x = dict(x)
            x["timesteps"] = torch.arange(d.T).view(1, 1, d.T, 1).expand_as(x["timesteps"]).contiguous()
        if fault == "embed_ln_eps":
            eps6 = lambda orig: lambda t, w, name: (F.layer_norm(t, (t.shape[-1],), w[name + ".weight"], w[name + ".bias"], 1e-6)
                                                    if name == "encoder.embed_ln" else orig(t, w, name))
            with _patched("_ln", eps6):
                return mo.embed_tokens(tw, x, d)
        out = mo.embed_tokens(tw, x, d)
        if fault == "return_token_unmasked":
            # the return token's row depends on the state only through existence, and embed_ln works row by row: its unmasked rows are
            # the return rows of the same inputs with every agent existing
            x1 = dict(x)
            st = x["agent_states"].clone()
            st[..., 7] = 1.0
            x1["agent_states"] = st
            tok = out[0].clone()
            tok[:, 1::3] = mo.embed_tokens(tw, x1, d)[0][:, 1::3]
            out = (tok,) + tuple(out[1:])
        return out


def stage_seg(tw, road_points, road_types, d, dtype, fault=None):
    """The road tensors -> (polyline embeddings [B, P, 256], valid [B, P])."""
    with fc.widened(dtype), torch.no_grad():
        if fault == "padded_point_pooled":
            npts = (road_points[..., 2] != 0).sum(-1).reshape(-1)

            def leak(orig):
                def mha(q, k, v, w, name, H, key_mask=None, attn_mask=None):
                    if name.endswith("road_pts_attn_layer"):
                        key_mask = key_mask.clone()
                        key_mask[npts == 1, 1] = False          # point 1 of every one-point polyline is no longer ignored
                    return orig(q, k, v, w, name, H, key_mask=key_mask, attn_mask=attn_mask)
                return mha
            with _patched("_mha", leak):
                return mo.map_encoder(tw, road_points, road_types, d.H)
        return mo.map_encoder(tw, road_points, road_types, d.H)


def stage_mem(tw, seg, init_rows, pad, d, dtype):
    """Scene-encoder source rows [polylines || initial states] and their key padding [B, P + A] (True = ignore) -> scene memory."""
    with fc.widened(dtype), torch.no_grad():
        mem = torch.cat([seg, init_rows], 1)
        for i in range(d.NE):
            mem = mo._enc_layer(mem, tw, f"encoder.transformer_encoder.layers.{i}", d.H, pad)
        return mem


def layer_weights(tw, l):
    return [tw[k] for k in lgr.names(l)]


def stage_layer(tw, l, x0, mem, pad, d):
    """Decoder layer l on the rows that enter it, from the definitions (layer_grad_ref.layer) -> (Y, X1, U) in the dtype of its operands."""
    with torch.no_grad():
        return lgr.layer(x0, mem, pad, torch.from_numpy(sgr.mask(d.T, d.A, _mode(d))), layer_weights(tw, l))


def oracle_layer(tw, l, x0, mem, pad, d, dtype, vis=None, fault=None):
    """The same stage in model_oracle's functions (its _dec_layer with the two inner rows kept) -> (Y, X1, U)."""
    p = f"decoder.transformer_decoder.layers.{l}"
    with fc.widened(dtype), torch.no_grad():
        if vis is None:
            vis = mo.causal_mask_closed_form(d.A, d.T, 3, 0, bool(getattr(d, "MASK_OWN", False)))
        x1 = mo._ln(x0 + mo._mha(x0, x0, x0, tw, p + ".self_attn", d.H, attn_mask=vis), tw, p + ".norm1")
        res = x0 if fault == "norm2_residual_from_x0" and l == d.ND - 1 else x1
        u = mo._ln(res + mo._mha(x1, mem, mem, tw, p + ".multihead_attn", d.H, key_mask=pad), tw, p + ".norm2")
        ff = mo._linear(F.relu(mo._linear(u, tw, p + ".linear1")), tw, p + ".linear2")
        return mo._ln(u + ff, tw, p + ".norm3"), x1, u


def heads(tw, x_out, d, dtype):
    """model_oracle.forward's three heads on the decoder output rows -> the three logit tensors [B, A, T, .]."""
    B = x_out.shape[0]
    with fc.widened(dtype), torch.no_grad():
        out = x_out.view(B, d.T * d.A, 3, -1)
        f = lambda k, name: mo._mlp(out[:, :, k], tw, name).view(B, d.T, d.A, -1).permute(0, 2, 1, 3)
        return {"action_preds": f(1, "decoder.predict_action"), "rtg_preds": f(0, "decoder.predict_rtg"),
                "state_preds": f(2, "decoder.predict_future_states")}


# the wrong-on-purpose twins: name -> the tensor in which the defect first appears
FAULTS = {
    "return_token_unmasked": "tokens",          # the return-token embedding is not multiplied by existence
    "agent_id_next_slot": "tokens",             # the agent-id embedding is taken from slot a + 1
    "timestep_is_window_position": "tokens",    # the timestep embedding is indexed by the window position, not by the timesteps value
    "embed_ln_eps": "tokens",                   # embed_ln with epsilon 1e-6
    "padded_point_pooled": "seg",               # one padded point of the one-point polyline takes part in the pooling
    "zero_polyline_is_key": "mem",              # the zero-point polyline in the middle is not key-padded in the scene encoder
    "late_agent_is_key": "mem",                 # the scene row of the agent absent at step 0 is not key-padded
    "norm2_residual_from_x0": "u_last",         # the last layer's norm2 takes its residual from X0 instead of X1
    "other_return_visible": "x0_1",             # the self-attention mask is visible at t_j == t_i for another agent's return token
}


def staged(tw, x, d, dtype, fault=None):
    """-> dict: tokens [B, 3 T A, 256]; seg [B, P, 256]; mem [B, P + A, 256] with pad [B, P + A] (bool, True = key-padded); x0: list of
    the ND tensors that enter the decoder layers (x0[0] is tokens); x1_last, u_last: the last layer's norm1 and norm2 outputs; x_out; the
    initial-state rows init_rows [B, A, 256]; and the three logit tensors of model_oracle.forward.  tw: torch weights in `dtype`, x:
    torch_inputs(inp, dtype).  fault: a key of FAULTS."""
    assert fault is None or fault in FAULTS
    tokens, init_rows, init_exist = stage_tokens(tw, x, d, dtype, fault)
    seg, valid = stage_seg(tw, x["road_points"], x["road_types"], d, dtype, fault)
    if fault == "zero_polyline_is_key":
        valid = valid.clone()
        for b, p in edges({k: v.numpy() for k, v in x.items()})["zero_mid"]:
            valid[b, p] = True
    if fault == "late_agent_is_key":
        init_exist = init_exist.clone()
        for b, a in edges({k: v.numpy() for k, v in x.items()})["late"]:
            init_exist[b, a] = True
    pad = ~torch.cat([valid, init_exist], 1)
    mem = stage_mem(tw, seg, init_rows, pad, d, dtype)
    vis = mo.causal_mask_closed_form(d.A, d.T, 3, 0, bool(getattr(d, "MASK_OWN", False)))
    if fault == "other_return_visible":
        i = torch.arange(3 * d.T * d.A)
        vis = vis | ((i[:, None] // (3 * d.A) == i[None, :] // (3 * d.A)) & (i[None, :] % 3 == 1))
    x0, xx = [], tokens
    for l in range(d.ND):
        x0.append(xx)
        xx, x1, u = oracle_layer(tw, l, xx, mem, pad, d, dtype, vis, fault)
    out = dict(tokens=tokens, seg=seg, mem=mem, pad=pad, x0=x0, x1_last=x1, u_last=u, x_out=xx, init_rows=init_rows)
    out.update(heads(tw, xx, d, dtype))
    return out


_STAGED = {}


def staged_of(kind, wkind, dtype, own=False):
    """staged() of a preset's recipe as float64 ndarrays (pad: bool), one evaluation per (preset, weights, model, dtype) and process."""
    d = cfg_dims(kind, own)[1]
    ck = (wkind, own, d.A, d.T, d.P, PRESETS[kind][2], dtype)
    if ck not in _STAGED:
        o = staged(torch_weights(make_weights(kind, wkind, own), dtype), torch_inputs(recipe(kind), dtype), d, dtype)
        f8 = lambda t: t.numpy() if t.dtype == torch.bool else t.double().numpy()
        _STAGED[ck] = {k: ([f8(t) for t in v] if isinstance(v, list) else f8(v)) for k, v in o.items()}
    return _STAGED[ck]


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def compared(s, pad):
    """The rows of a staged-form dict that the tests compare, by tensor kind (KINDS): every token row, every polyline row, the scene rows
    that are not key-padded (pad: the oracle's bool [B, P + A]), the rows entering the layers 1 .. ND-1, the last layer's two inner rows
    and the decoder output."""
    keep = ~np.asarray(pad, bool)
    return {"tokens": [s["tokens"]], "seg": [s["seg"]], "mem": [np.asarray(s["mem"])[:, :keep.shape[1]][keep]], "layer": list(s["x0"][1:]),
            "x1": [s["x1_last"]], "u": [s["u_last"]], "x_out": [s["x_out"]]}


def errors(got, want):
    """Two compared() dicts -> {kind: max |got - want| over the kind's tensors}."""
    return {k: max(dist(a, b) for a, b in zip(got[k], want[k])) for k in want if k in got}


def yardstick(kind, wkind, own=False):
    """e_ref per tensor kind: the float32 staged oracle's distance from the float64 one on the compared rows, over the whole batch."""
    s32, s64 = staged_of(kind, wkind, torch.float32, own), staged_of(kind, wkind, torch.float64, own)
    return errors(compared(s32, s64["pad"]), compared(s64, s64["pad"]))
