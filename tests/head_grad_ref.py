"""TEST INFRASTRUCTURE — the reference's training loss (models/ctrl_sim.py:48-214) as a function of the decoder output rows, restated
with torch autograd on the CPU from the definitions: three-line MLP heads (Linear, LayerNorm eps 1e-5, ReLU, Linear), masked
cross-entropy of the action softmax and of the three interleaved return softmaxes, the shifted future-state table with its
`100 * 2 * mask.sum()` divisor in the world and the local frame, the Trajeglish shift, and
final_loss = loss_actions (x loss_action_coef) + loss_rtg_goal + loss_rtg_veh + loss_rtg_road + loss_state.
Shares no code with the library.  dtype float64: the checker; dtype float32: the reference's own arithmetic (what torch computes on
the CPU in fp32), the yardstick of the accuracy bound.

Everything is in the LIBRARY's row order: X [B*T*A*3, 256], token type k of (b, t, a) is row ((b*T + t)*A + a)*3 + k; exist [B,T,A],
st12 [B,T,A,12], act_tok [B,T,A], rtg_bin [B,T,A,3], moving [B,A]."""
import numpy as np
import torch
import torch.nn.functional as F

HEADS = ("decoder.predict_action", "decoder.predict_rtg", "decoder.predict_future_states")
PARTS = (".mlp.0.weight", ".mlp.0.bias", ".mlp.1.weight", ".mlp.1.bias", ".mlp.3.weight", ".mlp.3.bias")


def head_names(weights):
    """State-dict names of the head tensors in `weights`, in parameter-table order."""
    return [h + p for h in HEADS for p in PARTS if h + p in weights]


def action_type(variant):
    """Token type the action head reads (csrc/forward.hip): the return token (CtRL-Sim), the action token (Trajeglish), else the state token."""
    return 1 if variant == 0 else 2 if variant == 2 else 0


def ctx_from_inputs(inp):
    """Reference-layout arrays of loss_ref.make_inputs ([B,A,T,..]) -> the library-order arrays this module takes."""
    st = np.asarray(inp["agent_states"], np.float64)
    B, A, T = st.shape[:3]
    types = np.broadcast_to(np.asarray(inp["agent_types"], np.float64)[:, :, None, :], (B, A, T, 5))
    st12 = np.concatenate([st[..., :7], types], -1).transpose(0, 2, 1, 3).astype(np.float32)
    return dict(st12=np.ascontiguousarray(st12), exist=np.ascontiguousarray(st[..., 7].transpose(0, 2, 1)).astype(np.float32),
                act_tok=np.ascontiguousarray(np.asarray(inp["actions"]).transpose(0, 2, 1)).astype(np.int64),
                rtg_bin=np.ascontiguousarray(np.asarray(inp["rtgs"]).transpose(0, 2, 1, 3)),
                moving=np.asarray(inp["moving_agent_mask"], np.float64))


def mlp(x, W, h):
    z = F.linear(x, W[h + ".mlp.0.weight"], W[h + ".mlp.0.bias"])
    z = F.relu(F.layer_norm(z, (z.shape[-1],), W[h + ".mlp.1.weight"], W[h + ".mlp.1.bias"], 1e-5))
    return F.linear(z, W[h + ".mlp.3.weight"], W[h + ".mlp.3.bias"])


def loss_and_grads(X, weights, ctx, variant=0, coef=1.0, supervise_moving=True, local_frame=False, dtype=torch.float64):
    """-> (losses {name: float}, final_loss float, grads {state-dict name: ndarray float64}, dX ndarray [B*T*A*3, 256] float64)."""
    names = head_names(weights)
    W = {k: torch.tensor(np.asarray(weights[k]), dtype=dtype, requires_grad=True) for k in names}
    X = torch.tensor(np.asarray(X), dtype=dtype, requires_grad=True)
    ex = torch.tensor(np.asarray(ctx["exist"]), dtype=dtype)
    B, T, A = ex.shape
    st = torch.tensor(np.asarray(ctx["st12"]), dtype=dtype)
    mov = torch.tensor(np.asarray(ctx["moving"]), dtype=dtype)[:, None, :] if supervise_moving else torch.ones(B, 1, A, dtype=dtype)
    mask = ex * mov                                                                          # [B,T,A]
    Xt = X.view(B, T, A, 3, -1)
    losses = {}
    logits = mlp(Xt[:, :, :, action_type(variant)], W, HEADS[0])                              # [B,T,A,V]
    tok = torch.tensor(np.asarray(ctx["act_tok"]), dtype=torch.int64)
    if variant == 2:                                       # Trajeglish: step t scored against the action of step t + 1, under its mask
        nll = F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), tok[:, 1:].reshape(-1), reduction="none")
        m = mask[:, 1:].reshape(-1)
    else:
        nll = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), tok.reshape(-1), reduction="none")
        m = mask.reshape(-1)
    losses["loss_actions"] = coef * (nll * m).sum() / m.sum()
    if HEADS[1] + PARTS[0] in W:
        bins = torch.tensor(np.asarray(ctx["rtg_bin"]), dtype=torch.int64)
        C = bins.shape[-1]
        rp = mlp(Xt[:, :, :, 0], W, HEADS[1]).reshape(B * T * A, -1, C)                       # bin-major, component-minor
        for c, name in enumerate(("loss_rtg_goal", "loss_rtg_veh", "loss_rtg_road")):
            nll = F.cross_entropy(rp[:, :, c], bins[..., c].reshape(-1), reduction="none")
            losses[name] = (nll * mask.reshape(-1)).sum() / mask.sum()
    if HEADS[2] + PARTS[0] in W:
        sp = mlp(Xt[:, :, :, 2], W, HEADS[2]).view(B, T, A, -1, 2)
        smask = ex if local_frame else mask
        tot, cnt = torch.zeros((), dtype=dtype), torch.zeros((), dtype=dtype)
        for i in range(T):                                 # the reference's full table: slots past the window are there, under mask 0
            for j in range(sp.shape[3]):
                if i + 1 + j >= T:
                    tot = tot + (((sp[:, i, :, j] - 0.0) ** 2).sum(-1) * torch.zeros_like(ex[:, 0])).sum()
                    continue
                tgt = st[:, i + 1 + j, :, :2]
                if local_frame:
                    d = tgt - st[:, i, :, :2]
                    yaw = st[:, i, :, 4]
                    c_, s_ = torch.cos(-yaw), torch.sin(-yaw)
                    tgt = torch.stack([c_ * d[..., 0] - s_ * d[..., 1], s_ * d[..., 0] + c_ * d[..., 1]], -1)
                mk = smask[:, i + 1 + j]
                tot = tot + (((sp[:, i, :, j] - tgt) ** 2).sum(-1) * mk).sum()
                cnt = cnt + mk.sum()
        losses["loss_state"] = tot / (100 * 2 * cnt)
    final = sum(losses.values())
    final.backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in W.items()}
    return {k: float(v.detach()) for k, v in losses.items()}, float(final.detach()), g, X.grad.double().numpy()


def errors(got, want):
    """(max |got - want|, ||got - want||_F) relative to (max |want|, ||want||_F)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = got - want
    return float(np.abs(d).max() / np.abs(want).max()), float(np.linalg.norm(d) / np.linalg.norm(want))
