"""What the op tests of both operand splits share (tests/test_gpu_ops.py, tests/test_gpu_model.py): the fixture that binds the split, the
parametrization over (split, case), the seeded "hot" inputs beyond the fp16 range with their float64 / float32 host references, and the
accuracy bound of the hot cases.

THE SPLIT IS BOUND BY THE TEST.  The autouse fixture of tests/conftest.py calls ctrlsim_bind(-1, None): "leave the split as it is".  A test
that launches a split-operand entry therefore asks for the `split` fixture, which binds scheme 1 (two fp16 planes, namespace s1) or 0
(three bf16 planes, s0) before the test packs a weight, and binds the process default (1) again when the test is over.

IDS.  split_cases() keeps the id every f16x3 instance had before the scheme became a parameter (the scheme they ran under was f16x3 in
every run of the whole suite), so their records stay comparable; the bf16x6 instances carry "split_bf16x6-" in front.

HOT CASES (bf16x6 only: the range the automatic fallback exists for).  The form of tests/test_gpu_attn_grads.py::_check: relative to
max |f64| (Frobenius: ||f64||), e_hip = max |hip - f64|, e_ref = max |torch float32 on the CPU - f64|, and
e_hip <= K_HOT max(e_ref, 2^-24), likewise in the Frobenius norm.  profiles/ops_bf16x6_parity.md holds every measured ratio."""
import math

import numpy as np
import pytest
import torch

from ctrlsim_amd import _lib

K_HOT = 4.0                 # largest measured ratio 2.37 (Linear + residual, 129 x 256 x 1024, max norm; profiles/ops_bf16x6_parity.md), rounded up
FLOOR = 2.0 ** -24
HOT_GAIN = 3e4              # the embedding gain of test_operand_split_is_a_runtime_choice_with_automatic_fallback
assert K_HOT <= 16.0

_INDIRECT = ("ws_option", "attn_impl")


@pytest.fixture
def split(request):
    """Binds the operand split named by the parameter ("f16x3" | "bf16x6") with the library's own guard pair; the process default
    (f16x3) is bound again on the way out."""
    lib = _lib.lib()
    _lib.check(lib.ctrlsim_bind(1 if request.param == "f16x3" else 0, None))
    assert lib.ctrlsim_split_scheme() == (1 if request.param == "f16x3" else 0)
    yield request.param
    lib.ctrlsim_bind(1, None)


def split_cases(argnames, f16x3, bf16x6, ids=None):
    """pytest.mark.parametrize over ("split", *argnames): the cases of the two-fp16-plane scheme and those of the three-bf16-plane scheme
    (its own, smaller, list where the issue of a kernel is its shape handling and not its size).  ids: {argname: {value: label}} for
    arguments that had labels of their own."""
    names = [n.strip() for n in argnames.split(",")]
    ids = ids or {}

    def tup(c):
        return tuple(c) if isinstance(c, (tuple, list)) else (c,)

    def label(c):
        return "-".join(str(ids.get(n, {}).get(v, v)) for n, v in zip(names, c))

    ps = [pytest.param("f16x3", *tup(c), id=label(tup(c))) for c in f16x3]
    ps += [pytest.param("bf16x6", *tup(c), id="split_bf16x6-" + label(tup(c))) for c in bf16x6]
    return pytest.mark.parametrize(["split"] + names, ps, indirect=["split"] + [n for n in names if n in _INDIRECT])


def errors(got, want):
    """(max |got - want| / max |want|, ||got - want||_F / ||want||_F) in float64."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = got - want
    return float(np.abs(d).max() / np.abs(want).max()), float(np.linalg.norm(d) / np.linalg.norm(want))


def check_hot(tag, got, want64, got32, k=K_HOT):
    """The hot cases' bound for one tensor; prints the figures before it asserts.  got: device result, want64 / got32: the host's float64
    and float32 evaluations (torch tensors or arrays)."""
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    got, want64, got32 = to_np(got).astype(np.float64), to_np(want64).astype(np.float64), to_np(got32).astype(np.float64)
    assert np.isfinite(want64).all() and np.isfinite(got32).all(), tag
    assert np.isfinite(got).all(), tag
    e_hip, f_hip = errors(got, want64)
    e_ref, f_ref = errors(got32, want64)
    r, rf = e_hip / max(e_ref, FLOOR), f_hip / max(f_ref, FLOOR)
    print(f"   HOT {tag}: max|f64| {np.abs(want64).max():.3e} e_hip {e_hip:.3e} e_ref {e_ref:.3e} ratio {r:.2f} | F: {f_hip:.3e} {f_ref:.3e} "
          f"ratio {rf:.2f}")
    assert e_hip <= k * max(e_ref, FLOOR), (tag, e_hip, e_ref)
    assert f_hip <= k * max(f_ref, FLOOR), (tag, f_hip, f_ref)
    return max(r, rf)


def hot_rows(M, K, g):
    """[M, K] activations beyond the fp16 range: rows of unit normals scaled by HOT_GAIN exp(randn)."""
    return torch.randn(M, K, generator=g) * (HOT_GAIN * torch.exp(torch.randn(M, 1, generator=g)))


def hot_gemm_case(M, N, K, resid, ln):
    """Seeded inputs of one hot Linear [+ residual] [+ LayerNorm] (host tensors) and its references -> (A, W, b, R, gam, bet, f64, f32)."""
    g = torch.Generator().manual_seed(1000 + M + N + K)
    A = hot_rows(M, K, g)
    W = torch.randn(N, K, generator=g) * 0.1
    b = torch.randn(N, generator=g)
    R = torch.randn(M, N, generator=g) if resid else None
    gam, bet = torch.randn(N, generator=g), torch.randn(N, generator=g)

    def ev(dt):
        y = A.to(dt) @ W.to(dt).T + b.to(dt)
        if resid:
            y = y + R.to(dt)
        return torch.nn.functional.layer_norm(y, (N,), gam.to(dt), bet.to(dt), 1e-5) if ln else y
    return A, W, b, R, gam, bet, ev(torch.float64), ev(torch.float32)


def hot_ffn_case(M, F):
    """Seeded inputs of one hot feed-forward block and its references -> (X, W1, b1, W2, b2, gam, bet, f64, f32)."""
    g = torch.Generator().manual_seed(2000 + M + F)
    X = hot_rows(M, 256, g)
    W1 = torch.randn(F, 256, generator=g) * 0.08
    W2 = torch.randn(256, F, generator=g) * 0.05
    b1 = torch.randn(F, generator=g) * 0.3
    b2 = torch.randn(256, generator=g) * 0.3
    gam, bet = torch.randn(256, generator=g), torch.randn(256, generator=g)

    def ev(dt):
        x = X.to(dt)
        h = torch.relu(x @ W1.to(dt).T + b1.to(dt))
        return torch.nn.functional.layer_norm(x + h @ W2.to(dt).T + b2.to(dt), (256,), gam.to(dt), bet.to(dt), 1e-5)
    return X, W1, b1, W2, b2, gam, bet, ev(torch.float64), ev(torch.float32)


def attn_host(q, k, v, vis, dt):
    """softmax(q k^T / sqrt(32) over the visible keys) v on the host in dtype dt; q [B,H,Lq,32], k / v [B,H,Lk,32], vis bool."""
    s = (q.to(dt) @ k.to(dt).transpose(-1, -2)) / math.sqrt(32)
    s = s.masked_fill(~vis, float("-inf"))
    return torch.softmax(s, -1) @ v.to(dt)


def top_two_gap(q, k, vis):
    """Smallest relative distance, over the rows, between the two largest visible scores in float64 (rows with one visible key: inf)."""
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(32)
    s = s.masked_fill(~vis, float("-inf"))
    if s.shape[-1] < 2:
        return float("inf")
    top = s.topk(2, -1).values
    two = torch.isfinite(top[..., 1])
    gap = (top[..., 0] - top[..., 1]).abs() / top[..., 0].abs()
    return gap[two].min().item() if two.any() else float("inf")


def hot_attn_inputs(B, Lq, Lk, logit_std, seed):
    """Q [B,Lq,256], K / V [B,Lk,256] (8 heads x 32) with V rows of magnitude 1e5 and scores q k / sqrt(32) of standard deviation
    logit_std (the gain is shared between q and k, so neither leaves the range the other operand needs)."""
    g = torch.Generator().manual_seed(seed)
    s = math.sqrt(logit_std)
    Q = torch.randn(B, Lq, 256, generator=g) * s
    K = torch.randn(B, Lk, 256, generator=g) * s
    V = torch.randn(B, Lk, 256, generator=g) * 1e5
    return Q, K, V, g


def heads(t):
    B, L, _ = t.shape
    return t.view(B, L, 8, 32).transpose(1, 2)
