"""The context index kernels of csrc/context.hip one by one through the C ABI against the straight loops of tests/sat_ref.py:
ctx_index_classes_kernel (a 256-thread scan with wave shuffles, an LDS hand-off between waves and a carry between rounds of 256
scenarios — rollout tests reach one round only), ctx_index_kernel, group_size_hist_kernel and groups_changed_kernel (the gate of the
K/V-cached phase)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import _lib  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402
import sat_ref  # noqa: E402

EINVAL = -22
SENT = -9
CHUNKS = (1, 63, 64, 65, 255, 256, 257, 513, 1000)


def _groups(seed, S, N):
    """Random group tables: scenarios without a group and with N groups, membership masks of 1 .. N vehicles (bit N - 1 included),
    owner / member groups with -1 entries."""
    rs = np.random.RandomState(seed)
    n_groups = rs.randint(0, N + 1, S)
    n_groups[[0, 1, 2, 6, S - 1]] = (0, N, 1, 0, N)
    pop = rs.randint(1, N + 1, (S, N))
    pop[1, :2] = (N, 1)
    keys = rs.uniform(size=(S, N, N))
    member = keys.argsort(-1).argsort(-1) < pop[..., None]                     # pop[s, g] random vehicles of N
    grp_ids = (member.astype(np.uint64) << np.arange(N, dtype=np.uint64)).sum(-1).astype(np.uint64)
    assert all(sat_ref.popcount(grp_ids[s, g]) == pop[s, g] for s in range(3) for g in range(N))
    draw = lambda: np.where(n_groups[:, None] > 0, rs.randint(-1, np.maximum(n_groups, 1)[:, None], (S, N)), -1)
    return n_groups.astype(np.int32), grp_ids, draw().astype(np.int32), draw().astype(np.int32)


def _i32(a):
    return dev(np.ascontiguousarray(a, dtype=np.int32))


def _u64(a):
    return dev(np.ascontiguousarray(a).view(np.int64))


def _sizes(kind, A):
    return {"one": [A], "two": [4, A], "sixteen": list(range(4, A + 1, 4))}[kind]


@pytest.fixture(scope="module", params=[3, 64])
def tables(request):
    N, S = request.param, 5 + 1000 + 3
    return (N, S) + _groups(17 + N, S, N)


@pytest.mark.parametrize("kind", ["one", "two", "sixteen"])
def test_ctx_index_classes_matches_the_loops(tables, kind):
    """Chunks of 1 .. 1000 scenarios from s0 = 0 and 5: one to four rounds of 256, chunk ends inside a wave, at a wave edge and one past
    a round — every output against sat_ref.ctx_index_classes; rows of other scenarios and context entries beyond the chunk's count keep
    their sentinels."""
    N, S, n_groups, grp_ids, own_g, mem_g = tables
    A = 64
    sizes = _sizes(kind, A)
    assert len(sizes) == {"one": 1, "two": 2, "sixteen": 16}[kind] and sizes[-1] == A
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    d_ng, d_ids, d_own, d_mem = _i32(n_groups), _u64(grp_ids), _i32(own_g), _i32(mem_g)
    csz = (C.c_int * len(sizes))(*sizes)
    max_ctx = int(n_groups.sum()) + 8
    for s0 in (0, 5):
        for n in CHUNKS:
            s1 = s0 + n
            ref = sat_ref.ctx_index_classes(n_groups, grp_ids, own_g, mem_g, sizes, A, s0, s1)
            ctx = {k: torch.full((max_ctx,), SENT, dtype=torch.int32, device=DEV) for k in ("ctx_scn", "ctx_grp", "ctx_row0")}
            sv = {k: torch.full((S, N), SENT, dtype=torch.int32, device=DEV)
                  for k in ("ctx_of_group", "own_ctx", "own_slot", "mem_ctx", "mem_slot")}
            _lib.check(lib.ctrlsim_ctx_index_classes(s0, s1, N, A, p(d_ng), p(d_ids), p(d_own), p(d_mem), len(sizes), csz,
                                                     p(ctx["ctx_scn"]), p(ctx["ctx_grp"]), p(ctx["ctx_row0"]), p(sv["ctx_of_group"]),
                                                     p(sv["own_ctx"]), p(sv["own_slot"]), p(sv["mem_ctx"]), p(sv["mem_slot"]), st))
            torch.cuda.synchronize()
            nc = len(ref["ctx_scn"])
            for k in ctx:
                got = ctx[k].cpu().numpy()
                assert np.array_equal(got[:nc], ref[k]), (k, s0, n)
                assert (got[nc:] == SENT).all(), (k, s0, n)
            for k in ("own_ctx", "own_slot", "mem_ctx", "mem_slot"):
                assert np.array_equal(sv[k].cpu().numpy(), ref[k]), (k, s0, n)
            cog = np.full((S, N), SENT, np.int64)
            for (s, g), c in ref["ctx_of_group"].items():
                cog[s, g] = c
            assert np.array_equal(sv["ctx_of_group"].cpu().numpy(), cog), (s0, n)


def test_ctx_index_classes_refusals():
    lib = _lib.lib()
    z = torch.zeros(64, dtype=torch.int64, device=DEV)
    a = [z.data_ptr()] * 4
    o = [z.data_ptr()] * 8
    assert lib.ctrlsim_ctx_index_classes(0, 1, 3, 64, *a, 17, (C.c_int * 17)(*range(4, 72, 4)), *o, _lib.stream_ptr()) == EINVAL
    assert lib.ctrlsim_ctx_index_classes(0, 1, 3, 64, *a, 2, (C.c_int * 2)(4, 24), *o, _lib.stream_ptr()) == EINVAL
    torch.cuda.synchronize()


def test_ctx_index_matches_the_loops(tables):
    N, S, n_groups, grp_ids, own_g, mem_g = tables
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    d_ng, d_ids, d_own, d_mem = _i32(n_groups), _u64(grp_ids), _i32(own_g), _i32(mem_g)
    d_focal = torch.zeros(S, N, dtype=torch.int32, device=DEV)
    max_ctx = int(n_groups.sum()) + 8
    for s0 in (0, 5):
        for n in CHUNKS:
            s1 = s0 + n
            ref = sat_ref.ctx_index(n_groups, grp_ids, own_g, mem_g, s0, s1)
            ctx = {k: torch.full((max_ctx,), SENT, dtype=torch.int32, device=DEV) for k in ("ctx_scn", "ctx_grp")}
            sv = {k: torch.full((S, N), SENT, dtype=torch.int32, device=DEV) for k in ("own_ctx", "own_slot", "mem_ctx", "mem_slot")}
            base = torch.full((S,), SENT, dtype=torch.int32, device=DEV)
            _lib.check(lib.ctrlsim_ctx_index(s0, s1, N, p(d_ng), p(d_focal), p(d_ids), p(d_own), p(d_mem), p(ctx["ctx_scn"]),
                                             p(ctx["ctx_grp"]), p(sv["own_ctx"]), p(sv["own_slot"]), p(sv["mem_ctx"]), p(sv["mem_slot"]),
                                             p(base), st))
            torch.cuda.synchronize()
            nc = len(ref["ctx_scn"])
            for k in ctx:
                got = ctx[k].cpu().numpy()
                assert np.array_equal(got[:nc], ref[k]) and (got[nc:] == SENT).all(), (k, s0, n)
            for k in sv:
                assert np.array_equal(sv[k].cpu().numpy(), ref[k]), (k, s0, n)
            assert np.array_equal(base.cpu().numpy(), ref["ctx_base"]), (s0, n)
    z = d_ng.data_ptr()
    assert lib.ctrlsim_ctx_index(0, 4096, N, *([z] * 12), st) == EINVAL         # more scenarios than the one-block scan holds
    torch.cuda.synchronize()


@pytest.mark.parametrize("S", [1, 256, 257])
def test_group_size_hist_matches_the_loops(tables, S):
    N, _, n_groups, grp_ids, _, _ = tables
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    first = 1 if S == 1 else 0                                                   # S = 1: the scenario with N groups
    ng, ids = n_groups[first:first + S], grp_ids[first:first + S]
    d_ng, d_ids = _i32(ng), _u64(ids)
    for kind in ("one", "two", "sixteen"):
        sizes = _sizes(kind, 64)
        hist = torch.full((S + 1, len(sizes)), SENT, dtype=torch.int32, device=DEV)
        _lib.check(lib.ctrlsim_group_size_hist(S, N, p(d_ng), p(d_ids), len(sizes), (C.c_int * len(sizes))(*sizes), p(hist), st))
        torch.cuda.synchronize()
        got = hist.cpu().numpy()
        assert np.array_equal(got[:S], sat_ref.group_size_hist(ng, ids, sizes)) and (got[S] == SENT).all(), kind


@pytest.mark.parametrize("S,N", [(85, 3), (4, 64), (257, 1), (4099, 1)])
def test_groups_changed_sees_every_live_difference_and_no_dead_one(S, N):
    """S * N = 255, 256, 257, 4099 threads.  Equal snapshots leave a zero flag at 0 and a set flag at 1; a different group count, focal
    vehicle or single mask bit (bit 63 too) in the first or in the last scenario sets it; a difference in a slot at or beyond
    n_groups[s] does not."""
    rs = np.random.RandomState(S)
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    n_groups = rs.randint(0, N + 1, S).astype(np.int32)
    n_groups[[0, S - 1]] = max(1, N - 1)                                        # live slot 0 in the first and the last scenario
    focal = rs.randint(0, N, (S, N)).astype(np.int32)
    ids = rs.randint(0, 2 ** 62, (S, N)).astype(np.uint64)
    ref = (_i32(n_groups), _i32(focal), _u64(ids))

    def flag_after(ng, fo, gi, preset=0):
        flag = torch.tensor([preset, SENT], dtype=torch.int32, device=DEV)
        now = (_i32(ng), _i32(fo), _u64(gi))
        _lib.check(lib.ctrlsim_groups_changed(S, N, p(now[0]), p(now[1]), p(now[2]), p(ref[0]), p(ref[1]), p(ref[2]), p(flag), st))
        torch.cuda.synchronize()
        want = sat_ref.groups_changed(ng, fo, gi, n_groups, focal, ids)
        got = flag.cpu().numpy()
        assert got[1] == SENT and got[0] == (1 if (want or preset) else 0), (got, want, preset)
        return int(got[0])

    assert flag_after(n_groups, focal, ids) == 0 and flag_after(n_groups, focal, ids, preset=1) == 1
    for s in (0, S - 1):
        ng = n_groups.copy(); ng[s] -= 1
        assert flag_after(ng, focal, ids) == 1
        fo = focal.copy(); fo[s, 0] += 1
        assert flag_after(n_groups, fo, ids) == 1
        for bit in (0, 63):
            gi = ids.copy(); gi[s, n_groups[s] - 1] ^= np.uint64(1 << bit)
            assert flag_after(n_groups, focal, gi) == 1
    dead = [(s, g) for s in (0, S - 1, int(np.argmin(n_groups))) for g in range(n_groups[s], N)]
    assert dead or N == 1
    if N == 1:
        s = int(np.argmin(n_groups)); assert n_groups[s] == 0
        dead = [(s, 0)]
    for (s, g) in dead:
        fo = focal.copy(); fo[s, g] += 1
        gi = ids.copy(); gi[s, g] ^= np.uint64(1 << 63)
        assert flag_after(n_groups, fo, gi) == 0
