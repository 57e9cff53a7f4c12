"""ctrlsim_ctx_index_classes after its split into a one-block class scan (group masks read once, classes kept in registers) and a grid
launch for the per-vehicle entries: every output against tests/sat_ref.ctx_index_classes for chunks that start inside the table
(s0 > 0) and end inside a wave, at 255 / 256 / 257 scenarios and in the middle of a block; group counts of 0 and N; pattern-filled outputs
— rows of scenarios outside [s0, s1) and context entries beyond the chunk's count keep the pattern.  The kernel's block holds 1024
scenarios per round in four register slots per thread: chunks of 1023 / 1024 / 1025 (the round edge), 2049 (third slot, one scenario)
and 4095 (all four slots, the largest chunk) run the carry between rounds; 4096 scenarios are refused."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ctrlsim_amd import _lib  # noqa: E402
from gpu_utils import DEV, dev  # noqa: E402
import sat_ref  # noqa: E402

SENT = -9
S0 = 3


def _tables(seed, S, N):
    rs = np.random.RandomState(seed)
    n_groups = rs.randint(0, N + 1, S)
    n_groups[[0, S0, S0 + 1, S0 + 2, S - 1]] = (N, 0, N, 1, N)
    grp_ids = rs.randint(0, 2 ** 63, (S, N), dtype=np.int64).astype(np.uint64) >> rs.randint(0, 64, (S, N)).astype(np.uint64)
    grp_ids |= np.uint64(1) << rs.randint(0, N, (S, N)).astype(np.uint64)      # never empty
    grp_ids &= np.uint64(2 ** N - 1)                                            # vehicles 0 .. N - 1 only
    draw = lambda: np.where(n_groups[:, None] > 0, rs.randint(-1, np.maximum(n_groups, 1)[:, None], (S, N)), -1)
    return n_groups.astype(np.int32), grp_ids, draw().astype(np.int32), draw().astype(np.int32)


@pytest.fixture(scope="module", params=[5, 64])
def tables(request):
    N, S = request.param, S0 + 600 + 4
    return (N, S) + _tables(23 + N, S, N)


@pytest.fixture(scope="module")
def long_tables():
    N, S = 3, S0 + 4096 + 4
    return (N, S) + _tables(41, S, N)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("sizes", [[64], [2, 5, 9, 64], list(range(4, 65, 4))])
def test_chunk_matches_the_loops(tables, n, sizes):
    _check_chunk(tables, n, sizes)


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2049, 4095])
@pytest.mark.parametrize("sizes", [[64], [2, 3, 64], list(range(4, 65, 4))])
def test_chunks_of_more_than_one_round(long_tables, n, sizes):
    _check_chunk(long_tables, n, sizes)


def test_more_than_4095_scenarios_are_refused(long_tables):
    N, S, n_groups, grp_ids, own_g, mem_g = long_tables
    lib, st = _lib.lib(), _lib.stream_ptr()
    z = torch.zeros(S * N, dtype=torch.int64, device=DEV)
    out = [torch.full((S * N,), SENT, dtype=torch.int32, device=DEV) for _ in range(8)]
    assert lib.ctrlsim_ctx_index_classes(S0, S0 + 4096, N, 64, *([z.data_ptr()] * 4), 1, (C.c_int * 1)(64), *[o.data_ptr() for o in out], st) == -22
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in out)                            # nothing was launched


def _check_chunk(tables, n, sizes):
    N, S, n_groups, grp_ids, own_g, mem_g = tables
    A = 64
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    i32 = lambda a: dev(np.ascontiguousarray(a, dtype=np.int32))
    d_ng, d_own, d_mem = i32(n_groups), i32(own_g), i32(mem_g)
    d_ids = dev(np.ascontiguousarray(grp_ids).view(np.int64))
    s0, s1 = S0, S0 + n
    assert n_groups[s0] == 0 and (n == 1 or n_groups[s0 + 1] == N)
    ref = sat_ref.ctx_index_classes(n_groups, grp_ids, own_g, mem_g, sizes, A, s0, s1)
    max_ctx = int(n_groups.sum()) + 8
    ctx = {k: torch.full((max_ctx,), SENT, dtype=torch.int32, device=DEV) for k in ("ctx_scn", "ctx_grp", "ctx_row0")}
    sv = {k: torch.full((S, N), SENT, dtype=torch.int32, device=DEV) for k in ("ctx_of_group", "own_ctx", "own_slot", "mem_ctx", "mem_slot")}
    _lib.check(lib.ctrlsim_ctx_index_classes(s0, s1, N, A, p(d_ng), p(d_ids), p(d_own), p(d_mem), len(sizes), (C.c_int * len(sizes))(*sizes),
                                             p(ctx["ctx_scn"]), p(ctx["ctx_grp"]), p(ctx["ctx_row0"]), p(sv["ctx_of_group"]),
                                             p(sv["own_ctx"]), p(sv["own_slot"]), p(sv["mem_ctx"]), p(sv["mem_slot"]), st))
    torch.cuda.synchronize()
    nc = len(ref["ctx_scn"])
    assert nc == int(n_groups[s0:s1].sum())
    for k in ctx:
        got = ctx[k].cpu().numpy()
        assert np.array_equal(got[:nc], ref[k]), k
        assert (got[nc:] == SENT).all(), k
    for k in ("own_ctx", "own_slot", "mem_ctx", "mem_slot"):
        assert np.array_equal(sv[k].cpu().numpy(), ref[k]), k                   # -9 in the rows outside the chunk
    cog = np.full((S, N), SENT, np.int64)
    for (s, g), c in ref["ctx_of_group"].items():
        cog[s, g] = c
    assert np.array_equal(sv["ctx_of_group"].cpu().numpy(), cog)
