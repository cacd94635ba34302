"""csrc/gather.hip's satrans_gather_fwd called straight through the C ABI, bit for bit against torch indexing (arena[lo_f + id]):
every instantiation (D = 16 / 32 / 64 / 128) and id dtype, the capped grid (the second trip of the grid-stride loop, proven from
native.GATHER_* as tests/test_pool_kernels_gpu.py proves it for the pooled gather) with an out-of-range id in the last sample, and
the rows-only form.  Output buffers start as NaN / -1, so an element the kernel skipped shows."""
import functools
from collections import namedtuple

import pytest
import torch

from satrans_amd import native as N
from tests.test_pool_kernels_gpu import DEV, DIMS, IDS, PAD, capped_batch, launch_shape

pytestmark = pytest.mark.gpu


def gather_shape(n_rows, D):
    return launch_shape(n_rows, D, N.GATHER_ROWS_PER_THREAD, N.GATHER_BLOCK, N.GATHER_MAX_BLOCKS)


class Case:
    """F tables of random sizes back to back in a `randn` arena; field f reads X column cols[f] - the columns in a permuted
    order, 3 unused columns at the end of a row."""

    def __init__(self, D, B, F, seed):
        g = torch.Generator().manual_seed(seed)
        self.D, self.B, self.F = D, B, F
        vocab = torch.randint(3, 40, (F,), generator=g)
        hi = vocab.cumsum(0)
        self.span = torch.stack([hi - vocab, hi], 1).contiguous()              # [F, 2] int64
        self.cols = torch.randperm(F, generator=g).to(torch.int32)
        assert not torch.equal(self.cols, torch.arange(F, dtype=torch.int32))
        self.arena = torch.randn(int(hi[-1]), D, generator=g)
        self.X = torch.full((B, F + 3), PAD)
        for f in range(F):
            self.X[:, int(self.cols[f])] = torch.randint(0, int(vocab[f]), (B,), generator=g).float()
        self.rows = (self.span[:, 0].unsqueeze(0) + self.X[:, self.cols.long()].long()).to(torch.int32)      # [B, F]
        self.out = self.arena[self.rows.long()]                                                                  # [B, F, D]


Out = namedtuple("Out", "rc out rows status")


def gather(case, ids="f32", X=None, want_out=True, status=None):
    X = case.X if X is None else X
    Xd = (X + 0.25 if ids == "f32" else X.to(torch.int32 if ids == "i32" else torch.int64)).to(DEV)      # (`.long()` truncates)
    arena, span, cols = case.arena.to(DEV), case.span.to(DEV), case.cols.to(DEV)
    out = torch.full((case.B, case.F, case.D), float("nan"), device=DEV) if want_out else None
    rows = torch.full((case.B, case.F), -1, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    rc = N.lib().satrans_gather_fwd(arena.data_ptr(), span.data_ptr(), cols.data_ptr(), Xd.data_ptr(), IDS[ids], Xd.stride(0),
                                    case.B, case.F, case.D, N.ptr(out), rows.data_ptr(), status.data_ptr(),
                                    N.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    return Out(rc, out, rows, status)


def check(case, got):
    assert got.rc == 0, N.lib().satrans_last_error()
    assert int(got.status.cpu()) == 0
    assert torch.equal(got.rows.cpu(), case.rows)
    if got.out is not None:
        assert torch.equal(got.out.cpu(), case.out)


@functools.lru_cache(maxsize=None)
def small_case(D):
    return Case(D, 37, 5, seed=300 + D)


@functools.lru_cache(maxsize=1)
def capped_case(D):
    return Case(D, capped_batch(D, 7, N.GATHER_ROWS_PER_THREAD, N.GATHER_BLOCK, N.GATHER_MAX_BLOCKS), 7, seed=400 + D)


def assert_crosses_the_cap(case):
    shape = gather_shape(case.B * case.F, case.D)
    assert shape.blocks == N.GATHER_MAX_BLOCKS and shape.trips == 2
    assert shape.stride_items % case.F != 0 and shape.stride_items // case.F > 0
    return shape


@pytest.mark.parametrize("ids", ["f32", "i32", "i64"])
@pytest.mark.parametrize("D", DIMS)
def test_every_instantiation_and_id_dtype(D, ids):
    case = small_case(D)
    assert (case.B * case.F) % N.GATHER_ROWS_PER_THREAD != 0 and gather_shape(case.B * case.F, D).trips == 1
    check(case, gather(case, ids))
    check(case, gather(case, ids, want_out=False))               # rows only


@pytest.mark.parametrize("D", DIMS)
def test_capped_grid_second_trip_and_an_out_of_range_id_in_it(D):
    case = capped_case(D)
    shape = assert_crosses_the_cap(case)
    full = gather(case)
    check(case, full)
    rows_only = gather(case, want_out=False)
    check(case, rows_only)
    assert torch.equal(rows_only.rows, full.rows)
    # one id equal to its vocabulary size in the last sample: flagged, zeros, the table's first row recorded; nothing else moves
    b, f = case.B - 1, 3
    assert b * case.F + f >= N.GATHER_ROWS_PER_THREAD * shape.stride_items       # a row of the second trip
    lo, hi = int(case.span[f, 0]), int(case.span[f, 1])
    X = case.X.clone()
    X[b, int(case.cols[f])] = hi - lo
    bad = gather(case, X=X)
    assert bad.rc == 0 and int(bad.status.cpu()) == 1
    rows, out = bad.rows.cpu(), bad.out.cpu()
    assert int(rows[b, f]) == lo and not bool(out[b, f].any())
    rows[b, f], out[b, f] = case.rows[b, f], case.out[b, f]
    assert torch.equal(rows, case.rows) and torch.equal(out, case.out)
    bad.status.zero_()
    check(case, gather(case, status=bad.status))                 # the id repaired, the status word cleared
