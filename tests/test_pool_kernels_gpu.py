"""csrc/pool.hip called straight through the C ABI, bit for bit against the table-driven fp32 restatement of
tests/varlen_reference.py (`pooled_reference`, `slot_gradients`): every instantiation (D = 16 / 32 / 64 / 128) and id dtype, maxlen
1 / 2 / 31 / 32, a field table of 64 entries, the capped grid (the forward's second loop trip, the backward's carried (sample,
field)), an out-of-range id that only the second trip sees, the forms without `out`, the refusals, and the engine at D = 32 / 64.

No SATrans model is needed for the direct cases: a random arena (`randn`; rows 1 and 2 of every varlen table equal, so `max` meets
ties), a field table, an X and a dx.  `out`, `rows_out`, `mask_out` and the backward's `gemb` (which is how `argmax_out` is checked,
without reading its layout) are compared with `torch.equal`; every output buffer starts as NaN / -1, so an element the kernel
skipped shows.  The cap-crossing cases PROVE that they cross it: `launch_shape` computes the block count and the trips of the
grid-stride loops from native.POOL_* (the header's SATRANS_POOL_*, which the kernels define their launch from)."""
import functools
from collections import namedtuple

import pytest
import torch

from satrans_amd import native as N
from tests import varlen_reference as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMB = {"copy": N.POOL_COPY, "sum": N.POOL_SUM, "mean": N.POOL_MEAN, "max": N.POOL_MAX}
IDS = {"f32": N.ID_F32, "i32": N.ID_I32, "i64": N.ID_I64}
DIMS = [16, 32, 64, 128]
PAD = 7777.0                # what the unused X columns hold: no table is that large, so reading one shows
SPARSE = ("copy", 1, False)

Launch = namedtuple("Launch", "blocks stride_items trips")


def ceil_div(a, b):
    return -(-a // b)


def launch_shape(n_items, D, per_thread, block, cap):
    """(workgroups, items one pass of the whole grid covers, trips of a thread's grid-stride loop) of a launch with D/4 lanes per
    item and `per_thread` items per thread and trip: enough workgroups for every item once, `cap` at most."""
    lpr = D // 4
    blocks = max(1, min(cap, ceil_div(ceil_div(n_items, per_thread) * lpr, block)))
    stride_items = blocks * block // lpr
    return Launch(blocks, stride_items, ceil_div(n_items, per_thread * stride_items))


def pool_fwd_shape(n_items, D):
    return launch_shape(n_items, D, N.POOL_ITEMS, N.POOL_BLOCK, N.POOL_MAX_BLOCKS)


def pool_bwd_shape(n_items, D):
    return launch_shape(n_items, D, 1, N.POOL_BLOCK, N.POOL_MAX_BLOCKS)


def capped_batch(D, F, per_thread, block, cap):
    """B with 4.5 capped strides of (sample, field) items: the second trip's first item is live for half of the threads, its
    other items are past the end."""
    stride = cap * block // (D // 4)
    assert stride % F != 0 and stride // F > 0                   # the carried (sample, field) advance has a carry to get wrong
    B = (per_thread * stride + stride // 2) // F
    assert per_thread * stride < B * F < (per_thread + 1) * stride
    return B


class Case:
    """A random problem: arena, field table, X (float32 holding integers, 3 unused columns at the end of a row), dx."""

    def __init__(self, D, B, layout, seed):
        g = torch.Generator().manual_seed(seed)
        self.D, self.B, self.g = D, B, g
        self.fields, col, slot, row, nv = [], 0, 0, 0, 0
        for comb, maxlen, length in layout:
            var = comb != "copy"
            vocab = int(torch.randint(6, 14, (1,), generator=g)) if var else int(torch.randint(3, 40, (1,), generator=g))
            self.fields.append(V.PoolSpec(col, maxlen, comb, col + maxlen if length else -1, slot, nv if var else -1, row,
                                          row + vocab))
            col += maxlen + (1 if length else 0)
            slot += maxlen
            row += vocab
            nv += 1 if var else 0
        self.F, self.R, self.Fv, self.x_stride = len(self.fields), slot, nv, col + 3
        self.arena = torch.randn(row, D, generator=g)
        X = torch.full((B, self.x_stride), PAD)
        for fd in self.fields:
            vocab = fd.hi - fd.lo
            if fd.varlen < 0:
                X[:, fd.col] = torch.randint(0, vocab, (B,), generator=g).float()
                continue
            self.arena[fd.lo + 2] = self.arena[fd.lo + 1]
            n = torch.randint(0, fd.maxlen + 1, (B,), generator=g)
            if fd.len_col < 0:          # exactly n valid slots at random places: padding zeros BETWEEN valid ids; empty lists
                n[::5] = 0
                ids = torch.randint(1, vocab, (B, fd.maxlen), generator=g)
                keep = torch.rand(B, fd.maxlen, generator=g).argsort(1).argsort(1) < n.unsqueeze(1)
                X[:, fd.col:fd.col + fd.maxlen] = torch.where(keep, ids, torch.zeros_like(ids)).float()
            else:                       # padding slots hold arbitrary in-range ids; lengths 0, above maxlen and negative
                n[5::7], n[1::7], n[3::7] = 0, fd.maxlen + 3, -2
                X[:, fd.col:fd.col + fd.maxlen] = torch.randint(0, vocab, (B, fd.maxlen), generator=g).float()
                X[:, fd.len_col] = n.float()
        self.X = X
        self._ref = self._grad = None

    def field_array(self, fields=None):
        fields = self.fields if fields is None else fields
        return (N.PoolField * len(fields))(*[N.PoolField(f.col, f.maxlen, COMB[f.combiner], f.len_col, f.slot, f.varlen, f.lo, f.hi)
                                             for f in fields])

    def reference(self):
        """(out, rows, mask words) - computed once, shared by the tests of this case, never written to."""
        if self._ref is None:
            self._ref = V.pooled_reference(self.arena, self.X, self.fields, self.D)
        return self._ref

    def gradient(self):
        """(dx, per-slot row gradient [B * R, D])"""
        if self._grad is None:
            dx = torch.randn(self.B, self.F, self.D, generator=torch.Generator().manual_seed(self.B + self.D))
            self._grad = (dx, V.slot_gradients(self.arena, self.X, self.fields, self.D, dx).reshape(self.B * self.R, self.D))
        return self._grad

    def device_ids(self, ids, X=None):
        """X on the device in the id dtype; float ids carry a fraction (the kernel truncates as `.long()` does)."""
        X = self.X if X is None else X
        if ids == "f32":
            return torch.where(X >= 0, X + 0.25, X).to(DEV)
        return X.to(torch.int32 if ids == "i32" else torch.int64).to(DEV)


Out = namedtuple("Out", "rc out rows mask argmax status")


def forward(case, ids="f32", X=None, want_out=True, want_mask=True, want_argmax=True, status=None, fields=None, F=None):
    """One satrans_pool_gather_fwd; the outputs stay on the device.  Unwritten elements keep NaN / -1."""
    lib = N.lib()
    Xd = case.device_ids(ids, X)
    arena = case.arena.to(DEV)
    out = torch.full((case.B, case.F, case.D), float("nan"), device=DEV) if want_out else None
    rows = torch.full((case.B, case.R), -1, dtype=torch.int32, device=DEV)
    mask = torch.full((case.B, case.Fv), -1, dtype=torch.int32, device=DEV) if want_mask else None
    argmax = torch.zeros(lib.satrans_pool_argmax_bytes(case.B, case.Fv, case.D), dtype=torch.uint8, device=DEV) if want_argmax else None
    status = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    rc = lib.satrans_pool_gather_fwd(arena.data_ptr(), arena.shape[0], None, None, case.field_array(fields),
                                     case.F if F is None else F, case.R, case.Fv, Xd.data_ptr(), IDS[ids], Xd.stride(0), case.B,
                                     case.D, N.ptr(out), rows.data_ptr(), N.ptr(mask), N.ptr(argmax), status.data_ptr(),
                                     N.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    return Out(rc, out, rows, mask, argmax, status)


def backward(case, fwd, dx):
    lib = N.lib()
    gemb = torch.full((case.B * case.R, case.D), float("nan"), device=DEV)
    dxd = dx.to(DEV)
    rc = lib.satrans_pool_bwd(dxd.data_ptr(), case.field_array(), case.F, case.R, case.Fv, case.B, case.D, fwd.mask.data_ptr(),
                              fwd.argmax.data_ptr(), gemb.data_ptr(), N.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, gemb


def words(mask):
    """The uint32 mask words of a device int32 tensor, as the reference's int64."""
    return mask.cpu().long() & 0xFFFFFFFF


def check_forward_and_backward(case, ids="f32"):
    """Every output of the forward and the backward's slot gradients equal the reference; the status word stays 0."""
    want_out, want_rows, want_words = case.reference()
    fwd = forward(case, ids)
    assert fwd.rc == 0, N.lib().satrans_last_error()
    assert int(fwd.status.cpu()) == 0
    assert torch.equal(fwd.rows.cpu(), want_rows)
    assert torch.equal(words(fwd.mask), want_words)
    assert torch.equal(fwd.out.cpu(), want_out)
    dx, want_g = case.gradient()
    rc, gemb = backward(case, fwd, dx)
    assert rc == 0, N.lib().satrans_last_error()
    assert torch.equal(gemb.cpu(), want_g)
    return fwd


# ---- a. every instantiation, small ----------------------------------------------------------------------------------------------
SMALL_LAYOUT = (SPARSE,) * 5 + (("sum", 1, False), ("mean", 2, False), ("max", 3, False), ("max", 4, True), ("mean", 5, True))


@functools.lru_cache(maxsize=None)
def small_case(D):
    return Case(D, 37, SMALL_LAYOUT, seed=100 + D)


@pytest.mark.parametrize("ids", ["f32", "i32", "i64"])
@pytest.mark.parametrize("D", DIMS)
def test_every_instantiation_and_id_dtype(D, ids):
    case = small_case(D)
    assert (case.B * case.F) % N.POOL_ITEMS != 0 and case.x_stride == max(
        max(f.col + f.maxlen, f.len_col + 1) for f in case.fields) + 3
    X, (_, _, want_words) = case.X, case.reference()
    for fd in case.fields:                                       # the case holds what it claims
        if fd.len_col >= 0:
            n = X[:, fd.len_col]
            assert bool((n == 0).any()) and bool((n > fd.maxlen).any()) and bool((n < 0).any())
        elif fd.maxlen >= 3:                                     # a padding zero between two valid ids
            x = X[:, fd.col:fd.col + fd.maxlen]
            assert bool(((x[:, :-2] != 0) & (x[:, 1:-1] == 0) & (x[:, 2:] != 0)).any())
    assert bool((want_words == 0).any())
    assert pool_fwd_shape(case.B * case.F, D).trips == 1
    check_forward_and_backward(case, ids)


# ---- b. maxlen edges ------------------------------------------------------------------------------------------------------------
def edge_case(maxlen, combiner, length):
    """2 sparse fields and one list of `maxlen` slots.  Rows 1 and 2 of its table are equal and above every other row, so where
    ids 1 / 2 sit decides where `max` is reached.  Sample 0: every slot valid; 1: only the last slot (with a length column: only
    the first - a length is a prefix); 2: none; 3: a length above maxlen; 4, 5: id 1 in slot 1 and id 2 in slot 2 (a tie across
    the boundary between two slot pairs); 6, 7: id 1 in the last slot alone."""
    case = Case(32, 33, (SPARSE, SPARSE, (combiner, maxlen, length)), seed=1000 + 8 * maxlen + 2 * ("sum", "mean", "max").index(combiner) + length)
    fd = case.fields[2]
    case.arena[fd.lo + 1] = case.arena[fd.lo + 1].abs() + 8.0
    case.arena[fd.lo + 2] = case.arena[fd.lo + 1]
    X, c = case.X, fd.col
    X[:8, c:c + maxlen] = torch.randint(3, fd.hi - fd.lo, (8, maxlen), generator=case.g).float()      # ordinary rows, all valid
    if length:
        X[:8, fd.len_col] = torch.tensor([maxlen, 1, 0, maxlen + 5, maxlen, maxlen, maxlen, maxlen]).float()
    else:
        X[1, c:c + maxlen - 1] = 0
        X[2, c:c + maxlen] = 0
    if maxlen >= 3:
        X[4:6, c + 1], X[4:6, c + 2] = 1.0, 2.0
    X[6:8, c + maxlen - 1] = 1.0
    return case


@pytest.mark.parametrize("length", [False, True], ids=["mask", "length"])
@pytest.mark.parametrize("combiner", ["sum", "mean", "max"])
@pytest.mark.parametrize("maxlen", [1, 2, 31, 32])
def test_maxlen_edges(maxlen, combiner, length):
    case = edge_case(maxlen, combiner, length)
    fd = case.fields[2]
    want_out, _, want_words = case.reference()
    full = (1 << maxlen) - 1
    assert int(want_words[0, 0]) == full and int(want_words[3, 0]) == full and int(want_words[2, 0]) == 0
    assert int(want_words[1, 0]) == (1 if length else 1 << (maxlen - 1))
    if maxlen == 32:
        assert full == 0xFFFFFFFF
    E = case.arena[fd.lo + case.X[:, fd.col:fd.col + maxlen].long()]
    valid = V.slot_mask(case.X, fd.var())
    if combiner == "mean" and maxlen == 32:                      # divided by 32 + 1e-8f, a true division
        acc = E[0, 0]
        for s in range(1, 32):
            acc = acc + E[0, s]
        assert torch.equal(want_out[0, 2], acc / (torch.tensor(32.0) + torch.tensor(1e-8)))
    if combiner == "max":                                        # count what the case was built for, in the reference's terms
        w = E - (1 - valid.float().unsqueeze(-1)) * 1e9
        top = w == w.max(1, keepdim=True)[0]
        first = top & (top.long().cumsum(1) == 1)
        if maxlen >= 3:
            assert int((first[:, 1] & top[:, 2]).sum()) >= 2 * case.D       # first reached in slot 1, equalled in slot 2
        assert int((first[:, maxlen - 1] & (top.sum(1) == 1)).sum()) >= 2 * case.D      # reached in the last slot alone
        assert bool((want_out[2, 2] < -9e8).all())               # every slot padding: the reference's value, kept
    check_forward_and_backward(case)


# ---- c. the widest field table --------------------------------------------------------------------------------------------------
def wide_layout(n_sparse):
    return (SPARSE,) * n_sparse + tuple((("sum", "mean", "max")[j % 3], 1 + j % 6, j % 2 == 1) for j in range(24))


def test_sixty_four_fields_and_one_more_is_refused():
    case = Case(32, 21, wide_layout(40), seed=64)
    assert case.F == N.POOL_MAX_FIELDS == 64 and case.Fv == 24
    check_forward_and_backward(case)
    # 65 fields: refused before anything is launched (the 65th entry is a further list behind the others)
    last = case.fields[-1]
    more = case.fields + [V.PoolSpec(last.col, 1, "sum", -1, case.R, case.Fv, last.lo, last.hi)]
    big = Case(32, 21, wide_layout(40), seed=64)
    big.R, big.Fv = case.R + 1, case.Fv + 1
    fwd = forward(big, fields=more, F=65)
    assert fwd.rc != 0 and b"F = 65" in N.lib().satrans_last_error()
    assert bool(torch.isnan(fwd.out).all()) and bool((fwd.rows == -1).all()) and int(fwd.status.cpu()) == 0
    lib = N.lib()
    gemb = torch.full((big.B * big.R, 32), float("nan"), device=DEV)
    dx = torch.zeros(big.B, 65, 32, device=DEV)
    assert lib.satrans_pool_bwd(dx.data_ptr(), big.field_array(more), 65, big.R, big.Fv, big.B, 32, fwd.mask.data_ptr(),
                                fwd.argmax.data_ptr(), gemb.data_ptr(), N.stream_handle(torch.device(DEV))) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(gemb).all())


# ---- d. second trip of the forward, carried state of the backward ---------------------------------------------------------------
CAPPED_LAYOUT = (SPARSE,) * 5 + (("max", 4, False), ("mean", 3, True))      # F = 7, R = 12: the smallest shapes past the cap


@functools.lru_cache(maxsize=1)      # (one at a time: a case holds some 100 MB of reference; D = 32 comes last and is used again)
def capped_case(D):
    B = capped_batch(D, len(CAPPED_LAYOUT), N.POOL_ITEMS, N.POOL_BLOCK, N.POOL_MAX_BLOCKS)
    return Case(D, B, CAPPED_LAYOUT, seed=200 + D)


def assert_crosses_the_cap(case):
    n_items = case.B * case.F
    fwd, bwd = pool_fwd_shape(n_items, case.D), pool_bwd_shape(n_items, case.D)
    assert fwd.blocks == bwd.blocks == N.POOL_MAX_BLOCKS
    assert fwd.trips == 2 and bwd.trips >= 3
    assert fwd.stride_items % case.F != 0 and fwd.stride_items // case.F > 0
    return fwd


@pytest.mark.parametrize("D", [16, 64, 128, 32])
def test_capped_grid_second_trip_and_carried_sample_field(D):
    case = capped_case(D)
    assert_crosses_the_cap(case)
    check_forward_and_backward(case)


# ---- e. an out-of-range id that only the second trip sees -----------------------------------------------------------------------
def test_out_of_range_id_in_the_second_trip():
    case = capped_case(32)
    shape = assert_crosses_the_cap(case)
    fd, b, s = case.fields[5], case.B - 1, 2
    assert fd.combiner == "max" and b * case.F + 5 >= N.POOL_ITEMS * shape.stride_items      # an item of the second trip
    want_out, want_rows, want_words = case.reference()
    X = case.X.clone()
    X[b, fd.col + s] = fd.hi - fd.lo                             # the vocabulary size: one past the table
    fwd = forward(case, "f32", X=X)
    assert fwd.rc == 0 and int(fwd.status.cpu()) == 1
    rows = fwd.rows.cpu()
    assert int(rows[b, fd.slot + s]) == fd.lo
    rows[b, fd.slot + s] = want_rows[b, fd.slot + s]
    assert torch.equal(rows, want_rows)
    out = fwd.out.cpu()
    assert torch.equal(out[:b], want_out[:b]) and torch.equal(out[b, :5], want_out[b, :5]) and torch.equal(out[b, 6], want_out[b, 6])
    fwd.status.zero_()
    again = forward(case, "f32", status=fwd.status)              # the id repaired, the status word cleared
    assert again.rc == 0 and int(again.status.cpu()) == 0
    assert torch.equal(again.out.cpu(), want_out) and torch.equal(again.rows.cpu(), want_rows)
    assert torch.equal(words(again.mask), want_words)


# ---- f. the forms without `out` -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["small", "capped"])
def test_rows_only_and_mask_only_forms(shape):
    case = small_case(32) if shape == "small" else capped_case(32)
    if shape == "capped":
        assert_crosses_the_cap(case)
    _, want_rows, want_words = case.reference()
    full = forward(case)
    assert full.rc == 0
    rows_only = forward(case, want_out=False, want_mask=False, want_argmax=False)
    assert rows_only.rc == 0 and int(rows_only.status.cpu()) == 0
    assert torch.equal(rows_only.rows, full.rows) and torch.equal(rows_only.rows.cpu(), want_rows)
    masks = forward(case, want_out=False, want_argmax=False)
    assert masks.rc == 0 and int(masks.status.cpu()) == 0
    assert torch.equal(masks.rows, full.rows) and torch.equal(masks.mask, full.mask)
    assert torch.equal(words(masks.mask), want_words)


# ---- g. refusals that launch nothing --------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib, st = N.lib(), N.stream_handle(torch.device(DEV))
    case = small_case(32)
    # B * R = 2^20 * 2048 = 2^31 slots: refused by its size alone, so small stand-in buffers suffice
    wide = [V.PoolSpec(33 * j, 32, "sum", 33 * j + 32, 32 * j, j, 0, 8) for j in range(64)]
    R, B = 2048, 1 << 20
    assert B * R == 1 << 31
    arena = torch.zeros(8, 32, device=DEV)
    X = torch.zeros(1, 64 * 33, device=DEV)
    rows = torch.full((64,), -1, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.satrans_pool_gather_fwd(arena.data_ptr(), 8, None, None, case.field_array(wide), 64, R, 64, X.data_ptr(), N.ID_F32,
                                       X.stride(0), B, 32, None, rows.data_ptr(), None, None, status.data_ptr(), st) == -1
    assert b"31 bits" in lib.satrans_last_error()
    assert lib.satrans_pool_bwd(X.data_ptr(), case.field_array(wide), 64, R, 64, B, 32, rows.data_ptr(), rows.data_ptr(),
                                arena.data_ptr(), st) == -1
    assert b"31 bits" in lib.satrans_last_error()
    # an embedding size without an instantiation; src_rows without src; a pooled output without its mask
    Xd, ar = case.device_ids("f32"), case.arena.to(DEV)
    out = torch.full((case.B, case.F, 48), float("nan"), device=DEV)
    r2 = torch.full((case.B, case.R), -1, dtype=torch.int32, device=DEV)
    mask = torch.full((case.B, case.Fv), -1, dtype=torch.int32, device=DEV)
    argmax = torch.zeros(case.B * case.Fv * 48, dtype=torch.uint8, device=DEV)

    def call(D, src_rows, mask_ptr):
        return lib.satrans_pool_gather_fwd(ar.data_ptr(), ar.shape[0], None, src_rows, case.field_array(), case.F, case.R, case.Fv,
                                           Xd.data_ptr(), N.ID_F32, Xd.stride(0), case.B, D, out.data_ptr(), r2.data_ptr(), mask_ptr,
                                           argmax.data_ptr(), status.data_ptr(), st)
    assert call(48, None, mask.data_ptr()) == -2 and b"embedding_dim 48" in lib.satrans_last_error()
    assert call(32, r2.data_ptr(), mask.data_ptr()) == -1 and b"src_rows without src" in lib.satrans_last_error()
    assert call(32, None, None) == -1 and b"needs mask_out" in lib.satrans_last_error()
    assert lib.satrans_pool_bwd(out.data_ptr(), case.field_array(), case.F, case.R, case.Fv, case.B, 48, mask.data_ptr(),
                                argmax.data_ptr(), out.data_ptr(), st) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((r2 == -1).all()) and bool((mask == -1).all()) and bool((rows == -1).all())
    assert int(status.cpu()) == 0 and not bool(argmax.any()) and not bool(arena.any())


# ---- h. through the engine, at the D the product runs ---------------------------------------------------------------------------
@pytest.mark.parametrize("length", [False, True], ids=["mask", "length"])
@pytest.mark.parametrize("D,maxlen", [(32, 8), (64, 1)])
def test_engine_layer_input_and_slot_gradients(D, maxlen, length):
    """tests/test_varlen_gpu.py's two bit-exact checks (their code, not a copy) on models of D = 32 / maxlen 8 and D = 64 /
    maxlen 1, at B = 96."""
    from tests import test_varlen_gpu as T
    model = T._model(("max", "mean", "sum"), length=length, D=D, maxlen=maxlen)
    T._tie(model)
    X, _ = V.batch(model, 96, seed=21)
    eng, got, want, _ = T.layer_input_and_reference(model, X, "f32")
    assert (eng.D, eng.R) == (D, 5 + 3 * maxlen)
    assert torch.equal(got, want)
    T.check_slot_gradients(model, X)
