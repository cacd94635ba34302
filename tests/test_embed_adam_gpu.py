"""csrc/embed_adam.hip through the C ABI against the fp64 restatements of tests/embed_adam_reference.py: the gathered-row optimizer
chain at every embedding width (D = 16 / 32 / 64 put 4 / 2 / 1 superchunks in a workgroup and walk them at the tail of the chunk
kernel, D = 128 walks them in a launch of its own) on id lists whose runs are placed on the chunk and superchunk boundaries of
the ordered sum, the streaming step of the untouched rows at every row range and grid, the other optimizers, the small reductions,
and 200 steps of the flat Adam in both arithmetics.  tests/test_embed_adam_cpu.py checks the restatements, the layouts and the
premises of the bounds without a GPU.

Every bound is counted from roundings, taken from test_optimizer_kernels_exact (tests/test_gpu_parity.py) or measured on the CPU
against fp64; none is taken from what the kernels give.  The largest ratios of error to bound seen on an MI355X stand in the
docstrings."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from satrans_amd import native as N
from tests import embed_adam_reference as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, B1, B2, EPS, L2, T = 0.005, 0.9, 0.999, 1e-8, 1e-5, 4
ARITHS = ("exact", "fast")
STREAM_SLOTS = 2048          # kStreamBlocks: the partial-sum slots of the streaming kernel, and its largest grid
SENTINEL = -7                # what `last` holds where no kernel wrote it


def stream():
    return torch.cuda.current_stream().cuda_stream


def hp(arith, l2=L2, t=T):
    """satrans_adam_hparams of step t, filled as engine._hparams fills it."""
    h = N.AdamHParams()
    h.lr_over_bc1, h.bc2_sqrt = LR / (1.0 - B1 ** t), math.sqrt(1.0 - B2 ** t)
    h.beta1, h.beta2, h.eps, h.l2 = B1, B2, EPS, l2
    h.arith = N.ADAM_FAST if arith == "fast" else N.ADAM_EXACT
    return h


def ref_hp(l2=L2, t=T):
    return E.hparams(LR, B1, B2, EPS, l2, t)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def step_ratios(got, before, want):
    """Error over bound of one Adam step, (p, m, v): got / before float32 (P, M, V), want float64.  The bounds are those of
    test_optimizer_kernels_exact: m and v at rtol 1e-6 with atol 2e-7 max|.|, p' - p at rtol 2e-5 with atol 1e-6 lr."""
    (gp, gm, gv), (wp, wm, wv) = got, want
    p0 = before[0].double()
    dp_got, dp_want = (gp - before[0]).double(), wp - p0           # (the float32 difference, as the existing test takes it)
    rp = ((dp_got - dp_want).abs() / (1e-6 * LR + 2e-5 * dp_want.abs())).max()
    rm = ((gm.double() - wm).abs() / (2e-7 * wm.abs().max() + 1e-6 * wm.abs())).max()
    rv = ((gv.double() - wv).abs() / (2e-7 * wv.abs().max() + 1e-6 * wv.abs())).max()
    return float(rp), float(rm), float(rv)


# ---- section 3: ordered sums and the touched-row step ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layout(name):
    rows, src = E.layout_rows(name)
    return SimpleNamespace(name=name, rows=rows, src=src, n=rows.numel(), rows_d=rows.to(DEV), src_d=src.to(DEV),
                           distinct=torch.unique(rows).long())


@functools.lru_cache(maxsize=4)
def problem(name, D):
    """The step's inputs on the CPU and its fp64 result: exact-sum gradients, G = dense_grad, adam_step on the whole arena."""
    L = layout(name)
    P, M, V = E.tables(E.R, D, seed=D)
    gemb = E.exact_grads(L.n, D, seed=1000 + D)
    G = E.dense_grad(L.rows, gemb[L.src.long()], E.R)              # sorted position j takes gemb[src[j]]
    assert bool((G.float().double() == G).all()), "exact in float32"
    return SimpleNamespace(L=L, D=D, P=P, M=M, V=V, gemb=gemb, G=G, want=E.adam_step(P, M, V, G, ref_hp()), reg=E.reg(P, L2))


def workspace(n, D):
    return torch.zeros(int(N.lib().satrans_embed_partial_ws_floats(n, D)), device=DEV)


def reg_slots(n, D):
    return torch.ones(int(N.lib().satrans_embed_reg_partials(E.R, n, D)), dtype=torch.float64, device=DEV)


def sum_f64(vals, count=None, out=None, accumulate=0):
    out = torch.zeros(1, dtype=torch.float64, device=DEV) if out is None else out
    N.check(N.lib().satrans_sum_f64(vals.data_ptr(), vals.numel() if count is None else count, out.data_ptr(), accumulate, stream()),
            "sum_f64")
    return float(out.item())


def segment_sums(L, D, gemb_d, part, regp, rows=E.R):
    G = torch.zeros(rows, D, device=DEV)
    N.check(N.lib().satrans_embed_segment_sums(L.rows_d.data_ptr(), L.src_d.data_ptr(), L.n, gemb_d.data_ptr(), D, part.data_ptr(),
                                               regp.data_ptr(), G.data_ptr(), stream()), "segment_sums")
    return G


def touched_form(pr, arith, part=None, src_d=None, gemb_d=None):
    """satrans_embed_adam_touched with last / t, satrans_embed_mark_touched, satrans_embed_adam_untouched(first_row = 0)."""
    lib, L, D = N.lib(), pr.L, pr.D
    P, M, V = (x.to(DEV) for x in (pr.P, pr.M, pr.V))
    gemb_d = pr.gemb.to(DEV) if gemb_d is None else gemb_d
    src_d = L.src_d if src_d is None else src_d
    part = workspace(L.n, D) if part is None else part
    regp = reg_slots(L.n, D)
    last = torch.full((E.R,), SENTINEL, dtype=torch.int32, device=DEV)
    touched = torch.full(((E.R + 31) // 32,), -1, dtype=torch.int32, device=DEV)        # (mark_touched clears it)
    N.check(lib.satrans_embed_adam_touched(P.data_ptr(), M.data_ptr(), V.data_ptr(), D, L.rows_d.data_ptr(), src_d.data_ptr(), L.n,
                                           gemb_d.data_ptr(), part.data_ptr(), C.byref(hp(arith)), regp.data_ptr(), last.data_ptr(),
                                           T, stream()), "touched")
    after_touched = SimpleNamespace(P=P.cpu(), M=M.cpu(), V=V.cpu(), last=last.cpu(), regp=regp.cpu())
    N.check(lib.satrans_embed_mark_touched(L.rows_d.data_ptr(), L.n, E.R, touched.data_ptr(), stream()), "mark_touched")
    N.check(lib.satrans_embed_adam_untouched(P.data_ptr(), M.data_ptr(), V.data_ptr(), 0, E.R, D, touched.data_ptr(),
                                             C.byref(hp(arith)), regp.data_ptr(), 0, stream()), "untouched")
    torch.cuda.synchronize()
    return SimpleNamespace(P=P.cpu(), M=M.cpu(), V=V.cpu(), last=last.cpu(), regp=regp, after_touched=after_touched)


@pytest.mark.parametrize("D", E.DIMS)
@pytest.mark.parametrize("name", list(E.LAYOUTS))
def test_segment_sums_are_exact(name, D):
    """satrans_embed_segment_sums into a zeroed G [R, D]: bit for bit dense_grad (fp64 index_add) on the touched rows, zero on every
    other row.  The gradients are integers in [-8, 8] times 2^-20, whose sums are exact in any order, so there is no bound: a piece of
    a run left out, taken twice or given to the wrong row is an exact mismatch."""
    pr = problem(name, D)
    G = segment_sums(pr.L, D, pr.gemb.to(DEV), workspace(pr.L.n, D), reg_slots(pr.L.n, D)).cpu()
    assert same_bits(G, pr.G.float()), f"rows that differ: {torch.nonzero((G.double() != pr.G).any(1)).flatten().tolist()[:8]}"
    other = torch.ones(E.R, dtype=torch.bool)
    other[pr.L.distinct] = False
    assert not G[other].any() and bool(pr.G[pr.L.distinct].abs().sum() > 0)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("D", E.DIMS)
@pytest.mark.parametrize("name", list(E.LAYOUTS))
def test_touched_row_step_is_adam_on_the_whole_arena(name, D, arith):
    """adam_touched (with last / t), mark_touched, adam_untouched(first_row = 0) against E.adam_step on the whole arena with G =
    dense_grad, in both arithmetics.  Bounds of test_optimizer_kernels_exact: m and v at rtol 1e-6 with atol 2e-7 max|.|, p' - p at
    rtol 2e-5 with atol 1e-6 lr; the gradient sums are exact, so a row stepped twice or not at all misses them by orders of magnitude.
    `last` is t exactly on the touched rows and keeps its sentinel elsewhere.  reg_partials starts as 1.0 in every slot, and its sum
    through satrans_sum_f64 is float32(l2) * sum(P^2) to 1e-12 relative (double sums of double products): an unwritten slot adds 1.0.
    Largest error / bound seen over all layouts and widths, the same in both arithmetics: p 0.36, m 0.06, v 0.09."""
    pr = problem(name, D)
    got = touched_form(pr, arith)
    ratios = step_ratios((got.P, got.M, got.V), (pr.P, pr.M, pr.V), pr.want)
    print(f"touched step {name} D={D} {arith}: error / bound p {ratios[0]:.3f} m {ratios[1]:.3f} v {ratios[2]:.3f}")
    assert max(ratios) <= 1.0, ratios
    want_last = torch.full((E.R,), SENTINEL, dtype=torch.int32)
    want_last[pr.L.distinct] = T
    assert torch.equal(got.last, want_last)
    assert sum_f64(got.regp) == pytest.approx(pr.reg, rel=1e-12)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("D", E.DIMS)
@pytest.mark.parametrize("name", list(E.LAYOUTS))
def test_the_forms_of_a_step_leave_the_same_bits(name, D, arith):
    """The same step as segment_sums + adam_rows(row0 = 0, rows = R), and as adam_touched on pack_rows' output with the identity as
    `src`, leaves the tables of the touched + untouched form bit for bit (the sums are exact and every form runs adam4).  pack_rows is
    gemb[src] exactly."""
    lib, pr = N.lib(), problem(name, D)
    L = pr.L
    base = touched_form(pr, arith)
    gemb_d = pr.gemb.to(DEV)
    # dense form
    P, M, V = (x.to(DEV) for x in (pr.P, pr.M, pr.V))
    G = segment_sums(L, D, gemb_d, workspace(L.n, D), reg_slots(L.n, D))
    regr = torch.ones(int(lib.satrans_embed_adam_rows_partials(E.R, D)), dtype=torch.float64, device=DEV)
    last = torch.full((E.R,), SENTINEL, dtype=torch.int32, device=DEV)
    N.check(lib.satrans_embed_adam_rows(P.data_ptr(), M.data_ptr(), V.data_ptr(), last.data_ptr(), 0, E.R, D, G.data_ptr(),
                                        C.byref(hp(arith)), T, regr.data_ptr(), stream()), "adam_rows")
    torch.cuda.synchronize()
    assert same_bits(P.cpu(), base.P) and same_bits(M.cpu(), base.M) and same_bits(V.cpu(), base.V), "segment_sums + adam_rows"
    assert bool((last == T).all()) and sum_f64(regr) == pytest.approx(pr.reg, rel=1e-12)
    # packed form
    packed = torch.full((L.n, D), float("nan"), device=DEV)
    N.check(lib.satrans_embed_pack_rows(L.src_d.data_ptr(), L.n, gemb_d.data_ptr(), D, packed.data_ptr(), stream()), "pack_rows")
    assert same_bits(packed.cpu(), pr.gemb[L.src.long()])
    ident = torch.arange(L.n, dtype=torch.int32, device=DEV)
    got = touched_form(pr, arith, src_d=ident, gemb_d=packed)
    assert same_bits(got.P, base.P) and same_bits(got.M, base.M) and same_bits(got.V, base.V), "pack_rows + adam_touched"
    assert torch.equal(got.last, base.last)


@pytest.mark.parametrize("D", E.DIMS)
@pytest.mark.parametrize("first,second", [("one_row", "distinct"), ("mixture", "short"), ("aligned", "off_by_one")])
def test_a_stale_workspace_changes_nothing(first, second, D):
    """Layout A, then layout B on the same partial_ws (sized for the larger): B's tables, `last`, partial sums and segment sums are
    those of B on a fresh zeroed workspace, bit for bit.  The leftovers are what a real step finds: the records of another id list
    (in-range rows), at offsets that belong to other arrays of B's layout."""
    A, Bp = problem(first, D), problem(second, D)
    n_big = max(A.L.n, Bp.L.n)
    fresh = touched_form(Bp, "fast").after_touched
    fresh_G = segment_sums(Bp.L, D, Bp.gemb.to(DEV), workspace(Bp.L.n, D), reg_slots(Bp.L.n, D)).cpu()
    part = workspace(n_big, D)
    touched_form(A, "fast", part=part)
    got = touched_form(Bp, "fast", part=part).after_touched
    for k in ("P", "M", "V"):
        assert same_bits(getattr(got, k), getattr(fresh, k)), k
    assert torch.equal(got.last, fresh.last) and torch.equal(got.regp, fresh.regp)
    touched_form(A, "fast", part=part)
    assert same_bits(segment_sums(Bp.L, D, Bp.gemb.to(DEV), part, reg_slots(Bp.L.n, D)).cpu(), fresh_G)


@pytest.mark.parametrize("D", E.DIMS)
def test_segment_sums_of_rounding_gradients(D):
    """`mixture` with seeded normal gradients: every element of G is within (len - 1) * 2^-24 * sum|g| of the fp64 sum, len the
    row's run length - the bound of a float32 sum of len terms taken in any order (len - 1 additions, each within 2^-24 of its own
    result, which no partial sum of |g| exceeds).  Two calls give the same bits: the order is fixed.
    Largest error / bound seen: 1.00, on runs of two (one addition, half an ulp right above a power of two); 0.88 on longer runs."""
    L = layout("mixture")
    gemb = torch.randn(L.n, D, generator=torch.Generator().manual_seed(50 + D)) * 1e-3
    sorted_g = gemb[L.src.long()]
    want, mass = E.dense_grad(L.rows, sorted_g, E.R), E.dense_grad(L.rows, sorted_g.abs(), E.R)
    length = torch.bincount(L.rows.long(), minlength=E.R).double()
    part = workspace(L.n, D)
    G = segment_sums(L, D, gemb.to(DEV), part, reg_slots(L.n, D)).cpu()
    bound = (length - 1).clamp(min=0).unsqueeze(1) * 2.0 ** -24 * mass
    err = (G.double() - want).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    many = length > 1
    longer = length > 2
    print(f"rounding gradients D={D}: largest error / bound {float((err[many] / bound[many]).max()):.3f}, "
          f"on runs longer than two {float((err[longer] / bound[longer]).max()):.3f}")
    assert bool((err[many] > 0).any()), "the gradients do round"
    assert same_bits(segment_sums(L, D, gemb.to(DEV), part, reg_slots(L.n, D)).cpu(), G)


# ---- section 4: untouched rows -----------------------------------------------------------------------------------------------------
# rows next to the `first_row` values of the test below: these step (or keep their bits, when they lie below first_row) ...
FORCED_UNTOUCHED = (0, 30, 31, 36, 37, 63, 64, E.R - 1)
FORCED_TOUCHED = (1, 32, 38, 65, E.R - 2)          # ... and these never do


@functools.lru_cache(maxsize=None)
def touched_set():
    """-> (is_touched [R] bool, bitmap [ceil(R / 32)] int32 on the device): a seeded third of the rows."""
    rng = np.random.RandomState(9)
    on = np.zeros(E.R, dtype=bool)
    on[rng.choice(E.R, E.R // 3, replace=False)] = True
    on[list(FORCED_UNTOUCHED)], on[list(FORCED_TOUCHED)] = False, True
    words = np.zeros((E.R + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, np.flatnonzero(on) >> 5, np.uint32(1) << (np.flatnonzero(on) & 31).astype(np.uint32))
    return torch.from_numpy(on), torch.from_numpy(words.view(np.int32)).to(DEV)


def untouched(P, M, V, first_row, D, arith, grid=0, slots=None, bitmap=None, rows=E.R):
    """-> (rc, P, M, V on the CPU, reg_partials): one call of satrans_embed_adam_untouched on device copies of P, M, V."""
    Pd, Md, Vd = (x.to(DEV) for x in (P, M, V))
    slots = torch.ones(STREAM_SLOTS + 16, dtype=torch.float64, device=DEV) if slots is None else slots
    bitmap = touched_set()[1] if bitmap is None else bitmap
    rc = N.lib().satrans_embed_adam_untouched(Pd.data_ptr(), Md.data_ptr(), Vd.data_ptr(), first_row, rows, D, bitmap.data_ptr(),
                                              C.byref(hp(arith)), slots.data_ptr(), grid, stream())
    torch.cuda.synchronize()
    return rc, Pd.cpu(), Md.cpu(), Vd.cpu(), slots.cpu()


@pytest.mark.parametrize("D", E.DIMS)
@pytest.mark.parametrize("first_row", [0, 1, 31, 37, 64, E.R - 1, E.R])
def test_untouched_rows_from_any_first_row(first_row, D):
    """satrans_embed_adam_untouched over [first_row, R) for first rows that are no multiple of the bitmap word, in both arithmetics:
    rows below first_row and touched rows keep their bits; every other row is E.adam_step with G = 0 inside the bounds of
    test_optimizer_kernels_exact (m, v: rtol 1e-6, atol 2e-7 max|.|; p' - p: rtol 2e-5, atol 1e-6 lr); the partial sums add up to
    float32(l2) * sum(p^2) over the stepped rows to 1e-12 relative.  first_row = R changes nothing and returns OK.
    Largest error / bound seen, the same in both arithmetics: p 0.36, m 0.05, v 0.09."""
    on, _ = touched_set()
    P, M, V = E.tables(E.R, D, seed=D)
    stepped = ~on
    stepped[:first_row] = False
    assert int(stepped.sum()) == (0 if first_row == E.R else int((~on[first_row:]).sum())) and (first_row == E.R or stepped.any())
    want = E.adam_step(P[stepped], M[stepped], V[stepped], torch.zeros_like(P[stepped]), ref_hp())
    for arith in ARITHS:
        rc, Pg, Mg, Vg, slots = untouched(P, M, V, first_row, D, arith)
        assert rc == 0, N.lib().satrans_last_error()
        for got, before in ((Pg, P), (Mg, M), (Vg, V)):
            assert same_bits(got[~stepped], before[~stepped]), "a row below first_row or a touched row moved"
        assert math.fsum(slots[:STREAM_SLOTS].tolist()) == pytest.approx(E.reg(P[stepped], L2), rel=1e-12, abs=0.0)
        assert bool((slots[STREAM_SLOTS:] == 1.0).all())
        if first_row < E.R:
            ratios = step_ratios((Pg[stepped], Mg[stepped], Vg[stepped]), (P[stepped], M[stepped], V[stepped]), want)
            print(f"untouched first_row={first_row} D={D} {arith}: error / bound p {ratios[0]:.3f} m {ratios[1]:.3f} v {ratios[2]:.3f}")
            assert max(ratios) <= 1.0, ratios
            assert not (Pg[stepped] == P[stepped]).all(1).any(), "every row that should step did"


@pytest.mark.parametrize("D", E.DIMS)
def test_untouched_rows_at_every_grid(D):
    """grid_blocks 0 (= 512), 1, 7, 2048 and 5000 (clamped to 2048): the same bits in the tables, and the first 2048 partial-sum slots,
    which start as 1.0, add up to float32(l2) * sum(p^2) over the stepped rows to 1e-12 relative for every grid - the slots beyond the
    grid are cleared, the slots beyond 2048 are not written.  At 7 blocks a lane's loop makes several passes (four elements in flight
    per lane and pass)."""
    assert E.R * (D // 4) > 2 * 7 * 256 * 4, "several passes of the 7-block grid"
    on, _ = touched_set()
    P, M, V = E.tables(E.R, D, seed=D)
    want_reg = E.reg(P[~on], L2)
    base = None
    for grid in (0, 1, 7, 2048, 5000):
        rc, Pg, Mg, Vg, slots = untouched(P, M, V, 0, D, "fast", grid=grid)
        assert rc == 0, N.lib().satrans_last_error()
        assert math.fsum(slots[:STREAM_SLOTS].tolist()) == pytest.approx(want_reg, rel=1e-12), grid
        assert bool((slots[STREAM_SLOTS:] == 1.0).all()), grid
        used = {0: 512, 5000: 2048}.get(grid, grid)
        assert not slots[used:STREAM_SLOTS].any(), grid
        if base is None:
            base = (Pg, Mg, Vg)
            assert not same_bits(Pg, P)
        assert all(same_bits(a, b) for a, b in zip((Pg, Mg, Vg), base)), grid


@pytest.mark.parametrize("arith", ARITHS)
def test_untouched_step_does_not_depend_on_the_width(arith):
    """One flat buffer of 515 * 128 floats taken as 515 * 128 / D rows of D, nothing touched: the same bits at every D, and those are
    the bits of satrans_adam_flat with g = 0 and the same l2 (every form runs adam1 on g = 0 + 2 l2 p)."""
    rows128 = 515
    P, M, V = E.tables(rows128, 128, seed=3)
    n = P.numel()
    pd, md, vd, gd = P.flatten().to(DEV), M.flatten().to(DEV), V.flatten().to(DEV), torch.zeros(n, device=DEV)
    N.check(N.lib().satrans_adam_flat(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, C.byref(hp(arith)), stream()), "flat")
    flat = (pd.cpu(), md.cpu(), vd.cpu())
    assert not same_bits(flat[0], P.flatten())
    for D in E.DIMS:
        rows = n // D
        bitmap = torch.zeros((rows + 31) // 32, dtype=torch.int32, device=DEV)
        rc, *got, _ = untouched(P.view(rows, D), M.view(rows, D), V.view(rows, D), 0, D, arith, bitmap=bitmap, rows=rows)
        assert rc == 0, N.lib().satrans_last_error()
        assert all(same_bits(a.flatten(), b) for a, b in zip(got, flat)), D


# ---- section 5: the other optimizers, the dense gradient, the small reductions -----------------------------------------------------
OPT_EPS = {E.SGD: 0.0, E.ADAGRAD: 1e-10, E.RMSPROP: 1e-8}        # compile()'s defaults


@pytest.mark.parametrize("n", [1, 255, 256, 257, 10007])
@pytest.mark.parametrize("kind", [E.SGD, E.ADAGRAD, E.RMSPROP])
def test_optim_flat_against_fp64(kind, n):
    """satrans_optim_flat against E.other_step on identical inputs, bounds counted from the kernel's explicit roundings.
    SGD: |err| <= 2^-23 (|p| + |lr g|) (a product and a sum, half an ulp each).  Adagrad, RMSprop: the state within 1.01 * 2^-23
    relative (two roundings of positive terms); the parameter within 2^-21 |update| + 2^-23 |p| (the update takes at most six
    roundings of 2^-24 - state 2, square root 1, add eps 1, divide 1, times lr 1 - and the final sum one more).  Where g = 0 the
    parameter keeps its bits, also where the state is 0 as well (Adagrad then divides 0 by eps): no NaN.  SGD leaves `state` alone
    and takes a null one; the others refuse it.  (RMSprop's weight 1 - alpha is restated as the kernel forms it, 1.0f - alpha, which is
    9.3e-7 below torch's float32(1 - alpha): tests/test_embed_adam_cpu.py::test_what_the_rmsprop_weight_costs.)
    Largest error / bound seen: SGD 0.50; Adagrad state 0.49 of 2^-23, parameter 0.48; RMSprop state 0.96 of 2^-23, parameter 0.46."""
    lib = N.lib()
    g_ = torch.Generator().manual_seed(100 * kind + n % 97)
    p = torch.randn(n, generator=g_) * 0.05
    g = torch.randn(n, generator=g_) * 1e-3
    s = torch.rand(n, generator=g_) * 1e-5
    g[3::7], s[3::14] = 0.0, 0.0
    lr, alpha, eps = 0.01, 0.99, OPT_EPS[kind]
    pd, gd, sd = p.to(DEV), g.to(DEV), s.to(DEV)
    N.check(lib.satrans_optim_flat(kind, pd.data_ptr(), gd.data_ptr(), sd.data_ptr(), n, lr, alpha, eps, stream()), "optim_flat")
    got_p, got_s = pd.cpu(), sd.cpu()
    want_p, want_s = E.other_step(kind, p, s, g, lr, alpha, eps)
    upd = (want_p - p.double()).abs()
    err = (got_p.double() - want_p).abs()
    assert not torch.isnan(got_p).any() and same_bits(got_p[g == 0], p[g == 0])
    if kind == E.SGD:
        bound = 2.0 ** -23 * (p.double().abs() + upd)
        assert same_bits(got_s, s), "SGD has no state"
        p2 = p.to(DEV)
        N.check(lib.satrans_optim_flat(kind, p2.data_ptr(), gd.data_ptr(), None, n, lr, alpha, eps, stream()), "optim_flat, null state")
        assert same_bits(p2.cpu(), got_p)
    else:
        bound = 2.0 ** -21 * upd + 2.0 ** -23 * p.double().abs()
        s_err = (got_s.double() - want_s).abs()
        assert bool((s_err <= 1.01 * 2.0 ** -23 * want_s).all()), float((s_err / want_s.clamp(min=1e-300)).max() * 2 ** 23)
        print(f"optim_flat kind {kind} n={n}: state error {float((s_err / want_s.clamp(min=1e-300)).max() * 2 ** 23):.3f} of 2^-23")
        assert lib.satrans_optim_flat(kind, pd.data_ptr(), gd.data_ptr(), None, n, lr, alpha, eps, stream()) != 0, "a null state is refused"
        torch.cuda.synchronize()
        assert same_bits(pd.cpu(), got_p), "... before anything is launched"
    assert bool((err <= bound).all()), float((err / bound).max())
    print(f"optim_flat kind {kind} n={n}: parameter error / bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
    assert n < 8 or bool((got_p != p).any())


@pytest.mark.parametrize("l2", [0.0, 1e-5])
@pytest.mark.parametrize("D", E.DIMS)
@pytest.mark.parametrize("name", ["off_by_one", "mixture"])
def test_grad_dense_adds_the_dense_gradient(name, D, l2):
    """satrans_embed_grad_dense ADDS onto g_arena, which starts as integers times 2^-20.  With l2 = 0 and exact-sum gradients the result
    is prefill + dense_grad bit for bit; with l2 = 1e-5 every element is within 2^-23 (|G| + |2 l2 p|) of G + 2 l2 p, G the exact
    prefill + dense_grad: the product and the sum round once each (or once together, as an fma).
    Largest error / bound seen with l2: 0.50."""
    pr = problem(name, D)
    L = pr.L
    prefill = torch.randint(-64, 65, (E.R, D), generator=torch.Generator().manual_seed(D)).float() * 2.0 ** -20
    ga, P_d, gemb_d = prefill.to(DEV), pr.P.to(DEV), pr.gemb.to(DEV)
    N.check(N.lib().satrans_embed_grad_dense(P_d.data_ptr(), L.rows_d.data_ptr(), L.src_d.data_ptr(), L.n, gemb_d.data_ptr(), E.R, D,
                                             l2, ga.data_ptr(), stream()), "grad_dense")
    G = prefill.double() + pr.G
    if l2 == 0.0:
        assert same_bits(ga.cpu(), G.float()) and bool((G.float().double() == G).all())
        return
    reg_g = 2.0 * E.f32(l2) * pr.P.double()
    err, bound = (ga.cpu().double() - (G + reg_g)).abs(), 2.0 ** -23 * (G.abs() + reg_g.abs())
    assert bool((err <= bound).all()), float((err / bound).max())
    print(f"grad_dense {name} D={D}: error / bound {float((err / bound).max()):.3f}")
    assert bool((ga.cpu() != G.float()).any())


COUNTS = [0, 1, 1023, 16384, 16389, 40000]


def _vals(count):
    return torch.rand(max(count, 1), dtype=torch.float64, generator=torch.Generator().manual_seed(count + 1)) + 0.25


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 10007])
def test_adam_flat_sum_is_adam_flat_and_a_sum(n):
    """satrans_adam_flat_sum for every count in COUNTS, in both arithmetics: p, m and v are the bits of satrans_adam_flat, and out[0],
    which starts at 0.5, grows by math.fsum(vals[:count]) to 1e-12 relative (a double sum of positive terms in a fixed order: at most
    40,000 * 2^-53 relative) - by exactly nothing when count = 0."""
    lib = N.lib()
    g_ = torch.Generator().manual_seed(n)
    alloc = max(n, 1)
    p, g, m, v = (torch.randn(alloc, generator=g_) * 0.05, torch.randn(alloc, generator=g_) * 1e-3,
                  torch.randn(alloc, generator=g_) * 1e-3, torch.rand(alloc, generator=g_) * 1e-6)
    for arith in ARITHS:
        a = [x.to(DEV) for x in (p, g, m, v)]
        N.check(lib.satrans_adam_flat(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), n, C.byref(hp(arith, 0.0)),
                                      stream()), "adam_flat")
        want = [x.cpu() for x in a]
        assert n == 0 or not same_bits(want[0], p)
        for count in COUNTS:
            vals = _vals(count)
            vals_d, out = vals.to(DEV), torch.full((1,), 0.5, dtype=torch.float64, device=DEV)
            b = [x.to(DEV) for x in (p, g, m, v)]
            N.check(lib.satrans_adam_flat_sum(b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(), n,
                                              C.byref(hp(arith, 0.0)), vals_d.data_ptr(), count, out.data_ptr(), stream()),
                    "adam_flat_sum")
            assert all(same_bits(x.cpu(), y) for x, y in zip(b, want)), (arith, count)
            grew = float(out.item()) - 0.5
            assert grew == pytest.approx(math.fsum(vals[:count].tolist()), rel=1e-12, abs=0.0), (arith, count)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("count", COUNTS)
def test_sum_f64(count, accumulate):
    """satrans_sum_f64 over counts below, at and beyond the sixteen-deep strided loop of 1024 lanes: math.fsum to 1e-12 relative,
    written over out[0] (which starts at 0.5) or added to it."""
    vals = _vals(count)
    out = torch.full((1,), 0.5, dtype=torch.float64, device=DEV)
    got = sum_f64(vals.to(DEV), count=count, out=out, accumulate=accumulate)
    assert got == pytest.approx(math.fsum(vals[:count].tolist()) + (0.5 if accumulate else 0.0), rel=1e-12, abs=0.0)


def test_lazy_mark_sets_the_distinct_rows():
    """satrans_embed_lazy_mark on `off_by_one`: last == t exactly on its distinct rows, the sentinel everywhere else."""
    L = layout("off_by_one")
    last = torch.full((E.R,), SENTINEL, dtype=torch.int32, device=DEV)
    N.check(N.lib().satrans_embed_lazy_mark(L.rows_d.data_ptr(), L.n, last.data_ptr(), T, stream()), "lazy_mark")
    want = torch.full((E.R,), SENTINEL, dtype=torch.int32)
    want[L.distinct] = T
    assert torch.equal(last.cpu(), want) and int((want == T).sum()) == len(E.LAYOUTS["off_by_one"])


# ---- section 6: many steps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2", [0.0, 1e-5])
def test_two_hundred_steps_of_both_arithmetics(l2):
    """T = 200 steps of satrans_adam_flat on E.many_step_problem() (n = 4096, lr = 0.005, about 30 % of the gradients exactly zero), the
    bias corrections set per step as the engine forms them, against fp64 Adam on the same sequence with the hyper-parameters as the
    kernels see them:
        max |p_T - p64_T| <= 4 * e32 + (fast ? T * 3.2e-7 * lr : 0)
    e32 is what float32 rounding alone costs on this sequence: torch.optim.Adam in float32 on the CPU against the fp64 restatement
    of torch's own step, 1.74e-7 at l2 = 0 and 1.69e-7 at l2 = 1e-5, measured by tests/test_embed_adam_cpu.py and pinned as E.E32 =
    1.8e-7 / 1.7e-7 - not taken from the kernels.  The factor 4: hipcc contracts m + w (g - m) into an fma where torch's CPU lerp
    may not, up to an ulp of m per step (test_optimizer_kernels_exact).  3.2e-7 lr per step is adam_core_fast's own stated bound.
    The bounds, 7.2e-7 and 1.04e-6 at l2 = 0, are 1.2e-5 and 1.8e-5 of the parameters' mean movement of 0.058: a misplaced eps, a
    wrong bias correction or reciprocal misses them.  (The kernels' weights 1 - beta are restated as make_adamk forms them, from the
    float32 betas; against torch's weights they would be 1.8e-6 off: test_what_the_weights_from_float32_betas_cost.)
    At l2 = 0 the gradients do not depend on p and both arithmetics form the moments with the same instructions: m and v of the two
    are equal bit for bit after every 50th step.
    Seen: 1.62e-7 (exact) and 1.38e-7 (fast) at l2 = 0; 1.53e-7 and 1.49e-7 at l2 = 1e-5."""
    lib, M = N.lib(), E.MANY
    assert (M["lr"], M["b1"], M["b2"], M["eps"]) == (LR, B1, B2, EPS)
    p0, grads = E.many_step_problem()
    want = E.many_step_reference(l2)
    grads_d = grads.to(DEV)
    snaps = {}
    for arith in ARITHS:
        p, m, v = p0.to(DEV), torch.zeros(M["n"], device=DEV), torch.zeros(M["n"], device=DEV)
        for t in range(1, M["T"] + 1):
            N.check(lib.satrans_adam_flat(p.data_ptr(), grads_d[t - 1].data_ptr(), m.data_ptr(), v.data_ptr(), M["n"],
                                          C.byref(hp(arith, l2, t)), stream()), "adam_flat")
            if t % 50 == 0:
                snaps[arith, t] = (m.cpu(), v.cpu())
        err = float((p.cpu().double() - want).abs().max())
        bound = 4 * E.E32[l2] + (M["T"] * 3.2e-7 * M["lr"] if arith == "fast" else 0.0)
        print(f"many steps l2={l2} {arith}: max |p_T - p64_T| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (err, bound)
    if l2 == 0.0:
        for t in (50, 100, 150, 200):
            assert all(same_bits(a, b) for a, b in zip(snaps["exact", t], snaps["fast", t])), t
