"""The lazy replay's fast loop is one loop per WAVE (embed_adam.hip: replay_element4): a scalar step counter from the wave's
smallest `from`, a lane joining once the counter has passed its own, the step constants converted to fp32 once per workgroup for
the last 128 steps.  These tests hold `satrans_embed_lazy_flush` and `satrans_embed_lazy_replay` bit for bit against the same
steps taken one launch at a time by the streaming kernel, on tables whose `last[]` puts every mixture of pending steps into one
wave."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T = 210                       # the step every row is brought to
STAGED = 128                  # kStagedSteps of embed_adam.hip
OLDEST = T - 200              # the row 200 steps behind: beyond the staged steps, its wave takes the loop that reads the table
LR_, B1, B2, EPS = 0.005, 0.9, 0.999, 1e-8
STREAM_SLOTS = 2048           # partial sums of the streaming kernel (kStreamBlocks)
FLUSH_SLOTS = 4096            # ... and of the flush (kFlushBlocks)


def _last(R, D, g):
    """`last[]` by wave: a wave of either kernel form holds 256 / D consecutive rows (positions).  Eight kinds of wave, cycled:
    0 every row the same `from`; 1 every `from` different; 2 nothing to do (from == T): an empty wave; 3 from == T - 1;
    4 nothing / one step / a few steps mixed; 5 one row 200 steps behind among recent ones; 6 the oldest `from` the staged
    steps still cover (T - 128); 7 one step older than that in one row."""
    rpw = 256 // D
    last = torch.empty(R, dtype=torch.int32)
    for w in range((R + rpw - 1) // rpw):
        lo, hi = w * rpw, min(R, (w + 1) * rpw)
        n, kind = hi - lo, w % 8
        if kind == 0:
            row = torch.full((n,), T - 7)
        elif kind == 1:
            row = T - 1 - torch.arange(n)
        elif kind == 2:
            row = torch.full((n,), T)
        elif kind == 3:
            row = torch.full((n,), T - 1)
        elif kind == 4:
            row = T - torch.tensor([0, 1, 30, 0, 2, 1, 0, 17])[torch.randint(0, 8, (n,), generator=g)]
        elif kind == 5:
            row = torch.full((n,), T - 3)
            row[int(torch.randint(0, n, (1,), generator=g))] = OLDEST
        elif kind == 6:
            row = torch.full((n,), T - STAGED)
        else:
            row = torch.full((n,), T - STAGED)
            row[int(torch.randint(0, n, (1,), generator=g))] = T - STAGED - 1
        last[lo:hi] = row.to(torch.int32)
    return last


def _state(R, D, g):
    """Ordinary table values with +-0, subnormals, 1e-30 and large magnitudes mixed into the same lanes, rows that are decaying
    (magnitudes log-uniform from 1e-8 through the subnormals, as in test_lazy_flush_equals_streaming_steps_on_edge_values) and
    whole rows of signed zeros.  Every |p| stays below 1e15, so that p^2 is finite in fp32 (the lazy form's regulariser term)."""
    P = torch.randn(R, D, generator=g) * 1e-4
    M = torch.randn(R, D, generator=g) * 1e-9
    V = torch.rand(R, D, generator=g) * 1e-17
    odd = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 3e-39, 1e-30, -1e-30, 1e15, -3e12, 1.0, 1e-12], dtype=torch.float32)
    pick = torch.randint(0, odd.numel(), (R, D), generator=g)
    P = torch.where(torch.rand(R, D, generator=g) < 0.05, odd[pick], P)
    M = torch.where(torch.rand(R, D, generator=g) < 0.03, odd[pick.flip(1)] * 1e-6, M)
    V = torch.where(torch.rand(R, D, generator=g) < 0.03, odd[pick].abs() ** 2, V)

    def tiny(lo_exp, hi_exp):
        u = torch.rand(R, D, generator=g, dtype=torch.float64) * (hi_exp - lo_exp) + lo_exp
        sign = torch.where(torch.rand(R, D, generator=g) < 0.5, -1.0, 1.0).double()
        return (sign * torch.pow(torch.tensor(10.0, dtype=torch.float64), u)).to(torch.float32)
    kind = torch.rand(R, 1, generator=g).expand(R, D)
    decayed, zero_row = (kind >= 0.5) & (kind < 0.8), kind >= 0.8
    P = torch.where(decayed, tiny(-46.0, -8.0), P)
    M = torch.where(decayed, tiny(-47.0, -13.0), M)
    V = torch.where(decayed, tiny(-46.0, -17.0).abs(), V)
    signed_zero = lambda: torch.where(torch.rand(R, D, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    P = torch.where(zero_row, signed_zero(), P)
    M = torch.where(zero_row, signed_zero(), M)
    return P.contiguous(), M.contiguous(), V.contiguous()


def _check_lazy_forms(D, arith, l2, R):
    from satrans_amd import native as N
    lib = N.lib()
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(1000 + D + (7 if arith == "fast" else 0))
    P, M, V = _state(R, D, g)
    last0 = _last(R, D, g)
    assert int(last0.min()) == OLDEST and int((last0 == T).sum()) > 0 and int((last0 == T - 1).sum()) > 0
    f32 = lambda x: float(np.float32(x))
    table = torch.tensor([(0.0, 1.0)] + [(f32(LR_ / (1.0 - B1 ** s)), 1.0 / f32(math.sqrt(1.0 - B2 ** s))) for s in range(1, T + 1)],
                         dtype=torch.float64, device=DEV)

    def hp(t):
        h = N.AdamHParams()
        h.lr_over_bc1, h.bc2_sqrt = LR_ / (1 - B1 ** t), math.sqrt(1 - B2 ** t)
        h.beta1, h.beta2, h.eps, h.l2 = B1, B2, EPS, l2
        h.arith = N.ADAM_FAST if arith == "fast" else N.ADAM_EXACT
        return h

    # ---- reference: step t of the streaming kernel moves the rows with last < t (the others carry the `touched` bit) ----------
    Ps, Ms, Vs = (x.clone().to(DEV) for x in (P, M, V))
    words = (R + 31) // 32
    padded = torch.full((words * 32,), T, dtype=torch.int32, device=DEV)
    padded[:R] = last0.to(DEV)
    weights = (torch.ones(32, dtype=torch.int64, device=DEV) << torch.arange(32, device=DEV))
    regs = torch.zeros(int(lib.satrans_embed_reg_partials(R, 64, D)), dtype=torch.float64, device=DEV)
    reg_ref = torch.zeros((), dtype=torch.float64, device=DEV)
    reg_ref_rows = None
    for t in range(OLDEST + 1, T + 1):
        bits = ((padded >= t).view(words, 32).to(torch.int64) * weights).sum(1)
        touched = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32)
        N.check(lib.satrans_embed_adam_untouched(Ps.data_ptr(), Ms.data_ptr(), Vs.data_ptr(), 0, R, D, touched.data_ptr(),
                                                 C.byref(hp(t)), regs.data_ptr(), 0, st), "untouched")
        reg_ref += regs[:STREAM_SLOTS].sum()
    reg_ref = float(reg_ref)
    steps = int((T - last0).sum())
    # the lazy forms sum p^2 of one element over its <= 200 steps in fp32 (fma, one rounding per term, all terms >= 0): a
    # relative error of at most 201 * 2^-24 of the sum, plus 2^-149 for every term that falls below the fp32 range
    reg_rtol, reg_atol = 201 * 2.0 ** -24, l2 * steps * D * 2.0 ** -149

    def same_bits(a, b, what, sel=None):
        eq = a.view(torch.int32) == b.view(torch.int32)
        if sel is not None:
            eq = eq[sel]
        assert bool(eq.all()), f"{what}: {int((~eq).sum())} elements differ from the streaming steps"

    # ---- flush: every row to T in one launch --------------------------------------------------------------------------------
    Pf, Mf, Vf = (x.clone().to(DEV) for x in (P, M, V))
    last = last0.clone().to(DEV)
    n = 64
    head = (n * D + 255) // 256
    regl = torch.full((int(lib.satrans_embed_lazy_reg_partials(n, D)),), 7.0, dtype=torch.float64, device=DEV)
    N.check(lib.satrans_embed_lazy_flush(Pf.data_ptr(), Mf.data_ptr(), Vf.data_ptr(), last.data_ptr(), R, D, T, table.data_ptr(),
                                         C.byref(hp(T)), n, regl.data_ptr(), st), "flush")
    assert bool((last == T).all())
    for a, b, what in ((Pf, Ps, "p"), (Mf, Ms, "m"), (Vf, Vs, "v")):
        same_bits(a, b, f"flush {what}")
    assert not bool((regl[head:head + FLUSH_SLOTS] == 7.0).any()), "every partial-sum slot of the flush must be written"
    reg_flush = float(regl[head:head + FLUSH_SLOTS].sum())
    print(f"regulariser sum: streaming {reg_ref!r}, flush {reg_flush!r}")
    assert reg_flush == pytest.approx(reg_ref, rel=reg_rtol, abs=reg_atol)

    # ---- replay of a sorted row list with repeats, then a flush of the rest ---------------------------------------------------
    Pr, Mr, Vr = (x.clone().to(DEV) for x in (P, M, V))
    last = last0.clone().to(DEV)
    listed = torch.rand(R, generator=g) < 0.7
    listed[last0 == OLDEST] = True                      # (the rows that take the other loop are in the list)
    rows = torch.cat([torch.nonzero(listed).flatten(), torch.randint(0, R, (R // 2,), generator=g)])
    rows = torch.sort(rows.to(torch.int32)).values.to(DEV)
    listed = torch.zeros(R, dtype=torch.bool)
    listed[rows.cpu().long()] = True
    assert rows.numel() > int(listed.sum()) and not bool(listed.all())
    regr = torch.full((int(lib.satrans_embed_lazy_reg_partials(rows.numel(), D)),), 7.0, dtype=torch.float64, device=DEV)
    N.check(lib.satrans_embed_lazy_replay(Pr.data_ptr(), Mr.data_ptr(), Vr.data_ptr(), last.data_ptr(), D, rows.data_ptr(),
                                          rows.numel(), T, table.data_ptr(), C.byref(hp(T)), regr.data_ptr(), st), "replay")
    slots = (rows.numel() * D + 255) // 256
    assert not bool((regr[:slots] == 7.0).any()), "every partial-sum slot of the replay must be written"
    assert torch.equal(last.cpu(), torch.where(listed, torch.tensor(T, dtype=torch.int32), last0))
    on, off = listed.to(DEV), (~listed).to(DEV)
    for a, b, a0, what in ((Pr, Ps, P, "p"), (Mr, Ms, M, "m"), (Vr, Vs, V, "v")):
        same_bits(a, b, f"replay {what}", on)
        same_bits(a, a0.to(DEV), f"replay {what} (rows not listed must stay as they were)", off)
    reg_replay = float(regr[:slots].sum())
    N.check(lib.satrans_embed_lazy_flush(Pr.data_ptr(), Mr.data_ptr(), Vr.data_ptr(), last.data_ptr(), R, D, T, table.data_ptr(),
                                         C.byref(hp(T)), rows.numel(), regr.data_ptr(), st), "flush of the rest")
    assert bool((last == T).all())
    for a, b, what in ((Pr, Ps, "p"), (Mr, Ms, "m"), (Vr, Vs, "v")):
        same_bits(a, b, f"replay + flush {what}")
    reg_rest = float(regr[slots:slots + FLUSH_SLOTS].sum())
    print(f"regulariser sum: replay {reg_replay!r} + flush of the rest {reg_rest!r}")
    assert reg_replay + reg_rest == pytest.approx(reg_ref, rel=reg_rtol, abs=reg_atol)
    if l2 == 0.0:
        assert reg_ref == 0.0 and reg_flush == 0.0 and reg_replay == 0.0 and reg_rest == 0.0


@pytest.mark.parametrize("l2", [0.0, 1e-5])
@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_lazy_flush_and_replay_are_the_streaming_steps_for_every_mixture_in_a_wave(D, arith, l2):
    """2,531 rows (no multiple of a wave's rows: the last wave is partly past the table)."""
    _check_lazy_forms(D, arith, l2, 2531)


def test_lazy_flush_second_pass_over_the_rows():
    """D = 128: the flush grid covers 4096 * 8 rows in one pass; 37 rows more make some workgroups walk a second one."""
    _check_lazy_forms(128, "fast", 1e-5, 4096 * 8 + 37)
