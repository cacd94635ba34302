"""satrans_embed_lazy_replay_reg64 / satrans_embed_lazy_flush_reg64 against the calls they restate (csrc/embed_adam.hip): the same
arena, moments and `last` bit for bit in both arithmetics, and partial sums of the regulariser that equal l2 * sum(p^2) over the
replayed steps formed in double - checked against a host fp64 sum over the arenas the plain calls leave step by step."""
import ctypes as C

import numpy as np
import pytest
import torch

from satrans_amd import native as N
from satrans_amd.optim import ARITH, StepTable

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, TARGET = 301, 7                # several blocks of the replay at D = 32; rows 0 to 7 steps behind
L2 = float(np.float32(1e-3))         # (the kernels take l2 as a float)


def hparams(arith):
    h = N.AdamHParams()
    h.beta1, h.beta2, h.eps, h.l2, h.arith = 0.9, 0.999, 1e-8, L2, ARITH[arith]
    return h


def problem(D):
    g = torch.Generator().manual_seed(5 + D)
    P = (0.5 * torch.randn(ROWS, D, generator=g)).to(DEV)
    M = (0.01 * torch.randn(ROWS, D, generator=g)).to(DEV)
    V = (1e-4 * torch.rand(ROWS, D, generator=g)).to(DEV)
    last = torch.randint(0, TARGET + 1, (ROWS,), generator=g, dtype=torch.int32).to(DEV)
    steps = StepTable((0.9, 0.999))
    steps.note(1, 1e-2)
    return P, M, V, last, steps.device(TARGET, DEV)


def flush(name, state, table, arith, target=TARGET):
    P, M, V, last = (t.clone() for t in state)
    reg = torch.zeros(4096, dtype=torch.float64, device=DEV)
    h = hparams(arith)
    N.check(getattr(N.lib(), name)(P.data_ptr(), M.data_ptr(), V.data_ptr(), last.data_ptr(), ROWS, P.shape[1], target, table.data_ptr(),
                                   C.byref(h), 0, reg.data_ptr(), torch.cuda.current_stream().cuda_stream), name)
    return P, M, V, last, float(reg.sum())


def stepwise_reg(state, table, arith):
    """l2 * sum(p^2) in fp64 over every replayed step, from the arenas the plain flush leaves at targets 1 .. TARGET."""
    total, cur = 0.0, state
    for t in range(1, TARGET + 1):
        behind = (cur[3] < t).to(torch.float64).unsqueeze(1)
        total += L2 * float((cur[0].double() ** 2 * behind).sum())
        cur = flush("satrans_embed_lazy_flush", cur, table, arith, t)[:4]
    return total


@pytest.mark.parametrize("arith", ("fast", "exact"))
@pytest.mark.parametrize("D", (16, 32))
def test_flush(D, arith):
    *state, table = problem(D)
    plain = flush("satrans_embed_lazy_flush", state, table, arith)
    wide = flush("satrans_embed_lazy_flush_reg64", state, table, arith)
    for a, b in zip(plain[:4], wide[:4]):
        assert torch.equal(a, b)
    assert bool((wide[3] == TARGET).all())
    want = stepwise_reg(state, table, arith)
    print(f"D={D} {arith}: reg64 {wide[4]!r} fp64 {want!r} rel {abs(wide[4] - want) / want:.2e}; fp32 form rel {abs(plain[4] - want) / want:.2e}")
    assert abs(wide[4] - want) <= 1e-12 * want            # the same doubles in another grouping
    assert abs(plain[4] - want) <= 1e-6 * want


@pytest.mark.parametrize("arith", ("fast", "exact"))
@pytest.mark.parametrize("D", (16, 32))
def test_replay(D, arith):
    *state, table = problem(D)
    g = torch.Generator().manual_seed(9)
    rows = torch.sort(torch.randint(0, ROWS, (700,), generator=g, dtype=torch.int32)).values.to(DEV)      # runs of equal rows
    n = rows.numel()
    out = {}
    for name in ("satrans_embed_lazy_replay", "satrans_embed_lazy_replay_reg64"):
        P, M, V, last = (t.clone() for t in state)
        reg = torch.full((int(N.lib().satrans_embed_lazy_reg_partials(n, D)),), 3.0, dtype=torch.float64, device=DEV)
        h = hparams(arith)
        N.check(getattr(N.lib(), name)(P.data_ptr(), M.data_ptr(), V.data_ptr(), last.data_ptr(), D, rows.data_ptr(), n, TARGET,
                                       table.data_ptr(), C.byref(h), reg.data_ptr(), torch.cuda.current_stream().cuda_stream), name)
        slots = (n * D + 255) // 256
        assert bool((reg[slots:] == 3.0).all())             # the flush's slots stay as they were
        out[name] = (P, M, V, last, float(reg[:slots].sum()))
    plain, wide = out["satrans_embed_lazy_replay"], out["satrans_embed_lazy_replay_reg64"]
    for a, b in zip(plain[:4], wide[:4]):
        assert torch.equal(a, b)
    touched = torch.zeros(ROWS, dtype=torch.bool, device=DEV)
    touched[rows.long()] = True
    assert bool((wide[3][touched] == TARGET).all()) and torch.equal(wide[3][~touched], state[3][~touched])
    assert torch.equal(wide[0][~touched], state[0][~touched])
    # the rows of the batch, replayed alone by the flush on an arena in which every other row is already current
    only = (state[0], state[1], state[2], torch.where(touched, state[3], torch.full_like(state[3], TARGET)))
    want = stepwise_reg(only, table, arith)
    assert abs(wide[4] - want) <= 1e-12 * want and abs(plain[4] - want) <= 1e-6 * want
