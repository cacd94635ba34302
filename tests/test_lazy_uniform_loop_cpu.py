"""CPU side of the lazy replay's fast loop (embed_adam.hip: adam_step4_fast, stage_steps).

1. The fast step of the lazy forms takes the regulariser-only gradient as `2*l2*p`; the other kernel forms spell it
   `0 + 2*l2*p`.  The sum only turns a -0 product into +0.  A numpy-fp32 restatement of the step, with and without it, must
   give the same bits in every output - over the cross product of the values where a sign of zero could matter and over 10^6
   random bit patterns.
2. The step constants a workgroup stages are the fp32 values of the table's doubles, and those are the constants the streaming
   kernel derives from `satrans_adam_hparams` at the same step.
"""
import itertools
import math

import numpy as np

F32 = np.float32
LR, B1, B2, EPS = 0.005, 0.9, 0.999, 1e-8
STAGED = 128                                # kStagedSteps


def fma32(a, b, c):
    """Correctly rounded fp32 a * b + c: the product of two fp32 values is exact in fp64; the fp64 sum is made round-to-odd with
    the exact error of the addition (TwoSum), after which the rounding to fp32 is the rounding of the exact result."""
    a, b, c = (np.asarray(x, dtype=F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        ab = a * b
        s = ab + c
        bb = s - ab
        err = (ab - (s - bb)) + (c - bb)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        even = (s.view(np.int64) & 1) == 0
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        return np.where(inexact & even, odd, s).astype(F32)


def fast_step(p, m, v, l2, neg_step, rbc2f, add_zero):
    """One regulariser-only step of adam_step4_fast for arrays of elements, every operation rounded to fp32 as the packed
    instructions round it.  The hardware square root and reciprocal are functions of their operand's bits alone; they are
    restated as numpy's (a subnormal second moment counts as zero), which is all a comparison of two spellings needs."""
    p, m, v = (np.asarray(x, dtype=F32) for x in (p, m, v))
    w1, beta2, w2 = F32(1.0 - float(F32(B1))), F32(B2), F32(1.0 - float(F32(B2)))
    l2x2 = F32(2.0) * F32(l2)
    with np.errstate(all="ignore"):
        sq = fma32(p, p, F32(0.0))
        g = l2x2 * p
        if add_zero:
            g = F32(0.0) + g
        m = fma32(w1, g - m, m)
        v = fma32(w2 * g, g, v * beta2)
        a = F32(neg_step) * m
        root = np.sqrt(np.where(np.abs(v) < F32(2.0 ** -126), F32(0.0), v))
        den = fma32(root, F32(rbc2f), F32(EPS))
        p = fma32(a, F32(1.0) / den, p)
    return p, m, v, sq, g


def step_constants(s):
    """(neg_step, rbc2f) of step s as the streaming kernel's make_adamk derives them from the engine's hyper-parameters."""
    lr_over_bc1 = F32(LR / (1.0 - B1 ** s))                     # satrans_adam_hparams.lr_over_bc1 (a C float)
    bc2_sqrt = F32(math.sqrt(1.0 - B2 ** s))                    # ... .bc2_sqrt
    return -lr_over_bc1, F32(1.0 / float(bc2_sqrt))             # k.neg_step, k.rbc2f = (float)(1.0 / (double)bc2_sqrt)


def table(upto):
    """The engine's table of step constants: (fp32(lr / (1 - beta1^s)), 1 / fp32(sqrt(1 - beta2^s))) as doubles, row 0 unused."""
    f32 = lambda x: float(F32(x))
    return np.array([(0.0, 1.0)] + [(f32(LR / (1.0 - B1 ** s)), 1.0 / f32(math.sqrt(1.0 - B2 ** s))) for s in range(1, upto + 1)],
                    dtype=np.float64)


def stage_steps(tab, target):
    """stage_steps of embed_adam.hip: thread i < 128 converts step target - i when that is at least 1."""
    staged = {}
    for i in range(STAGED):
        s = target - i
        if s >= 1:
            staged[i] = (-F32(tab[s, 0]), F32(tab[s, 1]))
    return staged


def bits(x):
    return np.asarray(x, dtype=F32).view(np.uint32)


def assert_same_step(p, m, v, l2, s):
    neg_step, rbc2f = step_constants(s)
    with_zero = fast_step(p, m, v, l2, neg_step, rbc2f, True)
    without = fast_step(p, m, v, l2, neg_step, rbc2f, False)
    for name, a, b in zip(("p", "m", "v", "sq"), with_zero, without):
        differ = bits(a) != bits(b)
        assert not differ.any(), (f"{name}: {int(differ.sum())} outputs change without the `0 +` (l2={l2}, step {s}); first at "
                                  f"p={p[differ][0]!r} m={m[differ][0]!r} v={v[differ][0]!r}")
    return with_zero[4], without[4]


def test_fast_step_is_the_same_without_the_added_zero_on_the_values_where_a_zero_sign_matters():
    big, sub = np.finfo(F32).max, F32(2.0 ** -149)
    vals = np.array([0.0, -0.0, sub, 1e-30, 1.0, -1.0, big], dtype=F32)
    nonneg = np.array([0.0, sub, 1e-30, 1.0, big], dtype=F32)
    grid = np.array(list(itertools.product(vals, vals, nonneg)), dtype=F32)
    assert grid.shape == (7 * 7 * 5, 3)
    zero_signs_seen = 0
    for l2 in (0.0, 1e-5):
        for s in (1, 7, 200):
            g_with, g_without = assert_same_step(grid[:, 0].copy(), grid[:, 1].copy(), grid[:, 2].copy(), l2, s)
            zero_signs_seen += int((bits(g_with) != bits(g_without)).sum())
    # the two spellings do differ in the gradient itself (-0 against +0), or the comparison would be vacuous
    assert zero_signs_seen > 0


def test_fast_step_is_the_same_without_the_added_zero_on_random_bit_patterns():
    rng = np.random.RandomState(5)
    n = 1_000_000
    p = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(F32)
    m = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(F32)
    v = rng.randint(0, 2 ** 31, size=n, dtype=np.uint64).astype(np.uint32).view(F32)        # sign bit clear: v >= 0 (or NaN)
    for l2 in (0.0, 1e-5):
        assert_same_step(p, m, v, l2, 7)


def test_staged_constants_are_the_fp32_values_of_the_table_and_the_streaming_kernels_constants():
    upto = 400
    tab = table(upto)
    for target in (1, 5, 127, 128, 129, 210, upto):
        staged = stage_steps(tab, target)
        assert sorted(staged) == list(range(min(STAGED, target)))
        for i, (neg_step, rbc2f) in staged.items():
            s = target - i
            assert neg_step.dtype == F32 and rbc2f.dtype == F32
            assert bits(neg_step) == bits(F32(-tab[s, 0])) and bits(rbc2f) == bits(F32(tab[s, 1]))
            # the conversion loses nothing of the first column (it holds fp32 values) and rounds the second once, as make_adamk does
            assert float(-neg_step) == tab[s, 0]
            want = step_constants(s)
            assert bits(neg_step) == bits(want[0]) and bits(rbc2f) == bits(want[1]), s
        # a wave whose oldest row is at `first - 1` takes the staged steps when all of (first - 1, target] are there
        for first in range(max(1, target - 140), target + 2):
            if first >= 1 and target - first < STAGED:
                assert all((target - s) in staged for s in range(first, target + 1))
