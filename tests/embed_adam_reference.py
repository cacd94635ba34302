"""fp64 restatements of what csrc/embed_adam.hip computes, and the id lists its ordered sum is tested on.

Everything here is float64 torch on the CPU.  The hyper-parameters are the float32 numbers the kernels receive: the host forms
`lr_over_bc1`, `bc2_sqrt`, `float32(l2)` and `2 * float32(l2)` (engine._hparams, make_adamk), and the restatement takes them the same
way (the weights 1 - beta included, which make_adamk forms from the float32 betas), so the only difference between a kernel and its
restatement is the kernel's own rounding.  `fp32=False` keeps the python doubles
instead: that is the form torch.optim's float64 step takes, which tests/test_embed_adam_cpu.py pins the restatement against.

The id lists: `LAYOUTS` maps a name to run lengths.  A run is a stretch of equal ids in the sorted list, so its length and start
decide which chunk (kChunk = 16 positions) and superchunk (kSuper = 16 chunks) boundaries it crosses."""
import math
from collections import namedtuple

import numpy as np
import torch

K = 16            # kChunk: sorted positions per lane group
S = 16 * K        # a superchunk: kSuper chunks
R = 4099          # arena rows of the tests: no multiple of the bitmap word (32)
DIMS = (16, 32, 64, 128)

HP = namedtuple("HP", "lr_over_bc1 bc2_sqrt w1 beta2 w2 eps l2 l2x2")
SGD, ADAGRAD, RMSPROP = 1, 2, 3      # SATRANS_OPT_*


def f32(x):
    return float(np.float32(x))


def hparams(lr, b1, b2, eps, l2, t, fp32=True, weights="kernel"):
    """Step t's constants.  fp32: rounded where the host and make_adamk round them.  The weights 1 - beta, weights = "kernel": as
    make_adamk forms them, in double from the float32 beta of the hyper-parameter struct and rounded once.  weights = "torch": as
    torch applies them to a float32 tensor, float32(1 - beta) from the optimizer's double.  The two differ: 1 - float32(0.999) is
    1.3e-5 below float32(0.001) (tests/test_embed_adam_cpu.py measures what that costs)."""
    r = f32 if fp32 else float
    l2r = r(l2)
    w1, w2 = (r(1.0 - r(b1)), r(1.0 - r(b2))) if weights == "kernel" else (r(1.0 - b1), r(1.0 - b2))
    return HP(r(lr / (1.0 - b1 ** t)), r(math.sqrt(1.0 - b2 ** t)), w1, r(b2), w2, r(eps), l2r, 2.0 * l2r)


def adam_step(p, m, v, g, hp):
    """torch.optim.adam._single_tensor_adam with the regulariser's gradient folded in: g = G + 2 l2 p, exp_avg.lerp_(g, 1 - beta1),
    exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2), denom = sqrt(v) / bc2_sqrt + eps, p.addcdiv_(m, denom, -lr / bc1)."""
    p, m, v, g = (x.double() for x in (p, m, v, g))
    g = g + hp.l2x2 * p
    m = m + hp.w1 * (g - m)
    v = v * hp.beta2 + hp.w2 * g * g
    denom = v.sqrt() / hp.bc2_sqrt + hp.eps
    return p + (-hp.lr_over_bc1) * (m / denom), m, v


def dense_grad(rows, gemb, n_rows):
    """index_add of the gathered rows' gradients: out[rows[i]] += gemb[i]."""
    return torch.zeros(n_rows, gemb.shape[1], dtype=torch.float64).index_add_(0, rows.long(), gemb.double())


def other_step(kind, p, s, g, lr, alpha, eps, fp32=True):
    """torch.optim.SGD / Adagrad / RMSprop in their plain forms (no momentum, no decay): -> (p', s').  SGD passes `s` through."""
    r = f32 if fp32 else float
    p, g = p.double(), g.double()
    lr, eps = r(lr), r(eps)
    if kind == SGD:
        return p - lr * g, s
    s = s.double()
    if kind == ADAGRAD:
        s = s + g * g
    else:
        a = r(alpha)
        # the kernel forms 1 - alpha from the float32 alpha; torch applies float32(1 - alpha) from the double, 9.3e-7 larger for
        # alpha = 0.99 (tests/test_embed_adam_cpu.py::test_what_the_rmsprop_weight_costs)
        s = a * s + r(1.0 - a) * g * g
    return p - lr * (g / (s.sqrt() + eps)), s


def reg(p, l2):
    """The reference's regulariser of a table: float32(l2) * sum(p^2)."""
    return f32(l2) * math.fsum((p.double() ** 2).flatten().tolist())


# ---- run layouts -------------------------------------------------------------------------------------------------------------------
def _mixture():
    rng = np.random.RandomState(1234)
    runs = rng.geometric(1.0 / 8.0, 2500).tolist()
    for at, length in ((300, 33), (900, 64), (1500, 700), (2100, 1500)):
        runs.insert(at, length)
    return runs


LAYOUTS = {
    "one": [1],
    "short": [3, 1, 5],
    "distinct": [1] * 1000,
    "aligned": [16, 240, 256, 512, 16, 16, 224, 1],
    "off_by_one": [15, 2, 15, 17, 207, 257, 255, 1, 513, 31],
    "edge_of_super": [255, 2, 254, 1, 770],
    "one_row": [5000],
    "two_giants": [2500, 2500],
    "mixture": _mixture(),
}
# the layouts whose first run is row 0 and whose last run is row R - 1; every other layout leaves both rows out
WITH_END_ROWS = ("short", "off_by_one", "mixture")


def layout_rows(name):
    """-> (sorted_rows [n] int32, src [n] int32): run i holds the i-th of a seeded ascending choice of distinct rows, and `src` is a
    seeded permutation of 0..n-1, so the gradient rows lie in unsorted order as they do in a step."""
    runs = LAYOUTS[name]
    rng = np.random.RandomState(100 + sorted(LAYOUTS).index(name))
    ids = np.sort(rng.choice(np.arange(1, R - 1), size=len(runs), replace=False))
    if name in WITH_END_ROWS:
        ids[0], ids[-1] = 0, R - 1
    rows = np.repeat(ids, runs).astype(np.int32)
    src = rng.permutation(rows.size).astype(np.int32)
    return torch.from_numpy(rows), torch.from_numpy(src)


def run_bounds(name):
    """-> [(start, end)] of every run, end exclusive."""
    ends = np.cumsum(LAYOUTS[name])
    return list(zip((ends - LAYOUTS[name]).tolist(), ends.tolist()))


def step_blocks(n, D):
    """Workgroups of the three stepping bodies of one launch, by the kernels' own counts: (spans, finish, apply)."""
    lpr, chunks = D // 4, -(-n // K)
    supers = -(-chunks // 16)
    return -(-supers * lpr // 256), -(-chunks * lpr // 256), -(-n * lpr // 256)


def exact_grads(n, D, seed):
    """Integers in [-8, 8] times 2^-20: every sum of them is exact in float32 in any order (5,000 of them need 16 bits)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (n, D), generator=g).float() * 2.0 ** -20


def tables(n_rows, D, seed):
    """-> P, M, V [n_rows, D] float32 at the scales of a running model."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n_rows, D, generator=g) * 1e-2, torch.randn(n_rows, D, generator=g) * 1e-4,
            torch.rand(n_rows, D, generator=g) * 1e-8)


# ---- the many-step problem ---------------------------------------------------------------------------------------------------------
MANY = dict(T=200, n=4096, lr=0.005, b1=0.9, b2=0.999, eps=1e-8)
# e32 of the many-step bound, by l2: what float32 rounding alone costs over the sequence - the largest |p32 - p64| of any element after
# any step, p32 from torch.optim.Adam in float32 on the CPU and p64 from adam_step with torch's own weights (weights = "torch").
# Measured 1.74e-7 (l2 = 0) and 1.69e-7 (l2 = 1e-5) by tests/test_embed_adam_cpu.py, which holds the pin to the measurement.
E32 = {0.0: 1.8e-7, 1e-5: 1.7e-7}


def many_step_problem():
    """-> (p0 [n], grads [T, n]) float32: a fixed seeded sequence, about 30 % of the gradients exactly zero."""
    g = torch.Generator().manual_seed(77)
    T, n = MANY["T"], MANY["n"]
    p0 = torch.randn(n, generator=g) * 0.05
    grads = torch.randn(T, n, generator=g) * 1e-3
    grads[torch.rand(T, n, generator=g) < 0.3] = 0.0
    return p0, grads


def many_step_reference(l2, weights="kernel"):
    """fp64 Adam over the sequence, bias corrections formed per step as the engine forms them -> p_T (float64)."""
    p0, grads = many_step_problem()
    p, m, v = p0.double(), torch.zeros(MANY["n"], dtype=torch.float64), torch.zeros(MANY["n"], dtype=torch.float64)
    for t in range(1, MANY["T"] + 1):
        p, m, v = adam_step(p, m, v, grads[t - 1], hparams(MANY["lr"], MANY["b1"], MANY["b2"], MANY["eps"], l2, t, weights=weights))
    return p
