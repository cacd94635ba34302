"""Torch twin of a TableAdam run over FeatureEmbedding and LinearModel  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The two modules are tests/input_reference.py's restatement (generic in dtype) over `nn.Parameter`s; the regulariser is in the
loss as the reference has it, `sum(l2 * p * p)` over the embedding tables (l2_reg_embedding) and over the linear tables and
`weight` (l2_reg_linear); `torch.optim.Adam` steps all of them, and a StepLR halves the rate after step 5.

The loss is linear on purpose: `(emb * W).sum() + (logit * c).sum()` with W, c uniform in [0.5, 1.5], drawn once per batch, so
that a touched row's gradient is never near zero (Adam divides by sqrt(v) + 1e-8: a gradient of the size of fp32 noise is
amplified by lr / eps; with a head in the loop the fp32 twin itself leaves the project's bound).

Also here: the columns and the batches that the CPU and GPU tests share.  A draw is redrawn when, in the fp64 twin at any step,
two valid slots of a `max` list lie within 1e-6 of each other (the gradient would depend on rounding); the fp64 twin alone
decides that."""
from __future__ import annotations

import functools
from typing import Dict, Tuple

import torch

from tests import input_reference as R
from tests import varlen_reference as V

Tensor = torch.Tensor
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
STEPS, HALVE_AFTER = 9, 5
TIE_GAP = 1e-6


def columns(D: int):
    """a (7 rows), b (50), c (5000), d on c's table, a mean list masked by id != 0, a max list with a length column, two dense."""
    from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    return [SparseFeat("a", 7, embedding_dim=D), SparseFeat("b", 50, embedding_dim=D), SparseFeat("c", 5000, embedding_dim=D),
            SparseFeat("d", 5000, embedding_dim=D, embedding_name="c"),
            VarLenSparseFeat(SparseFeat("h1", 300, embedding_dim=D), maxlen=3, combiner="mean"),
            VarLenSparseFeat(SparseFeat("h2", 41, embedding_dim=D), maxlen=4, combiner="max", length_name="h2_len"),
            DenseFeat("p", 1), DenseFeat("q", 1)]


def min_max_gap(P: Dict[str, Tensor], X: Tensor, spec: R.InputSpec) -> float:
    """The smallest distance between the two largest VALID slots of a max-pooled list, over samples and elements."""
    gap = float("inf")
    for n, v in spec.varlen:
        if v.combiner != "max" or v.maxlen < 2:
            continue
        E = P[R.key(n)].detach()[X[:, v.col:v.col + v.maxlen].long()].double()
        valid = V.slot_mask(X, v).unsqueeze(-1)
        w = torch.where(valid, E, torch.full_like(E, -float("inf")))
        top = w.topk(2, dim=1)[0]
        d = top[:, 0] - top[:, 1]
        d = d[torch.isfinite(d)]
        if d.numel():
            gap = min(gap, float(d.min()))
    return gap


def train(Pl, Pe, batches, spec, dtype, l2, steps=None, lr=LR, halve_after=HALVE_AFTER):
    """-> (linear parameters, embedding tables, smallest max-list gap seen) after one Adam step per batch."""
    Ll = {k: torch.nn.Parameter(t.detach().to(dtype).clone()) for k, t in Pl.items()}
    Le = {k: torch.nn.Parameter(t.detach().to(dtype).clone()) for k, t in Pe.items()}
    opt = torch.optim.Adam(list(Ll.values()) + list(Le.values()), lr=lr, betas=BETAS, eps=EPS)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=halve_after, gamma=0.5)
    gap = float("inf")
    for X, W, c in batches[:steps]:
        gap = min(gap, min_max_gap(Ll, X, spec), min_max_gap(Le, X, spec))
        opt.zero_grad(set_to_none=True)
        loss = (R.lookup(Le, X, spec)[0] * W.to(dtype)).sum() + (R.linear(Ll, X, spec) * c.to(dtype).reshape(-1, 1)).sum()
        for p in Le.values():
            loss = loss + torch.sum(l2 * p * p)
        for p in Ll.values():
            loss = loss + torch.sum(l2 * p * p)
        loss.backward()
        opt.step()
        sched.step()
    return {k: p.detach() for k, p in Ll.items()}, {k: p.detach() for k, p in Le.items()}, gap


def _draw(cols, fi, B, D, seed, constant_a):
    g = torch.Generator().manual_seed(seed)
    Pl, Pe = R.draw_params(cols, D, g)
    F = 6
    batches = []
    for _ in range(STEPS):
        X = R.draw_X(cols, fi, B, g)
        if constant_a:
            X[:, fi["a"][0]] = 3.0      # a run of B equal rows in the sorted list
        batches.append((X, torch.rand(B, F, D, generator=g) + 0.5, torch.rand(B, generator=g) + 0.5))
    return Pl, Pe, batches


@functools.lru_cache(maxsize=None)
def draw(D: int, B: int = 64, constant_a: bool = False, seed: int = 11):
    """-> (cols, fi, spec, Pl, Pe, batches of (X, W, c)); left unchanged by everyone.  Redrawn (next seed) while the fp64 twin, at
    either l2 of the tests, meets a near-tie under max."""
    from satrans_amd.inputs import build_input_features
    cols = columns(D)
    fi = build_input_features(cols)
    spec = R.spec_of(cols, fi)
    for attempt in range(8):
        Pl, Pe, batches = _draw(cols, fi, B, D, seed + 1000 * attempt, constant_a)
        if all(train(Pl, Pe, batches, spec, torch.float64, l2)[2] >= TIE_GAP for l2 in (0.0, 1e-5)):
            return cols, fi, spec, Pl, Pe, batches
    raise AssertionError("eight draws in a row come within 1e-6 of a tie under max")


@functools.lru_cache(maxsize=None)
def twin(D: int, l2: float, dtype) -> Tuple[Dict[str, Tensor], Dict[str, Tensor]]:
    """The parameters after the nine steps in `dtype`, computed once per (D, l2, dtype)."""
    _cols, _fi, spec, Pl, Pe, batches = draw(D)
    Ll, Le, _ = train(Pl, Pe, batches, spec, dtype, l2)
    return Ll, Le


def worst_ratio(got: Dict[str, Tensor], want: Dict[str, Tensor]) -> float:
    """max over the parameters of max|got - want| / (GRAD_REL max|want| + GRAD_ABS)."""
    worst = 0.0
    for k, w in want.items():
        w = w.double()
        err = float((got[k].double().cpu() - w).abs().max())
        worst = max(worst, err / (R.GRAD_REL * float(w.abs().max()) + R.GRAD_ABS))
    return worst
