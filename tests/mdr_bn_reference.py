"""Torch restatement of the partitioned normalisation (one batch-norm per scenario over a mixed batch: the reference's
MDR_BatchNorm, models/submodules.py:107-175, inside the loop of models/star.py:147-154), forward and backward, written from
the arithmetic of F.batch_norm  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Everything runs in the dtype of `x` (fp64 for what the kernels are held against).  Scenario s owns the rows with
`sid == s`; `State` carries the per-scenario parameters and buffers stacked [S,C].

  training statistics   mean and BIASED variance over the scenario's rows, by the two-pass form  sum((x - mean)^2) / n
  y                     (x - mean) / sqrt(var + eps) * (weight[s] * shared_weight) + (bias[s] + shared_bias)
  running update        r = (1 - f) * r + f * stat, the UNBIASED variance (n / (n - 1)) going into running_var;
                        f = momentum, or 1 / num_batches_tracked (after its increment) for momentum=None;
                        a scenario without rows is counted but keeps its running statistics
  evaluation            the running statistics in place of the batch's (unless there are none: track=False)
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

Tensor = torch.Tensor


@dataclass
class State:
    weight: Tensor                        # [S,C]
    bias: Tensor                          # [S,C]
    running_mean: Optional[Tensor]        # [S,C] or None (track_running_stats=False)
    running_var: Optional[Tensor]
    num_batches_tracked: List[int] = field(default_factory=list)

    @staticmethod
    def fresh(S: int, C: int, dtype=torch.float64, track: bool = True) -> "State":
        return State(torch.ones(S, C, dtype=dtype), torch.zeros(S, C, dtype=dtype),
                     torch.zeros(S, C, dtype=dtype) if track else None, torch.ones(S, C, dtype=dtype) if track else None,
                     [0] * S if track else [])

    def double(self) -> "State":
        f = lambda t: None if t is None else t.detach().double().clone()      # noqa: E731
        return State(f(self.weight), f(self.bias), f(self.running_mean), f(self.running_var), list(self.num_batches_tracked))


@dataclass
class Cache:
    """What the backward needs of a forward."""
    x: Tensor
    sid: Tensor
    mean: Tensor        # [S,C] as used by the forward (zero for a scenario without rows)
    invstd: Tensor      # [S,C]
    weight: Tensor
    shared_weight: Tensor
    batch_stats: bool


def forward(x: Tensor, sid: Tensor, st: State, shared_weight: Tensor, shared_bias: Tensor, eps: float = 1e-5,
            momentum: Optional[float] = 0.1, training: bool = True):
    """y [B,C] and the Cache; updates st's buffers in place exactly when the reference would."""
    S, C = st.weight.shape
    tracked = st.running_mean is not None
    batch_stats = training or not tracked
    update = training and tracked
    counts = [int((sid == s).sum()) for s in range(S)]
    if batch_stats and 1 in counts:
        raise ValueError("Expected more than 1 value per channel when training, got input size {}".format(torch.Size([1, C])))
    zero = torch.zeros(C, dtype=x.dtype)
    mean, invstd = [zero] * S, [zero] * S
    y = torch.empty_like(x)
    for s in range(S):
        rows = sid == s
        n = counts[s]
        if update:
            st.num_batches_tracked[s] += 1
        if batch_stats:
            if n == 0:
                continue
            xs = x[rows]
            m = xs.sum(0) / n
            var = ((xs - m) ** 2).sum(0) / n
            if update:
                f = 1.0 / st.num_batches_tracked[s] if momentum is None else momentum
                st.running_mean[s] = (1 - f) * st.running_mean[s] + f * m.detach()
                st.running_var[s] = (1 - f) * st.running_var[s] + f * var.detach() * n / (n - 1)
        else:
            m, var = st.running_mean[s], st.running_var[s]
        mean[s], invstd[s] = m, 1.0 / torch.sqrt(var + eps)
        if n:
            y[rows] = (x[rows] - mean[s]) * invstd[s] * (st.weight[s] * shared_weight) + (st.bias[s] + shared_bias)
    return y, Cache(x, sid, torch.stack(mean), torch.stack(invstd), st.weight.clone(), shared_weight.clone(), batch_stats)


def backward(dy: Tensor, c: Cache) -> Dict[str, Tensor]:
    """Gradients of sum(y * dy): x, weight [S,C], bias [S,C], shared_weight [C], shared_bias [C]."""
    S, C = c.weight.shape
    dx = torch.zeros_like(c.x)
    g_w, g_b = torch.zeros_like(c.weight), torch.zeros_like(c.weight)
    g_sw, g_sb = torch.zeros_like(c.shared_weight), torch.zeros_like(c.shared_weight)
    for s in range(S):
        rows = c.sid == s
        n = int(rows.sum())
        if n == 0:
            continue
        g = dy[rows]
        xhat = (c.x[rows] - c.mean[s]) * c.invstd[s]
        s_dy, s_dyx = g.sum(0), (g * xhat).sum(0)
        gamma = c.weight[s] * c.shared_weight
        if c.batch_stats:
            dx[rows] = (gamma * c.invstd[s] / n) * (n * g - s_dy - xhat * s_dyx)
        else:
            dx[rows] = g * gamma * c.invstd[s]
        g_w[s], g_b[s] = c.shared_weight * s_dyx, s_dy
        g_sw += c.weight[s] * s_dyx
        g_sb += s_dy
    return {"x": dx, "weight": g_w, "bias": g_b, "shared_weight": g_sw, "shared_bias": g_sb}


def conditioning_rows(n: int = 300, C: int = 64, seed: int = 7) -> Tensor:
    """fp32 rows of mean 100 and standard deviation 0.1: E[x^2] - E[x]^2 in fp32 loses the variance (1e-2 under 1e4, whose
    fp32 spacing is 1e-3), a two-pass or merged-moments form does not."""
    g = torch.Generator().manual_seed(seed)
    return (100.0 + 0.1 * torch.randn(n, C, generator=g, dtype=torch.float64)).float()
