"""Torch restatement of STAR's star-topology towers (the reference's models/star.py:156-170 inside the loop of star.py:147-170),
forward and the explicit backward formulas  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Everything runs in the dtype of `x` (fp64 for what the kernels are held against).  Scenario s owns the rows with `sid == s`.
`P` holds, per layer l = 0 .. L-1 (the last one is the logit layer of width 1):

    P["w_dom"][l] [S, n_l, n_{l-1}]   P["b_dom"][l] [S, n_l]   P["w_sh"][l] [n_l, n_{l-1}]   P["b_sh"][l] [n_l]

    W_eff[s,l] = w_dom[l][s] * w_sh[l]            b_eff[s,l] = b_dom[l][s] + b_sh[l]
    h_l[i]     = relu(h_{l-1}[i] W_eff[s,l]^T + b_eff[s,l])            l < L-1
    logit[i]   = h_{L-2}[i] W_eff[s,L-1]^T + b_eff[s,L-1]

`head_forward` puts tests/mdr_bn_reference.py's partitioned normalisation in front (the reference's use_domain_bn).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import torch

from tests import mdr_bn_reference as BN

Tensor = torch.Tensor
GROUPS = ("w_dom", "b_dom", "w_sh", "b_sh")


@dataclass
class Cache:
    """What the backward needs of a forward."""
    sid: Tensor
    P: Dict[str, List[Tensor]]
    h: List[Tensor]      # h[0] = x, h[l + 1] = output of hidden layer l


def forward(x: Tensor, sid: Tensor, P: Dict[str, List[Tensor]]):
    """logit [B,1] and the Cache.  A row whose id owns no scenario would stay at logit 0 (the reference's loop); the product
    code raises IndexError for it instead."""
    L, S = len(P["w_sh"]), P["w_dom"][0].shape[0]
    h = [x]
    for l in range(L):
        out = torch.zeros(x.shape[0], P["w_sh"][l].shape[0], dtype=x.dtype)
        for s in range(S):
            rows = sid == s
            z = h[l][rows] @ (P["w_dom"][l][s] * P["w_sh"][l]).T + (P["b_dom"][l][s] + P["b_sh"][l])
            out[rows] = z if l == L - 1 else torch.relu(z)
        h.append(out)
    return h[L], Cache(sid, P, h[:L])


def backward(dlogit: Tensor, c: Cache) -> Dict[str, object]:
    """Gradients of sum(logit * dlogit): {"x": [B,C], "w_dom": [...], "b_dom": [...], "w_sh": [...], "b_sh": [...]}, by
        dz_l = dh_l * (h_l > 0)  (dz_{L-1} = dlogit),  dh_{l-1} = dz_l W_eff[s,l],  dW_eff[s,l] = dz_l^T h_{l-1} over the scenario,
        g_w_dom = dW_eff * w_sh,  g_b_dom = sum of dz_l,  g_w_sh = sum_s dW_eff[s] * w_dom[s],  g_b_sh = sum_s g_b_dom[s]."""
    P = c.P
    L, S = len(P["w_sh"]), P["w_dom"][0].shape[0]
    g = {k: [torch.zeros_like(t) for t in P[k]] for k in GROUPS}
    dz = dlogit
    for l in range(L - 1, -1, -1):
        dh = torch.zeros_like(c.h[l])
        for s in range(S):
            rows = c.sid == s
            if not bool(rows.any()):
                continue
            dw = dz[rows].T @ c.h[l][rows]
            g["w_dom"][l][s] = dw * P["w_sh"][l]
            g["b_dom"][l][s] = dz[rows].sum(0)
            g["w_sh"][l] += dw * P["w_dom"][l][s]
            g["b_sh"][l] += g["b_dom"][l][s]
            dh[rows] = dz[rows] @ (P["w_dom"][l][s] * P["w_sh"][l])
        dz = dh * (c.h[l] > 0) if l > 0 else dh
    g["x"] = dz
    return g


def head_forward(x: Tensor, sid: Tensor, P, st: BN.State, shared_weight: Tensor, shared_bias: Tensor, eps: float = 1e-5,
                 momentum=0.1, training: bool = True):
    """The partitioned normalisation, then the towers -> logit, (normalisation cache, towers cache)."""
    y, bn_cache = BN.forward(x, sid, st, shared_weight, shared_bias, eps, momentum, training)
    logit, cache = forward(y, sid, P)
    return logit, (bn_cache, cache)


def head_backward(dlogit: Tensor, caches) -> Dict[str, object]:
    bn_cache, cache = caches
    g = backward(dlogit, cache)
    gb = BN.backward(g["x"], bn_cache)
    g["x"] = gb["x"]
    g["bn"] = {k: gb[k] for k in ("weight", "bias", "shared_weight", "shared_bias")}
    return g


def params_from_state(sd, S: int, n_hidden: int, dtype=torch.float64) -> Dict[str, List[Tensor]]:
    """The stacked form of a state_dict with the reference Star_Net's tower keys."""
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)      # noqa: E731
    dom = [[f"domain_dnns.{s}.linears.{l}" for s in range(S)] for l in range(n_hidden)] + \
          [[f"domain_dnn_linears.{s}" for s in range(S)]]
    sh = [f"shared_dnn.linears.{l}" for l in range(n_hidden)] + ["shared_dnn_linear"]
    return dict(w_dom=[torch.stack([t(k + ".weight") for k in layer]) for layer in dom],
                b_dom=[torch.stack([t(k + ".bias") for k in layer]) for layer in dom],
                w_sh=[t(k + ".weight") for k in sh], b_sh=[t(k + ".bias") for k in sh])


def grads_by_key(g, S: int, n_hidden: int) -> Dict[str, Tensor]:
    """The gradients of `backward` under the reference's parameter names."""
    out = {}
    for l in range(n_hidden + 1):
        for s in range(S):
            k = f"domain_dnns.{s}.linears.{l}" if l < n_hidden else f"domain_dnn_linears.{s}"
            out[k + ".weight"], out[k + ".bias"] = g["w_dom"][l][s], g["b_dom"][l][s]
        k = f"shared_dnn.linears.{l}" if l < n_hidden else "shared_dnn_linear"
        out[k + ".weight"], out[k + ".bias"] = g["w_sh"][l], g["b_sh"][l]
    if "bn" in g:
        for s in range(S):
            out[f"bns.{s}.weight"], out[f"bns.{s}.bias"] = g["bn"]["weight"][s], g["bn"]["bias"][s]
        out["shared_bn_weight"], out["shared_bn_bias"] = g["bn"]["shared_weight"], g["bn"]["shared_bias"]
    return out


def draw(B: int, C: int, hidden, S: int, seed: int):
    """Seeded fp32 inputs of the GPU tests: x [B,C], upstream weights w [B,1], parameters scaled n_in^-1/4 (so that the
    elementwise product W_dom * W_sh is about n_in^-1/2 and every layer keeps its activations at order 1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g)
    w = torch.randn(B, 1, generator=g)
    widths = [C] + list(hidden) + [1]
    P = {k: [] for k in GROUPS}
    for l in range(len(widths) - 1):
        n, k = widths[l + 1], widths[l]
        P["w_dom"].append(torch.randn(S, n, k, generator=g) * k ** -0.25)
        P["b_dom"].append(0.3 * torch.randn(S, n, generator=g))
        P["w_sh"].append(torch.randn(n, k, generator=g) * k ** -0.25)
        P["b_sh"].append(0.3 * torch.randn(n, generator=g))
    return x, w, P


def double(P):
    return {k: [t.double() for t in v] for k, v in P.items()}


def hidden_pre_activations(x: Tensor, sid: Tensor, P) -> List[Tensor]:
    """z_l = h_{l-1} W_eff^T + b_eff of every hidden layer (h_l = relu(z_l)), in the dtype of x."""
    L, S = len(P["w_sh"]), P["w_dom"][0].shape[0]
    h, zs = x, []
    for l in range(L - 1):
        z = torch.zeros(x.shape[0], P["w_sh"][l].shape[0], dtype=x.dtype)
        for s in range(S):
            rows = sid == s
            z[rows] = h[rows] @ (P["w_dom"][l][s] * P["w_sh"][l]).T + (P["b_dom"][l][s] + P["b_sh"][l])
        zs.append(z)
        h = torch.relu(z)
    return zs


def redraw_rows_at_a_kink(x: Tensor, sid: Tensor, P, rel: float, seed: int):
    """x with fresh N(0,1) rows wherever a hidden pre-activation of the fp64 forward lies within rel * max|h_l| of zero, and the
    number of rows drawn again.

    relu's derivative jumps at zero.  A pre-activation that the fp64 forward puts closer to zero than the precision the forward
    is held to (`rel`, the output bound) has no derivative any fp32 forward could be held to: rounding alone decides the side, and
    the other side moves that row's gradients by a whole unit's contribution, a percent of their size.  The chance is about
    0.3 * 2 * (fp32 error of z) per hidden element, negligible for a few hundred rows and about one per batch at 20,000 rows of
    384 hidden units.  The margin comes from the fp64 forward and the output bound alone, never from the code under test."""
    g = torch.Generator().manual_seed(seed)
    x, Pd, redrawn = x.clone(), double(P), 0
    while True:
        zs = hidden_pre_activations(x.double(), sid, Pd)
        near = torch.zeros(x.shape[0], dtype=torch.bool)
        for z in zs:
            near |= (z.abs() < rel * float(torch.relu(z).max())).any(1)
        idx = near.nonzero().flatten()
        if idx.numel() == 0:
            return x, redrawn
        x[idx] = torch.randn(idx.numel(), x.shape[1], generator=g)
        redrawn += idx.numel()


def torch_loop(x: Tensor, ids: Tensor, P, offset: int = 0) -> Tensor:
    """The reference's loop (star.py:147-170) written with torch ops: boolean-mask selects, F.linear, masked write-back."""
    import torch.nn.functional as F
    L, S = len(P["w_sh"]), P["w_dom"][0].shape[0]
    logit = torch.zeros(x.shape[0], 1, dtype=x.dtype, device=x.device)
    for s in range(S):
        h = x[ids == s + offset]
        for l in range(L):
            h = F.linear(h, P["w_dom"][l][s] * P["w_sh"][l], P["b_dom"][l][s] + P["b_sh"][l])
            if l < L - 1:
                h = torch.relu(h)
        logit[ids == s + offset] = h
    return logit


def sweep_ids(row_tile: int, dw_chunk: int, seed: int = 3) -> Tensor:
    """S = 5, interleaved: scenario 0 runs one row past the kernels' row tile, scenario 3 one row past the weight-gradient row
    chunk, scenario 2 has exactly one row, scenario 4 none, scenario 1 a partial tile."""
    counts = [row_tile + 1, 40, 1, dw_chunk + 1, 0]
    ids = torch.cat([torch.full((n,), s, dtype=torch.long) for s, n in enumerate(counts)])
    ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(seed))]
    assert [int((ids == s).sum()) for s in range(5)] == counts
    return ids
