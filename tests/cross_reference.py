"""Torch restatement of DCN's cross network (deepctr-torch 0.2.9's CrossNet, which the reference's models/dcn.py:70,101 calls),
forward and the explicit backward formulas  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Everything runs in the dtype of `x` (fp64 for what the kernels are held against).  `P` holds the parameters without deepctr's
trailing axis of one:  P["kernels"] [L, N] (vector) or [L, N, N] (matrix, W_l [n_out, n_in]),  P["bias"] [L, N].  With x_0 = x0:

    vector:  s_l[b]   = sum_n x_l[b,n] w_l[n]          x_{l+1} = x0 s_l[b] + b_l + x_l
    matrix:  u_l[b,:] = W_l x_l[b,:] + b_l             x_{l+1} = x0 * u_l + x_l
    result = x_L

`head_forward` is the part of the reference's DCN.forward behind the embedding lookup, over a state_dict with the reference's
keys.  The cross network has no kink, so a draw needs no second look.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import torch

Tensor = torch.Tensor
# the shape sweep of tests/test_cross_gpu.py, whose premise tests/test_cross_cpu.py checks: (B, N, L), each in both forms
SHAPES = [
    (70, 9, 2),         # contraction shorter than one k step
    (131, 608, 3),      # AliCCP 19 x 32; several row tiles and gradient chunks with remainders
    (37, 165, 2),       # N = 2 tiles + 37
    (37, 65, 1),        # one column past a tile, one layer
    (20, 609, 4),       # 608 + one dense column (odd N: no 16-byte alignment of rows)
    (5, 3, 1),          # smaller than any tile
    (9, 4096, 1),       # N at its limit
    (300, 33, 8),       # L at its limit, values grow to ~1e3
]
SWEEP = [s + (m,) for s in SHAPES for m in (False, True)]
ALONE = [s + (m,) for s in (SHAPES[2], SHAPES[1]) for m in (False, True)]      # the shapes of the alone-equals-batch test


def case_id(c) -> str:
    return f"B{c[0]}-N{c[1]}-L{c[2]}-{'matrix' if c[3] else 'vector'}"


def sweep_draw(case):
    B, N, L, matrix = case
    return draw(B, N, L, matrix, 4000 + B + N + L + int(matrix))


def double(P):
    return {k: v.double() for k, v in P.items()}


@dataclass
class Cache:
    """What the backward needs of a forward."""
    P: Dict[str, Tensor]
    matrix: bool
    xs: List[Tensor]          # xs[l] = x_l, the input of layer l (xs[0] = x0)
    mid: List[Tensor]         # s_l [B] (vector) or u_l [B, N] (matrix)


def forward(x: Tensor, P, matrix: bool):
    """result [B, N] and the Cache."""
    xs, mid = [x], []
    for w, b in zip(P["kernels"], P["bias"]):
        xl = xs[-1]
        if matrix:
            u = xl @ w.T + b
            xs.append(x * u + xl)
            mid.append(u)
        else:
            s = xl @ w
            xs.append(x * s[:, None] + b + xl)
            mid.append(s)
    return xs[-1], Cache(P, matrix, xs, mid)


def backward(dres: Tensor, c: Cache) -> Dict[str, Tensor]:
    """Gradients of sum(result * dres): "kernels", "bias" (shaped like P's) and "x" [B, N].  With g_L = dres, l = L-1 .. 0:
        vector:  ds_l = sum_n g_{l+1} x0       dx0 += g_{l+1} s_l     g_l = g_{l+1} + w_l ds_l
                 dw_l = sum_b ds_l x_l         db_l = sum_b g_{l+1}
        matrix:  du_l = g_{l+1} * x0           dx0 += g_{l+1} * u_l   g_l = g_{l+1} + du_l W_l
                 dW_l = du_l^T x_l             db_l = sum_b du_l
        finally  dx0 += g_0"""
    P, x0 = c.P, c.xs[0]
    L = P["kernels"].shape[0]
    dk, db = torch.zeros_like(P["kernels"]), torch.zeros_like(P["bias"])
    dx0, g = torch.zeros_like(x0), dres
    for l in range(L - 1, -1, -1):
        w, xl = P["kernels"][l], c.xs[l]
        if c.matrix:
            du = g * x0
            dx0 = dx0 + g * c.mid[l]
            dk[l], db[l] = du.T @ xl, du.sum(0)
            g = g + du @ w
        else:
            ds = (g * x0).sum(1)
            dx0 = dx0 + g * c.mid[l][:, None]
            dk[l], db[l] = ds @ xl, g.sum(0)
            g = g + w[None, :] * ds[:, None]
    return {"kernels": dk, "bias": db, "x": dx0 + g}


def keys_of(n_dnn: int) -> List[str]:
    """state_dict() keys of the reference DCN's head entries, in its order (`out` first: the reference's BaseModel registers it
    before DCN builds its own modules)."""
    return (["out.bias"] + [f"dnn.linears.{l}.{p}" for l in range(n_dnn) for p in ("weight", "bias")] +
            ["dnn_linear.weight", "crossnet.kernels", "crossnet.bias"])


def params_from_state(sd, prefix: str = "", dtype=torch.float64):
    """P of a state_dict holding deepctr's `<prefix>kernels` [L, N, 1 or N] and `<prefix>bias` [L, N, 1]."""
    k = torch.as_tensor(sd[f"{prefix}kernels"]).to(dtype)
    b = torch.as_tensor(sd[f"{prefix}bias"]).to(dtype)
    matrix = k.dim() == 3 and k.shape[2] == k.shape[1] and k.shape[1] != 1
    return {"kernels": k if matrix else k.squeeze(-1), "bias": b.squeeze(-1)}


def state_from_params(P, prefix: str = "") -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by deepctr's parameter names, in its shapes."""
    k = P["kernels"]
    return {f"{prefix}kernels": k if k.dim() == 3 else k.unsqueeze(-1), f"{prefix}bias": P["bias"].unsqueeze(-1)}


def head_forward(emb: Tensor, dense, linear_logit, sd, cross_out: Tensor = None):
    """logit [B,1] of the reference's DCN.forward behind the lookup (dcn.py:90-111, before `out`'s sigmoid).  `cross_out`
    replaces the cross network's result when given (a leaf for the explicit backward)."""
    x = emb.flatten(1) if dense is None else torch.cat([emb.flatten(1), dense], -1)
    parts = []
    if sd["crossnet.kernels"].shape[0] > 0:
        if cross_out is None:
            P = params_from_state(sd, "crossnet.", emb.dtype)
            cross_out = forward(x, P, P["kernels"].dim() == 3)[0]
        parts.append(cross_out)
    if "dnn.linears.0.weight" in sd:
        h, l = x, 0
        while f"dnn.linears.{l}.weight" in sd:
            h = torch.relu(h @ sd[f"dnn.linears.{l}.weight"].T + sd[f"dnn.linears.{l}.bias"])
            l += 1
        parts.append(h)
    h = torch.cat(parts, -1) @ sd["dnn_linear.weight"].T
    logit = h if linear_logit is None else linear_logit + h
    return logit + sd["out.bias"]


def reg_loss(sd, l2_linear: float = 1e-5, l2_cross: float = 1e-5) -> Tensor:
    """[1]: the entries DCN.__init__ adds to regularization_weight with a non-zero factor, as get_regularization_loss sums."""
    total = torch.zeros((1,), dtype=sd["dnn_linear.weight"].dtype)
    total = total + torch.sum(l2_linear * torch.square(sd["dnn_linear.weight"]))
    return total + torch.sum(l2_cross * torch.square(sd["crossnet.kernels"]))


def draw(B: int, N: int, L: int, matrix: bool, seed: int):
    """Seeded fp32 inputs of the GPU tests, all from one generator: x [B,N] N(0,1), then an upstream weight per result element
    up [B,N] N(0,1), then kernels N(0,1) N^-1/2, then bias 0.3 N(0,1)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, generator=g)
    up = torch.randn(B, N, generator=g)
    kernels = torch.randn((L, N, N) if matrix else (L, N), generator=g) * N ** -0.5
    bias = 0.3 * torch.randn(L, N, generator=g)
    return x, up, {"kernels": kernels, "bias": bias}
