"""Torch restatement of the compressed interaction network (deepctr-torch 0.2.9's CIN, which the reference's
models/xdeepfm.py:73,96-98 calls), forward and the explicit backward formulas  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Everything runs in the dtype of `x` (fp64 for what the kernels are held against).  `P` holds the parameters as lists over the
layers:  P["w"][i] [O_i, H_i M]  (the Conv1d weight without its last axis),  P["b"][i] [O_i].  With X0 = x [B, M, D], H_0 = M:

    z_i[b,o,d] = b_i[o] + sum_{h,m} W_i[o, h M + m] X_i[b,h,d] X0[b,m,d]        a_i = relu(z_i)            (X_0 = X0)
    split and i not last:  X_{i+1} = a_i[:, :O_i/2],  direct_i = a_i[:, O_i/2:]        otherwise:  X_{i+1} = direct_i = a_i
    result = cat_i(direct_i, dim=1).sum(-1)

`head_forward` is the part of the reference's xDeepFM.forward behind the embedding lookup, over a state_dict with the
reference's keys.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import torch

Tensor = torch.Tensor
# the shape sweep of tests/test_cin_gpu.py, whose premise tests/test_cin_cpu.py checks: (B, M, D, layers, split_half)
SWEEP = [
    (70, 3, 4, (8, 6), True),               # contraction 9 < one k step; 16 samples per row tile
    (131, 19, 32, (16, 8), True),           # the AliCCP M and D; contraction 361; B D = several gradient chunks and a remainder
    (37, 5, 33, (66, 10), True),            # D straddles row tiles; hidden half 33; a k step crosses h boundaries
    (37, 7, 16, (65,), False),              # one layer, one column past a column tile
    (20, 19, 32, (256, 128), True),         # the real widths; layer 2's contraction is 2432
    (16, 39, 8, (128, 128, 64), False),     # three layers, H = 128 unsplit
    (5, 3, 4, (4, 1), True),                # B D smaller than a tile, last layer one channel
    (9, 64, 8, (4,), False),                # M at its limit
]
ALONE = [SWEEP[2], SWEEP[1]]      # the shapes of the alone-equals-batch test


def case_id(c) -> str:
    return f"B{c[0]}-M{c[1]}-D{c[2]}-{'x'.join(map(str, c[3]))}-{'split' if c[4] else 'whole'}"


def sweep_draw(case):
    B, M, D, layers, split = case
    return draw(B, M, D, layers, split, 3000 + B + M + D + sum(layers))


def double(P):
    return {k: [t.double() for t in v] for k, v in P.items()}


def flat(g) -> Dict[str, Tensor]:
    """{"w[0]": .., "b[0]": .., "x": ..} of a dict of lists (and tensors)."""
    out = {}
    for k, v in g.items():
        if isinstance(v, (list, tuple)):
            out.update({f"{k}[{i}]": t for i, t in enumerate(v)})
        else:
            out[k] = v
    return out


def featuremap_num(layers, split: bool) -> int:
    return sum(layers[:-1]) // 2 + layers[-1] if split else sum(layers)


@dataclass
class Cache:
    """What the backward needs of a forward."""
    P: Dict[str, List[Tensor]]
    split: bool
    xs: List[Tensor]          # xs[i] = X_i, the input of layer i (xs[0] = X0)
    zs: List[Tensor]          # pre-activations [B, O_i, D]
    direct: List[slice]       # the channels of a_i that go to the result


def outer(xi: Tensor, x0: Tensor) -> Tensor:
    """[B, H M, D]: element (h M + m) = X_i[b,h,d] X0[b,m,d]"""
    B, H, D = xi.shape
    return (xi[:, :, None, :] * x0[:, None, :, :]).reshape(B, H * x0.shape[1], D)


def forward(x: Tensor, P, split: bool):
    """result [B, featuremap_num] and the Cache."""
    L = len(P["w"])
    xs, zs, direct, parts = [x], [], [], []
    for i, (w, b) in enumerate(zip(P["w"], P["b"])):
        z = torch.einsum('ok,bkd->bod', w, outer(xs[-1], x)) + b[None, :, None]
        a = torch.relu(z)
        zs.append(z)
        half = w.shape[0] // 2 if split and i != L - 1 else 0
        if split and i != L - 1 and w.shape[0] % 2:
            raise ValueError("layer_size must be even number except for the last layer when split_half=True")
        direct.append(slice(half, w.shape[0]))
        parts.append(a[:, half:])
        xs.append(a[:, :half] if half else a)
    return torch.cat(parts, dim=1).sum(-1), Cache(P, split, xs, zs, direct)


def backward(dres: Tensor, c: Cache) -> Dict[str, object]:
    """Gradients of sum(result * dres), keyed like P, and "x" [B,M,D]:
        dz_i = (dres of the direct channels, broadcast over d, + dX_{i+1} on the channels handed on) (z_i > 0)
        dW_i = sum_{b,d} dz_i[b,o,d] outer_i[b,k,d],   db_i = sum_{b,d} dz_i,   dA = dz_i W_i  [B, H, M, D]
        dX_i = sum_m dA X0,   dX0 += sum_h dA X_i      (layer 0: both are dX0)"""
    P, x0 = c.P, c.xs[0]
    L, (B, M, D) = len(P["w"]), x0.shape
    g = {"w": [None] * L, "b": [None] * L}
    dx0 = torch.zeros_like(x0)
    col = sum(s.stop - s.start for s in c.direct)
    dxn = None
    for i in range(L - 1, -1, -1):
        O, s = P["w"][i].shape[0], c.direct[i]
        col -= s.stop - s.start
        up = torch.zeros_like(c.zs[i])
        up[:, s] += dres[:, col:col + s.stop - s.start, None]
        if dxn is not None:
            up[:, :dxn.shape[1]] += dxn
        dz = up * (c.zs[i] > 0)
        xi = c.xs[i]
        g["w"][i] = torch.einsum('bod,bkd->ok', dz, outer(xi, x0))
        g["b"][i] = dz.sum((0, 2))
        dA = torch.einsum('bod,ok->bkd', dz, P["w"][i]).reshape(B, xi.shape[1], M, D)
        dxn = (dA * x0[:, None]).sum(2)
        dx0 = dx0 + (dA * xi[:, :, None]).sum(1)
    g["x"] = dx0 + dxn
    return g


def keys_of(n_dnn: int, n_cin: int) -> List[str]:
    """state_dict() keys of the reference xDeepFM's head entries, in its order (`out` first: the reference's BaseModel
    registers it before xDeepFM builds its own modules)."""
    return (["out.bias"] + [f"dnn.linears.{l}.{p}" for l in range(n_dnn) for p in ("weight", "bias")] +
            (["dnn_linear.weight"] if n_dnn else []) +
            [f"cin.conv1ds.{i}.{p}" for i in range(n_cin) for p in ("weight", "bias")] + (["cin_linear.weight"] if n_cin else []))


def params_from_state(sd, prefix: str = "", dtype=torch.float64):
    """P of a state_dict holding `<prefix>conv1ds.{i}.{weight,bias}`."""
    P, i = {"w": [], "b": []}, 0
    while f"{prefix}conv1ds.{i}.weight" in sd:
        P["w"].append(torch.as_tensor(sd[f"{prefix}conv1ds.{i}.weight"]).to(dtype).squeeze(-1))
        P["b"].append(torch.as_tensor(sd[f"{prefix}conv1ds.{i}.bias"]).to(dtype))
        i += 1
    return P


def state_from_params(P, prefix: str = "") -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by deepctr's parameter names."""
    out = {}
    for i, (w, b) in enumerate(zip(P["w"], P["b"])):
        out[f"{prefix}conv1ds.{i}.weight"], out[f"{prefix}conv1ds.{i}.bias"] = w.unsqueeze(-1), b
    return out


def head_forward(emb: Tensor, dense, linear_logit, sd, split: bool, cin_out: Tensor = None):
    """logit [B,1] of the reference's xDeepFM.forward behind the lookup (xdeepfm.py:94-115, before `out`'s sigmoid), in the
    reference's order of the sum.  `cin_out` replaces the CIN's result when given (a leaf for the explicit backward)."""
    logit = linear_logit
    if "dnn_linear.weight" in sd:
        h = emb.flatten(1) if dense is None else torch.cat([emb.flatten(1), dense], -1)
        l = 0
        while f"dnn.linears.{l}.weight" in sd:
            h = torch.relu(h @ sd[f"dnn.linears.{l}.weight"].T + sd[f"dnn.linears.{l}.bias"])
            l += 1
        h = h @ sd["dnn_linear.weight"].T
        logit = h if logit is None else logit + h
    if "cin_linear.weight" in sd:
        if cin_out is None:
            cin_out = forward(emb, params_from_state(sd, "cin.", emb.dtype), split)[0]
        h = cin_out @ sd["cin_linear.weight"].T
        logit = h if logit is None else logit + h
    return logit + sd["out.bias"]


def near_kink(c: Cache, rel: float) -> Tensor:
    """[B] bool: the samples with a pre-activation within rel * max(relu z of that layer) of zero."""
    near = torch.zeros(c.xs[0].shape[0], dtype=torch.bool)
    for z in c.zs:
        near |= (z.abs() < rel * float(torch.relu(z).max())).flatten(1).any(1)
    return near


def draw(B: int, M: int, D: int, layers, split: bool, seed: int, rel: float = 2e-5, rounds: int = 64):
    """Seeded fp32 inputs of the GPU tests: x [B,M,D] N(0,1), an upstream weight per result element up [B, featuremap_num],
    weights N(0,1) (H M)^-1/2, biases 0.3 N(0,1).

    The samples that put a pre-activation of the fp64 forward within rel * max(relu z of that layer) of zero are drawn again
    from the same generator, until none is left: relu's derivative jumps at zero, so a forward held to a relative bound `rel`
    has a derivative to be held to only off that margin.  Which samples are drawn again is decided by the fp64 restatement
    alone, never by the code under test.  RuntimeError when `rounds` rounds do not suffice."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, M, D, generator=g)
    up = torch.randn(B, featuremap_num(layers, split), generator=g)
    P = {"w": [], "b": []}
    h = M
    for i, o in enumerate(layers):
        P["w"].append(torch.randn(o, h * M, generator=g) * (h * M) ** -0.5)
        P["b"].append(0.3 * torch.randn(o, generator=g))
        h = o // 2 if split and i != len(layers) - 1 else o
    for _ in range(rounds):
        _, c = forward(x.double(), double(P), split)
        idx = near_kink(c, rel).nonzero().flatten()
        if idx.numel() == 0:
            return x, up, P
        x[idx] = torch.randn(idx.numel(), M, D, generator=g)
    raise RuntimeError(f"draw: samples near a kink are left after {rounds} rounds")


def kink_margin(c: Cache) -> float:
    """The smallest |pre-activation| / max(activation of its layer) of a forward."""
    return min(float(z.abs().min() / torch.relu(z).max()) for z in c.zs)
