"""Torch restatement of the scenario-routed SharedBottom head (the reference's models/sharedbottom.py:120-133 under the
one-task-per-scenario loss of mtl_basemodel.py:268-269), forward and the explicit backward formulas  --  TEST INFRASTRUCTURE,
NOT PRODUCT CODE.

Everything runs in the dtype of `x` (fp64 for what the kernels are held against).  Task t owns the rows with `sid == t`.
`P` holds the parameters, the towers' stacked over the tasks (lists run over the hidden layers of a DNN):

    P["bottom_w"][l] [n_l, n_{l-1}]      P["bottom_b"][l] [n_l]                          n_0 = C
    P["tower_w"][l]  [T, n_l, n_{l-1}]   P["tower_b"][l]  [T, n_l]   P["tower_final_w"] [T, 1, n]   P["out_bias"] [T]

    bottom = the relu DNN over x                                                           (all rows)
    logit  = (the relu DNN of tower t over bottom) tower_final_w[t]^T + out_bias[t]        (rows of task t)

`torch_loop` is the reference's unrouted form (every task's tower over every row -> [B,T] probabilities) and `masked_loss`
the loss that reads one column per row.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import torch
import torch.nn.functional as F

from tests.mmoe_reference import double, flat, masked_loss  # noqa: F401  (the same helpers)
from tests.star_reference import sweep_ids  # noqa: F401  (the id patterns of the GPU tests)

Tensor = torch.Tensor
# the shape sweep of tests/test_sharedbottom_gpu.py, whose premise tests/test_sharedbottom_cpu.py checks: (C, bottom, tower);
# every value of C in {1, 33, 609}, 1 to 3 bottom layers, 0 to 3 tower layers and every last tower width of
# {1, 16, 64, 65, 130} occurs at least once (65 and 130: the tail's chain crosses column tiles); one case without a tower
# layer over a bottom wider than a column tile
SWEEP = [(1, (16,), (1,)), (33, (48, 32), (16,)), (609, (24, 24, 24), (16, 16, 64)), (33, (48, 32), (24, 65)),
         (33, (40,), (130,)), (33, (48, 72), ())]
SWEEP_T, SWEEP_OFFSET = 5, 2

LISTS = ("bottom_w", "bottom_b", "tower_w", "tower_b")
SINGLES = ("tower_final_w", "out_bias")
ROUTED = ("tower_w", "tower_b", "tower_final_w", "out_bias")      # leading index = task


def sweep_draw(case, row_tile: int, dw_chunk: int):
    """ids (before the offset) and the seeded draw of one SWEEP case."""
    C, bottom, tower = case
    ids = sweep_ids(row_tile, dw_chunk)
    return (ids,) + draw(ids.numel(), C, SWEEP_T, bottom, tower, 2000 + C + sum(bottom) + sum(tower), sid=ids)


@dataclass
class Cache:
    """What the backward needs of a forward."""
    sid: Tensor
    P: Dict[str, object]
    bh: List[Tensor]      # bh[0] = x, bh[l + 1] = output of bottom layer l
    th: List[Tensor]      # th[0] = the bottom's output, th[l + 1] = output of tower hidden layer l
    zs: List[Tensor]      # every hidden pre-activation (bottom, tower)


def forward(x: Tensor, sid: Tensor, P):
    """logit [B,1] and the Cache.  A row whose id owns no task would stay at logit 0; the product code raises IndexError."""
    B, T = x.shape[0], P["out_bias"].shape[0]
    zs, bh = [], [x]
    for w, b in zip(P["bottom_w"], P["bottom_b"]):
        z = bh[-1] @ w.T + b
        zs.append(z)
        bh.append(torch.relu(z))
    th = [bh[-1]]
    for w, b in zip(P["tower_w"], P["tower_b"]):
        z = torch.zeros(B, w.shape[1], dtype=x.dtype)
        for t in range(T):
            rows = sid == t
            z[rows] = th[-1][rows] @ w[t].T + b[t]
        zs.append(z)
        th.append(torch.relu(z))
    logit = torch.zeros(B, 1, dtype=x.dtype)
    for t in range(T):
        rows = sid == t
        logit[rows] = th[-1][rows] @ P["tower_final_w"][t].T + P["out_bias"][t]
    return logit, Cache(sid, P, bh, th, zs)


def backward(dlogit: Tensor, c: Cache) -> Dict[str, object]:
    """Gradients of sum(logit * dlogit), keyed like P, and "x" [B,C]:
        routed layer:   dW[t] = dz^T h over the task's rows,  db[t] = sum of dz,  dh = dz W[t],  dz_{l-1} = dh (h_{l-1} > 0)
        bottom:         the same layer formulas over all rows; the first layer's dh is dx."""
    P = c.P
    T = P["out_bias"].shape[0]
    g = {k: [torch.zeros_like(t) for t in P[k]] for k in LISTS}
    g.update({k: torch.zeros_like(P[k]) for k in SINGLES})
    nt = len(P["tower_w"])
    dz = dlogit
    for l in range(nt, -1, -1):
        W = P["tower_final_w"] if l == nt else P["tower_w"][l]
        dh = torch.zeros_like(c.th[l])
        for t in range(T):
            rows = c.sid == t
            if not bool(rows.any()):
                continue
            dw, db = dz[rows].T @ c.th[l][rows], dz[rows].sum(0)
            if l == nt:
                g["tower_final_w"][t], g["out_bias"][t] = dw, db[0]
            else:
                g["tower_w"][l][t], g["tower_b"][l][t] = dw, db
            dh[rows] = dz[rows] @ W[t]
        dz = dh * (c.th[l] > 0)      # th[0] is the bottom's relu output: the mask of the bottom's last layer
    for l in range(len(P["bottom_w"]) - 1, -1, -1):
        g["bottom_w"][l] = dz.T @ c.bh[l]
        g["bottom_b"][l] = dz.sum(0)
        dh = dz @ P["bottom_w"][l]
        dz = dh * (c.bh[l] > 0) if l > 0 else dh
    g["x"] = dz
    return g


def torch_loop(x: Tensor, P, sigmoid: bool = True) -> Tensor:
    """The reference's unrouted form with torch ops: every task's tower over every row -> probabilities [B,T] (the logits in
    front of PredictionLayer's sigmoid with sigmoid=False)."""
    T = P["out_bias"].shape[0]
    h = x
    for w, b in zip(P["bottom_w"], P["bottom_b"]):
        h = torch.relu(F.linear(h, w, b))
    bottom = h
    cols = []
    for t in range(T):
        h = bottom
        for w, b in zip(P["tower_w"], P["tower_b"]):
            h = torch.relu(F.linear(h, w[t], b[t]))
        cols.append(F.linear(h, P["tower_final_w"][t]) + P["out_bias"][t])
    out = torch.cat(cols, -1)
    return torch.sigmoid(out) if sigmoid else out


def keys_of(T: int, nb: int, nt: int) -> List[str]:
    """state_dict() keys of the reference SharedBottom's head entries, in its order: `out` comes first, because the reference's
    BaseModel registers a module under that name before SharedBottom builds its own and re-assigning a name keeps its place."""
    return ([f"out.{t}.bias" for t in range(T)] + [f"bottom_dnn.linears.{l}.{p}" for l in range(nb) for p in ("weight", "bias")] +
            [f"tower_dnn.{t}.linears.{l}.{p}" for t in range(T) for l in range(nt) for p in ("weight", "bias")] +
            [f"tower_dnn_final_layer.{t}.weight" for t in range(T)])


def params_from_state(sd, T: int, nb: int, nt: int, dtype=torch.float64):
    """The stacked form of a state_dict with the reference SharedBottom's keys."""
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)      # noqa: E731
    st = lambda l, p: torch.stack([t(f"tower_dnn.{i}.linears.{l}.{p}") for i in range(T)])      # noqa: E731
    return dict(bottom_w=[t(f"bottom_dnn.linears.{l}.weight") for l in range(nb)],
                bottom_b=[t(f"bottom_dnn.linears.{l}.bias") for l in range(nb)],
                tower_w=[st(l, "weight") for l in range(nt)], tower_b=[st(l, "bias") for l in range(nt)],
                tower_final_w=torch.stack([t(f"tower_dnn_final_layer.{i}.weight") for i in range(T)]),
                out_bias=torch.cat([t(f"out.{i}.bias") for i in range(T)]))


def state_from_params(P) -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by the reference's parameter names."""
    out = {}
    for l, (w, b) in enumerate(zip(P["bottom_w"], P["bottom_b"])):
        out[f"bottom_dnn.linears.{l}.weight"], out[f"bottom_dnn.linears.{l}.bias"] = w, b
    for l, (w, b) in enumerate(zip(P["tower_w"], P["tower_b"])):
        for i in range(w.shape[0]):
            out[f"tower_dnn.{i}.linears.{l}.weight"], out[f"tower_dnn.{i}.linears.{l}.bias"] = w[i], b[i]
    for i in range(P["out_bias"].shape[0]):
        out[f"tower_dnn_final_layer.{i}.weight"] = P["tower_final_w"][i]
        out[f"out.{i}.bias"] = P["out_bias"][i:i + 1]
    return out


def draw(B: int, C: int, T: int, bottom, tower, seed: int, sid: Tensor = None, rel: float = 2e-5):
    """Seeded fp32 inputs of the GPU tests: x [B,C], upstream weights w [B,1], weights scaled n_in^-1/2 (activations stay at
    order 1), biases 0.3 N(0,1).

    With `sid`, the rows of x that put a hidden pre-activation of the fp64 forward within rel * max(activation of that layer)
    of zero are drawn again from the same generator, until none is left (see kink_margin; the argument is that of
    tests/mmoe_reference.py::draw).  Which rows are drawn again is decided by the fp64 forward alone, never by the code under
    test."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g)
    w = torch.randn(B, 1, generator=g)
    P = {"bottom_w": [], "bottom_b": [], "tower_w": [], "tower_b": []}
    n_in = C
    for n in bottom:
        P["bottom_w"].append(torch.randn(n, n_in, generator=g) * n_in ** -0.5)
        P["bottom_b"].append(0.3 * torch.randn(n, generator=g))
        n_in = n
    for n in tower:
        P["tower_w"].append(torch.randn(T, n, n_in, generator=g) * n_in ** -0.5)
        P["tower_b"].append(0.3 * torch.randn(T, n, generator=g))
        n_in = n
    P["tower_final_w"] = torch.randn(T, 1, n_in, generator=g) * n_in ** -0.5
    P["out_bias"] = 0.3 * torch.randn(T, generator=g)
    while sid is not None:
        _, c = forward(x.double(), sid, double(P))
        near = torch.zeros(B, dtype=torch.bool)
        for z in c.zs:
            near |= (z.abs() < rel * float(torch.relu(z).max())).any(1)
        idx = near.nonzero().flatten()
        if idx.numel() == 0:
            break
        x[idx] = torch.randn(idx.numel(), C, generator=g)
    return x, w, P


def kink_margin(c: Cache) -> float:
    """The smallest |hidden pre-activation| / max(hidden activation of its layer) of a forward: relu's derivative jumps at zero,
    so a forward held to a relative output bound `rel` has a derivative to be held to only when this exceeds rel."""
    return min(float(z.abs().min() / torch.relu(z).max()) for z in c.zs)
