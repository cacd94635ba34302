"""Torch restatement of the scenario-routed MMoE head (the reference's models/mmoe.py:142-171 under the one-task-per-scenario
loss of mtl_basemodel.py:268-269), forward and the explicit backward formulas  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Everything runs in the dtype of `x` (fp64 for what the kernels are held against).  Task t owns the rows with `sid == t`.
`P` holds the stacked parameters (lists run over the hidden layers of a DNN):

    P["expert_w"][l] [E, n_l, n_{l-1}]   P["expert_b"][l] [E, n_l]                       n_0 = C
    P["gate_w"][l]   [T, n_l, n_{l-1}]   P["gate_b"][l]   [T, n_l]   P["gate_final_w"]  [T, E, n]      (n = C without hidden layers)
    P["tower_w"][l]  [T, n_l, n_{l-1}]   P["tower_b"][l]  [T, n_l]   P["tower_final_w"] [T, 1, n]   P["out_bias"] [T]

    expert_out[e] = the relu DNN of expert e over x                 (all rows)
    scores        = (the relu DNN of gate t over x) gate_final_w[t]^T,   g = softmax(scores)
    m             = sum_e g[e] expert_out[e]
    logit         = (the relu DNN of tower t over m) tower_final_w[t]^T + out_bias[t]      (rows of task t)

`torch_loop` is the reference's unrouted form (every task's gate and tower over every row -> [B,T] probabilities) and
`masked_loss` the loss that reads one column per row.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import torch
import torch.nn.functional as F

from tests.star_reference import sweep_ids  # noqa: F401  (the id patterns of the GPU tests)

Tensor = torch.Tensor
# the shape sweep of tests/test_mmoe_gpu.py, whose premise tests/test_mmoe_cpu.py checks: (C, E, expert, gate, tower); every
# value of C in {1, 33, 609}, E in {2, 3, 8} and of the three lists of hidden units occurs at least once
SWEEP = [(1, 2, (16,), (), ()), (33, 3, (48, 32), (8,), (64,)), (609, 8, (24, 24, 24), (64,), (16, 16, 16)),
         (33, 8, (48, 32), (), (16, 16, 16))]
SWEEP_T, SWEEP_OFFSET = 5, 2


def sweep_draw(case, row_tile: int, dw_chunk: int):
    """ids (before the offset) and the seeded draw of one SWEEP case."""
    C, E, expert, gate, tower = case
    ids = sweep_ids(row_tile, dw_chunk)
    return (ids,) + draw(ids.numel(), C, SWEEP_T, E, expert, gate, tower, 1000 + C + E, sid=ids)

LISTS = ("expert_w", "expert_b", "gate_w", "gate_b", "tower_w", "tower_b")
SINGLES = ("gate_final_w", "tower_final_w", "out_bias")
ROUTED = ("gate_w", "gate_b", "gate_final_w", "tower_w", "tower_b", "tower_final_w", "out_bias")      # leading index = task


@dataclass
class Cache:
    """What the backward needs of a forward."""
    sid: Tensor
    P: Dict[str, object]
    xh: List[Tensor]      # xh[0] = x, xh[l + 1] = [B, E, n_l] output of expert layer l
    gh: List[Tensor]      # gh[0] = x, gh[l + 1] = output of gate hidden layer l
    th: List[Tensor]      # th[0] = m, th[l + 1] = output of tower hidden layer l
    scores: Tensor
    gates: Tensor
    zs: List[Tensor]      # every hidden pre-activation (experts, gate, tower)


def forward(x: Tensor, sid: Tensor, P):
    """logit [B,1] and the Cache.  A row whose id owns no task would stay at logit 0; the product code raises IndexError."""
    B, T = x.shape[0], P["out_bias"].shape[0]
    zs = []
    xh = [x]
    h = x.unsqueeze(1)                                        # [B, 1 or E, n]
    for w, b in zip(P["expert_w"], P["expert_b"]):
        z = torch.einsum("bek,enk->ben", h.expand(B, w.shape[0], h.shape[2]), w) + b
        zs.append(z)
        h = torch.relu(z)
        xh.append(h)
    eo = h

    def routed(h0, ws, bs, final, bias):
        hs = [h0]
        for w, b in zip(ws, bs):
            z = torch.zeros(B, w.shape[1], dtype=x.dtype)
            for t in range(T):
                rows = sid == t
                z[rows] = hs[-1][rows] @ w[t].T + b[t]
            zs.append(z)
            hs.append(torch.relu(z))
        out = torch.zeros(B, final.shape[1], dtype=x.dtype)
        for t in range(T):
            rows = sid == t
            out[rows] = hs[-1][rows] @ final[t].T + (bias[t] if bias is not None else 0)
        return hs, out

    gh, scores = routed(x, P["gate_w"], P["gate_b"], P["gate_final_w"], None)
    gates = torch.softmax(scores, 1)
    m = torch.einsum("be,ben->bn", gates, eo)
    th, logit = routed(m, P["tower_w"], P["tower_b"], P["tower_final_w"], P["out_bias"])
    return logit, Cache(sid, P, xh, gh, th, scores, gates, zs)


def backward(dlogit: Tensor, c: Cache) -> Dict[str, object]:
    """Gradients of sum(logit * dlogit), keyed like P, and "x" [B,C]:
        routed layer:   dW[t] = dz^T h over the task's rows,  db[t] = sum of dz,  dh = dz W[t],  dz_{l-1} = dh (h_{l-1} > 0)
        mixture:        d expert_out[e] = g[e] dm,  dg[e] = dm . expert_out[e],  dscores = g (dg - sum_e g[e] dg[e])
        experts:        the same layer formulas per expert over all rows;  dx = experts' dx + gate's dx."""
    P = c.P
    T = P["out_bias"].shape[0]
    g = {k: [torch.zeros_like(t) for t in P[k]] for k in LISTS}
    g.update({k: torch.zeros_like(P[k]) for k in SINGLES})

    def routed(dz, hs, ws, final, kw, kb, kf, kbias):
        for l in range(len(ws), -1, -1):
            W = final if l == len(ws) else ws[l]
            dh = torch.zeros_like(hs[l])
            for t in range(T):
                rows = c.sid == t
                if not bool(rows.any()):
                    continue
                dw, db = dz[rows].T @ hs[l][rows], dz[rows].sum(0)
                if l == len(ws):
                    g[kf][t] = dw
                    if kbias:
                        g[kbias][t] = db[0]
                else:
                    g[kw][l][t], g[kb][l][t] = dw, db
                dh[rows] = dz[rows] @ W[t]
            dz = dh * (hs[l] > 0) if l > 0 else dh
        return dz

    dm = routed(dlogit, c.th, P["tower_w"], P["tower_final_w"], "tower_w", "tower_b", "tower_final_w", "out_bias")
    eo = c.xh[-1]
    d_eo = c.gates.unsqueeze(2) * dm.unsqueeze(1)
    dg = torch.einsum("bn,ben->be", dm, eo)
    dscores = c.gates * (dg - (c.gates * dg).sum(1, keepdim=True))
    dx_gate = routed(dscores, c.gh, P["gate_w"], P["gate_final_w"], "gate_w", "gate_b", "gate_final_w", None)
    dz = d_eo * (eo > 0)
    for l in range(len(P["expert_w"]) - 1, -1, -1):
        hin = c.xh[l] if l > 0 else c.xh[0].unsqueeze(1).expand(-1, dz.shape[1], -1)
        g["expert_w"][l] = torch.einsum("ben,bek->enk", dz, hin)
        g["expert_b"][l] = dz.sum(0)
        dh = torch.einsum("ben,enk->bek", dz, P["expert_w"][l])
        dz = dh * (c.xh[l] > 0) if l > 0 else dh
    g["x"] = dz.sum(1) + dx_gate
    return g


def torch_loop(x: Tensor, P, sigmoid: bool = True) -> Tensor:
    """The reference's unrouted form with torch ops: every task's gate and tower over every row -> probabilities [B,T]
    (the logits in front of PredictionLayer's sigmoid with sigmoid=False)."""
    E, T = P["expert_w"][0].shape[0], P["out_bias"].shape[0]
    outs = []
    for e in range(E):
        h = x
        for w, b in zip(P["expert_w"], P["expert_b"]):
            h = torch.relu(F.linear(h, w[e], b[e]))
        outs.append(h)
    eo = torch.stack(outs, 1)
    cols = []
    for t in range(T):
        h = x
        for w, b in zip(P["gate_w"], P["gate_b"]):
            h = torch.relu(F.linear(h, w[t], b[t]))
        gate = F.linear(h, P["gate_final_w"][t]).softmax(1)
        h = torch.matmul(gate.unsqueeze(1), eo).squeeze(1)
        for w, b in zip(P["tower_w"], P["tower_b"]):
            h = torch.relu(F.linear(h, w[t], b[t]))
        cols.append(F.linear(h, P["tower_final_w"][t]) + P["out_bias"][t])
    out = torch.cat(cols, -1)
    return torch.sigmoid(out) if sigmoid else out


def masked_loss(y_pred: Tensor, labels: Tensor, ids: Tensor, offset: int = 0) -> Tensor:
    """mtl_basemodel.py:268-269: the summed BCE of column t over the rows whose id is t + offset, summed over t."""
    T = y_pred.shape[1]
    return sum(F.binary_cross_entropy(y_pred[:, t][ids == t + offset], labels[ids == t + offset], reduction='sum') for t in range(T))


def keys_of(E: int, T: int, nx: int, ng: int, nt: int) -> List[str]:
    """state_dict() keys of the reference MMOE's head entries, in its order: `out` comes first, because the reference's
    BaseModel registers a module under that name before MMOE builds its own and re-assigning a name keeps its place."""
    dnn = lambda name, n, layers: [f"{name}.{i}.linears.{l}.{p}" for i in range(n) for l in range(layers) for p in ("weight", "bias")]  # noqa: E731
    return ([f"out.{t}.bias" for t in range(T)] + dnn("expert_dnn", E, nx) + dnn("gate_dnn", T, ng) +
            [f"gate_dnn_final_layer.{t}.weight" for t in range(T)] + dnn("tower_dnn", T, nt) +
            [f"tower_dnn_final_layer.{t}.weight" for t in range(T)])


def params_from_state(sd, E: int, T: int, nx: int, ng: int, nt: int, dtype=torch.float64):
    """The stacked form of a state_dict with the reference MMOE's keys."""
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)      # noqa: E731
    st = lambda name, n, l, p: torch.stack([t(f"{name}.{i}.linears.{l}.{p}") for i in range(n)])      # noqa: E731
    return dict(expert_w=[st("expert_dnn", E, l, "weight") for l in range(nx)], expert_b=[st("expert_dnn", E, l, "bias") for l in range(nx)],
                gate_w=[st("gate_dnn", T, l, "weight") for l in range(ng)], gate_b=[st("gate_dnn", T, l, "bias") for l in range(ng)],
                gate_final_w=torch.stack([t(f"gate_dnn_final_layer.{i}.weight") for i in range(T)]),
                tower_w=[st("tower_dnn", T, l, "weight") for l in range(nt)], tower_b=[st("tower_dnn", T, l, "bias") for l in range(nt)],
                tower_final_w=torch.stack([t(f"tower_dnn_final_layer.{i}.weight") for i in range(T)]),
                out_bias=torch.cat([t(f"out.{i}.bias") for i in range(T)]))


def state_from_params(P) -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by the reference's parameter names."""
    out = {}
    for name, kw, kb in (("expert_dnn", "expert_w", "expert_b"), ("gate_dnn", "gate_w", "gate_b"), ("tower_dnn", "tower_w", "tower_b")):
        for l, (w, b) in enumerate(zip(P[kw], P[kb])):
            for i in range(w.shape[0]):
                out[f"{name}.{i}.linears.{l}.weight"], out[f"{name}.{i}.linears.{l}.bias"] = w[i], b[i]
    for i in range(P["out_bias"].shape[0]):
        out[f"gate_dnn_final_layer.{i}.weight"] = P["gate_final_w"][i]
        out[f"tower_dnn_final_layer.{i}.weight"] = P["tower_final_w"][i]
        out[f"out.{i}.bias"] = P["out_bias"][i:i + 1]
    return out


def draw(B: int, C: int, T: int, E: int, expert, gate, tower, seed: int, sid: Tensor = None, rel: float = 2e-5):
    """Seeded fp32 inputs of the GPU tests: x [B,C], upstream weights w [B,1], weights scaled n_in^-1/2 (activations stay at
    order 1), biases 0.3 N(0,1).

    With `sid`, the rows of x that put a hidden pre-activation of the fp64 forward within rel * max(activation of that layer)
    of zero are drawn again from the same generator, until none is left (see kink_margin; the argument is that of
    tests/star_reference.py::redraw_rows_at_a_kink).  A batch of a few hundred rows has some 1e5 hidden units, each within the
    output bound 2e-5 of relu's kink with probability about 1e-4, so a plain draw nearly always holds a few such rows; which
    rows are drawn again is decided by the fp64 forward alone, never by the code under test."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g)
    w = torch.randn(B, 1, generator=g)

    def dnn(G, n_in, units):
        ws, bs = [], []
        for n in units:
            ws.append(torch.randn(G, n, n_in, generator=g) * n_in ** -0.5)
            bs.append(0.3 * torch.randn(G, n, generator=g))
            n_in = n
        return ws, bs, n_in

    P = {}
    P["expert_w"], P["expert_b"], n_x = dnn(E, C, expert)
    P["gate_w"], P["gate_b"], n_g = dnn(T, C, gate)
    P["gate_final_w"] = torch.randn(T, E, n_g, generator=g) * n_g ** -0.5
    P["tower_w"], P["tower_b"], n_t = dnn(T, n_x, tower)
    P["tower_final_w"] = torch.randn(T, 1, n_t, generator=g) * n_t ** -0.5
    P["out_bias"] = 0.3 * torch.randn(T, generator=g)
    while sid is not None:
        _, c = forward(x.double(), sid, double(P))
        near = torch.zeros(B, dtype=torch.bool)
        for z in c.zs:
            near |= (z.abs() < rel * float(torch.relu(z).max())).flatten(1).any(1)
        idx = near.nonzero().flatten()
        if idx.numel() == 0:
            break
        x[idx] = torch.randn(idx.numel(), C, generator=g)
    return x, w, P


def double(P):
    return {k: ([t.double() for t in v] if isinstance(v, list) else v.double()) for k, v in P.items()}


def flat(g) -> Dict[str, Tensor]:
    """{"expert_w[0]": tensor, ...}: the tensors of P or of a gradient dict, one key each."""
    out = {}
    for k, v in g.items():
        if isinstance(v, list):
            out.update({f"{k}[{l}]": t for l, t in enumerate(v)})
        else:
            out[k] = v
    return out


def kink_margin(c: Cache) -> float:
    """The smallest |hidden pre-activation| / max(hidden activation of its layer) of a forward: relu's derivative jumps at zero,
    so a forward held to a relative output bound `rel` has a derivative to be held to only when this exceeds rel."""
    return min(float(z.abs().min() / torch.relu(z).max()) for z in c.zs)
