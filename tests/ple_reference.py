"""Torch restatement of the scenario-routed PLE head (the reference's models/ple.py:161-248 under the one-task-per-scenario
loss of mtl_basemodel.py:268-269), one or two CGC levels  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

`forward` is the ROUTED form, written with torch ops so that autograd gives its backward (`grads`); everything runs in the
dtype of `x` (fp64 for what the kernels are held against).  Task t owns the rows with `sid == t`.  `P` holds the stacked
parameters under the names of satrans_ple_desc (lists run over the hidden layers of a DNN; E0 = T ns + nsh, Eo = ns + nsh):

    level 0 of two    P["e0_w"][l] [E0, n_l, n_{l-1}]  P["e0_b"][l] [E0, n_l]      blocks: task 0's ns experts, ..., the nsh shared
                      P["g0_w"][l] [T, ...]  P["g0_b"][l]  P["g0_final_w"] [T, Eo, n]        the tasks' own gates
                      P["sg0_w"][l] [n_l, n_{l-1}]  P["sg0_b"][l]  P["sg0_final_w"] [E0, n]   the shared gate
    last level        P["spec_w"][l] [T ns, ...]  P["spec_b"][l]      P["shared_w"][l] [nsh, ...]  P["shared_b"][l]
                      P["gate_w"][l] [T, ...]  P["gate_b"][l]  P["gate_final_w"] [T, Eo, n]
                      P["tower_w"][l]  P["tower_b"][l]  P["tower_final_w"] [T, 1, n]  P["out_bias"] [T]

With one level the level-0 entries are empty lists / absent.  The reference's parameters that take no part (the last level's
shared gate, the surplus shared experts) are not in P.  `torch_loop` is the reference's unrouted form (every task's experts,
gates and towers over every row at every level -> [B,T]) and `masked_loss` the loss that reads one column per row.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from tests.mmoe_reference import double, flat, masked_loss  # noqa: F401
from tests.star_reference import sweep_ids  # noqa: F401  (the id patterns of the GPU tests)

Tensor = torch.Tensor
# the shape sweep of tests/test_ple_gpu.py, whose premise tests/test_ple_cpu.py checks: (C, ns, nsh, levels, expert, gate, tower)
SWEEP = [(1, 1, 1, 1, (16,), (), ()), (33, 2, 1, 2, (48, 32), (8,), (64,)), (609, 1, 1, 2, (24, 24, 24), (64,), (16, 16, 16)),
         (33, 4, 4, 2, (48, 32), (), (16,))]
SWEEP_T, SWEEP_OFFSET = 5, 2

LISTS = ("e0_w", "e0_b", "g0_w", "g0_b", "sg0_w", "sg0_b", "spec_w", "spec_b", "shared_w", "shared_b", "gate_w", "gate_b", "tower_w",
         "tower_b")
SINGLES = ("g0_final_w", "sg0_final_w", "gate_final_w", "tower_final_w", "out_bias")
ROUTED = ("g0_w", "g0_b", "g0_final_w", "spec_w", "spec_b", "gate_w", "gate_b", "gate_final_w", "tower_w", "tower_b", "tower_final_w",
          "out_bias")      # leading index = task (spec_*: task * ns + expert)


def sizes(P) -> Tuple[int, int, int, bool]:
    """T, ns, nsh and whether P has two levels."""
    T, Eo = P["out_bias"].shape[0], P["gate_final_w"].shape[1]
    ns = P["spec_w"][0].shape[0] // T
    return T, ns, Eo - ns, bool(P.get("e0_w"))


def of_task(key: str, g: Tensor, t: int, ns: int) -> Tensor:
    """Task t's part of a tensor (or gradient) whose flat key is `key` and which is one of ROUTED."""
    return g[t * ns:(t + 1) * ns] if key.startswith("spec_") else g[t]


@dataclass
class Cache:
    gates: Tensor                        # the last level's, [B, Eo]
    mixture: Tensor                      # the last level's, [B, n]
    zs: List[Tuple[Tensor, Tensor]]      # (row indices or None for all rows, hidden pre-activations of one DNN layer over them)


def _dnn(h, ws, bs, i, idx, zs):
    for w, b in zip(ws, bs):
        z = F.linear(h, w if i is None else w[i], b if i is None else b[i])
        zs.append((idx, z))
        h = torch.relu(z)
    return h


def forward(x: Tensor, sid: Tensor, P):
    """logit [B,1] and the Cache.  A row whose id owns no task would stay at logit 0; the product code raises IndexError."""
    T, ns, nsh, two = sizes(P)
    B, Eo, E0 = x.shape[0], ns + nsh, T * ns + nsh
    zs = []
    tasks = [(t, (sid == t).nonzero().flatten()) for t in range(T)]
    tasks = [(t, idx) for t, idx in tasks if idx.numel()]
    in_own = in_sh = x
    if two:
        eo0 = torch.stack([_dnn(x, P["e0_w"], P["e0_b"], e, None, zs) for e in range(E0)], 1)
        g_sh = F.linear(_dnn(x, P["sg0_w"], P["sg0_b"], None, None, zs), P["sg0_final_w"]).softmax(1)
        in_sh = torch.einsum("be,ben->bn", g_sh, eo0)
        in_own = torch.zeros(B, eo0.shape[2], dtype=x.dtype)
        for t, idx in tasks:
            g = F.linear(_dnn(x[idx], P["g0_w"], P["g0_b"], t, idx, zs), P["g0_final_w"][t]).softmax(1)
            blocks = list(range(t * ns, (t + 1) * ns)) + list(range(T * ns, E0))
            in_own[idx] = torch.einsum("be,ben->bn", g, eo0[idx][:, blocks])
    shared = [_dnn(in_sh, P["shared_w"], P["shared_b"], k, None, zs) for k in range(nsh)]
    n = shared[0].shape[1]
    logit, gates, mix = torch.zeros(B, 1, dtype=x.dtype), torch.zeros(B, Eo, dtype=x.dtype), torch.zeros(B, n, dtype=x.dtype)
    for t, idx in tasks:
        h = in_own[idx]
        eo = torch.stack([_dnn(h, P["spec_w"], P["spec_b"], t * ns + j, idx, zs) for j in range(ns)] + [s[idx] for s in shared], 1)
        g = F.linear(_dnn(h, P["gate_w"], P["gate_b"], t, idx, zs), P["gate_final_w"][t]).softmax(1)
        m = torch.einsum("be,ben->bn", g, eo)
        logit[idx] = F.linear(_dnn(m, P["tower_w"], P["tower_b"], t, idx, zs), P["tower_final_w"][t]) + P["out_bias"][t]
        gates[idx], mix[idx] = g, m
    return logit, Cache(gates, mix, zs)


def leaves(P, dtype=torch.float64):
    """P in `dtype`, every tensor a leaf that requires a gradient."""
    mk = lambda t: t.detach().to(dtype).clone().requires_grad_(True)      # noqa: E731
    return {k: ([mk(t) for t in v] if isinstance(v, list) else mk(v)) for k, v in P.items()}


def grads(x: Tensor, sid: Tensor, P, w: Tensor, fn=None):
    """(logit, Cache or None, gradients of sum(logit * w) keyed like flat(P), and "x") by autograd in the dtype of x; `fn`
    replaces the routed forward (torch_loop's own-task column)."""
    Pl = leaves(P, x.dtype)
    xl = x.detach().clone().requires_grad_(True)
    if fn is None:
        y, cache = forward(xl, sid, Pl)
    else:
        y, cache = fn(xl, Pl), None
    (y * w.to(x.dtype)).sum().backward()
    g = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in flat(Pl).items()}
    g["x"] = xl.grad
    return y.detach(), cache, g


def torch_loop(x: Tensor, P, sigmoid: bool = True) -> Tensor:
    """The reference's unrouted form with torch ops: every task's experts, gates and towers over every row at every level ->
    probabilities [B,T] (the logits in front of PredictionLayer's sigmoid with sigmoid=False).  The last level's shared gate,
    whose mixture nothing reads, is left out."""
    T, ns, nsh, two = sizes(P)
    zs = []
    inputs = [x] * (T + 1)
    for level in range(2 if two else 1):
        if two and level == 0:
            E0 = T * ns + nsh
            spec = [_dnn(inputs[e // ns], P["e0_w"], P["e0_b"], e, None, zs) for e in range(T * ns)]
            shared = [_dnn(inputs[-1], P["e0_w"], P["e0_b"], e, None, zs) for e in range(T * ns, E0)]
            gw, gb, gf = P["g0_w"], P["g0_b"], P["g0_final_w"]
        else:
            spec = [_dnn(inputs[e // ns], P["spec_w"], P["spec_b"], e, None, zs) for e in range(T * ns)]
            shared = [_dnn(inputs[-1], P["shared_w"], P["shared_b"], k, None, zs) for k in range(nsh)]
            gw, gb, gf = P["gate_w"], P["gate_b"], P["gate_final_w"]
        outs = []
        for t in range(T):
            cur = torch.stack(spec[t * ns:(t + 1) * ns] + shared, 1)
            g = F.linear(_dnn(inputs[t], gw, gb, t, None, zs), gf[t]).softmax(1)
            outs.append(torch.matmul(g.unsqueeze(1), cur).squeeze(1))
        if two and level == 0:
            g = F.linear(_dnn(inputs[-1], P["sg0_w"], P["sg0_b"], None, None, zs), P["sg0_final_w"]).softmax(1)
            outs.append(torch.matmul(g.unsqueeze(1), torch.stack(spec + shared, 1)).squeeze(1))
        inputs = outs
    cols = [F.linear(_dnn(inputs[t], P["tower_w"], P["tower_b"], t, None, zs), P["tower_final_w"][t]) + P["out_bias"][t]
            for t in range(T)]
    out = torch.cat(cols, -1)
    return torch.sigmoid(out) if sigmoid else out


def _dnn_keys(name, layers):
    return [f"{name}.linears.{l}.{p}" for l in range(layers) for p in ("weight", "bias")]


def keys_of(T: int, ns: int, nsh: int, levels: int, nx: int, ng: int, nt: int) -> List[str]:
    """state_dict() keys of the reference PLE's head entries, in its order (`out` first: the reference's BaseModel registers a
    module under that name before PLE builds its own).  shared_experts has ns experts per level - the reference's quirk."""
    lv = range(levels)
    return ([f"out.{t}.bias" for t in range(T)] +
            [k for l in lv for t in range(T) for j in range(ns) for k in _dnn_keys(f"specific_experts.{l}.{t}.{j}", nx)] +
            [k for l in lv for j in range(ns) for k in _dnn_keys(f"shared_experts.{l}.0.{j}", nx)] +
            [k for l in lv for t in range(T) for k in _dnn_keys(f"specific_gate_dnn.{l}.{t}.0", ng)] +
            [f"specific_gate_dnn_final_layer.{l}.{t}.weight" for l in lv for t in range(T)] +
            [k for l in lv for k in _dnn_keys(f"shared_gate_dnn.{l}", ng)] +
            [f"shared_gate_dnn_final_layer.{l}.weight" for l in lv] +
            [k for t in range(T) for k in _dnn_keys(f"tower_dnn.{t}", nt)] +
            [f"tower_dnn_final_layer.{t}.weight" for t in range(T)])


def dead_keys(T: int, ns: int, nsh: int, levels: int, nx: int, ng: int, nt: int) -> List[str]:
    """The keys that take no part: the last level's shared gate and shared_experts.{l}.0.{k} for k >= nsh."""
    last = levels - 1
    return ([k for l in range(levels) for j in range(nsh, ns) for k in _dnn_keys(f"shared_experts.{l}.0.{j}", nx)] +
            _dnn_keys(f"shared_gate_dnn.{last}", ng) + [f"shared_gate_dnn_final_layer.{last}.weight"])


def _names(T, ns, nsh, levels):
    """{key of P: module names stacked under it (a list, or one name for an unstacked DNN)} for the DNNs, and for the finals."""
    last = levels - 1
    spec = lambda l: [f"specific_experts.{l}.{t}.{j}" for t in range(T) for j in range(ns)]      # noqa: E731
    shared = lambda l: [f"shared_experts.{l}.0.{k}" for k in range(nsh)]      # noqa: E731
    dnns = {"spec": spec(last), "shared": shared(last), "gate": [f"specific_gate_dnn.{last}.{t}.0" for t in range(T)],
            "tower": [f"tower_dnn.{t}" for t in range(T)]}
    finals = {"gate_final_w": [f"specific_gate_dnn_final_layer.{last}.{t}.weight" for t in range(T)],
              "tower_final_w": [f"tower_dnn_final_layer.{t}.weight" for t in range(T)]}
    if levels == 2:
        dnns.update({"e0": spec(0) + shared(0), "g0": [f"specific_gate_dnn.0.{t}.0" for t in range(T)], "sg0": "shared_gate_dnn.0"})
        finals.update({"g0_final_w": [f"specific_gate_dnn_final_layer.0.{t}.weight" for t in range(T)],
                       "sg0_final_w": "shared_gate_dnn_final_layer.0.weight"})
    return dnns, finals


def params_from_state(sd, T: int, ns: int, nsh: int, levels: int, nx: int, ng: int, nt: int, dtype=torch.float64):
    """The stacked form of a state_dict with the reference PLE's keys."""
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)      # noqa: E731
    layers = {"spec": nx, "shared": nx, "e0": nx, "gate": ng, "g0": ng, "sg0": ng, "tower": nt}
    dnns, finals = _names(T, ns, nsh, levels)
    P = {k: [] for k in LISTS}
    for name, mods in dnns.items():
        for l in range(layers[name]):
            for p, suffix in (("w", "weight"), ("b", "bias")):
                P[f"{name}_{p}"].append(t(f"{mods}.linears.{l}.{suffix}") if isinstance(mods, str) else
                                        torch.stack([t(f"{m}.linears.{l}.{suffix}") for m in mods]))
    for name, keys in finals.items():
        P[name] = t(keys) if isinstance(keys, str) else torch.stack([t(k) for k in keys])
    P["out_bias"] = torch.cat([t(f"out.{i}.bias") for i in range(T)])
    return P


def state_from_params(P) -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by the reference's parameter names (live keys only)."""
    T, ns, nsh, two = sizes(P)
    dnns, finals = _names(T, ns, nsh, 2 if two else 1)
    out = {}
    for name, mods in dnns.items():
        for l, (w, b) in enumerate(zip(P[f"{name}_w"], P[f"{name}_b"])):
            for i, m in enumerate([mods] if isinstance(mods, str) else mods):
                out[f"{m}.linears.{l}.weight"], out[f"{m}.linears.{l}.bias"] = (w, b) if isinstance(mods, str) else (w[i], b[i])
    for name, keys in finals.items():
        if isinstance(keys, str):
            out[keys] = P[name]
        else:
            out.update({k: P[name][i] for i, k in enumerate(keys)})
    out.update({f"out.{i}.bias": P["out_bias"][i:i + 1] for i in range(T)})
    return out


def kink_rows(c: Cache, B: int, rel: float) -> Tensor:
    """[B] bool: rows with a hidden pre-activation within rel * max(activation of that DNN layer over its rows) of zero."""
    near = torch.zeros(B, dtype=torch.bool)
    for idx, z in c.zs:
        hit = (z.detach().abs() < rel * float(torch.relu(z.detach()).max())).flatten(1).any(1)
        if idx is None:
            near |= hit
        else:
            near[idx] |= hit
    return near


def kink_margin(c: Cache) -> float:
    """The smallest |hidden pre-activation| / max(hidden activation of its layer) of a forward (see tests/mmoe_reference.py)."""
    return min(float(z.detach().abs().min() / torch.relu(z.detach()).max()) for _, z in c.zs)


def draw(B: int, C: int, T: int, ns: int, nsh: int, levels: int, expert, gate, tower, seed: int, sid: Tensor = None,
         rel: float = 2e-5):
    """Seeded fp32 inputs of the GPU tests: x [B,C], upstream weights w [B,1], weights scaled n_in^-1/2 (activations stay at
    order 1), biases 0.3 N(0,1).  With `sid`, the rows of x that put a hidden pre-activation of the fp64 forward within rel of
    relu's kink are drawn again from the same generator until none is left (the argument of tests/mmoe_reference.py::draw);
    which rows are drawn again is decided by the fp64 forward alone, never by the code under test."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g)
    w = torch.randn(B, 1, generator=g)

    def dnn(G, n_in, units):
        ws, bs = [], []
        for n in units:
            lead = () if G is None else (G,)
            ws.append(torch.randn(*lead, n, n_in, generator=g) * n_in ** -0.5)
            bs.append(0.3 * torch.randn(*lead, n, generator=g))
            n_in = n
        return ws, bs, n_in

    P = {k: [] for k in LISTS}
    Eo, E0, n = ns + nsh, T * ns + nsh, expert[-1]
    kin = C
    if levels == 2:
        P["e0_w"], P["e0_b"], _ = dnn(E0, C, expert)
        P["g0_w"], P["g0_b"], n_g = dnn(T, C, gate)
        P["g0_final_w"] = torch.randn(T, Eo, n_g, generator=g) * n_g ** -0.5
        P["sg0_w"], P["sg0_b"], n_g = dnn(None, C, gate)
        P["sg0_final_w"] = torch.randn(E0, n_g, generator=g) * n_g ** -0.5
        kin = n
    P["spec_w"], P["spec_b"], _ = dnn(T * ns, kin, expert)
    P["shared_w"], P["shared_b"], _ = dnn(nsh, kin, expert)
    P["gate_w"], P["gate_b"], n_g = dnn(T, kin, gate)
    P["gate_final_w"] = torch.randn(T, Eo, n_g, generator=g) * n_g ** -0.5
    P["tower_w"], P["tower_b"], n_t = dnn(T, n, tower)
    P["tower_final_w"] = torch.randn(T, 1, n_t, generator=g) * n_t ** -0.5
    P["out_bias"] = 0.3 * torch.randn(T, generator=g)
    while sid is not None:
        with torch.no_grad():
            _, c = forward(x.double(), sid, double(P))
        idx = kink_rows(c, B, rel).nonzero().flatten()
        if idx.numel() == 0:
            break
        x[idx] = torch.randn(idx.numel(), C, generator=g)
    return x, w, P


def sweep_draw(case, row_tile: int, dw_chunk: int):
    """ids (before the offset) and the seeded draw of one SWEEP case."""
    C, ns, nsh, levels, expert, gate, tower = case
    ids = sweep_ids(row_tile, dw_chunk)
    return (ids,) + draw(ids.numel(), C, SWEEP_T, ns, nsh, levels, expert, gate, tower, 2000 + C + ns + levels, sid=ids)
