"""fp64 restatement of the reference's ESMM.forward behind the embeddings (models/esmm.py:84-96) and of WDL's DNN half
(models/wdl.py:75-79), with an optional list of dropout keep masks multiplied in after each relu (times 1 / (1 - p)), and its
hand-written backward.  Test infrastructure: torch on the CPU, no kernels.

Parameters P (a dict of tensors; `towers` = 2 for ESMM, 1 for WDL - the stacked form the kernels take):
    w[l] [towers, n_l, n_{l-1}], b[l] [towers, n_l]      the hidden layers (n_0 = C)
    wf [towers, n_last]                                  the bias-free final layers
    ob [1]                                               out.bias
Masks: a list over the hidden layers of bool [towers, B, n_l]; `keep_masks` makes them from oracle.satrans_oracle.dropout_keep with
the key (seed, step, layer l, site = tower, row + row_offset, column n) - the contract of csrc/esmm.hip.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle.satrans_oracle import dropout_keep

# (B, C, hidden): the smallest shapes where a 64-row tile, a 64-column tile, a 32-wide k step, a 256-row gradient chunk or a
# 4-column mask block can go wrong
SWEEP = (
    (1, 5, (3,)),
    (64, 32, (64,)),                 # exactly one of everything; the tail is the whole head
    (70, 45, (37, 9)),               # a ragged second row tile, odd K, N not a multiple of 4
    (260, 608, (130, 64, 8)),        # two gradient chunks, three column tiles, three layers, AliCCP's C
)
DROP_SEED = 0x5EED1234
# (p, step) of the dropout runs of the GPU tests; `draw` keeps every pre-activation away from its kink under each of them
DROP_RUNS = ((0.5, 1), (0.1, 2))
KINK = 1e-4


def case_id(case):
    B, C, hidden = case
    return f"B{B}-C{C}-{'x'.join(map(str, hidden))}"


def keep_masks(seed, step, B, hidden, towers, p, row_offset=0):
    rows = (np.arange(B, dtype=np.int64) + row_offset)[:, None]
    return [torch.from_numpy(np.stack([dropout_keep(seed, step, l, t, rows, np.arange(n)[None, :], p) for t in range(towers)]))
            for l, n in enumerate(hidden)]


def double(P):
    return {k: [t.double() for t in v] if isinstance(v, list) else v.double() for k, v in P.items()}


def forward(x, P, masks=None, p=0.0):
    """-> out [B, towers] (towers = 2: (ctr, ctcvr) probabilities; towers = 1: the logit with out.bias), cache."""
    towers = P["wf"].shape[0]
    scale = 1.0 / (1.0 - p)
    h = [[x] * towers]
    z = []
    for l, (w, b) in enumerate(zip(P["w"], P["b"])):
        zl = [h[-1][t] @ w[t].T + b[t] for t in range(towers)]
        hl = [torch.relu(v) for v in zl]
        if masks is not None:
            hl = [v * masks[l][t].to(v.dtype) * scale for t, v in enumerate(hl)]
        z.append(zl)
        h.append(hl)
    logit = [h[-1][t] @ P["wf"][t] + P["ob"][0] for t in range(towers)]
    if towers == 1:
        out, prob = logit[0][:, None], None
    else:
        prob = [torch.sigmoid(v) for v in logit]
        out = torch.stack([prob[0], prob[0] * prob[1]], dim=1)
    return out, dict(P=P, h=h, z=z, prob=prob, masks=masks, scale=scale, towers=towers)


def backward(dout, cache):
    """-> dx [B, C], G (the gradients, shaped as P)."""
    P, h, z, prob, masks, scale, towers = (cache[k] for k in ("P", "h", "z", "prob", "masks", "scale", "towers"))
    if towers == 1:
        dlogit = [dout[:, 0]]
    else:
        dp = [dout[:, 0] + dout[:, 1] * prob[1], dout[:, 1] * prob[0]]
        dlogit = [dp[t] * prob[t] * (1 - prob[t]) for t in range(towers)]
    G = {"w": [None] * len(P["w"]), "b": [None] * len(P["w"]), "ob": sum(d.sum() for d in dlogit).reshape(1),
         "wf": torch.stack([dlogit[t] @ h[-1][t] for t in range(towers)])}
    dh = [dlogit[t][:, None] * P["wf"][t][None, :] for t in range(towers)]
    for l in range(len(P["w"]) - 1, -1, -1):
        dz = []
        for t in range(towers):
            d = dh[t] * (z[l][t] > 0).to(dh[t].dtype)
            if masks is not None:
                d = d * masks[l][t].to(d.dtype) * scale
            dz.append(d)
        G["w"][l] = torch.stack([dz[t].T @ h[l][t] for t in range(towers)])
        G["b"][l] = torch.stack([dz[t].sum(0) for t in range(towers)])
        dh = [dz[t] @ P["w"][l][t] for t in range(towers)]
    return sum(dh), G


def flat(G, dx=None):
    """{"x": dx, "w[l]", "b[l]", "wf", "ob"} of a dict shaped as P."""
    out = {} if dx is None else {"x": dx}
    for k, v in G.items():
        for l, t in enumerate(v if isinstance(v, list) else [v]):
            out[f"{k}[{l}]" if isinstance(v, list) else k] = t
    return out


def l2_loss(P, l2):
    """What esmm.py:71-76 / wdl.py:59-61 register, in get_regularization_loss's arithmetic."""
    return sum(torch.sum(l2 * torch.square(w)) for w in list(P["w"]) + [P["wf"]]).reshape(1)


def min_margin(x, P, towers_masks=()):
    """Per row the smallest |pre-activation| over every hidden layer, without masks and under each (masks, p) given."""
    worst = torch.full((x.shape[0],), float("inf"), dtype=torch.float64)
    for masks, p in ((None, 0.0),) + tuple(towers_masks):
        _, cache = forward(x.double(), double(P), masks, p)
        for zl in cache["z"]:
            for v in zl:
                worst = torch.minimum(worst, v.abs().min(dim=1).values)
    return worst


def draw(case, towers, rounds=64):
    """Seeded fp32 inputs of a case (seed 7700 + B + C + sum(hidden) + towers): x N(0, 1), weights N(0, 1) n_in^-1/2, biases
    0.3 N(0, 1), out.bias 0.3 N(0, 1), dout [B, towers] N(0, 1).  Rows with a relu pre-activation within KINK = 1e-4 of zero
    (a margin that covers the 2e-5 the sibling draws use) - without dropout or under the masks of any of DROP_RUNS at row offset
    0 - are drawn again.  -> x, dout, P, rounds used."""
    B, C, hidden = case
    g = torch.Generator().manual_seed(7700 + B + C + sum(hidden) + towers)
    x = torch.randn(B, C, generator=g)
    P = {"w": [], "b": []}
    n = C
    for width in hidden:
        P["w"].append(torch.randn(towers, width, n, generator=g) * n ** -0.5)
        P["b"].append(0.3 * torch.randn(towers, width, generator=g))
        n = width
    P["wf"] = torch.randn(towers, n, generator=g) * n ** -0.5
    P["ob"] = 0.3 * torch.randn(1, generator=g)
    dout = torch.randn(B, towers, generator=g)
    runs = tuple((keep_masks(DROP_SEED, step, B, hidden, towers, p), p) for p, step in DROP_RUNS)
    for used in range(rounds):
        bad = min_margin(x, P, runs) < KINK
        if not bad.any():
            return x, dout, P, used
        x[bad] = torch.randn(int(bad.sum()), C, generator=g)
    raise AssertionError(f"{case_id(case)}: a pre-activation stays within {KINK} of its kink")


# ---- the module's names ---------------------------------------------------------------------------------------------------------

def dnn_names(towers):
    return ("ctr_dnn", "cvr_dnn") if towers == 2 else ("dnn",)


def final_names(towers):
    return ("ctr_dnn_final_layer", "cvr_dnn_final_layer") if towers == 2 else ("dnn_linear",)


def state_from_params(P):
    """The state_dict of an ESMMHead (towers = 2) or a WDLHead (towers = 1) holding P, in the reference's order."""
    towers = P["wf"].shape[0]
    sd = {"out.bias": P["ob"].clone()}
    for t, name in enumerate(dnn_names(towers)):
        for l in range(len(P["w"])):
            sd[f"{name}.linears.{l}.weight"] = P["w"][l][t].clone()
            sd[f"{name}.linears.{l}.bias"] = P["b"][l][t].clone()
    for t, name in enumerate(final_names(towers)):
        sd[f"{name}.weight"] = P["wf"][t][None, :].clone()
    return sd


def params_from_state(sd, towers):
    names, n = dnn_names(towers), 0
    while f"{names[0]}.linears.{n}.weight" in sd:
        n += 1
    get = lambda k: torch.as_tensor(np.asarray(sd[k]))      # noqa: E731
    return {"w": [torch.stack([get(f"{m}.linears.{l}.weight") for m in names]) for l in range(n)],
            "b": [torch.stack([get(f"{m}.linears.{l}.bias") for m in names]) for l in range(n)],
            "wf": torch.cat([get(f"{m}.weight") for m in final_names(towers)]), "ob": get("out.bias")}
