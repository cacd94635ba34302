"""Torch restatement of deepctr-torch 0.2.9's InteractingLayer (which the reference's models/autoint.py builds, autoint.py:13,75-76)
and of the half of AutoInt.forward behind the lookup (autoint.py:93-121), forward in deepctr's LITERAL form and the explicit
backward formulas  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Everything runs in the dtype of its input (fp64 for what the kernels are held against).  `P` holds the parameters:
    P["int"]      a list, one dict per interacting layer: "W_Query", "W_key", "W_Value" [D, D] and, with the residual, "W_Res"
    P["dnn_w"], P["dnn_b"]   lists: the DNN's Linear layers (empty without a DNN)
    P["lin"] [1, F D + last width]   dnn_linear.weight (bias-free; without a DNN: [1, F D])
    P["out_bias"] [1]
Literal form: tensordot with the weights, split / stack over the heads, the einsum 'bnik,bnjk->bnij', softmax over the last dim,
matmul, cat of the split heads, the residual, relu.  Every layer's pre-activation o + r is kept (LayerCache.pre).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
FIXTURES = ("autoint", "autoint_nodnn", "autoint_nores")      # tests/golden/autoint/*.npz
LAYER_KEYS = ("W_Query", "W_key", "W_Value", "W_Res")
# the sweep of tests/test_autoint_gpu.py, whose premise tests/test_autoint_cpu.py checks: (B, F, D, H, layers, use_res, scaling)
SWEEP = [
    (1, 2, 16, 2, 1, True, False),        # the smallest: one sample, two fields, d_head 8
    (5, 3, 16, 1, 1, True, True),         # one head, d_head 16, scaling on, a part-filled workgroup
    (37, 19, 32, 2, 3, True, False),      # AutoInt's defaults at the AliCCP field count; F * samples no multiple of 16
    (37, 19, 32, 4, 1, False, True),      # no residual (three-block product), SATrans's head count
    (9, 23, 64, 4, 3, True, True),        # D = 64, the varlen field count
    (3, 64, 64, 2, 2, True, False),       # the largest F and d_head 32: the LDS budget's edge, one sample a workgroup
    (257, 19, 16, 2, 3, True, False),     # many sample groups: several partials per weight, the tail group
    (33, 5, 32, 2, 2, False, False),      # no residual over two layers
    (131, 19, 64, 8, 1, True, False),     # d_head 8 at D = 64
    (7, 17, 32, 1, 1, True, False),       # d_head 32 at D = 32
]
# beyond the sweep: more sample groups than the grid's cap (SATRANS_INTERACTING_MAX_WORKGROUPS = 512 of 16 samples), so that a
# workgroup walks several passes and its weight-gradient accumulators carry over; the last workgroup's walk is the shorter one
WALK = (512 * 16 + 77, 2, 16, 2, 1, True, False)
# (dnn_hidden_units, dense_dim) of the head tests, by the case's place in SWEEP
HEAD_EXTRAS = [((16, 8), 1), ((), 0), ((16, 8), 0), ((16, 8), 1), ((), 1), ((16, 8), 0), ((), 0), ((16, 8), 1), ((16, 8), 0), ((), 0)]
ALONE = [SWEEP[2], SWEEP[3], SWEEP[6], SWEEP[8]]


def case_id(c) -> str:
    return f"B{c[0]}-F{c[1]}-D{c[2]}-H{c[3]}-L{c[4]}{'' if c[5] else '-nores'}{'-scaled' if c[6] else ''}"


def double(P):
    conv = lambda v: ([conv(t) for t in v] if isinstance(v, list) else {k: conv(t) for k, t in v.items()} if isinstance(v, dict)  # noqa: E731
                      else v.double())
    return {k: conv(v) for k, v in P.items()}


# ---- the layer, literally ---------------------------------------------------------------------------------------------------------

@dataclass
class LayerCache:
    W: Dict
    head_num: int
    scaling: bool
    x: Tensor            # the input [B, F, D]
    q: Tensor            # [H, B, F, dh]
    k: Tensor
    v: Tensor
    p: Tensor            # normalized_att_scores [H, B, F, F]
    pre: Tensor          # o + r [B, F, D], before the relu


def layer_forward(x: Tensor, W: Dict, head_num: int, scaling: bool = False):
    """y [B, F, D] and the cache: deepctr's InteractingLayer.forward (use_res: "W_Res" in W)."""
    dh = x.shape[2] // head_num
    querys = torch.tensordot(x, W["W_Query"], dims=([-1], [0]))
    keys = torch.tensordot(x, W["W_key"], dims=([-1], [0]))
    values = torch.tensordot(x, W["W_Value"], dims=([-1], [0]))
    querys = torch.stack(torch.split(querys, dh, dim=2))
    keys = torch.stack(torch.split(keys, dh, dim=2))
    values = torch.stack(torch.split(values, dh, dim=2))
    inner_product = torch.einsum('bnik,bnjk->bnij', querys, keys)
    if scaling:
        inner_product = inner_product / dh ** 0.5
    p = F.softmax(inner_product, dim=-1)
    result = torch.matmul(p, values)
    result = torch.cat(torch.split(result, 1, ), dim=-1)
    result = torch.squeeze(result, dim=0)
    if "W_Res" in W:
        result = result + torch.tensordot(x, W["W_Res"], dims=([-1], [0]))
    return F.relu(result), LayerCache(W, head_num, scaling, x, querys, keys, values, p, result)


def _heads(t: Tensor, dh: int) -> Tensor:
    return torch.stack(torch.split(t, dh, dim=2))


def _merge(t: Tensor) -> Tensor:
    return torch.squeeze(torch.cat(torch.split(t, 1, ), dim=-1), dim=0)


def layer_backward(dy: Tensor, c: LayerCache):
    """dx [B, F, D] and the weight gradients under LAYER_KEYS of sum(y * dy)."""
    D = c.x.shape[2]
    dh = D // c.head_num
    dt = dy * (c.pre > 0)
    do = _heads(dt, dh)
    dv = torch.einsum('hbij,hbid->hbjd', c.p, do)
    dp = torch.einsum('hbid,hbjd->hbij', do, c.v)
    ds = c.p * (dp - (c.p * dp).sum(-1, keepdim=True))
    if c.scaling:
        ds = ds / dh ** 0.5
    dq = torch.einsum('hbij,hbjd->hbid', ds, c.k)
    dk = torch.einsum('hbij,hbid->hbjd', ds, c.q)
    parts = {"W_Query": _merge(dq), "W_key": _merge(dk), "W_Value": _merge(dv)}
    if "W_Res" in c.W:
        parts["W_Res"] = dt
    x2 = c.x.reshape(-1, D)
    dx = sum(g @ c.W[k].T for k, g in parts.items())
    return dx, {k: x2.T @ g.reshape(-1, D) for k, g in parts.items()}


# ---- the head ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Cache:
    """What the backward needs of the head's forward."""
    P: Dict
    emb: Tensor
    dense: Optional[Tensor]
    layers: List[LayerCache]
    att: Tensor                  # att_output [B, F D]
    X: Optional[Tensor]          # the DNN input (None without a DNN)
    zs: List[Tensor]             # the DNN's pre-activations


def stack_forward(x: Tensor, layers: List[Dict], head_num: int, scaling: bool = False):
    caches = []
    for W in layers:
        x, c = layer_forward(x, W, head_num, scaling)
        caches.append(c)
    return x, caches


def forward(emb: Tensor, dense, P, head_num: int, scaling: bool = False):
    """logit [B, 1] and the Cache (autoint.py:93-121; the caller applies the sigmoid)."""
    y, caches = stack_forward(emb, P["int"], head_num, scaling)
    att = torch.flatten(y, start_dim=1)
    X, zs, stack_out = None, [], att
    if P["dnn_w"]:
        flat_emb = torch.flatten(emb, start_dim=1)
        X = flat_emb if dense is None else torch.cat([flat_emb, dense], dim=-1)
        h = X
        for w, b in zip(P["dnn_w"], P["dnn_b"]):
            zs.append(h @ w.T + b)
            h = torch.relu(zs[-1])
        stack_out = torch.cat([att, h], dim=-1)
    return stack_out @ P["lin"].T + P["out_bias"], Cache(P, emb, dense, caches, att, X, zs)


def backward(dlogit: Tensor, c: Cache) -> Dict:
    """Gradients of sum(logit * dlogit): "int" (a list of dicts), "dnn_w", "dnn_b", "lin", "out_bias", "emb", "dense" (None
    without dense columns read)."""
    P = c.P
    B, F_, D = c.emb.shape
    n_att = F_ * D
    hs = [c.X] + [torch.relu(z) for z in c.zs]
    stack_out = torch.cat([c.att, hs[-1]], dim=-1) if c.zs else c.att
    g = {"out_bias": dlogit.sum(0), "lin": dlogit.T @ stack_out, "dense": None, "dnn_w": [None] * len(c.zs),
         "dnn_b": [None] * len(c.zs), "int": [None] * len(c.layers)}
    dstack = dlogit @ P["lin"]
    de = torch.zeros_like(c.emb)
    if c.zs:
        dh = dstack[:, n_att:]
        for l in range(len(c.zs) - 1, -1, -1):
            dz = dh * (c.zs[l] > 0)
            g["dnn_w"][l], g["dnn_b"][l] = dz.T @ hs[l], dz.sum(0)
            dh = dz @ P["dnn_w"][l]
        de = de + dh[:, :n_att].reshape(B, F_, D)
        if c.dense is not None:
            g["dense"] = dh[:, n_att:]
    dy = dstack[:, :n_att].reshape(B, F_, D)
    for l in range(len(c.layers) - 1, -1, -1):
        dy, g["int"][l] = layer_backward(dy, c.layers[l])
    g["emb"] = de + dy
    return g


def flat(g: Dict) -> Dict[str, Tensor]:
    """The gradient (or parameter) dict spread: one tensor per name ("int.{l}.{W}", "dnn_w.{l}", ...)."""
    out = {}
    for k, v in g.items():
        if k == "int":
            out.update({f"int.{l}.{name}": t for l, W in enumerate(v) for name, t in W.items()})
        elif isinstance(v, list):
            out.update({f"{k}.{l}": t for l, t in enumerate(v)})
        elif v is not None:
            out[k] = v
    return out


# ---- the reference's names --------------------------------------------------------------------------------------------------------

def keys_of(n_layers: int, n_dnn: int, use_res: bool = True) -> List[str]:
    """state_dict() keys of the reference model's head entries, in its order: `out` first (the reference's BaseModel registers it
    before the model builds its own modules), dnn_linear before dnn (autoint.py:66-72), the interacting layers last."""
    dnn = [f"dnn.linears.{l}.{p}" for l in range(n_dnn) for p in ("weight", "bias")]
    names = LAYER_KEYS if use_res else LAYER_KEYS[:3]
    return ["out.bias", "dnn_linear.weight"] + dnn + [f"int_layers.{l}.{k}" for l in range(n_layers) for k in names]


def params_from_state(sd, dtype=torch.float64):
    """P of a state_dict with the reference's keys."""
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)      # noqa: E731
    n = 0
    while f"dnn.linears.{n}.weight" in sd:
        n += 1
    L = 0
    while f"int_layers.{L}.W_Query" in sd:
        L += 1
    return {"int": [{k: t(f"int_layers.{l}.{k}") for k in LAYER_KEYS if f"int_layers.{l}.{k}" in sd} for l in range(L)],
            "dnn_w": [t(f"dnn.linears.{l}.weight") for l in range(n)], "dnn_b": [t(f"dnn.linears.{l}.bias") for l in range(n)],
            "lin": t("dnn_linear.weight"), "out_bias": t("out.bias")}


def state_from_params(P) -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by the reference's names, in its order."""
    sd = {"out.bias": P["out_bias"], "dnn_linear.weight": P["lin"]}
    for l, (w, b) in enumerate(zip(P["dnn_w"], P["dnn_b"])):
        sd[f"dnn.linears.{l}.weight"], sd[f"dnn.linears.{l}.bias"] = w, b
    for l, W in enumerate(P["int"]):
        sd.update({f"int_layers.{l}.{k}": W[k] for k in LAYER_KEYS if k in W})
    return sd


# ---- seeded draws -----------------------------------------------------------------------------------------------------------------

def kink_margins(c: Cache) -> List[float]:
    """Per relu tensor (every interacting layer's o + r, then the DNN's pre-activations): min|z| / max|z|."""
    return [float(z.abs().min() / z.abs().max()) for z in [lc.pre for lc in c.layers] + c.zs]


def near_kink(c: Cache, rel: float) -> Tensor:
    """[B] bool: samples with a relu pre-activation (a layer's o + r, the DNN's) within rel * max|.| of its tensor of zero."""
    bad = torch.zeros(c.emb.shape[0], dtype=torch.bool)
    for z in [lc.pre.flatten(1) for lc in c.layers] + c.zs:
        bad |= (z.abs() < rel * z.abs().max()).any(1)
    return bad


@functools.lru_cache(maxsize=None)
def draw(case, dnn=(), dense_dim=0, rel: float = 1.01e-4, rounds: int = 4000):
    """Seeded fp32 inputs of a case, all from one generator (seed 9300 + B + F + D + H + layers + DNN layers + dense_dim): emb
    [B, F, D] N(0, 1), dense [B, dense_dim] N(0, 1) (or None), the interacting weights N(0, 1 / D), the DNN's weights N(0, 1)
    n_in^-1/2 and biases 0.3 N(0, 1), dnn_linear N(0, 1) n_in^-1/2, out.bias 0.3 N(0, 1); upstream weights up_y [B, F, D] (for a
    layer or the stack alone) and up [B, 1] (for the logit), N(0, 1).  Samples whose fp64 forward puts a relu pre-activation
    within `rel` of its tensor's max|.| of zero are drawn again from the same generator until none is left: a differently
    ordered fp32 sum then cannot flip a relu.  That is decided by the fp64 restatement alone, never by the code under test.  The
    loop ends on the forward whose tensors it checked, so the margins of the returned draw are at least `rel`: the premise
    test asks 1e-4 of them.
    -> emb, dense, up_y, up, P, rounds used.  Drawn once per argument set and shared: callers leave the tensors unchanged."""
    B, F_, D, H, L, use_res, scaling = case
    g = torch.Generator().manual_seed(9300 + B + F_ + D + H + L + len(dnn) + dense_dim)
    emb = torch.randn(B, F_, D, generator=g)
    dense = torch.randn(B, dense_dim, generator=g) if dense_dim else None
    up_y, up = torch.randn(B, F_, D, generator=g), torch.randn(B, 1, generator=g)
    P = {"int": [{k: torch.randn(D, D, generator=g) * D ** -0.5 for k in (LAYER_KEYS if use_res else LAYER_KEYS[:3])}
                 for _ in range(L)], "dnn_w": [], "dnn_b": []}
    n = F_ * D + dense_dim
    for width in dnn:
        P["dnn_w"].append(torch.randn(width, n, generator=g) * n ** -0.5)
        P["dnn_b"].append(0.3 * torch.randn(width, generator=g))
        n = width
    n = F_ * D + (dnn[-1] if dnn else 0)
    P["lin"] = torch.randn(1, n, generator=g) * n ** -0.5
    P["out_bias"] = 0.3 * torch.randn(1, generator=g)
    Pd = double(P)
    for used in range(rounds):
        _, c = forward(emb.double(), None if dense is None or not dnn else dense.double(), Pd, H, scaling)
        idx = near_kink(c, rel).nonzero().flatten()
        if idx.numel() == 0:
            return emb, dense, up_y, up, P, used
        emb[idx] = torch.randn(idx.numel(), F_, D, generator=g)
        if dense is not None:
            dense[idx] = torch.randn(idx.numel(), dense_dim, generator=g)
    raise RuntimeError(f"draw: samples near a kink are left after {rounds} rounds")
