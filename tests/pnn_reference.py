"""Torch restatement of PNN's inner and outer product layers and head (deepctr-torch 0.2.9's InnerProductLayer and
OutterProductLayer, which the reference's models/pnn.py:14,61,65 calls, and pnn.py:91-114), forward in deepctr's LITERAL form and
the explicit backward formulas  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Everything runs in the dtype of its input (fp64 for what the kernels are held against).  `P` holds the parameters:
    P["kernel"]                             the outer product's: [D, P, D] ('mat'), [P, D] ('vec'), [P, 1] ('num'); absent
                                            without use_outter
    P["dnn_w"], P["dnn_b"]                  lists: the DNN's Linear layers
    P["lin"] [1, n], P["out_bias"] [1]      dnn_linear.weight, out.bias
Literal form: the two gathers p = cat(e_i over the pairs), q = cat(e_j over the pairs), each [B, P, D]; 'mat' as
mul(p.unsqueeze(1), kernel) -> sum(-1) -> transpose(2, 1) -> * q -> sum(-1), through the [B, D, P, D] product; 'vec' / 'num' as
sum(p * q * kernel.unsqueeze(0), -1) - not the per-pair products the kernels use.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

Tensor = torch.Tensor
TYPES = ("mat", "vec", "num")
FIXTURES = ("inner", "mat", "vec", "num", "both")      # tests/golden/pnn/*.npz
# what a fixture's name stands for: (use_inner, use_outter, kernel_type)
FIXTURE_CONFIG = {"inner": (True, False, "mat"), "mat": (False, True, "mat"), "vec": (False, True, "vec"),
                  "num": (False, True, "num"), "both": (True, True, "mat")}
# the shape sweep of tests/test_pnn_gpu.py, whose premise tests/test_pnn_cpu.py checks:
# (B, F, D, use_inner, use_outter, kernel_type, dnn_hidden_units, dense_dim).  SATRANS_PNN_DW_ROW_CHUNK is 256.
SWEEP = [
    (5, 2, 8, True, True, "mat", (16,), 0),                 # one pair
    (70, 4, 4, True, True, "vec", (16, 8), 1),              # D shorter than a k step; two row tiles; odd rows
    (131, 19, 32, True, True, "mat", (128, 128), 0),        # AliCCP's F, D; ragged row tile
    (37, 5, 33, False, True, "mat", (16,), 3),              # D one past a step; outer only
    (300, 3, 64, True, False, "mat", (8,), 0),              # inner only; two weight-gradient chunks (of the DNN's)
    (20, 7, 128, True, True, "mat", (), 1),                 # D at its limit, two column tiles in the reduction; no DNN
    (9, 64, 4, True, True, "num", (8,), 0),                 # F at its limit, P = 2016
    (260, 6, 16, True, True, "num", (64, 64, 64), 0),       # three layers; one row tile past a 256 chunk
    (33, 6, 16, False, False, "mat", (16,), 2),             # neither product
    (129, 19, 32, False, True, "vec", (32,), 0),            # 'vec' at AliCCP's shape
]
# the shapes of the alone-equals-batch test (cases 2 and 4) and of the two-runs test (cases 3 and 8), counted from one and from
# zero: both readings of the numbers are run
ALONE = [SWEEP[1], SWEEP[2], SWEEP[3], SWEEP[4]]
TWICE = [SWEEP[2], SWEEP[3], SWEEP[7], SWEEP[8]]


def case_id(c) -> str:
    return (f"B{c[0]}-F{c[1]}-D{c[2]}-{'i' if c[3] else ''}{'o' if c[4] else ''}{'' if c[3] or c[4] else 'plain'}-{c[5]}-"
            f"dnn{'x'.join(map(str, c[6])) or 'none'}-dense{c[7]}")


def pairs(F: int):
    """(i, j), i < j, in the order of deepctr's double loop."""
    return [(i, j) for i in range(F - 1) for j in range(i + 1, F)]


def kernel_shape(F: int, D: int, kind: str):
    n = F * (F - 1) // 2
    return {"mat": (D, n, D), "vec": (n, D), "num": (n, 1)}[kind]


def double(P):
    return {k: [t.double() for t in v] if isinstance(v, list) else v.double() for k, v in P.items()}


# ---- the layers, literally --------------------------------------------------------------------------------------------------------

def gathers(x: Tensor):
    """deepctr's p, q [B, P, D]: the pairs' first and second fields from the list of [B, 1, D] pieces."""
    pieces = torch.split(x, 1, dim=1)
    row, col = zip(*pairs(x.shape[1]))
    return torch.cat([pieces[i] for i in row], dim=1), torch.cat([pieces[j] for j in col], dim=1)


def inner(x: Tensor) -> Tensor:
    """[B, P, 1]: deepctr's InnerProductLayer(reduce_sum=True)."""
    p, q = gathers(x)
    return torch.sum(p * q, dim=2, keepdim=True)


def outer(x: Tensor, kernel: Tensor, kind: str) -> Tensor:
    """[B, P]: deepctr's OutterProductLayer."""
    p, q = gathers(x)
    if kind == "mat":
        p = p.unsqueeze(1)
        return torch.sum(torch.mul(torch.transpose(torch.sum(torch.mul(p, kernel), dim=-1), 2, 1), q), dim=-1)
    return torch.sum(p * q * kernel.unsqueeze(0), dim=-1)


def inner_backward(dout: Tensor, x: Tensor) -> Tensor:
    """dx of sum(inner(x)[:, :, 0] * dout), dout [B, P]:  de_i += g_p e_j,  de_j += g_p e_i."""
    dx = torch.zeros_like(x)
    for p, (i, j) in enumerate(pairs(x.shape[1])):
        g = dout[:, p:p + 1]
        dx[:, i] += g * x[:, j]
        dx[:, j] += g * x[:, i]
    return dx


def outer_backward(dout: Tensor, x: Tensor, kernel: Tensor, kind: str):
    """dx, dkernel of sum(outer(x) * dout), dout [B, P]."""
    dx, dk = torch.zeros_like(x), torch.zeros_like(kernel)
    for p, (i, j) in enumerate(pairs(x.shape[1])):
        g = dout[:, p:p + 1]
        if kind == "mat":
            K = kernel[:, p, :]                      # [n, k]
            dx[:, j] += g * (x[:, i] @ K.T)          # g_p (K_p e_i)
            dx[:, i] += (g * x[:, j]) @ K            # K_p^T (g_p e_j)
            dk[:, p, :] += (g * x[:, j]).T @ x[:, i]
        else:
            c = kernel[p]                            # [D] or [1]
            dx[:, i] += g * c * x[:, j]
            dx[:, j] += g * c * x[:, i]
            gpq = g * x[:, i] * x[:, j]
            dk[p] += gpq.sum(0) if kind == "vec" else gpq.sum().reshape(1)
    return dx, dk


# ---- the head ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Cache:
    """What the backward needs of a forward."""
    P: Dict
    cfg: tuple               # (use_inner, use_outter, kernel_type)
    emb: Tensor
    dense: Optional[Tensor]
    X: Tensor                # the DNN input [B, F D + P use_inner + P use_outter + dense]
    zs: List[Tensor]         # the DNN's pre-activations


def dnn_input(emb: Tensor, dense, P, cfg):
    use_inner, use_outter, kind = cfg
    parts = [torch.flatten(emb, start_dim=1)]
    if use_inner:
        parts.append(torch.flatten(inner(emb), start_dim=1))
    if use_outter:
        parts.append(outer(emb, P["kernel"], kind))
    if dense is not None:
        parts.append(dense)
    return torch.cat(parts, dim=1)


def blocks(F: int, D: int, cfg, dense_dim: int):
    """name -> (first column, width) of the DNN input's blocks."""
    n = F * (F - 1) // 2
    out, at = {}, 0
    for name, width in (("linear", F * D), ("inner", n if cfg[0] else 0), ("outer", n if cfg[1] else 0), ("dense", dense_dim)):
        if width:
            out[name] = (at, width)
        at += width
    return out


def forward(emb: Tensor, dense, P, cfg):
    """logit [B,1] and the Cache."""
    X = dnn_input(emb, dense, P, cfg)
    h, zs = X, []
    for w, b in zip(P["dnn_w"], P["dnn_b"]):
        zs.append(h @ w.T + b)
        h = torch.relu(zs[-1])
    return h @ P["lin"].T + P["out_bias"], Cache(P, tuple(cfg), emb, dense, X, zs)


def backward(dlogit: Tensor, c: Cache) -> Dict:
    """Gradients of sum(logit * dlogit): "kernel" (with use_outter), "dnn_w", "dnn_b" (lists), "lin", "out_bias", "emb", "dense"
    (None without dense columns)."""
    P = c.P
    hs = [c.X] + [torch.relu(z) for z in c.zs]
    g = {"out_bias": dlogit.sum(0), "lin": dlogit.T @ hs[-1], "dnn_w": [None] * len(c.zs), "dnn_b": [None] * len(c.zs)}
    dh = dlogit @ P["lin"]
    for l in range(len(c.zs) - 1, -1, -1):
        dz = dh * (c.zs[l] > 0)
        g["dnn_w"][l], g["dnn_b"][l] = dz.T @ hs[l], dz.sum(0)
        dh = dz @ P["dnn_w"][l]
    B, F, D = c.emb.shape
    where = blocks(F, D, c.cfg, 0 if c.dense is None else c.dense.shape[1])
    cut = lambda name: dh[:, where[name][0]:where[name][0] + where[name][1]]      # noqa: E731
    de = cut("linear").reshape(B, F, D).clone()
    if c.cfg[0]:
        de = de + inner_backward(cut("inner"), c.emb)
    if c.cfg[1]:
        dx, g["kernel"] = outer_backward(cut("outer"), c.emb, P["kernel"], c.cfg[2])
        de = de + dx
    g["emb"] = de
    g["dense"] = None if c.dense is None else cut("dense")
    return g


def flat(g: Dict) -> Dict[str, Tensor]:
    """The gradient (or parameter) dict with the lists spread: one tensor per name."""
    out = {}
    for k, v in g.items():
        if isinstance(v, list):
            out.update({f"{k}.{l}": t for l, t in enumerate(v)})
        elif v is not None:
            out[k] = v
    return out


# ---- the reference's names --------------------------------------------------------------------------------------------------------

def keys_of(use_outter: bool, n_dnn: int) -> List[str]:
    """state_dict() keys of the reference PNN's head entries, in its order (`out` first: the reference's BaseModel registers it
    before PNN builds its own modules; the inner product layer has no parameters)."""
    return (["out.bias"] + (["outterproduct.kernel"] if use_outter else []) +
            [f"dnn.linears.{l}.{p}" for l in range(n_dnn) for p in ("weight", "bias")] + ["dnn_linear.weight"])


def params_from_state(sd, dtype=torch.float64):
    """P of a state_dict with the reference's keys."""
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)      # noqa: E731
    n = 0
    while f"dnn.linears.{n}.weight" in sd:
        n += 1
    P = {"dnn_w": [t(f"dnn.linears.{l}.weight") for l in range(n)], "dnn_b": [t(f"dnn.linears.{l}.bias") for l in range(n)],
         "lin": t("dnn_linear.weight"), "out_bias": t("out.bias")}
    if "outterproduct.kernel" in sd:
        P["kernel"] = t("outterproduct.kernel")
    return P


def state_from_params(P) -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by the reference's names, in its order."""
    sd = {"out.bias": P["out_bias"]}
    if P.get("kernel") is not None:
        sd["outterproduct.kernel"] = P["kernel"]
    for l, (w, b) in enumerate(zip(P["dnn_w"], P["dnn_b"])):
        sd[f"dnn.linears.{l}.weight"], sd[f"dnn.linears.{l}.bias"] = w, b
    sd["dnn_linear.weight"] = P["lin"]
    return sd


def reg_loss(sd, l2_reg_dnn: float) -> Tensor:
    """[1]: what the entries PNN.__init__ itself appends to regularization_weight sum to (pnn.py:74-76): the DNN's weights
    (not biases) and dnn_linear.weight, each torch.sum(l2 * torch.square(w))."""
    total = torch.zeros((1,), dtype=sd["dnn_linear.weight"].dtype)
    for k, v in sd.items():
        if (k.startswith("dnn.") and k.endswith("weight")) or k == "dnn_linear.weight":
            total = total + torch.sum(l2_reg_dnn * torch.square(v))
    return total


# ---- seeded draws -----------------------------------------------------------------------------------------------------------------

def near_kink(c: Cache, rel: float) -> Tensor:
    """[B] bool: samples with a DNN pre-activation within rel * max(relu z of its layer) of zero."""
    bad = torch.zeros(c.emb.shape[0], dtype=torch.bool)
    for z in c.zs:
        bad |= (z.abs() < rel * torch.relu(z).max()).any(1)
    return bad


def draw(B: int, F: int, D: int, use_inner: bool, use_outter: bool, kind: str, dnn, dense_dim: int, seed: int, rel: float = 2e-5,
         rounds: int = 64):
    """Seeded fp32 inputs of the GPU tests, all from one generator: emb [B,F,D] N(0.5,1), dense [B,dense_dim] N(0,1) (or None),
    an upstream weight per logit up [B,1] N(0,1), kernel N(0,1) D^-1/2 (with use_outter), DNN weights N(0,1) n_in^-1/2, biases
    0.3 N(0,1), out.bias 0.3 N(0,1).

    The samples that put a pre-activation of the fp64 forward near a kink (near_kink) are drawn again from the same generator
    until none is left.  That is decided by the fp64 restatement alone, never by the code under test.  RuntimeError when
    `rounds` rounds do not suffice."""
    g = torch.Generator().manual_seed(seed)
    cfg = (use_inner, use_outter, kind)
    emb = torch.randn(B, F, D, generator=g) + 0.5
    dense = torch.randn(B, dense_dim, generator=g) if dense_dim else None
    up = torch.randn(B, 1, generator=g)
    P = {"dnn_w": [], "dnn_b": []}
    if use_outter:
        P["kernel"] = torch.randn(*kernel_shape(F, D, kind), generator=g) * D ** -0.5
    n = sum(w for _, w in blocks(F, D, cfg, dense_dim).values())
    for width in dnn:
        P["dnn_w"].append(torch.randn(width, n, generator=g) * n ** -0.5)
        P["dnn_b"].append(0.3 * torch.randn(width, generator=g))
        n = width
    P["lin"] = torch.randn(1, n, generator=g) * n ** -0.5
    P["out_bias"] = 0.3 * torch.randn(1, generator=g)
    for _ in range(rounds):
        _, c = forward(emb.double(), None if dense is None else dense.double(), double(P), cfg)
        idx = near_kink(c, rel).nonzero().flatten()
        if idx.numel() == 0:
            return emb, dense, up, P
        emb[idx] = torch.randn(idx.numel(), F, D, generator=g) + 0.5
        if dense is not None:
            dense[idx] = torch.randn(idx.numel(), dense_dim, generator=g)
    raise RuntimeError(f"draw: samples near a kink are left after {rounds} rounds")


def sweep_draw(case):
    B, F, D, use_inner, use_outter, kind, dnn, dense_dim = case
    return draw(B, F, D, use_inner, use_outter, kind, dnn, dense_dim, 7000 + B + F + D + len(dnn))
