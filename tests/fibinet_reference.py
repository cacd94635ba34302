"""Torch restatement of FiBiNET's SENet layer, bilinear interaction and head (deepctr-torch 0.2.9's SENETLayer and
BilinearInteraction, which the reference's models/fibinet.py:51-52,93-95 calls, and fibinet.py:91-112), forward in deepctr's
LITERAL form and the explicit backward formulas  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Everything runs in the dtype of its input (fp64 for what the kernels are held against).  `P` holds the parameters:
    P["w1"] [R, F], P["w2"] [F, R]          the excitation's two bias-free Linears
    P["bil"] [nW, D, D]                     the bilinear Linears' weights stacked in deepctr's order (nW = 1, F or F (F - 1) / 2)
    P["dnn_w"], P["dnn_b"]                  lists: the DNN's Linear layers
    P["lin"] [1, n], P["out_bias"] [1]      dnn_linear.weight, out.bias
Literal form: the SENet block is Bilinear applied to V = e * A, the raw block Bilinear applied to e - two runs of the same
module, a Linear and a product per pair, a cat over the pairs - not the factored a_i a_j (W e_i * e_j) the kernels use.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

Tensor = torch.Tensor
TYPES = ("all", "each", "interaction")
# the shape sweep of tests/test_fibinet_gpu.py, whose premise tests/test_fibinet_cpu.py checks:
# (B, F, D, type, reduction_ratio, dnn_hidden_units, dense_dim)
SWEEP = [
    (5, 2, 8, "interaction", 3, (16,), 0),              # one pair, R = 1
    (70, 4, 4, "interaction", 3, (16, 8), 1),           # D shorter than a k step; two row tiles; rows of odd length
    (131, 19, 32, "interaction", 3, (128, 128), 0),     # AliCCP; ragged row tiles and chunks
    (37, 5, 33, "each", 1, (16,), 3),                   # D one past a step, odd rows, R = F, the unused last weight
    (300, 3, 64, "all", 3, (8,), 0),                    # the shared weight summed over pairs and two chunks
    (20, 7, 128, "interaction", 7, (), 1),              # D at its limit (two column tiles), no DNN
    (9, 64, 4, "all", 3, (8,), 0),                      # F at its limit, P = 2016
    (260, 6, 16, "each", 2, (64, 64, 64), 0),           # three DNN layers, one row past a chunk
]
ALONE = [SWEEP[1], SWEEP[3]]      # the shapes of the alone-equals-batch test


def case_id(c) -> str:
    return f"B{c[0]}-F{c[1]}-D{c[2]}-{c[3]}-r{c[4]}-dnn{'x'.join(map(str, c[5])) or 'none'}-dense{c[6]}"


def pairs(F: int):
    return list(itertools.combinations(range(F), 2))


def n_weights(F: int, kind: str) -> int:
    return {"all": 1, "each": F, "interaction": F * (F - 1) // 2}[kind]


def weight_index(kind: str, i: int, p: int) -> int:
    return {"all": 0, "each": i, "interaction": p}[kind]


def double(P):
    return {k: [t.double() for t in v] if isinstance(v, list) else v.double() for k, v in P.items()}


# ---- the layers, literally --------------------------------------------------------------------------------------------------------

def senet(x: Tensor, w1: Tensor, w2: Tensor):
    """V [B,F,D] and (Z, pre1, pre2): the mean, the two pre-activations."""
    Z = torch.mean(x, dim=-1)
    pre1 = Z @ w1.T
    pre2 = torch.relu(pre1) @ w2.T
    return x * torch.relu(pre2).unsqueeze(2), (Z, pre1, pre2)


def senet_backward(dV: Tensor, x: Tensor, w1: Tensor, w2: Tensor, mid):
    """dx, dw1, dw2 of sum(V * dV)."""
    Z, pre1, pre2 = mid
    h, A = torch.relu(pre1), torch.relu(pre2)
    dp2 = (dV * x).sum(-1) * (pre2 > 0)
    dp1 = (dp2 @ w2) * (pre1 > 0)
    dZ = dp1 @ w1
    return dV * A.unsqueeze(2) + dZ.unsqueeze(2) / x.shape[2], dp1.T @ Z, dp2.T @ h


def bilinear(x: Tensor, bil: Tensor, kind: str) -> Tensor:
    """[B,P,D]: cat over the pairs of Linear_w(x_i) * x_j."""
    out = [(x[:, i:i + 1] @ bil[weight_index(kind, i, p)].T) * x[:, j:j + 1] for p, (i, j) in enumerate(pairs(x.shape[1]))]
    return torch.cat(out, dim=1)


def bilinear_backward(dout: Tensor, x: Tensor, bil: Tensor, kind: str):
    """dx, dbil of sum(bilinear(x) * dout): per pair  dq = dout_p * x_j,  dx_j += dout_p * q,  dx_i += dq W,  dW += dq^T x_i."""
    dx, dbil = torch.zeros_like(x), torch.zeros_like(bil)
    for p, (i, j) in enumerate(pairs(x.shape[1])):
        w = weight_index(kind, i, p)
        q = x[:, i] @ bil[w].T
        dq = dout[:, p] * x[:, j]
        dx[:, j] += dout[:, p] * q
        dx[:, i] += dq @ bil[w]
        dbil[w] += dq.T @ x[:, i]
    return dx, dbil


# ---- the head ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Cache:
    """What the backward needs of a forward."""
    P: Dict
    kind: str
    emb: Tensor
    dense: Optional[Tensor]
    V: Tensor
    mid: tuple               # (Z, pre1, pre2) of the excitation
    X: Tensor                # the DNN input [B, 2 P D + dense]
    zs: List[Tensor]         # the DNN's pre-activations


def dnn_input(emb: Tensor, dense, P, kind: str):
    V, mid = senet(emb, P["w1"], P["w2"])
    both = torch.cat((bilinear(V, P["bil"], kind), bilinear(emb, P["bil"], kind)), dim=1)
    X = both.flatten(1) if dense is None else torch.cat([both.flatten(1), dense], -1)
    return X, V, mid


def forward(emb: Tensor, dense, P, kind: str):
    """logit [B,1] (without linear_logit) and the Cache."""
    X, V, mid = dnn_input(emb, dense, P, kind)
    h, zs = X, []
    for w, b in zip(P["dnn_w"], P["dnn_b"]):
        zs.append(h @ w.T + b)
        h = torch.relu(zs[-1])
    return h @ P["lin"].T + P["out_bias"], Cache(P, kind, emb, dense, V, mid, X, zs)


def backward(dlogit: Tensor, c: Cache) -> Dict:
    """Gradients of sum(logit * dlogit): "w1", "w2", "bil", "dnn_w", "dnn_b" (lists), "lin", "out_bias", "emb", "dense"
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
    n = F * (F - 1) // 2
    dS, dR = dh[:, :n * D].reshape(B, n, D), dh[:, n * D:2 * n * D].reshape(B, n, D)
    g["dense"] = None if c.dense is None else dh[:, 2 * n * D:]
    dV, dbil_s = bilinear_backward(dS, c.V, P["bil"], c.kind)
    de, dbil_r = bilinear_backward(dR, c.emb, P["bil"], c.kind)
    de_s, g["w1"], g["w2"] = senet_backward(dV, c.emb, P["w1"], P["w2"], c.mid)
    g["bil"], g["emb"] = dbil_s + dbil_r, de + de_s
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

def bilinear_keys(F: int, kind: str, prefix: str = "Bilinear.") -> List[str]:
    return [f"{prefix}bilinear.weight"] if kind == "all" else [f"{prefix}bilinear.{i}.weight" for i in range(n_weights(F, kind))]


def keys_of(F: int, kind: str, n_dnn: int) -> List[str]:
    """state_dict() keys of the reference FiBiNET's head entries, in its order (`out` first: the reference's BaseModel registers
    it before FiBiNET builds its own modules)."""
    return (["out.bias", "SE.excitation.0.weight", "SE.excitation.2.weight"] + bilinear_keys(F, kind) +
            [f"dnn.linears.{l}.{p}" for l in range(n_dnn) for p in ("weight", "bias")] + ["dnn_linear.weight"])


def params_from_state(sd, F: int, kind: str, dtype=torch.float64):
    """P of a state_dict with the reference's keys."""
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)      # noqa: E731
    n = 0
    while f"dnn.linears.{n}.weight" in sd:
        n += 1
    return {"w1": t("SE.excitation.0.weight"), "w2": t("SE.excitation.2.weight"),
            "bil": torch.stack([t(k) for k in bilinear_keys(F, kind)]),
            "dnn_w": [t(f"dnn.linears.{l}.weight") for l in range(n)], "dnn_b": [t(f"dnn.linears.{l}.bias") for l in range(n)],
            "lin": t("dnn_linear.weight"), "out_bias": t("out.bias")}


def state_from_params(P, F: int, kind: str) -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by the reference's names, in its order."""
    sd = {"out.bias": P["out_bias"], "SE.excitation.0.weight": P["w1"], "SE.excitation.2.weight": P["w2"]}
    sd.update({k: P["bil"][i] for i, k in enumerate(bilinear_keys(F, kind))})
    for l, (w, b) in enumerate(zip(P["dnn_w"], P["dnn_b"])):
        sd[f"dnn.linears.{l}.weight"], sd[f"dnn.linears.{l}.bias"] = w, b
    sd["dnn_linear.weight"] = P["lin"]
    return sd


def head_forward(emb: Tensor, dense, linear_logit, sd, kind: str):
    """logit [B,1] of the reference's FiBiNET.forward behind the lookup (fibinet.py:91-110, before `out`'s sigmoid)."""
    logit = forward(emb, dense, params_from_state(sd, emb.shape[1], kind, emb.dtype), kind)[0]
    return logit if linear_logit is None else linear_logit + logit


def reg_loss(sd) -> Tensor:
    """[1]: what the entries FiBiNET.__init__ itself appends to regularization_weight sum to.  It appends none (the
    reference's fibinet.py has no add_regularization_weight call; l2_reg_linear reaches BaseModel's linear model only)."""
    return torch.zeros((1,), dtype=sd["dnn_linear.weight"].dtype)


# ---- seeded draws -----------------------------------------------------------------------------------------------------------------

def near_kink(c: Cache, rel: float) -> Tensor:
    """[B] bool: samples with a pre-activation within rel * max(relu z of its layer) of zero.  The kinks are both excitation
    relus and every DNN relu.  A second excitation pre-activation that is EXACTLY zero does not count: it is the sum over hidden
    units that are all exactly zero, in any precision, and both derivatives there are zero on either side."""
    _, pre1, pre2 = c.mid
    bad = (pre1.abs() < rel * torch.relu(pre1).max()).any(1)
    bad |= ((pre2.abs() < rel * torch.relu(pre2).max()) & (pre2 != 0)).any(1)
    for z in c.zs:
        bad |= (z.abs() < rel * torch.relu(z).max()).any(1)
    return bad


def gates_ok(a: Tensor) -> bool:
    """At least one (row, field) with a = 0 and at least half with a > 0: a dead SENet block would hide its kernels, and so
    would one without a shut gate."""
    return bool((a == 0).any()) and int((a > 0).sum()) * 2 >= a.numel()


def draw(B: int, F: int, D: int, kind: str, ratio: int, dnn, dense_dim: int, seed: int, rel: float = 2e-5, rounds: int = 64):
    """Seeded fp32 inputs of the GPU tests, all from one generator: emb [B,F,D] N(0.5,1) (a mean, so that the excitation sees
    more than noise), dense [B,dense_dim] N(0,1) (or None), an upstream weight per logit up [B,1], w1 (N(0,1) + 0.8) F^-1/2, w2
    (N(0,1) + 0.8) R^-1/2 (the shifts open most gates and leave some shut), bilinear weights N(0,1) D^-1/2, DNN weights N(0,1)
    n_in^-1/2, biases 0.3 N(0,1), out.bias 0.3 N(0,1).

    The samples that put a pre-activation of the fp64 forward near a kink (near_kink) are drawn again from the same generator
    until none is left; then, unless the gates of the fp64 forward satisfy gates_ok, the excitation's two weights are drawn
    again and the kinks looked at anew.  All of that is decided by the fp64 restatement alone, never by the code under test.
    RuntimeError when `rounds` rounds do not suffice."""
    g = torch.Generator().manual_seed(seed)
    R = max(1, F // ratio)
    emb = torch.randn(B, F, D, generator=g) + 0.5
    dense = torch.randn(B, dense_dim, generator=g) if dense_dim else None
    up = torch.randn(B, 1, generator=g)
    P = {"w1": None, "w2": None, "bil": torch.randn(n_weights(F, kind), D, D, generator=g) * D ** -0.5, "dnn_w": [], "dnn_b": []}
    n = F * (F - 1) * D + dense_dim
    for width in dnn:
        P["dnn_w"].append(torch.randn(width, n, generator=g) * n ** -0.5)
        P["dnn_b"].append(0.3 * torch.randn(width, generator=g))
        n = width
    P["lin"] = torch.randn(1, n, generator=g) * n ** -0.5
    P["out_bias"] = 0.3 * torch.randn(1, generator=g)
    for _ in range(rounds):
        P["w1"] = (torch.randn(R, F, generator=g) + 0.8) * F ** -0.5
        P["w2"] = (torch.randn(F, R, generator=g) + 0.8) * R ** -0.5
        for _ in range(rounds):
            _, c = forward(emb.double(), None if dense is None else dense.double(), double(P), kind)
            idx = near_kink(c, rel).nonzero().flatten()
            if idx.numel() == 0:
                break
            emb[idx] = torch.randn(idx.numel(), F, D, generator=g) + 0.5
            if dense is not None:
                dense[idx] = torch.randn(idx.numel(), dense_dim, generator=g)
        else:
            raise RuntimeError(f"draw: samples near a kink are left after {rounds} rounds")
        if gates_ok(gates(c)):
            return emb, dense, up, P
    raise RuntimeError(f"draw: no excitation with open and shut gates in {rounds} rounds")


def sweep_draw(case):
    B, F, D, kind, ratio, dnn, dense_dim = case
    return draw(B, F, D, kind, ratio, dnn, dense_dim, 7000 + B + F + D + len(dnn))


def gates(case_or_cache) -> Tensor:
    """a [B, F] of a Cache."""
    return torch.relu(case_or_cache.mid[2])
