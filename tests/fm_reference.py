"""Torch restatement of FM, BiInteractionPooling and AFMLayer (deepctr-torch 0.2.9, which the reference's models/deepfm.py, nfm.py
and afm.py import) and of the three heads behind the lookup (deepfm.py:87-113, nfm.py:73-83, afm.py:66-73), forward in deepctr's
LITERAL form and the explicit backward formulas  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Everything runs in the dtype of its input (fp64 for what the kernels are held against).  `P` holds the parameters:
    AFM      P["W"] [D, A], P["b"] [A], P["h"] [A, 1], P["p"] [D, 1], P["out_bias"] [1]
    DNN      P["dnn_w"], P["dnn_b"] (lists: the DNN's Linear layers), P["lin"] [1, n] (dnn_linear.weight; absent without a DNN),
             P["out_bias"] [1]
Literal form: FM and the pooling through pow(sum(x, 1), 2) - sum(x * x, 1); AFM through the two gathers p = cat(e_i over the
pairs), q = cat(e_j over the pairs), each [B, P, D], tensordot with attention_W and projection_h, softmax over dim 1 - the
[B, P, D] tensors the kernels never form.
"""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
FIXTURES = ("deepfm", "deepfm_nodnn", "nfm", "afm", "afm_wide")      # tests/golden/fm/*.npz
FIXTURE_KIND = {"deepfm": "deepfm", "deepfm_nodnn": "deepfm", "nfm": "nfm", "afm": "afm", "afm_wide": "afm"}
# the AFM sweep of tests/test_fm_gpu.py, whose premise tests/test_fm_cpu.py checks: (B, F, D, A)
AFM_SWEEP = [
    (5, 2, 8, 4),           # one pair: the softmax is exactly 1; d attention_W, d attention_b, d projection_h exactly zero
    (70, 4, 4, 8),          # D shorter than a k step
    (131, 19, 32, 8),       # AliCCP
    (129, 15, 32, 8),       # Alimama's F
    (37, 5, 33, 5),         # odd D and odd A
    (20, 7, 128, 16),       # D at its limit
    (9, 64, 8, 4),          # F at its limit, P = 2016
    (260, 6, 16, 64),       # A at its limit; more than one partial of the parameter gradients
    (1, 3, 16, 8),          # one sample
]
# the head sweep: (kind, B, F, D, dnn_hidden_units, dense_dim, use_fm)
HEAD_SWEEP = [
    ("deepfm", 131, 19, 32, (128, 128), 0, True),       # AliCCP's F, D; ragged row tile
    ("deepfm", 70, 4, 4, (16, 8), 1, True),             # small D; two row tiles; a dense column
    ("deepfm", 37, 5, 33, (16,), 3, False),             # odd D; the DNN alone (`nofm`)
    ("deepfm", 20, 7, 128, (), 0, True),                # D at its limit; the FM term alone (`nodnn`)
    ("nfm", 131, 19, 32, (128, 128), 0, True),          # AliCCP
    ("nfm", 260, 6, 16, (64, 64, 64), 2, True),         # three layers; one row tile past a 256 chunk
    ("nfm", 9, 64, 4, (8,), 0, True),                   # F at its limit
    ("nfm", 300, 3, 64, (8,), 0, True),                 # two weight-gradient chunks; D of one wave exactly
]
AFM_ALONE = [AFM_SWEEP[1], AFM_SWEEP[2], AFM_SWEEP[4], AFM_SWEEP[7]]
HEAD_ALONE = [HEAD_SWEEP[0], HEAD_SWEEP[1], HEAD_SWEEP[5], HEAD_SWEEP[7]]


def afm_id(c) -> str:
    return f"B{c[0]}-F{c[1]}-D{c[2]}-A{c[3]}"


def head_id(c) -> str:
    return f"{c[0]}-B{c[1]}-F{c[2]}-D{c[3]}-dnn{'x'.join(map(str, c[4])) or 'none'}-dense{c[5]}{'' if c[6] else '-nofm'}"


def pairs(F_: int):
    """(i, j), i < j, in itertools.combinations order."""
    return list(itertools.combinations(range(F_), 2))


def double(P):
    return {k: [t.double() for t in v] if isinstance(v, list) else v.double() for k, v in P.items()}


# ---- the layers, literally --------------------------------------------------------------------------------------------------------

def fm(x: Tensor) -> Tensor:
    """[B, 1]: deepctr's FM."""
    square_of_sum = torch.pow(torch.sum(x, dim=1, keepdim=True), 2)
    sum_of_square = torch.sum(x * x, dim=1, keepdim=True)
    return 0.5 * torch.sum(square_of_sum - sum_of_square, dim=2, keepdim=False)


def bipool(x: Tensor) -> Tensor:
    """[B, 1, D]: deepctr's BiInteractionPooling."""
    square_of_sum = torch.pow(torch.sum(x, dim=1, keepdim=True), 2)
    sum_of_square = torch.sum(x * x, dim=1, keepdim=True)
    return 0.5 * (square_of_sum - sum_of_square)


def fm_backward(dout: Tensor, x: Tensor) -> Tensor:
    """dx of sum(fm(x) * dout), dout [B, 1]:  de_f = dout (S - e_f)."""
    return dout[:, :, None] * (x.sum(1, keepdim=True) - x)


def bipool_backward(dout: Tensor, x: Tensor) -> Tensor:
    """dx of sum(bipool(x) * dout), dout [B, 1, D]:  de_fd = dout_d (S_d - e_fd)."""
    return dout * (x.sum(1, keepdim=True) - x)


def gathers(x: Tensor):
    """deepctr's p, q [B, P, D] from the list of [B, 1, D] pieces."""
    pieces = torch.split(x, 1, dim=1)
    row, col = zip(*itertools.combinations(pieces, 2))
    return torch.cat(row, dim=1), torch.cat(col, dim=1)


@dataclass
class AfmCache:
    P: Dict
    x: Tensor            # the input [B, F, D]
    bi: Tensor           # p * q [B, P, D]
    z: Tensor            # the pre-activations [B, P, A]
    a: Tensor            # normalized_att_score [B, P, 1]
    ao: Tensor           # the attention output [B, D]


def afm(x: Tensor, P):
    """out [B, 1] (without linear_logit and out.bias) and the cache: deepctr's AFMLayer.forward."""
    p, q = gathers(x)
    bi = p * q
    z = torch.tensordot(bi, P["W"], dims=([-1], [0])) + P["b"]
    a = F.softmax(torch.tensordot(F.relu(z), P["h"], dims=([-1], [0])), dim=1)
    ao = torch.sum(a * bi, dim=1)
    return torch.tensordot(ao, P["p"], dims=([-1], [0])), AfmCache(P, x, bi, z, a, ao)


def afm_backward(dout: Tensor, c: AfmCache) -> Dict:
    """Gradients of sum(afm(x) * dout), dout [B, 1]: "W", "b", "h", "p", "emb"."""
    P = c.P
    do = dout @ P["p"].T                                        # [B, D]
    da = (c.bi * do[:, None, :]).sum(-1, keepdim=True)          # [B, P, 1]
    ds = c.a * (da - (c.a * da).sum(1, keepdim=True))
    dt = ds * P["h"].T * (c.z > 0)                              # [B, P, A]
    dx = c.a * do[:, None, :] + dt @ P["W"].T                   # [B, P, D]
    de = torch.zeros_like(c.x)
    for n, (i, j) in enumerate(pairs(c.x.shape[1])):
        de[:, i] += dx[:, n] * c.x[:, j]
        de[:, j] += dx[:, n] * c.x[:, i]
    return {"W": torch.einsum("bpd,bpa->da", c.bi, dt), "b": dt.sum((0, 1)), "h": (ds * torch.relu(c.z)).sum((0, 1))[:, None],
            "p": (c.ao * dout).sum(0)[:, None], "emb": de}


# ---- the heads --------------------------------------------------------------------------------------------------------------------

@dataclass
class Cache:
    """What the backward needs of a head's forward."""
    P: Dict
    kind: str
    use_fm: bool
    emb: Tensor
    dense: Optional[Tensor]
    X: Optional[Tensor]          # the DNN input (None without a DNN)
    zs: List[Tensor]             # the DNN's pre-activations
    afm: Optional[AfmCache]


def blocks(kind: str, F_: int, D: int, dense_dim: int):
    """name -> (first column, width) of the DNN input's blocks."""
    out, at = {}, 0
    for name, width in (("emb", D if kind == "nfm" else F_ * D), ("dense", dense_dim)):
        if width:
            out[name] = (at, width)
        at += width
    return out


def forward(kind: str, emb: Tensor, dense, lin_logit, P, use_fm=True):
    """logit [B, 1] and the Cache.  kind: "deepfm", "nfm", "afm"."""
    logit = torch.zeros(emb.shape[0], 1, dtype=emb.dtype) if lin_logit is None else lin_logit.clone()
    X, zs, ac = None, [], None
    if kind == "afm":
        out, ac = afm(emb, P)
        logit = logit + out
    else:
        if kind == "deepfm" and use_fm:
            logit = logit + fm(emb)
        if P["dnn_w"]:
            first = torch.flatten(bipool(emb), start_dim=1) if kind == "nfm" else torch.flatten(emb, start_dim=1)
            X = first if dense is None else torch.cat([first, dense], dim=-1)
            h = X
            for w, b in zip(P["dnn_w"], P["dnn_b"]):
                zs.append(h @ w.T + b)
                h = torch.relu(zs[-1])
            logit = logit + h @ P["lin"].T
    return logit + P["out_bias"], Cache(P, kind, use_fm, emb, dense, X, zs, ac)


def backward(dlogit: Tensor, c: Cache) -> Dict:
    """Gradients of sum(logit * dlogit): the parameters under P's names, "emb", "dense" (None without dense columns read),
    "lin_logit" (= dlogit)."""
    P = c.P
    g = {"out_bias": dlogit.sum(0), "lin_logit": dlogit.clone(), "dense": None}
    if c.kind == "afm":
        g.update(afm_backward(dlogit, c.afm))
        return g
    de = torch.zeros_like(c.emb)
    if c.kind == "deepfm" and c.use_fm:
        de = de + fm_backward(dlogit, c.emb)
    g["dnn_w"], g["dnn_b"] = [None] * len(c.zs), [None] * len(c.zs)
    if c.zs:
        hs = [c.X] + [torch.relu(z) for z in c.zs]
        g["lin"] = dlogit.T @ hs[-1]
        dh = dlogit @ P["lin"]
        for l in range(len(c.zs) - 1, -1, -1):
            dz = dh * (c.zs[l] > 0)
            g["dnn_w"][l], g["dnn_b"][l] = dz.T @ hs[l], dz.sum(0)
            dh = dz @ P["dnn_w"][l]
        B, F_, D = c.emb.shape
        where = blocks(c.kind, F_, D, 0 if c.dense is None else c.dense.shape[1])
        cut = lambda name: dh[:, where[name][0]:where[name][0] + where[name][1]]      # noqa: E731
        de = de + (bipool_backward(cut("emb")[:, None, :], c.emb) if c.kind == "nfm" else cut("emb").reshape(B, F_, D))
        if c.dense is not None:
            g["dense"] = cut("dense")
    g["emb"] = de
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

AFM_KEYS = {"fm.attention_W": "W", "fm.attention_b": "b", "fm.projection_h": "h", "fm.projection_p": "p"}


def keys_of(kind: str, n_dnn: int = 0) -> List[str]:
    """state_dict() keys of the reference model's head entries, in its order (`out` first: the reference's BaseModel registers it
    before the model builds its own modules; FM and BiInteractionPooling have no parameters)."""
    if kind == "afm":
        return ["out.bias"] + list(AFM_KEYS)
    dnn = [f"dnn.linears.{l}.{p}" for l in range(n_dnn) for p in ("weight", "bias")]
    return ["out.bias"] + dnn + (["dnn_linear.weight"] if n_dnn else [])


def params_from_state(sd, dtype=torch.float64):
    """P of a state_dict with the reference's keys."""
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)      # noqa: E731
    if "fm.attention_W" in sd:
        return {"out_bias": t("out.bias"), **{name: t(k) for k, name in AFM_KEYS.items()}}
    n = 0
    while f"dnn.linears.{n}.weight" in sd:
        n += 1
    P = {"dnn_w": [t(f"dnn.linears.{l}.weight") for l in range(n)], "dnn_b": [t(f"dnn.linears.{l}.bias") for l in range(n)],
         "out_bias": t("out.bias")}
    if n:
        P["lin"] = t("dnn_linear.weight")
    return P


def state_from_params(P) -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by the reference's names, in its order."""
    sd = {"out.bias": P["out_bias"]}
    if "W" in P:
        sd.update({k: P[name] for k, name in AFM_KEYS.items()})
        return sd
    for l, (w, b) in enumerate(zip(P["dnn_w"], P["dnn_b"])):
        sd[f"dnn.linears.{l}.weight"], sd[f"dnn.linears.{l}.bias"] = w, b
    if P.get("lin") is not None:
        sd["dnn_linear.weight"] = P["lin"]
    return sd


def reg_loss(sd, l2: float) -> Tensor:
    """[1]: what the entries the model's own __init__ appends to regularization_weight sum to, each torch.sum(l2 *
    torch.square(w)): DeepFM / NFM the DNN's weights (not biases) and dnn_linear.weight with l2_reg_dnn (deepfm.py:66-68,
    nfm.py:53-55); AFM fm.attention_W with l2_reg_att (afm.py:49)."""
    total = torch.zeros((1,), dtype=sd["out.bias"].dtype)
    for k, v in sd.items():
        if (k.startswith("dnn.") and k.endswith("weight")) or k in ("dnn_linear.weight", "fm.attention_W"):
            total = total + torch.sum(l2 * torch.square(v))
    return total


# ---- seeded draws -----------------------------------------------------------------------------------------------------------------

def near_kink(c: Cache, rel: float) -> Tensor:
    """[B] bool: samples with a relu pre-activation (the DNN's, AFM's [B, P, A]) within rel * max(relu z of its tensor) of zero."""
    bad = torch.zeros(c.emb.shape[0], dtype=torch.bool)
    for z in c.zs + ([c.afm.z.flatten(1)] if c.afm is not None else []):
        bad |= (z.abs() < rel * torch.relu(z).max()).any(1)
    return bad


def _redraw(kind, emb, dense, lin_logit, P, use_fm, g, rel, rounds):
    """Samples whose fp64 forward puts a pre-activation near a kink are drawn again from the same generator until none is
    left.  That is decided by the fp64 restatement alone, never by the code under test."""
    for used in range(rounds):
        _, c = forward(kind, emb.double(), None if dense is None else dense.double(), lin_logit.double(), double(P), use_fm)
        idx = near_kink(c, rel).nonzero().flatten()
        if idx.numel() == 0:
            return used
        emb[idx] = torch.randn(idx.numel(), *emb.shape[1:], generator=g) + 0.5
        if dense is not None:
            dense[idx] = torch.randn(idx.numel(), dense.shape[1], generator=g)
    raise RuntimeError(f"draw: samples near a kink are left after {rounds} rounds")


def afm_draw(case, rel: float = 2e-5, rounds: int = 64):
    """Seeded fp32 inputs of an AFM case, all from one generator (seed 9000 + B + F + D + A): emb [B, F, D] N(0.5, 1), lin_logit
    [B, 1] N(0, 1), an upstream weight per logit up [B, 1] N(0, 1), attention_W N(0, 1) D^-1/2, attention_b 0.3 N(0, 1),
    projection_h N(0, 1) A^-1/2, projection_p N(0, 1) D^-1/2, out.bias 0.3 N(0, 1).  -> emb, lin_logit, up, P, rounds used."""
    B, F_, D, A = case
    g = torch.Generator().manual_seed(9000 + B + F_ + D + A)
    emb = torch.randn(B, F_, D, generator=g) + 0.5
    lin_logit, up = torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g)
    P = {"W": torch.randn(D, A, generator=g) * D ** -0.5, "b": 0.3 * torch.randn(A, generator=g),
         "h": torch.randn(A, 1, generator=g) * A ** -0.5, "p": torch.randn(D, 1, generator=g) * D ** -0.5,
         "out_bias": 0.3 * torch.randn(1, generator=g)}
    used = _redraw("afm", emb, None, lin_logit, P, True, g, rel, rounds)
    return emb, lin_logit, up, P, used


def head_draw(case, rel: float = 2e-5, rounds: int = 64):
    """Seeded fp32 inputs of a head case (seed 9100 + B + F + D + layers): emb N(0.5, 1), dense [B, dense_dim] N(0, 1) (or None),
    lin_logit, up [B, 1] N(0, 1), DNN weights N(0, 1) n_in^-1/2, biases 0.3 N(0, 1), out.bias 0.3 N(0, 1).
    -> emb, dense, lin_logit, up, P, rounds used."""
    kind, B, F_, D, dnn, dense_dim, use_fm = case
    g = torch.Generator().manual_seed(9100 + B + F_ + D + len(dnn))
    emb = torch.randn(B, F_, D, generator=g) + 0.5
    dense = torch.randn(B, dense_dim, generator=g) if dense_dim else None
    lin_logit, up = torch.randn(B, 1, generator=g), torch.randn(B, 1, generator=g)
    P = {"dnn_w": [], "dnn_b": []}
    n = sum(w for _, w in blocks(kind, F_, D, dense_dim).values())
    for width in dnn:
        P["dnn_w"].append(torch.randn(width, n, generator=g) * n ** -0.5)
        P["dnn_b"].append(0.3 * torch.randn(width, generator=g))
        n = width
    if dnn:
        P["lin"] = torch.randn(1, n, generator=g) * n ** -0.5
    P["out_bias"] = 0.3 * torch.randn(1, generator=g)
    used = _redraw(kind, emb, dense, lin_logit, P, use_fm, g, rel, rounds)
    return emb, dense, lin_logit, up, P, used
