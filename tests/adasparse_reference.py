"""Torch restatement of AdaSparse's scenario-pruned DNN and its logit layer (the reference's models/adasparse.py:88-106 with
use_bn = False, relu, no dropout, and :185-189), forward and the explicit backward formulas  --  TEST INFRASTRUCTURE, NOT
PRODUCT CODE.

Everything runs in the dtype of `x` (fp64 for what the kernels are held against).  `P` holds (lists run over the layers):

    P["lin_w"][l] [n_l, n_{l-1}]        P["lin_b"][l] [n_l]                       n_0 = C
    P["prn_w"][l] [n_l, n_{l-1} + E]    P["prn_b"][l] [n_l]
    P["final_w"]  [1, n_L]              P["out_bias"] [1]

    fc = h W^T + b,   z = [h | e] P^T + c,   pi = beta sigmoid(alpha z),  pi = 0 where |pi| - epsilon <= 0,   h' = relu(fc pi)
    logit = h_L final_w^T + out_bias

`consts` = (alpha, beta, epsilon); the reference's defaults are (1, 2.0, 0.25).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
DEFAULTS = (1.0, 2.0, 0.25)
LISTS = ("lin_w", "lin_b", "prn_w", "prn_b")
SINGLES = ("final_w", "out_bias")
# the shape sweep of tests/test_adasparse_gpu.py, whose premise tests/test_adasparse_cpu.py checks: (C, E, widths).  The second
# puts the x / embedding seam inside a contraction step of 32, the third on a step's edge with a whole embedding-only step.
SWEEP = [(1, 1, (16,)), (33, 4, (48, 32)), (64, 32, (80, 24, 24)), (609, 32, (24, 24, 24))]
# the pruners' weight scale of a sweep case (2.0 unless listed): a condition of the draw - per layer a pruned share in [0.1, 0.6]
PRUNER_SCALE: Dict[tuple, float] = {}


@dataclass
class Cache:
    """What the backward needs of a forward."""
    P: Dict[str, object]
    consts: tuple
    e: Tensor
    hs: List[Tensor]       # hs[0] = x, hs[l + 1] = output of layer l
    fcs: List[Tensor]
    zs: List[Tensor]       # the pruners' pre-activations
    raw: List[Tensor]      # beta sigmoid(alpha z) before the cut
    pis: List[Tensor]      # after it


def forward(x: Tensor, e: Tensor, P, consts=DEFAULTS, head: bool = True):
    """logit [B,1] (h_L with head=False) and the Cache."""
    alpha, beta, eps = consts
    hs, fcs, zs, raw, pis = [x], [], [], [], []
    for W, b, Pw, c in zip(P["lin_w"], P["lin_b"], P["prn_w"], P["prn_b"]):
        h = hs[-1]
        fc = h @ W.T + b
        z = torch.cat([h, e], 1) @ Pw.T + c
        r = beta * torch.sigmoid(alpha * z)
        pi = torch.where(r.abs() - eps <= 0, torch.zeros_like(r), r)
        fcs.append(fc), zs.append(z), raw.append(r), pis.append(pi)
        hs.append(torch.relu(fc * pi))
    cache = Cache(P, consts, e, hs, fcs, zs, raw, pis)
    if not head:
        return hs[-1], cache
    return hs[-1] @ P["final_w"].T + P["out_bias"], cache


def backward(dout: Tensor, c: Cache, head: bool = True) -> Dict[str, object]:
    """Gradients of sum(out * dout), keyed like P, and "x" [B,C], "emb" [B,E].  With g = dh (fc pi > 0):
        dfc = g pi,   dz = g fc alpha pi (1 - pi / beta) where pi != 0 and exactly 0 where pruned,
        dh_below = dfc W + dz P[:, :K],   demb += dz P[:, K:],   dW = dfc^T h,  dP = dz^T [h | e],  db, dc the column sums."""
    P = c.P
    alpha, beta, _ = c.consts
    g: Dict[str, object] = {k: [None] * len(P[k]) for k in LISTS}
    if head:
        g["final_w"] = dout.T @ c.hs[-1]
        g["out_bias"] = dout.sum().reshape(1)
        dh = dout @ P["final_w"]
    else:
        dh = dout
    de = torch.zeros_like(c.e)
    for l in range(len(P["lin_w"]) - 1, -1, -1):
        h, fc, pi = c.hs[l], c.fcs[l], c.pis[l]
        K = h.shape[1]
        gm = dh * (fc * pi > 0)
        dfc = gm * pi
        dz = torch.where(pi != 0, gm * fc * alpha * pi * (1 - pi / beta), torch.zeros_like(pi))
        g["lin_w"][l], g["lin_b"][l] = dfc.T @ h, dfc.sum(0)
        g["prn_w"][l], g["prn_b"][l] = dz.T @ torch.cat([h, c.e], 1), dz.sum(0)
        dh = dfc @ P["lin_w"][l] + dz @ P["prn_w"][l][:, :K]
        de = de + dz @ P["prn_w"][l][:, K:]
    g["x"], g["emb"] = dh, de
    return g


def torch_form(x: Tensor, e: Tensor, P, consts=DEFAULTS, head: bool = True) -> Tensor:
    """The reference's DNN_w_Pruner.forward statement with torch ops (autograd gives its backward), then dnn_linear and the
    out bias: the baseline of tools/adasparse_time.py and the other side of the explicit backward's test."""
    alpha, beta, eps = consts
    h = x
    for W, b, Pw, c in zip(P["lin_w"], P["lin_b"], P["prn_w"], P["prn_b"]):
        fc = F.linear(h, W, b)
        pi = beta * torch.sigmoid(alpha * F.linear(torch.cat([h, e], dim=1), Pw, c))
        pi[(pi.abs() - eps) <= 0] = 0.0
        h = torch.relu(fc * pi)
    return F.linear(h, P["final_w"]) + P["out_bias"] if head else h


def keys_of(L: int) -> List[str]:
    """state_dict() keys of the reference AdaSparse's head entries, in its order (`out` first: BaseModel registers it)."""
    return (["out.bias"] + [f"dnn.linears.{l}.{p}" for l in range(L) for p in ("weight", "bias")] +
            [f"dnn.pruners.{l}.{p}" for l in range(L) for p in ("weight", "bias")] + ["dnn_linear.weight"])


def params_from_state(sd, L: int, dtype=torch.float64):
    t = lambda k: torch.as_tensor(sd[k]).to(dtype)      # noqa: E731
    return dict(lin_w=[t(f"dnn.linears.{l}.weight") for l in range(L)], lin_b=[t(f"dnn.linears.{l}.bias") for l in range(L)],
                prn_w=[t(f"dnn.pruners.{l}.weight") for l in range(L)], prn_b=[t(f"dnn.pruners.{l}.bias") for l in range(L)],
                final_w=t("dnn_linear.weight"), out_bias=t("out.bias"))


def state_from_params(P) -> Dict[str, Tensor]:
    """The inverse of params_from_state: tensors (or gradients) keyed by the reference's parameter names."""
    out = {"out.bias": P["out_bias"], "dnn_linear.weight": P["final_w"]}
    for l in range(len(P["lin_w"])):
        out[f"dnn.linears.{l}.weight"], out[f"dnn.linears.{l}.bias"] = P["lin_w"][l], P["lin_b"][l]
        out[f"dnn.pruners.{l}.weight"], out[f"dnn.pruners.{l}.bias"] = P["prn_w"][l], P["prn_b"][l]
    return out


def near_a_discontinuity(c: Cache, rel: float) -> Tensor:
    """[B] bool: the rows with a unit within rel * (largest value of that layer) of relu's kink (fc pi at 0 for an unpruned
    unit) or of the pruning threshold (beta sigmoid(alpha z) at epsilon)."""
    eps = c.consts[2]
    near = torch.zeros(c.hs[0].shape[0], dtype=torch.bool)
    for fc, r, pi, h in zip(c.fcs, c.raw, c.pis, c.hs[1:]):
        near |= ((pi != 0) & ((fc * pi).abs() < rel * float(h.max()))).any(1)
        near |= ((r - eps).abs() < rel * float(r.max())).any(1)
    return near


def margins(c: Cache):
    """(relu margin, threshold margin): the smallest |fc pi| / max h of an unpruned unit and the smallest
    |beta sigmoid(alpha z) - epsilon| / max of it, over the layers.  Derivatives and the cut can be held to an output bound
    `rel` only when both exceed it."""
    eps = c.consts[2]
    relu = min(float((fc * pi).abs()[pi != 0].min() / h.max()) for fc, pi, h in zip(c.fcs, c.pis, c.hs[1:]))
    thr = min(float((r - eps).abs().min() / r.max()) for r in c.raw)
    return relu, thr


def pruned_shares(c: Cache) -> List[float]:
    return [float((pi == 0).double().mean()) for pi in c.pis]


def draw(B: int, C: int, E: int, widths, seed: int, consts=DEFAULTS, rel: float = 2e-5, pruner_scale: float = 2.0, tweak=None,
         emb_of=None):
    """Seeded fp32 inputs of the GPU tests: x [B,C], emb [B,E] and upstream weights w [B,1] N(0,1); weights N(0,1) n_in^-1/2,
    biases 0.3 N(0,1); the pruners' weights times `pruner_scale` and their biases shifted by -1 (at torch's default
    initialisation nothing is ever pruned).

    Rows that the fp64 forward puts within rel * (largest value of the layer) of either discontinuity - relu's kink or the
    pruning threshold - are drawn again (x and emb) from the same generator until none is left; rows are replaced, never
    dropped.  The argument is that of tests/star_reference.py::redraw_rows_at_a_kink: on the wrong side of either, a unit's
    whole contribution moves, and rounding alone decides the side.  Decided by the fp64 forward alone, never by the code under
    test.  Asserted: the loop ends within 20 rounds, and every layer prunes between 0.1 and 0.6 of its units (a condition on
    the inputs: the tests are about pruning).

    `tweak(P)` edits the drawn parameters in place before the loop (a test that forces units pruned or kept; the share is then
    not asserted).  `emb_of(emb)` maps the drawn emb to the embeddings the rows use (rows sharing a table's rows); only x is
    drawn again then, and the mapped emb is returned."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g)
    e = torch.randn(B, E, generator=g)
    w = torch.randn(B, 1, generator=g)
    P = {k: [] for k in LISTS}
    n_in = C
    for n in widths:
        P["lin_w"].append(torch.randn(n, n_in, generator=g) * n_in ** -0.5)
        P["lin_b"].append(0.3 * torch.randn(n, generator=g))
        P["prn_w"].append(pruner_scale * torch.randn(n, n_in + E, generator=g) * (n_in + E) ** -0.5)
        P["prn_b"].append(0.3 * torch.randn(n, generator=g) - 1.0)
        n_in = n
    P["final_w"] = torch.randn(1, n_in, generator=g) * n_in ** -0.5
    P["out_bias"] = 0.3 * torch.randn(1, generator=g)
    if tweak is not None:
        tweak(P)
    if emb_of is not None:
        e = emb_of(e)
    for _ in range(20):
        _, c = forward(x.double(), e.double(), double(P), consts)
        idx = near_a_discontinuity(c, rel).nonzero().flatten()
        if idx.numel() == 0:
            break
        x[idx] = torch.randn(idx.numel(), C, generator=g)
        if emb_of is None:
            e[idx] = torch.randn(idx.numel(), E, generator=g)
    else:
        raise AssertionError("rows near a discontinuity were still left after 20 rounds")
    shares = pruned_shares(c)
    assert tweak is not None or all(0.1 <= s <= 0.6 for s in shares), shares
    return x, e, w, P


def sweep_draw(case, B: int):
    C, E, widths = case
    return draw(B, C, E, widths, 2000 + C + E, pruner_scale=PRUNER_SCALE.get(case, 2.0))


def double(P):
    return {k: ([t.double() for t in v] if isinstance(v, list) else v.double()) for k, v in P.items()}


def flat(g) -> Dict[str, Tensor]:
    """{"lin_w[0]": tensor, ...}: the tensors of P or of a gradient dict, one key each."""
    out = {}
    for k, v in g.items():
        if isinstance(v, list):
            out.update({f"{k}[{l}]": t for l, t in enumerate(v)})
        else:
            out[k] = v
    return out
