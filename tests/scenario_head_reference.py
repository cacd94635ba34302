"""fp64 restatements of csrc/scenario.hip and csrc/head.hip, the seeded inputs of their direct tests and the per-element
error bounds those tests hold the kernels to  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The restatements are plain torch in the dtype of their inputs (fp64 for what the kernels are held against, fp32 for the
premise test), the backward is autograd.  tests/test_scenario_head_cpu.py pins each of them to the oracle's own functions
(O.scenario_embedding / _encoder / _vectors, the tail of O.forward, O.bce_sum, F.mse_loss, F.l1_loss).

Bounds.  u = 2^-24.  An fp32 sum of n terms - in any order, with or without fma - obeys |err| <= (n + 2) u sum|terms|
(`sum_bound`); sum|terms| is the same product taken on absolute values, n the kernel's longest chain of dependent additions:

    tab[s,p]          ceil(De/32) fma per lane (scenario.hip:20) + 5 butterfly steps (:22) + the bias add (:23); |bias| in the sum
    head logit        4 ceil(FD/256) fma per lane (head.hip:38-44) + ceil(n_dense/64) (:45-46) + 6 butterfly steps (:17) + bias (:47)
    g_W, g_bias       S (scenario.hip:84-88)
    g_emb             ceil(ceil(P/kSlices)/kSub) fma of a sub-slice (:97-103) + kSub (:110) + kSlices (:122)
    E                 C adds and one division (:149-150): (C + 1) u sum|rows| / C; one column: the row itself, exactly;
                      the position columns: one add (:152)
    g_tables, g_lay,  the rows of g_E that are summed (:168-172, :183-184, :192-193), plus one for the division by C
    g_role
    head g_w, g_b,    kSamplesPerBlock = 8 in the block (head.hip:79-96) + ceil(nblk/kReduceGroups) of a group's share (:114-118)
    fp32 loss part    + kReduceGroups (:127,:132)

In the chain inputs_fwd -> table_fwd -> table_bwd -> inputs_bwd the kernels pass their rounding on, so the bounds add what
the previous stage's bound can do to this stage's result: relu is 1-Lipschitz, every later stage is linear in the passed
value (`table_reference(e_emb=...)`, `inputs_bwd_reference(e_gE=...)`).

The head is checked in two stages, because fp32 BCE is not close to fp64 BCE once 1 - p loses bits: the logit against the
fp64 logit within the bound above, the probability within 0.25 of it + 4 u (sigmoid' <= 1/4; expf, one add, one division),
and the loss / gradient pieces against the kernel's formulas (head.hip:55-66, clamps included) evaluated in fp64 ON THE
KERNEL'S OWN STORED fp32 PROBABILITY (`loss_pieces`): dlogit within 4 u, the loss within 4 u (1 + |loss|) per sample.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn.functional as F

Tensor = torch.Tensor
U = 2.0 ** -24
K_SLICES, K_SUB = 32, 8            # scenario.hip:46
SAMPLES_PER_BLOCK = 8              # head.hip:13
REDUCE_GROUPS = 16                 # common.h:18
MAX_SCENARIO_COLUMNS = 8           # scenario.hip:132
BCE, MSE, MAE = 0, 1, 2            # SATRANS_LOSS_*
LOSS_NAMES = {BCE: "bce", MSE: "mse", MAE: "mae"}
DLOGIT_BOUND = 4 * U               # per sample
LOSS_REL = 4 * U                   # per sample: LOSS_REL * (1 + |loss|)


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def sum_bound(n, abs_terms: Tensor) -> Tensor:
    """|fp32 sum - exact sum| of n terms whose absolute values add up to `abs_terms` (n: int or a tensor of counts)."""
    return (n + 2) * U * abs_terms


def ratio(got: Tensor, want: Tensor, bound: Tensor) -> float:
    """The largest |got - want| / bound; an element with bound 0 must be exact (ratio 0 when it is, inf when not)."""
    err = (got.double() - want.double()).abs().reshape(-1)
    bound = bound.double().expand_as(got.double()).reshape(-1)
    if err.numel() == 0:
        return 0.0
    if bool(torch.isnan(err).any()):
        return float("inf")
    zero = bound == 0
    if bool((err[zero] != 0).any()):
        return float("inf")
    rest = ~zero
    return float((err[rest] / bound[rest]).max()) if bool(rest.any()) else 0.0


# =====================================================================================================================
# csrc/scenario.hip
# =====================================================================================================================
def table_fwd(emb: Tensor, W: Tensor, bias: Tensor) -> Tensor:
    """tab = relu(emb) W^T + bias  (O.scenario_embedding's relu, O.scenario_encoder's Linear)."""
    return F.linear(torch.relu(emb), W, bias)


def n_tab(De: int) -> int:
    return ceil_div(De, 32) + 5 + 1


def n_g_emb(P: int) -> int:
    return ceil_div(ceil_div(P, K_SLICES), K_SUB) + K_SUB + K_SLICES


def table_bounds(e: Tensor, w: Tensor, b: Tensor, g: Tensor, e_emb: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """Bounds of tab, g_emb, g_W, g_bias for fp64 copies e [S,De], w [P,De], b [P], g = g_tab [S,P] of the fp32 operands.
    `e_emb` [S,De]: what the kernel's own `emb` may be off by (the chain: emb is the E of inputs_fwd); None = exact input."""
    S, De = e.shape
    P = w.shape[0]
    r = torch.relu(e)
    out = {"tab": sum_bound(n_tab(De), r @ w.abs().T + b.abs()),
           "g_W": sum_bound(S, g.abs().T @ r),
           "g_bias": sum_bound(S, g.abs().sum(0)),
           "g_emb": sum_bound(n_g_emb(P), (g.abs() @ w.abs()) * (e > 0))}
    if e_emb is not None:
        out["tab"] = out["tab"] + e_emb @ w.abs().T
        out["g_W"] = out["g_W"] + g.abs().T @ e_emb
    return out


def table_reference(emb: Tensor, W: Tensor, bias: Tensor, g_tab: Tensor):
    """(want, bound): fp64 tab, g_emb, g_W, g_bias of the fp32 operands and their bounds."""
    e, w, b = (t.double().requires_grad_(True) for t in (emb, W, bias))
    g = g_tab.double()
    tab = table_fwd(e, w, b)
    (tab * g).sum().backward()
    want = {"tab": tab.detach(), "g_emb": e.grad, "g_W": w.grad, "g_bias": b.grad}
    return want, table_bounds(e.detach(), w.detach(), b.detach(), g)


def composite_index(sizes: Sequence[int]) -> Tensor:
    """The engine's index of a model with several scenario columns (engine.py: one row per id tuple, the last column
    running fastest): index[c][s] = (s // stride_c) % sizes[c], int32 [C, S]."""
    S = math.prod(sizes)
    strides, acc = [], 1
    for v in reversed(sizes):
        strides.insert(0, acc)
        acc *= v
    comp = torch.arange(S)
    return torch.stack([(comp // st) % v for st, v in zip(strides, sizes)]).to(torch.int32)


def inputs_fwd(tables: List[Tensor], index: Optional[Tensor], S: int, lay: Optional[Tensor], role: Optional[Tensor]) -> Tensor:
    """E [LR * S, De]: the encoder's input rows BEFORE its relu.  Columns [0, D): the mean over the scenario columns of
    their table rows (O.scenario_embedding without its relu); with positions, row (2 l + r) S + s carries
    layerid_emb[l] + qkvid_emb[r] in [D, 2 D) (O.scenario_vectors, roles Q and K)."""
    if index is None:
        dom = tables[0][:S]
    else:
        rows = [tables[c][index[c].long()] for c in range(len(tables))]
        dom = torch.stack(rows, dim=-1).mean(-1) if len(tables) > 1 else rows[0]
    if lay is None:
        return dom
    out = []
    for l in range(lay.shape[0]):
        for r in range(2):
            out.append(torch.cat([dom, (lay[l] + role[r]).expand(S, -1)], dim=1))
    return torch.cat(out, dim=0)


def inputs_fwd_bound(tables: List[Tensor], index: Optional[Tensor], S: int, lay: Optional[Tensor], role: Optional[Tensor]) -> Tensor:
    """Bound of E for fp64 copies of the operands.  One scenario column: the row itself (0.f + x, no division), exact."""
    C, D = len(tables), tables[0].shape[1]
    if C == 1:
        dom = torch.zeros(S, D, dtype=torch.float64)
    else:
        dom = (C + 1) * U * sum(tables[c][index[c].long()].abs() for c in range(C)) / C
    if lay is None:
        return dom
    out = []
    for l in range(lay.shape[0]):
        for r in range(2):
            out.append(torch.cat([dom, sum_bound(1, lay[l].abs() + role[r].abs()).expand(S, -1)], dim=1))
    return torch.cat(out, dim=0)


def _selectors(index: Optional[Tensor], C: int, S: int, LR: int, table_rows: Sequence[int]) -> List[Tensor]:
    """Per scenario column a 0/1 matrix [table rows, LR * S]: which rows of g_E a table row's gradient sums."""
    out = []
    for c in range(C):
        M = torch.zeros(table_rows[c], LR * S, dtype=torch.float64)
        for s in range(S):
            r = int(index[c][s]) if index is not None else s
            for lr in range(LR):
                M[r, lr * S + s] = 1.0
        out.append(M)
    return out


def inputs_bwd_bounds(gE: Tensor, index: Optional[Tensor], C: int, S: int, D: int, L: int, pos: bool, table_rows: Sequence[int],
                      e_gE: Optional[Tensor] = None) -> Dict[str, object]:
    """Bounds of g_tables (a list), g_lay, g_role for the fp64 g_E [LR * S, De]; `e_gE`: what the kernel's own g_E may be
    off by (the chain), None = exact input.  A table row that no scenario names sums nothing: bound 0, exactly the prior."""
    LR = 2 * L if pos else 1
    e_gE = torch.zeros_like(gE) if e_gE is None else e_gE
    out: Dict[str, object] = {"g_tables": []}
    for M in _selectors(index, C, S, LR, table_rows):
        n = M.sum(1, keepdim=True) + 1                                     # the rows summed, and the division by C
        out["g_tables"].append((sum_bound(n, M @ gE[:, :D].abs()) * (M.sum(1, keepdim=True) > 0) + M @ e_gE[:, :D]) / C)
    if pos:
        a, e = gE[:, D:].abs().reshape(L, 2, S, D), e_gE[:, D:].reshape(L, 2, S, D)
        out["g_lay"] = sum_bound(2 * S, a.sum((1, 2))) + e.sum((1, 2))
        out["g_role"] = sum_bound(L * S, a.sum((0, 2))) + e.sum((0, 2))
    return out


def inputs_bwd_reference(gE: Tensor, index: Optional[Tensor], C: int, S: int, D: int, L: int, pos: bool, table_rows: Sequence[int]):
    """(want, bound) of satrans_scenario_inputs_bwd ALONE on an fp32 g_E: autograd of inputs_fwd on zero-valued leaves
    (it is linear), in fp64."""
    tables = [torch.zeros(n, D, dtype=torch.float64, requires_grad=True) for n in table_rows]
    lay = torch.zeros(L, D, dtype=torch.float64, requires_grad=True) if pos else None
    role = torch.zeros(2, D, dtype=torch.float64, requires_grad=True) if pos else None
    (inputs_fwd(tables, index, S, lay, role) * gE.double()).sum().backward()
    want = {"g_tables": [t.grad if t.grad is not None else torch.zeros_like(t) for t in tables]}
    if pos:
        want["g_lay"], want["g_role"] = lay.grad, role.grad
    return want, inputs_bwd_bounds(gE.double(), index, C, S, D, L, pos, table_rows)


def chain_reference(tables: List[Tensor], index: Optional[Tensor], S: int, lay: Optional[Tensor], role: Optional[Tensor],
                    W: Tensor, bias: Tensor, g_tab: Tensor):
    """(want, bound) of inputs_fwd -> table_fwd -> table_bwd -> inputs_bwd: autograd of the WHOLE fp64 composition; the
    bounds pass each stage's bound on to the next.  `role` holds the Q and K rows only."""
    C, D, pos = len(tables), tables[0].shape[1], lay is not None
    L = lay.shape[0] if pos else 1
    T = [t.double().requires_grad_(True) for t in tables]
    la, ro = (lay.double().requires_grad_(True), role.double().requires_grad_(True)) if pos else (None, None)
    w, b = W.double().requires_grad_(True), bias.double().requires_grad_(True)
    g = g_tab.double()
    E = inputs_fwd(T, index, S, la, ro)
    E.retain_grad()
    tab = table_fwd(E, w, b)
    (tab * g).sum().backward()
    want = {"E": E.detach(), "tab": tab.detach(), "g_E": E.grad, "g_W": w.grad, "g_bias": b.grad,
            "g_tables": [t.grad if t.grad is not None else torch.zeros_like(t) for t in T]}
    with torch.no_grad():
        e_E = inputs_fwd_bound([t.detach() for t in T], index, S, la, ro)
        tb = table_bounds(E.detach(), w.detach(), b.detach(), g, e_emb=e_E)
        bound = {"E": e_E, "tab": tb["tab"], "g_E": tb["g_emb"], "g_W": tb["g_W"], "g_bias": tb["g_bias"]}
        bound.update(inputs_bwd_bounds(E.grad, index, C, S, D, L, pos, [t.shape[0] for t in T], e_gE=tb["g_emb"]))
    if pos:
        want["g_lay"], want["g_role"] = la.grad, ro.grad
    return want, bound


def kink_free(E64: Tensor, e_E: Tensor) -> bool:
    """No entry of the fp64 E within its forward bound of relu's kink, except the entries that are exactly 0 (an exact
    zero is computed as the same exact zero by every evaluation order)."""
    return not bool(((E64 != 0) & (E64.abs() <= e_E)).any())


# ---- seeded inputs ------------------------------------------------------------------------------------------------------
# (S, De, P): every value of S in {1, 3, 37, 240}, De in {1, 4, 20, 32, 36, 64, 256}, P in {1, 7, 8, 9, 31, 33, 255, 257, 2080}
# at least twice with different partners, every De with at least three values of S and of P (the full pair table of De x P
# alone has 63 entries).  P = 1..31: slices without a p; 33: span 2, half of the slices empty; 255: span 8 = kSub, one p per
# sub-slice; 257: span 9, sub-slices of 2 with the last one short and three empty; 2080: span 65, sub-slices of 9, the last of 2.
TABLE_CASES = [(1, 1, 1), (240, 256, 33), (3, 32, 2080), (37, 20, 257), (3, 1, 7), (37, 1, 2080), (1, 4, 8), (3, 4, 255),
               (240, 4, 31), (1, 20, 9), (240, 20, 1), (37, 32, 7), (1, 32, 257), (3, 36, 33), (240, 36, 8), (37, 36, 255),
               (1, 64, 31), (3, 64, 9), (37, 64, 2080), (1, 256, 255), (3, 256, 1), (240, 64, 257), (37, 256, 9)]


def draw_table(case, seed_offset: int = 0):
    """emb [S,De] (about half negative; exact 0.0 and -0.0 at fixed places), W [P,De], bias [P], g_tab [S,P], fp32."""
    S, De, P = case
    g = torch.Generator().manual_seed(7000 + 1000003 * seed_offset + S * 100000 + De * 10000 + P)
    emb = torch.randn(S, De, generator=g)
    flat = emb.view(-1)
    flat[::5] = 0.0
    flat[2::7] = -0.0
    W = torch.randn(P, De, generator=g) * De ** -0.5
    bias = 0.3 * torch.randn(P, generator=g)
    g_tab = torch.randn(S, P, generator=g)
    return emb, W, bias, g_tab


# name: (sizes of the scenario columns [None: one column, index = NULL], explicit index or None, table rows, D, L [0: no positions], P)
CHAIN_CASES = {
    "c1_pos_l1_d4": dict(sizes=None, S=3, rows=(5,), D=4, L=1, P=33),                   # a table with more rows than S
    "c1_pos_l3_d16": dict(sizes=None, S=37, rows=(37,), D=16, L=3, P=257),
    "c1_index_pos": dict(sizes=None, S=5, index=[[2, 0, 0, 1, 2]], rows=(4,), D=4, L=1, P=9),      # rows named twice, row 3 unnamed
    "c2": dict(sizes=(3, 4), rows=(5, 4), D=16, L=0, P=31),                             # rows 3, 4 of table 0 unnamed
    "c3": dict(sizes=(2, 3, 2), rows=(2, 3, 2), D=4, L=0, P=255),
    "c8": dict(sizes=(2, 1, 2, 1, 1, 2, 1, 1), rows=(2, 1, 2, 1, 1, 2, 1, 3), D=16, L=0, P=7),
    "c2_pos_l3_d4": dict(sizes=(3, 4), rows=(3, 6), D=4, L=3, P=33),                    # two columns AND positions
    "c2_pos_l1_d16": dict(sizes=(5, 2), rows=(5, 2), D=16, L=1, P=2080),
}


def draw_chain(name: str):
    """tables, index [C,S] int32 or None, S, lay [L,D], role [3,D] (the V row unused) or None, W [P,De], bias, g_tab
    [LR*S,P], g_E [LR*S,De] (for inputs_bwd alone), fp32.  Column 1 of every table and column 0 of lay / role are exactly 0
    (signed), so E holds exact zeros; the draw is repeated until the fp64 E is `kink_free`."""
    c = CHAIN_CASES[name]
    sizes, D, L, P = c["sizes"], c["D"], c["L"], c["P"]
    if "index" in c:
        index, S = torch.tensor(c["index"], dtype=torch.int32), c["S"]
    elif sizes is None:
        index, S = None, c["S"]
    else:
        index, S = composite_index(sizes), math.prod(sizes)
    pos = L > 0
    LR, De = (2 * L, 2 * D) if pos else (1, D)
    g = torch.Generator().manual_seed(9000 + sorted(CHAIN_CASES).index(name))
    while True:
        tables = [torch.randn(n, D, generator=g) for n in c["rows"]]
        for t in tables:
            if D > 1:
                t[:, 1] = 0.0
                t[::2, 1] = -0.0
        lay = role = None
        if pos:
            lay, role = torch.randn(L, D, generator=g), torch.randn(3, D, generator=g)
            lay[:, 0], role[:, 0] = 0.0, 0.0
        E = inputs_fwd([t.double() for t in tables], index, S, lay.double() if pos else None, role[:2].double() if pos else None)
        e_E = inputs_fwd_bound([t.double() for t in tables], index, S, lay.double() if pos else None, role[:2].double() if pos else None)
        if kink_free(E, e_E):
            break
    W = torch.randn(P, De, generator=g) * De ** -0.5
    bias = 0.3 * torch.randn(P, generator=g)
    g_tab = torch.randn(LR * S, P, generator=g)
    g_E = torch.randn(LR * S, De, generator=g)
    return dict(tables=tables, index=index, S=S, lay=lay, role=role, W=W, bias=bias, g_tab=g_tab, g_E=g_E, D=D, L=max(L, 1),
                pos=pos, LR=LR, De=De, P=P, C=len(tables), rows=list(c["rows"]))


# =====================================================================================================================
# csrc/head.hip
# =====================================================================================================================
def head_forward(a: Tensor, dense: Optional[Tensor], cols: Optional[Tensor], w: Tensor, bias: Tensor):
    """(prob [B], logit [B], flat [B, ncol]): the tail of O.forward - flatten, the dense columns behind it, Linear, sigmoid."""
    flat = a if dense is None or cols is None or cols.numel() == 0 else torch.cat([a, dense[:, cols.long()].to(a.dtype)], dim=-1)
    logit = F.linear(flat, w.unsqueeze(0), bias).squeeze(-1)
    return torch.sigmoid(logit), logit, flat


def n_logit(FD: int, n_dense: int) -> int:
    return 4 * ceil_div(FD, 256) + ceil_div(n_dense, 64) + 6 + 1


def n_head_sum(B: int) -> int:
    return SAMPLES_PER_BLOCK + ceil_div(ceil_div(B, SAMPLES_PER_BLOCK), REDUCE_GROUPS) + REDUCE_GROUPS


def logit_bound(flat64: Tensor, w64: Tensor, bias64: Tensor, FD: int, n_dense: int) -> Tensor:
    return sum_bound(n_logit(FD, n_dense), flat64.abs() @ w64.abs() + bias64.abs())


def prob_bound(lb: Tensor) -> Tensor:
    return 0.25 * lb + 4 * U


def loss_pieces(p: Tensor, t: Tensor, kind: int):
    """(loss [B], dlogit [B]) by the kernel's formulas (head.hip:54-66, clamps included) in the dtype of p: the per-sample
    term of F.binary_cross_entropy / F.mse_loss / F.l1_loss(reduction='sum') and its derivative through p = sigmoid(z)."""
    pq = (1.0 - p) * p
    if kind == MSE:
        return (p - t) * (p - t), 2.0 * (p - t) * pq
    if kind == MAE:
        return (p - t).abs(), torch.sign(p - t) * pq
    lp, lq = torch.log(p).clamp(min=-100.0), torch.log(1.0 - p).clamp(min=-100.0)
    return -(t * lp + (1.0 - t) * lq), (p - t) / pq.clamp(min=1e-12) * pq


def torch_loss(p: Tensor, t: Tensor, kind: int) -> Tensor:
    if kind == MSE:
        return F.mse_loss(p, t, reduction="sum")
    if kind == MAE:
        return F.l1_loss(p, t, reduction="sum")
    return F.binary_cross_entropy(p, t, reduction="sum")


def torch_loss_and_dlogit(p: Tensor, t: Tensor, kind: int = BCE):
    """torch's own evaluation in the dtype of p (the saturated rows: fp32 on the CPU), FED THE GIVEN PROBABILITY: the summed
    loss, and d loss / d logit = autograd's d loss / d p times sigmoid's backward p (1 - p) at that p (what autograd through
    p = sigmoid(z) computes from the saved p; tests/test_scenario_head_cpu.py holds it to that autograd bit for bit)."""
    leaf = p.detach().clone().requires_grad_(True)
    loss = torch_loss(leaf, t, kind)
    loss.backward()
    return loss.detach(), leaf.grad * ((1.0 - p) * p)


def head_stage2(prob32: Tensor, t32: Tensor, flat64: Tensor, w64: Tensor, kind: int):
    """(want, bound) of loss_sum, dlogit [B], g_w [ncol], g_b from the kernel's stored fp32 probability: the formulas in
    fp64; per-sample bounds added up, plus the summation bound of the fp32 sums."""
    B = prob32.numel()
    loss, dl = loss_pieces(prob32.double(), t32.double(), kind)
    n = n_head_sum(B)
    want = {"loss_sum": loss.sum(), "dlogit": dl, "g_b": dl.sum(), "g_w": dl @ flat64}
    bound = {"dlogit": torch.full_like(dl, DLOGIT_BOUND),
             "loss_sum": (LOSS_REL * (1 + loss.abs())).sum() + sum_bound(n, loss.abs().sum()),
             "g_b": torch.as_tensor(B * DLOGIT_BOUND) + sum_bound(n, dl.abs().sum()),
             "g_w": DLOGIT_BOUND * flat64.abs().sum(0) + sum_bound(n, dl.abs() @ flat64.abs())}
    return want, bound


# (B, FD, n_dense, loss): every B in {1, 7, 8, 9, 131, 269} (nblk = 17 and 34: above kReduceGroups, shares of 2 and 3), FD in
# {4, 252, 256, 260, 736}, n_dense in {0, 1, 2, 65} and loss at least three times; ncol + 2 = 256, a multiple of 32, at
# (7, 252, 2); ncol + 2 = 257, one past it, needs ncol = 3 mod 4, which n_dense in {0, 1, 2, 65} cannot give: (9, 252, 3).
HEAD_CASES = [(1, 4, 0, BCE), (7, 252, 2, BCE), (8, 256, 1, MSE), (9, 260, 65, MAE), (131, 736, 0, BCE), (269, 4, 65, BCE),
              (269, 252, 1, MSE), (131, 256, 2, MAE), (1, 260, 1, MSE), (7, 736, 65, MAE), (8, 4, 2, MAE), (9, 252, 3, BCE),
              (131, 260, 0, MSE), (269, 736, 2, BCE), (7, 256, 0, BCE), (9, 736, 1, MSE), (8, 260, 2, BCE), (1, 252, 65, MAE)]
Z_MAX = 8.0


def draw_head(case, seed_offset: int = 0):
    """fp32 a [B,FD], dense [B,stride] (stride = 3 more columns than the largest one used; unused columns hold 7777), cols
    [n_dense] int32 UNSORTED, w [ncol] with w[0] = 1 exactly (so da[:, 0] IS the kernel's dlogit), bias [1], y [B].
    Labels are 0 / 1; MSE and MAE get fractional labels on every other row.  The weights behind w[0] are halved until the
    fp64 |z| <= 8; for MAE the draw is repeated until no fp64 |p - t| lies within the probability bound (fp64 alone decides)."""
    B, FD, n_dense, kind = case
    g = torch.Generator().manual_seed(11000 + 1000003 * seed_offset + B * 10000 + FD * 10 + n_dense + 7 * kind)
    ncol = FD + n_dense
    while True:
        a = torch.randn(B, FD, generator=g)
        dense = cols = None
        if n_dense:
            width = n_dense + 5
            cols = torch.randperm(width, generator=g)[:n_dense].to(torch.int32)
            if n_dense > 1 and bool((cols[1:] > cols[:-1]).all()):
                cols = cols.flip(0)
            dense = torch.full((B, int(cols.max()) + 4), 7777.0)
            dense[:, cols.long()] = torch.randn(B, n_dense, generator=g)
        w = torch.randn(ncol, generator=g) * ncol ** -0.5
        w[0] = 1.0
        bias = 0.3 * torch.randn(1, generator=g)
        y = (torch.rand(B, generator=g) < 0.5).float()
        if kind != BCE:
            frac = torch.rand(B, generator=g)
            y[1::2] = frac[1::2]
        while True:
            p, z, flat = head_forward(a.double(), None if dense is None else dense.double(), cols, w.double(), bias.double())
            if float(z.abs().max()) <= Z_MAX:
                break
            w[1:] *= 0.5
            a[:, 0] *= 0.5
        if kind != MAE:
            break
        pb = prob_bound(logit_bound(flat, w.double(), bias.double(), FD, n_dense))
        if not bool(((p - y.double()).abs() <= pb).any()):
            break
    return dict(a=a, dense=dense, cols=cols, w=w, bias=bias, y=y, B=B, FD=FD, n_dense=n_dense, kind=kind, ncol=ncol,
                stride=0 if dense is None else dense.shape[1])


SATURATED_Z = (20.0, -20.0, 90.0, -90.0, 104.0, -104.0)


def draw_saturated(mixed: bool):
    """A BCE batch whose logits are exactly z for z in SATURATED_Z x t in {0, 1}: the row is zero but for a[b, 0] = z - bias
    with w[0] = 1 and bias = 0.5 (all exact in fp32).  Alone: B = 12.  `mixed`: B = 9, rows 1, 2, 4, 5, 6, 8 of an ordinary
    batch replaced (z = 20, -20, 90, -90, 104, -104 with t = 0, 1, 1, 0, 0, 1).  Returns the draw and {row: (z, t)}."""
    if mixed:
        d = draw_head((9, 260, 2, BCE), seed_offset=5)
        rows = {1: (20.0, 0.0), 2: (-20.0, 1.0), 4: (90.0, 1.0), 5: (-90.0, 0.0), 6: (104.0, 0.0), 8: (-104.0, 1.0)}
    else:
        d = draw_head((12, 256, 1, BCE), seed_offset=5)
        rows = {2 * i + j: (z, float(j)) for i, z in enumerate(SATURATED_Z) for j in range(2)}
    d["bias"] = torch.tensor([0.5])
    for b, (z, t) in rows.items():
        d["a"][b] = 0.0
        d["a"][b, 0] = z - 0.5
        d["dense"][b, d["cols"].long()] = 0.0
        d["y"][b] = t
    return d, rows
