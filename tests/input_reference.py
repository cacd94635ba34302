"""Torch restatement of the reference's front end - deepctr's `Linear.forward` (models/meta_basemodel.py:63-92) and
`BaseModel.input_from_feature_columns` (:519-545) - in their literal forms, generic in dtype  --  TEST INFRASTRUCTURE, NOT
PRODUCT CODE.  The pooling of the varlen fields is tests/varlen_reference.py's (`slot_mask`, `pool_rows`).

Parameters travel as a dict by state_dict key: `embedding_dict.<embedding_name>.weight` ([V, 1] for the linear tables, [V, D]
for the lookup) and `weight` [n_dense, 1].  Ids are read from X with the reference's `.long()` truncation; X may be the fp32
matrix or any float / integer copy of it.  The tests run these forms in fp64 (what the product is held against) and in fp32
(torch's own run: the premise of the bounds).

Also here: the feature-column draws that the CPU and GPU tests share (SWEEP, SKEW), with parameters of order 0.1 so that a
bound relative to max|.| means something, and max-pooled lists without ties among their valid slots."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from tests import varlen_reference as V

Tensor = torch.Tensor
# the project's sibling bounds
OUT_BOUND, GRAD_REL, GRAD_ABS = 2e-5, 1e-4, 5e-9


@dataclass
class InputSpec:
    """The columns as the reference's two functions walk them: sparse fields (embedding_name, X column), varlen fields
    (embedding_name, VarSpec), the X columns of the dense values in concatenation order."""
    sparse: List[Tuple[str, int]]
    varlen: List[Tuple[str, V.VarSpec]]
    dense_cols: List[int]
    names: List[str] = field(default_factory=list)      # the distinct embedding names in creation order


def spec_of(feature_columns, feature_index) -> InputSpec:
    from satrans_amd.inputs import split_columns
    sparse, dense, varlen = split_columns(feature_columns)
    fi = feature_index
    vs = [(c.embedding_name, V.VarSpec(c.name, fi[c.name][0], c.maxlen, c.combiner,
                                       fi[c.length_name][0] if c.length_name is not None else None)) for c in varlen]
    names = list(dict.fromkeys(c.embedding_name for c in sparse + varlen))
    return InputSpec([(c.embedding_name, fi[c.name][0]) for c in sparse], vs,
                     [j for c in dense for j in range(*fi[c.name])], names)


def key(name: str) -> str:
    return f"embedding_dict.{name}.weight"


def _lists(P: Dict[str, Tensor], X: Tensor, spec: InputSpec):
    """sparse_embedding_list + varlen_embedding_list: [B, 1, width] each, in the reference's order."""
    out = [P[key(n)][X[:, c:c + 1].long()] for n, c in spec.sparse]
    for n, v in spec.varlen:
        E = P[key(n)][X[:, v.col:v.col + v.maxlen].long()]
        out.append(V.pool_rows(E, V.slot_mask(X, v), v).unsqueeze(1))
    return out


def dense_values(X: Tensor, spec: InputSpec) -> Optional[Tensor]:
    return X[:, spec.dense_cols] if spec.dense_cols else None


def linear(P: Dict[str, Tensor], X: Tensor, spec: InputSpec) -> Tensor:
    """Linear.forward: zeros + sum(cat(lists, -1), -1) + cat(dense) @ weight -> [B, 1] in the dtype of the parameters."""
    any_p = next(iter(P.values())) if P else X
    logit = torch.zeros(X.shape[0], 1, dtype=any_p.dtype)
    lists = _lists(P, X, spec)
    if lists:
        logit = logit + torch.sum(torch.cat(lists, dim=-1), dim=-1, keepdim=False)
    if spec.dense_cols:
        logit = logit + dense_values(X, spec).to(any_p.dtype).matmul(P["weight"])
    return logit


def lookup(P: Dict[str, Tensor], X: Tensor, spec: InputSpec):
    """input_from_feature_columns, concatenated along the fields: (emb [B, F, D], dense [B, n_dense] or None)."""
    return torch.cat(_lists(P, X, spec), dim=1), dense_values(X, spec)


def loss_and_grads(Pl, Pe, X, spec, c, Cw, dtype):
    """loss = sum_b c_b linear_b + sum C * emb under autograd on leaves of `dtype` (either half is left out with empty parameters).
    -> (linear_logit, emb, {key: grad} of the linear parameters, {key: grad} of the embedding tables)."""
    Ll = {k: t.detach().to(dtype).clone().requires_grad_(True) for k, t in Pl.items()}
    Le = {k: t.detach().to(dtype).clone().requires_grad_(True) for k, t in Pe.items()}
    logit = linear(Ll, X, spec) if Ll else None
    emb = lookup(Le, X, spec)[0] if Le else None
    loss = torch.zeros((), dtype=dtype)
    if logit is not None:
        loss = loss + (logit * c.to(dtype).reshape(-1, 1)).sum()
    if emb is not None:
        loss = loss + (emb * Cw.to(dtype)).sum()
    if loss.requires_grad:
        loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
    return (logit.detach() if logit is not None else None, emb.detach() if emb is not None else None,
            {k: zero(t) for k, t in Ll.items()}, {k: zero(t) for k, t in Le.items()})


def max_ties(P: Dict[str, Tensor], X: Tensor, spec: InputSpec) -> int:
    """How many (sample, max-pooled field, element) have more than one VALID slot at the maximum (the gradient is undefined
    there), counted from the restatement alone."""
    ties = 0
    for n, v in spec.varlen:
        if v.combiner != "max":
            continue
        E = P[key(n)][X[:, v.col:v.col + v.maxlen].long()].double()
        valid = V.slot_mask(X, v).unsqueeze(-1)
        w = torch.where(valid, E, torch.full_like(E, -float("inf")))
        top = (w == w.max(1, keepdim=True)[0]) & valid
        ties += int((top.sum(1) > 1).sum())
    return ties


# ---- the draws the CPU and GPU tests share ---------------------------------------------------------------------------------------
COMBOS = [(c, length) for c in ("sum", "mean", "max") for length in (False, True)]


@dataclass
class Case:
    name: str
    B: int
    n_sparse: int
    varlen: List[Tuple[int, str, bool]]      # (maxlen, combiner, length column)
    n_dense: int
    ids: str = "f32"                         # "f32": the reference's matrix; "i32" / "i64": integer ids (PackedInput with dense)
    D: int = 16


def _varlen(maxlens):
    return [(m, c, length) for m in maxlens for c, length in COMBOS]


SWEEP = [
    Case("one", 1, 1, [], 0),
    Case("one_list", 260, 0, [(3, "mean", False)], 0, ids="i64"),
    Case("dense_only", 37, 0, [], 13),
    Case("b37_f19", 37, 13, _varlen((3,)), 1),
    Case("b37_i64", 37, 13, _varlen((1,)), 1, ids="i64"),
    Case("b260_f64", 260, 46, _varlen((1, 3, 32)), 13),
    Case("b8269_f19", 8269, 13, [(1, "sum", False), (3, "mean", True), (32, "max", False), (32, "sum", True),
                                 (3, "max", True), (1, "mean", False)], 13, ids="i32"),
    Case("b8269_f64", 8269, 58, _varlen((3,)), 0),
]


def case_id(c: Case) -> str:
    return c.name


def columns_of(c: Case):
    """Sparse vocabularies of 3..60 rows, varlen vocabularies of 40..60 (more rows than slots: a max list can hold distinct ids);
    dense features of dimension 1 except one of dimension 3 when there is room."""
    from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = [SparseFeat(f"s{i}", 3 + (17 * i) % 58, embedding_dim=c.D) for i in range(c.n_sparse)]
    cols += [VarLenSparseFeat(SparseFeat(f"h{j}", 40 + (7 * j) % 21, embedding_dim=c.D), maxlen=m, combiner=comb,
                              length_name=f"h{j}_len" if length else None) for j, (m, comb, length) in enumerate(c.varlen)]
    left, j = c.n_dense, 0
    while left > 0:
        k = 3 if left >= 3 and j == 1 else 1
        cols.append(DenseFeat(f"d{j}", k))
        left, j = left - k, j + 1
    return cols


def draw_X(cols, fi, B, g, min_len_max=1):
    """fp32 X [B, C]: uniform sparse ids; lists of random length - sum / mean lists may be empty, max lists hold at least
    `min_len_max` valid slots and DISTINCT valid ids (no tie between valid slots); without a length column the valid slots sit at
    random places between zeros, with one the padding slots hold arbitrary in-range ids; dense values in [-1, 1)."""
    from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    X = torch.zeros(B, max(hi for _, hi in fi.values()))
    for c in cols:
        lo, hi = fi[c.name]
        if isinstance(c, SparseFeat):
            X[:, lo] = torch.randint(0, c.vocabulary_size, (B,), generator=g).float()
        elif isinstance(c, DenseFeat):
            X[:, lo:hi] = torch.rand(B, hi - lo, generator=g) * 2 - 1
        elif isinstance(c, VarLenSparseFeat):
            ids = 1 + torch.rand(B, c.vocabulary_size - 1, generator=g).argsort(1)[:, :c.maxlen]      # distinct, >= 1
            n = torch.randint(min_len_max if c.combiner == "max" else 0, c.maxlen + 1, (B,), generator=g)
            if c.length_name is None:
                keep = torch.rand(B, c.maxlen, generator=g).argsort(1).argsort(1) < n.unsqueeze(1)
                X[:, lo:hi] = torch.where(keep, ids, torch.zeros_like(ids)).float()
            else:
                X[:, lo:hi] = ids.float()
                X[:, fi[c.length_name][0]] = n.float()
    return X


def draw_params(cols, D, g, std=0.1):
    """(linear parameters, embedding tables) by state_dict key, fp32 N(0, std), one table per embedding_name."""
    from satrans_amd.inputs import split_columns
    sparse, dense, varlen = split_columns(cols)
    Pl, Pe = {}, {}
    for c in sparse + varlen:
        if key(c.embedding_name) not in Pl:
            Pl[key(c.embedding_name)] = torch.randn(c.vocabulary_size, 1, generator=g) * std
            Pe[key(c.embedding_name)] = torch.randn(c.vocabulary_size, D, generator=g) * std
    n_dense = sum(c.dimension for c in dense)
    if n_dense:
        Pl["weight"] = torch.randn(n_dense, 1, generator=g) * std
    return Pl, Pe


def draw(cols, B, D, seed):
    """-> (feature_index, spec, X fp32, Pl, Pe, c [B], C [B, F, D]); redrawn (next seed) until no max list ties."""
    from satrans_amd.inputs import build_input_features
    fi = build_input_features(cols)
    spec = spec_of(cols, fi)
    for attempt in range(8):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        X = draw_X(cols, fi, B, g)
        Pl, Pe = draw_params(cols, D, g)
        if max_ties(Pl, X, spec) == 0 and max_ties(Pe, X, spec) == 0:
            F = len(spec.sparse) + len(spec.varlen)
            return fi, spec, X, Pl, Pe, torch.randn(B, generator=g), torch.randn(B, F, D, generator=g)
    raise AssertionError("eight draws in a row tie under max")


def draw_case(c: Case):
    cols = columns_of(c)
    return (cols,) + draw(cols, c.B, c.D, seed=sum(map(ord, c.name)))


def skew_columns(B, D):
    """The segment sum's hard inputs at one batch size: `hot` (every sample on one id), `single` (a table of one row), `wide`
    (all ids distinct), `left` / `right` (two fields on one table, overlapping ids), a max list, and a dense feature."""
    from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    return [SparseFeat("hot", 50, embedding_dim=D), SparseFeat("single", 1, embedding_dim=D), SparseFeat("wide", B + 3, embedding_dim=D),
            SparseFeat("left", 29, embedding_dim=D, embedding_name="pair"), SparseFeat("right", 29, embedding_dim=D, embedding_name="pair"),
            VarLenSparseFeat(SparseFeat("hist", 45, embedding_dim=D), maxlen=3, combiner="max"), DenseFeat("price", 1)]


def draw_skew(B, D, seed=5):
    cols = skew_columns(B, D)
    fi, spec, X, Pl, Pe, c, Cw = draw(cols, B, D, seed)
    g = torch.Generator().manual_seed(seed + 1)
    X[:, fi["hot"][0]] = 7.0
    X[:, fi["single"][0]] = 0.0
    X[:, fi["wide"][0]] = torch.randperm(B, generator=g).float() + 2          # rows 0 and 1 and B + 2 stay ungathered
    X[:, fi["left"][0]] = torch.randint(0, 20, (B,), generator=g).float()    # rows 0..19 / 10..27 overlap; row 28 ungathered
    X[:, fi["right"][0]] = torch.randint(10, 28, (B,), generator=g).float()
    return cols, fi, spec, X, Pl, Pe, c, Cw


def gathered_rows(P: Dict[str, Tensor], X: Tensor, spec: InputSpec) -> Dict[str, Tensor]:
    """key -> bool [V]: the rows some slot of the batch reads (padding slots included: they are looked up too)."""
    hit = {k: torch.zeros(t.shape[0], dtype=torch.bool) for k, t in P.items() if k != "weight"}
    for n, c in spec.sparse:
        hit[key(n)][X[:, c].long()] = True
    for n, v in spec.varlen:
        hit[key(n)][X[:, v.col:v.col + v.maxlen].long().reshape(-1)] = True
    return hit


# ---- the recorded runs of the reference (tests/golden/input/*.npz, tools/gen_input_golden.py) ------------------------------------
GOLDEN_CASES = ("plain", "varlen", "shared")


def load_golden(name):
    import os

    import numpy as np
    root = os.path.dirname(os.path.abspath(__file__))
    with np.load(os.path.join(root, "golden", "input", f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def columns_from_fixture(fx):
    """The feature columns a fixture records as plain arrays, rebuilt with the product's column types."""
    from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    cols = []
    for i, kind in enumerate(fx["col/kind"]):
        name, dim = str(fx["col/name"][i]), int(fx["col/dim"][i])
        if kind == "dense":
            cols.append(DenseFeat(name, dim))
            continue
        sf = SparseFeat(name, int(fx["col/vocab"][i]), embedding_dim=dim, embedding_name=str(fx["col/embedding_name"][i]))
        if kind == "sparse":
            cols.append(sf)
        else:
            cols.append(VarLenSparseFeat(sf, maxlen=int(fx["col/maxlen"][i]), combiner=str(fx["col/combiner"][i]),
                                         length_name=str(fx["col/length_name"][i]) or None))
    return cols


def fixture_params(fx, prefix):
    return {k[len(prefix) + 1:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(prefix + "/")}
