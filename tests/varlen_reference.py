"""Torch restatement of VarLenSparseFeat pooling (deepctr-torch 0.2.9 SequencePoolingLayer as the reference's
BaseModel.input_from_feature_columns calls it, models/meta_basemodel.py:519-545) and of SATrans with such fields, composed
from the unchanged oracle's pieces  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A varlen field is described by `VarSpec(name, col, maxlen, combiner, len_col)`: X columns [col, col + maxlen) hold the ids,
`len_col` (or None) the list length.  Everything runs in the dtype of the tables (fp32 for bit-exact comparisons, fp64 for
the composition the product is held against).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

from oracle import satrans_oracle as O

Tensor = torch.Tensor


@dataclass
class VarSpec:
    name: str
    col: int
    maxlen: int
    combiner: str
    len_col: Optional[int] = None


def slot_mask(X: Tensor, v: VarSpec) -> Tensor:
    """[B, maxlen] bool: id != 0 (no length column: supports_masking), else slot < length (_sequence_mask)."""
    ids = X[:, v.col:v.col + v.maxlen].long()
    if v.len_col is None:
        return ids != 0
    length = X[:, v.len_col].long()
    return torch.arange(v.maxlen).unsqueeze(0) < length.unsqueeze(1)


def pool(table: Tensor, X: Tensor, v: VarSpec) -> Tensor:
    """[B, D] pooled embedding of one varlen field.  sum: slot order; mean: / (count + 1e-8) as a true division; max: of
    E - (1 - mask) * 1e9, the first maximal slot winning (torch.max)."""
    ids = X[:, v.col:v.col + v.maxlen].long()
    return pool_rows(table[ids], slot_mask(X, v), v)


def pool_rows(E: Tensor, valid: Tensor, v: VarSpec) -> Tensor:
    """The pooling of the gathered rows E [B, maxlen, D] (an autograd leaf gives the gradient of every slot)."""
    mask = valid.to(E.dtype).unsqueeze(-1)
    if v.combiner == "max":
        return torch.max(E - (1 - mask) * 1e9, dim=1)[0]
    if v.combiner not in ("sum", "mean"):
        raise ValueError(v.combiner)
    hist = E * mask
    acc = hist[:, 0]
    for s in range(1, v.maxlen):                                       # (fp32 in slot order)
        acc = acc + hist[:, s]
    if v.combiner == "mean":
        count = mask.sum(1)                                            # exact small integers
        acc = acc / (count + torch.tensor(1e-8, dtype=E.dtype))
    return acc


@dataclass
class PoolSpec:
    """One field of the pooled gather's table: the members of `satrans_pool_field` (include/satrans_hip.h), the combiner by name
    ("copy" for a SparseFeat, else "sum" / "mean" / "max")."""
    col: int
    maxlen: int
    combiner: str
    len_col: int      # -1: mask = id != 0
    slot: int
    varlen: int       # -1 for a SparseFeat
    lo: int
    hi: int

    def var(self) -> VarSpec:
        return VarSpec("", self.col, self.maxlen, self.combiner, self.len_col if self.len_col >= 0 else None)


def pooled_reference(arena: Tensor, X: Tensor, fields: List[PoolSpec], D: int):
    """What satrans_pool_gather_fwd computes from a field table, restated with `slot_mask` / `pool_rows` (fp32, slot order, true
    division): (layer input [B, F, D], slot rows [B, R] int32 = lo + id, valid-slot mask words [B, Fv] int64 in [0, 2^32): bit s =
    slot s valid).  Ids come from an integer or a float X with the `.long()` truncation; every id must lie inside its table."""
    assert arena.dtype == torch.float32 and arena.shape[1] == D
    out, rows, words = [], [], []
    for fd in fields:
        r = fd.lo + X[:, fd.col:fd.col + fd.maxlen].long()
        assert int(r.min()) >= fd.lo and int(r.max()) < fd.hi, "the reference reads no row outside the field's table"
        rows.append(r)
        if fd.combiner == "copy":
            out.append(arena[r[:, 0]])
            continue
        valid = slot_mask(X, fd.var())
        out.append(pool_rows(arena[r], valid, fd.var()))
        words.append((valid.long() << torch.arange(fd.maxlen)).sum(1))
    B = X.shape[0]
    return (torch.stack(out, 1), torch.cat(rows, 1).to(torch.int32),
            torch.stack(words, 1) if words else torch.zeros(B, 0, dtype=torch.int64))


def slot_gradients(arena: Tensor, X: Tensor, fields: List[PoolSpec], D: int, dx: Tensor) -> Tensor:
    """[B, R, D]: the gradient of every slot's row for the layer-input gradient dx [B, F, D] - dx itself for a SparseFeat, torch
    autograd through `pool_rows` on an fp32 leaf of the gathered rows for a varlen field (what satrans_pool_bwd writes)."""
    assert arena.dtype == torch.float32 and arena.shape[1] == D and dx.dtype == torch.float32
    g = []
    for f, fd in enumerate(fields):
        if fd.combiner == "copy":
            g.append(dx[:, f:f + 1])
            continue
        E = arena[fd.lo + X[:, fd.col:fd.col + fd.maxlen].long()].clone().requires_grad_(True)
        pool_rows(E, slot_mask(X, fd.var()), fd.var()).backward(dx[:, f])
        g.append(E.grad)
    return torch.cat(g, 1)


def pool_specs_of(model) -> List[PoolSpec]:
    """The field table of a product SATrans model over its embedding arena (sparse fields, then varlen ones)."""
    from satrans_amd.inputs import split_columns
    fi = model.feature_index
    sparse, _, varlen = split_columns(model.dnn_feature_columns)
    fields, slot = [], 0
    for c in sparse:
        lo, n = model._table_rows[c.embedding_name]
        fields.append(PoolSpec(fi[c.name][0], 1, "copy", -1, slot, -1, lo, lo + n))
        slot += 1
    for v, c in enumerate(varlen):
        lo, n = model._table_rows[c.embedding_name]
        fields.append(PoolSpec(fi[c.name][0], c.maxlen, c.combiner, fi[c.length_name][0] if c.length_name is not None else -1,
                               slot, v, lo, lo + n))
        slot += c.maxlen
    return fields


def layer_input(P: Dict[str, Tensor], X: Tensor, spec: O.PathSpec, varlen: List[VarSpec]) -> Tensor:
    """[B, F_sparse + F_varlen, D]: the SparseFeat rows, then the pooled varlen fields, concatenated along the fields."""
    x = O.gather_fields(P, X, spec)
    pooled = [pool(P[f"embedding_dict.{v.name}.weight"], X, v).unsqueeze(1) for v in varlen]
    return torch.cat([x] + pooled, dim=1) if pooled else x


def forward(P, X, spec, varlen, drop: Optional[O.Dropper] = None):
    """SATrans.forward (models/satrans.py:197-256) with the varlen fields in the layer input."""
    drop = drop or O.Dropper("off")
    x = layer_input(P, X, spec, varlen)
    vecs = O.scenario_vectors(P, X, spec)
    for l in range(spec.layer_num):
        x = O.layer_forward(P, l, x, vecs[l], spec, drop)
    flat = x.flatten(1)
    dense = O.dense_block(X, spec)
    if dense is not None:
        flat = torch.cat([flat, dense.to(flat.dtype)], dim=-1)
    logit = F.linear(flat, P["dnn_linear.weight"], P["dnn_linear.bias"])
    return torch.sigmoid(logit), logit


def regularization_loss(P, spec, varlen) -> Tensor:
    """l2 * sum(w^2) over every table of embedding_dict, the varlen ones included (meta_basemodel.py:168,179)."""
    total = O.regularization_loss(P, spec)
    if spec.l2_reg_embedding > 0:
        for v in varlen:
            total = total + torch.sum(spec.l2_reg_embedding * torch.square(P[f"embedding_dict.{v.name}.weight"]))
    return total


def loss_and_grads(P, X, y, spec, varlen, drop: Optional[O.Dropper] = None):
    """(bce_sum, reg, grads by key) as oracle.loss_and_grads, with the varlen fields."""
    leaves = O.make_leaves(P)
    prob, _ = forward(leaves, X, spec, varlen, drop)
    bce = F.binary_cross_entropy(prob.squeeze(-1), y.to(prob.dtype).reshape(-1), reduction="sum")
    reg = regularization_loss(leaves, spec, varlen)
    (bce + reg.sum()).backward()
    grads = {k: t.grad for k, t in leaves.items() if t.grad is not None}
    return float(bce.detach()), float(reg.detach().sum()), grads


def adam_steps(P, X, y, spec, varlen, lr, steps):
    """`steps` dense torch.optim.Adam steps (reference main.py:343) on BCE(sum) + reg, no dropout; -> parameters."""
    leaves = {k: t for k, t in O.make_leaves(P).items()}
    uniq = list({id(t): t for t in leaves.values()}.values())
    opt = torch.optim.Adam(uniq, lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        prob, _ = forward(leaves, X, spec, varlen)
        bce = F.binary_cross_entropy(prob.squeeze(-1), y.to(prob.dtype).reshape(-1), reduction="sum")
        (bce + regularization_loss(leaves, spec, varlen).sum()).backward()
        opt.step()
    return {k: t.detach() for k, t in leaves.items()}


def spec_of(model) -> (O.PathSpec, List[VarSpec]):
    """PathSpec + VarSpecs of a product SATrans model (its feature_index and columns)."""
    from satrans_amd.inputs import split_columns
    fi = model.feature_index
    sparse, dense, varlen = split_columns(model.dnn_feature_columns)
    units = list(model.meta_dnn_hidden_units)
    spec = O.PathSpec(
        sparse=[(c.embedding_name, fi[c.name][0]) for c in sparse],
        dense=[fi[c.name] for c in dense],
        domain_cols=[fi[c][0] for c in model.domain_column_list],
        embedding_dim=model.embedding_size, head_num=model.att_head_num, layer_num=model.domain_att_layer_num,
        flag=model.flag, meta_mode=model.meta_mode, meta_units=units, l2_reg_embedding=model.l2_reg_embedding,
        use_res=model.att_res)
    vs = [VarSpec(c.embedding_name, fi[c.name][0], c.maxlen, c.combiner,
                  fi[c.length_name][0] if c.length_name is not None else None) for c in varlen]
    return spec, vs


# ---- a small model and batches with padding, duplicates, empty lists and ties (shared by the CPU and GPU tests) -------------
SPARSE_VOCAB = [32, 11, 4, 19]
HIST_VOCAB = [23, 9, 40]


def columns(combiners=("max",), length=False, dense=False, D=16, maxlen=3):
    from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    sparse = [SparseFeat(f"f{i}", v, embedding_dim=D) for i, v in enumerate(SPARSE_VOCAB)] + [SparseFeat("dom", 5, embedding_dim=D)]
    var = [VarLenSparseFeat(SparseFeat(f"h{j}", HIST_VOCAB[j % len(HIST_VOCAB)], embedding_dim=D), maxlen=maxlen, combiner=c,
                            length_name=f"h{j}_len" if length else None) for j, c in enumerate(combiners)]
    return sparse + var + ([DenseFeat("price", 1)] if dense else [])


def build(device, combiners=("max",), length=False, dense=False, D=16, maxlen=3, seed=1021, flag="sota", mode="QK", L=2, H=2,
          units=(32, 16)):
    from satrans_amd import SATrans
    cols = columns(combiners, length, dense, D, maxlen)
    return SATrans(linear_feature_columns=cols, dnn_feature_columns=cols, domain_column_list=["dom"], num_domains_list=[3],
                   att_layer_num=0, domain_att_layer_num=L, att_head_num=H, use_linear=False, meta_mode=mode, use_dnn=False,
                   meta_dnn_hidden_units=(units[0], D), seed=seed, device=device, flag=flag)


def batch(model, B, seed=0, empty_every=5, min_len=0):
    """(X float32 [B, C] in feature_index order, y float32 [B]).  Varlen lists: random lengths (every `empty_every`-th sample
    empty), ids >= 1 in the valid slots (duplicates likely: small vocabularies), padding 0 - also BETWEEN valid ids in the mask
    form; with a length column the padding slots hold arbitrary in-range ids."""
    from satrans_amd.inputs import DenseFeat, SparseFeat, VarLenSparseFeat
    g = torch.Generator().manual_seed(seed)
    fi = model.feature_index
    X = torch.zeros(B, max(e for _, e in fi.values()))
    for c in model.dnn_feature_columns:
        lo, hi = fi[c.name]
        if isinstance(c, SparseFeat):
            X[:, lo] = torch.randint(1, 4, (B,), generator=g).float() if c.name == "dom" else \
                torch.randint(0, c.vocabulary_size, (B,), generator=g).float()
        elif isinstance(c, DenseFeat):
            X[:, lo:hi] = torch.rand(B, hi - lo, generator=g)
        elif isinstance(c, VarLenSparseFeat):
            ids = torch.randint(1, c.vocabulary_size, (B, c.maxlen), generator=g)
            n = torch.randint(min_len, c.maxlen + 1, (B,), generator=g)
            if empty_every:
                n[::empty_every] = 0
            if c.length_name is None:           # exactly n valid slots, at random places
                keep = torch.rand(B, c.maxlen, generator=g).argsort(1).argsort(1) < n.unsqueeze(1)
                X[:, lo:hi] = torch.where(keep, ids, torch.zeros_like(ids)).float()
            else:
                X[:, lo:hi] = torch.randint(0, c.vocabulary_size, (B, c.maxlen), generator=g).float()
                X[:, fi[c.length_name][0]] = n.float()
    y = (torch.rand(B, generator=g) < 0.4).float()
    return X, y


def params(model, dtype=torch.float64) -> Dict[str, Tensor]:
    """The model's state_dict on the CPU in `dtype` (aliased keys stay one tensor)."""
    sd = model.state_dict()
    out, seen = {}, {}
    for k, t in sd.items():
        key = (t.data_ptr(), tuple(t.shape))
        if key not in seen:
            seen[key] = t.detach().cpu().to(dtype).clone()
        out[k] = seen[key]
    return out
