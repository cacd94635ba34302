"""Generate tests/golden/input/*.npz by running the REFERENCE's own `Linear` and `BaseModel.input_from_feature_columns` (CPU; build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_input_golden.py          # writes tests/golden/input/{plain,varlen,shared}.npz

The reference (read-only, never copied) is imported exactly as oracle/gen_golden.py imports it, with the stand-in packages of
oracle/shims/.  The shim's two varlen functions only raise; for the run of this script they are replaced, in the reference's
module namespace, as tools/gen_varlen_golden.py replaces them (deepctr-torch 0.2.9's lookup and SequencePoolingLayer).  The
construction with its generator draws, both forwards, the concatenation and autograd are the reference's / torch's own.  After
construction every parameter is multiplied by 1000 (N(0, 1e-4) -> N(0, 0.1)) so that the recorded values are of a size at which
a bound relative to the largest element means something.  Recorded per case:

  col/kind, col/name, col/embedding_name, col/vocab, col/dim, col/maxlen, col/combiner, col/length_name
                             the feature columns as plain arrays (kind: sparse / dense / varlen; dim: embedding_dim or dimension)
  X                          float32 input matrix in feature_index order, B = 24
  linear/<key>, emb/<key>    the state_dict of linear_model and of embedding_dict as the run saw them
  out/linear_logit, out/emb, out/dense        the two forwards (emb: the list concatenated along the fields)
  c, C                       the weights of loss = sum_b c_b linear_logit_b + sum C * emb
  grad_linear/<key>, grad_emb/<key>           its gradients
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402,F401  (puts the shims and the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.meta_basemodel as ref_base  # noqa: E402  (the reference)
from deepctr_torch.inputs import DenseFeat, SparseFeat, VarLenSparseFeat, get_feature_names  # noqa: E402  (shim)
from tools.gen_varlen_golden import get_varlen_pooling_list, varlen_embedding_lookup  # noqa: E402

B, D, SEED = 24, 16, 1021


def plain():
    cols = [SparseFeat("user", 50, embedding_dim=D), DenseFeat("price", 1), SparseFeat("item", 37, embedding_dim=D),
            SparseFeat("cate", 4, embedding_dim=D), DenseFeat("stats", 3), SparseFeat("dom", 3, embedding_dim=D)]
    return cols, {}


def varlen():
    """sum and max masked by id != 0, mean with a length column; sample 3: the mean list empty (length 0), sample 5: the max
    list all padding (every id 0)."""
    cols = [SparseFeat("user", 50, embedding_dim=D), SparseFeat("cate", 4, embedding_dim=D),
            VarLenSparseFeat(SparseFeat("h_sum", 23, embedding_dim=D), maxlen=3, combiner="sum"),
            VarLenSparseFeat(SparseFeat("h_mean", 9, embedding_dim=D), maxlen=4, combiner="mean", length_name="h_mean_len"),
            VarLenSparseFeat(SparseFeat("h_max", 40, embedding_dim=D), maxlen=3, combiner="max"), DenseFeat("price", 1)]
    return cols, {"empty": ("h_mean", 3), "all_padding": ("h_max", 5)}


def shared():
    cols = [SparseFeat("user", 50, embedding_dim=D), SparseFeat("click_item", 31, embedding_dim=D, embedding_name="item"),
            SparseFeat("cart_item", 31, embedding_dim=D, embedding_name="item"), DenseFeat("price", 1)]
    return cols, {}


CASES = {"plain": plain, "varlen": varlen, "shared": shared}


def inputs(cols, special, rng):
    """Uniform ids; lists of 1..maxlen DISTINCT valid ids >= 1 (no tie between valid slots under max), zeros around them without
    a length column, arbitrary in-range ids behind the length with one; the two special samples of the varlen case."""
    out = {}
    for c in cols:
        if isinstance(c, SparseFeat):
            out[c.name] = rng.randint(0, c.vocabulary_size, size=B)
        elif isinstance(c, DenseFeat):
            out[c.name] = (rng.rand(B, c.dimension) * 2 - 1).astype(np.float32)
        else:
            ids = 1 + np.stack([rng.permutation(c.vocabulary_size - 1)[:c.maxlen] for _ in range(B)])
            n = rng.randint(1, c.maxlen + 1, size=B)
            if c.length_name is None:
                keep = rng.rand(B, c.maxlen).argsort(1).argsort(1) < n[:, None]
                out[c.name] = np.where(keep, ids, 0)
            else:
                out[c.name], out[c.length_name] = ids, n
    if special:
        name, b = special["empty"]
        out[name + "_len"][b] = 0
        name, b = special["all_padding"]
        out[name][b] = 0
    return out


def run_case(name, outdir):
    cols, special = CASES[name]()
    model = ref_base.BaseModel(cols, cols, seed=SEED, device="cpu")
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1000.0)
    names = get_feature_names(cols)
    rng = np.random.RandomState(sum(map(ord, name)))
    vals = inputs(cols, special, rng)
    X = np.concatenate([np.asarray(vals[n]).reshape(B, -1) for n in names], axis=-1).astype(np.float32)
    Xt = torch.from_numpy(X)
    out = {"X": X}
    kinds = {SparseFeat: "sparse", DenseFeat: "dense", VarLenSparseFeat: "varlen"}
    out["col/kind"] = np.array([kinds[type(c)] for c in cols])
    out["col/name"] = np.array([c.name for c in cols])
    out["col/embedding_name"] = np.array([getattr(c, "embedding_name", "") for c in cols])
    out["col/vocab"] = np.array([getattr(c, "vocabulary_size", 0) for c in cols])
    out["col/dim"] = np.array([c.dimension if isinstance(c, DenseFeat) else c.embedding_dim for c in cols])
    out["col/maxlen"] = np.array([getattr(c, "maxlen", 0) for c in cols])
    out["col/combiner"] = np.array([getattr(c, "combiner", "") for c in cols])
    out["col/length_name"] = np.array([getattr(c, "length_name", None) or "" for c in cols])
    for k, v in model.linear_model.state_dict().items():
        out[f"linear/{k}"] = v.detach().numpy().copy()
    for k, v in model.embedding_dict.state_dict().items():
        out[f"emb/embedding_dict.{k}"] = v.detach().numpy().copy()
    linear_logit = model.linear_model(Xt)
    emb_list, dense_list = model.input_from_feature_columns(Xt, cols, model.embedding_dict)
    emb = torch.cat(emb_list, dim=1)
    dense = torch.cat(dense_list, dim=-1)
    c = torch.from_numpy(rng.randn(B).astype(np.float32))
    Cw = torch.from_numpy(rng.randn(*emb.shape).astype(np.float32))
    ((linear_logit.squeeze(-1) * c).sum() + (emb * Cw).sum()).backward()
    out["out/linear_logit"], out["out/emb"], out["out/dense"] = linear_logit.detach().numpy(), emb.detach().numpy(), dense.numpy()
    out["c"], out["C"] = c.numpy(), Cw.numpy()
    for k, p in model.linear_model.named_parameters():
        out[f"grad_linear/{k}"] = p.grad.numpy().copy()
    for k, p in model.embedding_dict.named_parameters():
        out[f"grad_emb/embedding_dict.{k}"] = p.grad.numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    ref_base.varlen_embedding_lookup = varlen_embedding_lookup          # (this process only; the shim files are untouched)
    ref_base.get_varlen_pooling_list = get_varlen_pooling_list
    outdir = os.path.join(ROOT, "tests", "golden", "input")
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
