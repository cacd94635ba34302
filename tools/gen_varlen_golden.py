"""Generate tests/golden/varlen/varlen_*.npz by running the REFERENCE's SATrans with VarLenSparseFeat columns (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_varlen_golden.py          # writes tests/golden/varlen/varlen_*.npz

The reference (`/root/reference`, read-only, never copied) is imported exactly as oracle/gen_golden.py imports it, with the
stand-in packages of oracle/shims/.  The shim's two varlen functions only raise; for the run of this script they are replaced,
in the reference's module namespace, by deepctr-torch 0.2.9's lookup (`embedding_dict[embedding_name](X[:, lo:hi].long())`)
and the pooling of tests/varlen_reference.py (SequencePoolingLayer: mask by id != 0 or by the length column; sum / mean /
max).  Everything else - construction and its generator draws, concatenation, dnn_linear sizing, the regulariser over
embedding_dict, BCE(sum), torch.optim.Adam - is the reference's own code.  Recorded per case, in gen_golden.py's layout:

  param/<key>, alias/<key>   state_dict() right after construction
  X, y                       float32 input matrix in feature_index order (padding, duplicates and empty lists included)
  out/prob, out/logit        eval-mode forward
  train/bce, train/reg       loss pieces of the first train-mode step (every dropout p = 0)
  grad/<key>                 its gradients
  adam/<key>                 every unique tensor after `adam_steps` torch.optim.Adam steps
  meta                       json: fields, varlen (name, vocab, maxlen, combiner, length_name), dense, shapes, flags
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402  (puts the shims and the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import models.meta_basemodel as ref_base  # noqa: E402  (the reference)
from deepctr_torch.inputs import DenseFeat, SparseFeat, VarLenSparseFeat, get_feature_names  # noqa: E402  (shim)
from models.satrans import SATrans  # noqa: E402  (the reference)
from tests import varlen_reference as V  # noqa: E402

SPARSE = ['f0', 'f1', 'f2', 'f3', 'dom']
SPARSE_MAX = {'f0': 30, 'f1': 9, 'f2': 2, 'f3': 17, 'dom': 3}
HIST_VOCAB = [23, 9, 40]
CASES = {
    'varlen_sum': dict(combiners=('sum', 'sum'), length=False, dense=[]),
    'varlen_mean': dict(combiners=('mean', 'mean'), length=False, dense=[]),
    'varlen_max': dict(combiners=('max', 'max'), length=False, dense=[]),
    'varlen_length': dict(combiners=('mean', 'max'), length=True, dense=[]),
    'varlen_dense': dict(combiners=('max', 'sum'), length=False, dense=['price']),
}
D, H, L, UNITS, LR, SEED, B, ADAM_STEPS = 16, 2, 2, (32, 16), 0.005, '1021', 48, 2


def varlen_embedding_lookup(X, embedding_dict, sequence_input_dict, varlen_sparse_feature_columns):
    """deepctr-torch 0.2.9: {feature name: embedding of its [B, maxlen] id block} (every slot looked up, padding included)."""
    out = {}
    for c in varlen_sparse_feature_columns:
        lo, hi = sequence_input_dict[c.name]
        out[c.name] = embedding_dict[c.embedding_name](X[:, lo:hi].long())
    return out


def get_varlen_pooling_list(embedding_dict, features, feature_index, varlen_sparse_feature_columns, device):
    """deepctr-torch 0.2.9 SequencePoolingLayer per column, as tests/varlen_reference.py restates it: [B, 1, D] each."""
    out = []
    for c in varlen_sparse_feature_columns:
        lo = feature_index[c.name][0]
        len_col = feature_index[c.length_name][0] if c.length_name is not None else None
        v = V.VarSpec(c.name, lo, c.maxlen, c.combiner, len_col)
        out.append(V.pool_rows(embedding_dict[c.name], V.slot_mask(features, v), v).unsqueeze(1))
    return out


def build(cfg):
    columns = [SparseFeat(f, vocabulary_size=SPARSE_MAX[f] + 2, embedding_dim=D) for f in SPARSE]
    columns += [VarLenSparseFeat(SparseFeat(f"h{j}", vocabulary_size=HIST_VOCAB[j], embedding_dim=D), maxlen=3, combiner=c,
                                 length_name=f"h{j}_len" if cfg['length'] else None) for j, c in enumerate(cfg['combiners'])]
    columns += [DenseFeat(f, 1) for f in cfg['dense']]
    model = SATrans(linear_feature_columns=columns, dnn_feature_columns=columns, domain_column_list=['dom'],
                    num_domains_list=[SPARSE_MAX['dom']], att_layer_num=0, domain_att_layer_num=L, att_head_num=H,
                    share_domain_dnn_across_layers=False, use_domain_dnn_linear=False, use_linear=False, meta_mode='QK',
                    use_dnn=False, meta_dnn_hidden_units=UNITS, seed=SEED, device='cpu', flag='sota')
    return model, columns


def inputs(columns, rng):
    """Sparse ids, scenario ids 1..3, id lists of random length (every fourth sample empty) with 0 padding - also between valid
    ids when there is no length column - and small vocabularies (duplicates), dense values in [0, 1)."""
    cols = {}
    for c in columns:
        if isinstance(c, SparseFeat):
            cols[c.name] = rng.randint(1 if c.name == 'dom' else 0, SPARSE_MAX[c.name] + 1, size=B)
        elif isinstance(c, DenseFeat):
            cols[c.name] = rng.rand(B).astype(np.float32)
        else:
            n = rng.randint(0, c.maxlen + 1, size=B)
            n[::4] = 0
            ids = rng.randint(1, c.vocabulary_size, size=(B, c.maxlen))
            if c.length_name is None:
                keep = rng.rand(B, c.maxlen).argsort(1).argsort(1) < n[:, None]
                cols[c.name] = np.where(keep, ids, 0)
            else:
                cols[c.name] = rng.randint(0, c.vocabulary_size, size=(B, c.maxlen))
                cols[c.length_name] = n
    return cols, (rng.rand(B) < 0.3).astype(np.float32)


def run_case(name, outdir):
    cfg = CASES[name]
    model, columns = build(cfg)
    out = {}
    G.pack_state(model, "param", out)
    names = get_feature_names(columns)
    cols, y = inputs(columns, np.random.RandomState(sum(map(ord, name))))
    X = np.concatenate([np.asarray(cols[n]).reshape(B, -1) for n in names], axis=-1).astype(np.float32)
    Xt = torch.from_numpy(X)
    out["X"], out["y"] = X, y
    taps = {}
    hook = model.dnn_linear.register_forward_hook(lambda m, i, o: taps.__setitem__("logit", o.detach().clone()))
    model.eval()
    with torch.no_grad():
        out["out/prob"] = model(Xt).numpy().copy()
    hook.remove()
    out["out/logit"] = taps["logit"].numpy()
    G.zero_dropout(model)
    model.train()
    optim = torch.optim.Adam(model.parameters(), lr=LR)
    model.compile(optim, "binary_crossentropy", metrics=["binary_crossentropy"])
    yt = torch.from_numpy(y)
    for step in range(ADAM_STEPS):
        y_pred = model(Xt).squeeze()
        optim.zero_grad()
        loss = model.loss_func(y_pred, yt, reduction='sum')
        reg = model.get_regularization_loss()
        (loss + reg + model.aux_loss).backward()
        if step == 0:
            out["train/bce"] = np.array(loss.item(), dtype=np.float64)
            out["train/reg"] = np.array(reg.item(), dtype=np.float64)
            seen = set()
            for k, p in model.named_parameters():
                if p.grad is not None and p.data_ptr() not in seen:
                    seen.add(p.data_ptr())
                    out[f"grad/{k}"] = p.grad.detach().numpy().copy()
        optim.step()
    G.pack_state(model, "adam", out)
    meta = dict(name=name, sparse=SPARSE, vocab=[SPARSE_MAX[f] + 2 for f in SPARSE],
                varlen=[dict(name=f"h{j}", vocab=HIST_VOCAB[j], maxlen=3, combiner=c,
                             length_name=f"h{j}_len" if cfg['length'] else None) for j, c in enumerate(cfg['combiners'])],
                dense=cfg['dense'], domain=['dom'], num_domains_list=[SPARSE_MAX['dom']], D=D, H=H, L=L, units=list(UNITS),
                flag='sota', mode='QK', lr=LR, seed=SEED, adam_steps=ADAM_STEPS, feature_names=names, torch=torch.__version__)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    ref_base.varlen_embedding_lookup = varlen_embedding_lookup          # (this process only; the shim files are untouched)
    ref_base.get_varlen_pooling_list = get_varlen_pooling_list
    outdir = os.path.join(ROOT, "tests", "golden", "varlen")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
