"""Generate tests/golden/sharedbottom/*.npz by running the REFERENCE's own SharedBottom.forward (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_sharedbottom_golden.py          # writes tests/golden/sharedbottom/*.npz

The reference (read-only, never copied) is imported exactly as oracle/gen_golden.py imports it, with the stand-in packages of
oracle/shims/ on sys.path.  The shims make deepctr's `DNN` and `combined_dnn_input` raise (they are off the SATrans path), so
this script defines two small stand-ins of its own and assigns them to `models.sharedbottom` after importing it: a DNN of Linear
layers N(0, init_std) with relu between them (no dropout, no batch-norm: what main.py configures), and the
flatten-and-concatenate of the embedding and dense lists, which also keeps the `dnn_input` tensor so that its gradient is
recorded.

Cases (D = 4; columns: the domain column, two sparse fields, one dense field; ids offset by 1):
  plain    T = 3, bottom (16, 8), tower (8,); task 1 has no rows
  notower  T = 3, bottom (16, 8), no tower hidden units; every task has rows
The head's parameters are overwritten with random values of a visible size (weights N(0, 1) n_in^-1/2, biases 0.3 N(0, 1)):
at the default init_std = 1e-4 every gradient rounds away.  Recorded per case (arrays only; fp32 unless stated):

  X [B, columns], offset, labels [B]         the input matrix in feature_index order, the id offset, the labels
  keys, shapes                               state_dict() keys of the head's entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  dnn_input [B,C]                            what the bottom DNN receives
  y_pred [B,T]                               the probabilities of every task for every row
  loss                                       the masked-sum BCE of mtl_basemodel.py:268-269
  grad/<key>, grad/dnn_input                 its gradients: every recorded parameter and `dnn_input`
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
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from deepctr_torch.inputs import DenseFeat, SparseFeat  # noqa: E402  (shim)
import models.sharedbottom as sharedbottom  # noqa: E402  (the reference)

D, T, OFFSET = 4, 3, 1
HEAD_PREFIXES = ("bottom_dnn.", "tower_dnn.", "tower_dnn_final_layer.", "out.")
# task of every row, before the offset
CASES = {
    "plain": dict(bottom=(16, 8), tower=(8,), ids=[0, 2, 2, 0, 2, 0, 0, 2, 2, 0, 2, 2, 0, 0, 2, 0, 2, 2, 0, 2, 0, 0, 2, 2]),
    "notower": dict(bottom=(16, 8), tower=(), ids=[0, 1, 2, 2, 1, 0, 1, 2, 0, 0, 1, 2, 2, 2, 1, 0, 1, 1, 2, 0, 0, 2, 1, 2, 0]),
}


class PlainDNN(nn.Module):
    """deepctr's DNN as main.py configures it: Linear layers N(0, init_std), relu after each, no dropout, no batch-norm."""

    def __init__(self, inputs_dim, hidden_units, activation='relu', l2_reg=0, dropout_rate=0, use_bn=False, init_std=0.0001,
                 device='cpu'):
        super().__init__()
        assert activation == 'relu' and dropout_rate == 0 and not use_bn and len(hidden_units) > 0
        units = [inputs_dim] + list(hidden_units)
        self.linears = nn.ModuleList([nn.Linear(units[i], units[i + 1]) for i in range(len(units) - 1)])
        for name, tensor in self.linears.named_parameters():
            if 'weight' in name:
                nn.init.normal_(tensor, mean=0, std=init_std)

    def forward(self, x):
        for lin in self.linears:
            x = torch.relu(lin(x))
        return x


KEPT = {}


def combined_dnn_input(sparse_embedding_list, dense_value_list):
    parts = []
    if sparse_embedding_list:
        parts.append(torch.flatten(torch.cat(sparse_embedding_list, dim=-1), start_dim=1))
    if dense_value_list:
        parts.append(torch.flatten(torch.cat(dense_value_list, dim=-1), start_dim=1))
    out = torch.cat(parts, dim=-1)
    if out.requires_grad:
        out.retain_grad()
    KEPT["dnn_input"] = out
    return out


sharedbottom.DNN = PlainDNN
sharedbottom.combined_dnn_input = combined_dnn_input


def run_case(name, outdir):
    cfg = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    ids = np.asarray(cfg["ids"]) + OFFSET
    B = ids.size
    vocab = {"dom": T + OFFSET, "f0": 7, "f1": 5}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    torch.manual_seed(11)
    model = sharedbottom.SharedBottom(cols, bottom_dnn_hidden_units=cfg["bottom"], tower_dnn_hidden_units=cfg["tower"],
                                      init_std=0.0001, task_types=("binary",) * T, task_names=tuple(f"t{t}" for t in range(T)),
                                      device='cpu', domain_column="dom", flag="x")
    X = np.zeros((B, len(cols)), dtype=np.float32)
    for name_, (lo, hi) in model.feature_index.items():
        X[:, lo] = ids if name_ == "dom" else (rng.randn(B) if name_ == "price" else rng.randint(0, vocab[name_], B))
    labels = (rng.rand(B) > 0.5).astype(np.float32)
    keys = [k for k in model.state_dict() if k.startswith(HEAD_PREFIXES)]
    params = dict(model.named_parameters())
    with torch.no_grad():
        for emb in model.embedding_dict.values():      # embeddings of a visible size, so that dnn_input is not 1e-4 noise
            emb.weight.copy_(torch.from_numpy(rng.randn(*emb.weight.shape).astype(np.float32)))
        for k in keys:
            p = params[k]
            v = rng.randn(*p.shape) * p.shape[1] ** -0.5 if k.endswith("weight") else 0.3 * rng.randn(*p.shape)
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    out = dict(X=X, offset=np.array(OFFSET), labels=labels, keys=np.array(keys),
               shapes=np.array([str(tuple(sd[k].shape)) for k in keys]))
    for k in keys:
        out[f"param/{k}"] = sd[k].numpy().copy()
    Xt, y = torch.from_numpy(X), torch.from_numpy(labels)
    model.train()
    y_pred = model(Xt)
    domain_ids = Xt[:, model.feature_index["dom"][0]].long()
    # the loss of the reference's fit() for a list of loss functions, one task per scenario
    loss = sum([F.binary_cross_entropy(y_pred[:, i][domain_ids == (i + OFFSET)], y[domain_ids == (i + OFFSET)], reduction='sum')
                for i in range(T)])
    loss.backward()
    out["dnn_input"] = KEPT["dnn_input"].detach().numpy().copy()
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = loss.detach().numpy().copy()
    out["grad/dnn_input"] = KEPT["dnn_input"].grad.numpy().copy()
    for k in keys:
        g = params[k].grad
        out[f"grad/{k}"] = (g if g is not None else torch.zeros_like(params[k])).numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "sharedbottom")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
