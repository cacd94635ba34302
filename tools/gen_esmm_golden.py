"""Generate tests/golden/esmm/*.npz and tests/golden/wdl/*.npz by running the REFERENCE's own ESMM.forward and WDL.forward (CPU;
build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_esmm_golden.py          # writes tests/golden/esmm/*.npz, tests/golden/wdl/*.npz

The reference (read-only, never copied) is imported exactly as oracle/gen_golden.py imports it, with the stand-in packages of
oracle/shims/ on sys.path.  The shims make deepctr's `DNN` and `combined_dnn_input` raise (they are off the SATrans path), so
this script defines two small stand-ins of its own, as tools/gen_sharedbottom_golden.py does, and assigns them to `models.esmm`
and `models.wdl` after importing them: a DNN of Linear layers N(0, init_std) with relu between them, and the
flatten-and-concatenate of the embedding and dense lists, which also keeps the `dnn_input` tensor so that its gradient is
recorded.  main.py cannot build ESMM (it passes `flag=`, which ESMM's constructor does not take); the class itself constructs
and runs, and that is what is recorded here.

No dropout is recorded: the reference's masks come from torch's generator stream, which the kernels by design do not replay
(csrc/rng.h); the dropout arithmetic is tested against tests/esmm_reference.py with the kernels' own masks.

Cases (D = 4, B = 24; columns: the domain column, two sparse fields, one dense field):
  esmm/two_layers   ESMM, towers (16, 8)          esmm/one_layer   ESMM, towers (8,)
  wdl/two_layers    WDL, hidden units (16, 8), flag "None"
The head's parameters are overwritten with random values of a visible size (weights N(0, 1) n_in^-1/2, biases 0.3 N(0, 1)):
at the default init_std = 1e-4 every gradient rounds away.  Recorded per case (arrays only; fp32 unless stated):

  X [B, columns], labels [B, tasks]          the input matrix in feature_index order, the labels
  keys, shapes                               state_dict() keys of the head's entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  dnn_input [B,C]                            what the DNNs receive
  y_pred [B, tasks]                          ESMM: (ctr, ctcvr); WDL: the probability
  loss                                       the summed BCE over every column of y_pred
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
import models.esmm as esmm  # noqa: E402  (the reference)
import models.wdl as wdl  # noqa: E402  (the reference)

D, B = 4, 24
CASES = {
    "esmm/two_layers": dict(model="esmm", units=(16, 8)),
    "esmm/one_layer": dict(model="esmm", units=(8,)),
    "wdl/two_layers": dict(model="wdl", units=(16, 8)),
}
HEAD_PREFIXES = {"esmm": ("out.", "ctr_dnn.", "cvr_dnn.", "ctr_dnn_final_layer.", "cvr_dnn_final_layer."),
                 "wdl": ("out.", "dnn.", "dnn_linear.")}


class PlainDNN(nn.Module):
    """deepctr's DNN without its options: Linear layers N(0, init_std), relu after each, no dropout, no batch-norm."""

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


for module in (esmm, wdl):
    module.DNN = PlainDNN
    module.combined_dnn_input = combined_dnn_input


def run_case(name, outdir):
    cfg = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    vocab = {"dom": 3, "f0": 7, "f1": 5}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    torch.manual_seed(11)
    if cfg["model"] == "esmm":
        model = esmm.ESMM(cols, tower_dnn_hidden_units=cfg["units"], init_std=0.0001, device='cpu', domain_column="dom")
        tasks = 2
    else:
        model = wdl.WDL(cols, cols, dnn_hidden_units=cfg["units"], init_std=0.0001, device='cpu', flag="None", domain_column="dom",
                        num_domains=vocab["dom"])
        tasks = 1
    X = np.zeros((B, len(cols)), dtype=np.float32)
    for name_, (lo, hi) in model.feature_index.items():
        X[:, lo] = rng.randn(B) if name_ == "price" else rng.randint(0, vocab[name_], B)
    labels = (rng.rand(B, tasks) > 0.5).astype(np.float32)
    keys = [k for k in model.state_dict() if k.startswith(HEAD_PREFIXES[cfg["model"]])]
    params = dict(model.named_parameters())
    with torch.no_grad():
        for emb in model.embedding_dict.values():      # embeddings of a visible size, so that dnn_input is not 1e-4 noise
            emb.weight.copy_(torch.from_numpy(rng.randn(*emb.weight.shape).astype(np.float32)))
        for k in keys:
            p = params[k]
            v = rng.randn(*p.shape) * p.shape[1] ** -0.5 if k.endswith("weight") else 0.3 * rng.randn(*p.shape)
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    out = dict(X=X, labels=labels, keys=np.array(keys), shapes=np.array([str(tuple(sd[k].shape)) for k in keys]))
    for k in keys:
        out[f"param/{k}"] = sd[k].numpy().copy()
    Xt, y = torch.from_numpy(X), torch.from_numpy(labels)
    model.train()
    y_pred = model(Xt)
    assert tuple(y_pred.shape) == (B, tasks)
    loss = F.binary_cross_entropy(y_pred, y, reduction='sum')
    loss.backward()
    out["dnn_input"] = KEPT["dnn_input"].detach().numpy().copy()
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = loss.detach().numpy().copy()
    out["grad/dnn_input"] = KEPT["dnn_input"].grad.numpy().copy()
    for k in keys:
        g = params[k].grad
        out[f"grad/{k}"] = (g if g is not None else torch.zeros_like(params[k])).numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, keys {keys}, {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden")   # (directories of their own: tests/helpers.py lists golden/*.npz)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
