"""Generate tests/golden/star/*.npz by running the REFERENCE's own Star_Net.forward (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_star_golden.py          # writes tests/golden/star/*.npz

The reference (`/root/reference`, read-only, never copied) is imported exactly as oracle/gen_golden.py imports it, with the
stand-in packages of oracle/shims/ on sys.path.  The shims make deepctr's `DNN` and `combined_dnn_input` raise (they are off
the SATrans path), so this script defines two small stand-ins of its own and assigns them to `models.star` after importing
it: a module with `.linears`, `.activation_layers`, `.dropout` and `.use_bn` (what star.py:156-165 touches), and the
flatten-and-concatenate of the embedding and dense lists, which also keeps the `dnn_input` tensor so that its gradient is
recorded.  `model.domain_id_offset` is set by hand (the reference's fit() sets it from the data).

Cases: `plain` (use_domain_bn=False; scenario 1 has no rows) and `bn` (use_domain_bn=True; every scenario has >= 2 rows).
Columns: the domain column, two sparse fields, one dense field; D = 4, hidden (16, 8), S = 3, ids offset by 1.  The tower
parameters are overwritten with random values scaled n_in^-1/4 (so W_dom * W_sh is about n_in^-1/2): at the default
init_std = 1e-4 the products are 1e-8 and every gradient rounds away.  Recorded per case (arrays only; fp32 unless stated):

  X [B, columns], offset, w [B,1]            the input matrix in feature_index order, the id offset, the upstream weights
  keys, shapes                               state_dict() keys of the tower / normalisation entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  dnn_input [B,C]                            what the towers (or the normalisation in front of them) receive
  y_train, y_eval [B,1]                      y_pred in training mode (first) and in evaluation mode (after that one step)
  buf/<key>                                  (bn) the buffers after the training-mode forward
  grad_train/<key>, grad_eval/<key>          gradients of sum(y_pred * w): every recorded parameter and `dnn_input`
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

from deepctr_torch.inputs import DenseFeat, SparseFeat  # noqa: E402  (shim)
import models.star as star  # noqa: E402  (the reference)

HIDDEN, D, S, OFFSET = (16, 8), 4, 3, 1
TOWER_PREFIXES = ("shared_bn_", "bns.", "domain_dnns.", "domain_dnn_linears.", "shared_dnn.", "shared_dnn_linear.")
# scenario of every row, before the offset
CASES = {
    "plain": dict(bn=False, ids=[0, 2, 2, 0, 2, 0, 0, 2, 2, 0, 2, 2, 0, 0, 2, 0, 2, 2, 0, 2, 0, 0, 2, 2]),
    "bn": dict(bn=True, ids=[0, 1, 2, 2, 1, 0, 1, 2, 0, 0, 1, 2, 2, 2, 1, 0, 1, 1, 2, 0, 0, 2, 1, 2, 0]),
}


class TowerDNN(nn.Module):
    """What star.py:156-165 touches of deepctr's DNN: Linear layers N(0, init_std), relu, no dropout, no batch-norm."""

    def __init__(self, inputs_dim, hidden_units, activation='relu', l2_reg=0, dropout_rate=0, use_bn=False, init_std=0.0001,
                 device='cpu'):
        super().__init__()
        assert activation == 'relu' and dropout_rate == 0 and not use_bn
        units = [inputs_dim] + list(hidden_units)
        self.use_bn = use_bn
        self.dropout = nn.Dropout(dropout_rate)
        self.linears = nn.ModuleList([nn.Linear(units[i], units[i + 1]) for i in range(len(units) - 1)])
        self.activation_layers = nn.ModuleList([nn.ReLU(inplace=False) for _ in range(len(units) - 1)])
        for name, tensor in self.linears.named_parameters():
            if 'weight' in name:
                nn.init.normal_(tensor, mean=0, std=init_std)


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


star.DNN = TowerDNN
star.combined_dnn_input = combined_dnn_input


def run_case(name, outdir):
    cfg = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    ids = np.asarray(cfg["ids"]) + OFFSET
    B = ids.size
    vocab = {"dom": S + OFFSET, "f0": 7, "f1": 5}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    torch.manual_seed(11)
    model = star.Star_Net(cols, cols, "dom", S, domain_id_as_feature=True, att_layer_num=0, dnn_hidden_units=HIDDEN,
                          use_domain_dnn=True, use_domain_bn=cfg["bn"], init_std=0.0001, device='cpu', flag="x")
    model.domain_id_offset = OFFSET
    X = np.zeros((B, len(cols)), dtype=np.float32)
    for name_, (lo, hi) in model.feature_index.items():
        X[:, lo] = ids if name_ == "dom" else (rng.randn(B) if name_ == "price" else rng.randint(0, vocab[name_], B))
    w = rng.randn(B, 1).astype(np.float32)
    keys = [k for k in model.state_dict() if k.startswith(TOWER_PREFIXES)]
    params = dict(model.named_parameters())
    with torch.no_grad():
        for emb in model.embedding_dict.values():      # embeddings of a visible size, so that dnn_input is not 1e-4 noise
            emb.weight.copy_(torch.from_numpy(rng.randn(*emb.weight.shape).astype(np.float32)))
        for k in keys:
            if k not in params:
                continue
            p = params[k]
            if k.startswith("shared_bn_") or k.startswith("bns."):
                base = 1.0 if k.endswith("weight") else 0.0
                v = base + 0.3 * rng.randn(*p.shape)
            elif k.endswith("weight"):
                v = rng.randn(*p.shape) * p.shape[1] ** -0.25
            else:
                v = 0.3 * rng.randn(*p.shape)
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    out = dict(X=X, offset=np.array(OFFSET), w=w, keys=np.array(keys), shapes=np.array([str(tuple(sd[k].shape)) for k in keys]))
    for k in keys:
        if k in params:
            out[f"param/{k}"] = sd[k].numpy().copy()
    Xt, wt = torch.from_numpy(X), torch.from_numpy(w)
    for mode in ("train", "eval"):
        model.train(mode == "train")
        model.zero_grad(set_to_none=True)
        y = model(Xt)
        out[f"y_{mode}"] = y.detach().numpy().copy()
        if mode == "train":
            out["dnn_input"] = KEPT["dnn_input"].detach().numpy().copy()
            for k in keys:
                if k not in params:
                    out[f"buf/{k}"] = model.state_dict()[k].numpy().copy()
        (y * wt).sum().backward()
        out[f"grad_{mode}/dnn_input"] = KEPT["dnn_input"].grad.numpy().copy()
        for k in keys:
            if k in params and params[k].grad is not None:
                out[f"grad_{mode}/{k}"] = params[k].grad.numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "star")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
