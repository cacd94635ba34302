"""Generate tests/golden/dcn/*.npz by running the REFERENCE's own DCN.forward (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_dcn_golden.py          # writes tests/golden/dcn/*.npz

The reference (read-only, never copied) is imported exactly as tools/gen_cin_golden.py imports it, with the stand-in packages of
oracle/shims/ on sys.path.  models/dcn.py takes `CrossNet`, `DNN` and `concat_fun` from deepctr_torch.layers; the shims have
`concat_fun`, no `CrossNet`, and a `DNN` that raises (both are off the SATrans path), and deepctr-torch itself is not part of
the reference tree.  So BEFORE the import this script assigns two stand-ins of its own to deepctr_torch.layers: a DNN of Linear
layers N(0, init_std) with relu between them (no dropout, no batch-norm: what main.py configures), and a CrossNet written from
deepctr-torch 0.2.9's definition - `kernels` [L, N, 1] or [L, N, N] and `bias` [L, N, 1], xavier_normal_ per layer, the
tensordot / matmul forms - with deepctr's parameter names.

The stand-in DNN accepts an EMPTY hidden_units (no layers, the identity).  deepctr's own DNN raises there, so the case
`cross_only` pins the reference's `elif self.cross_num > 0` branch of DCN.forward, not a configuration deepctr-torch itself can
construct.

What the fixtures pin, and what they do not.  They pin the reference's WIRING: what goes into the cross network and the DNN (the
flattened embeddings of ALL sparse fields, the domain column included, then the dense values), the concatenation order (cross,
then deep), `dnn_linear`, `out`, the state_dict key names and their order, and which parameters DCN regularises.  The CrossNet
ARITHMETIC comes from the stand-in below, not from deepctr's code: the fixtures hold the product code and
tests/cross_reference.py to that definition as written here.

Cases (D = 4; columns: the domain column, three sparse fields, one dense field, so N = 17; B = 24; flag "x"):
  vector      cross_num 2, 'vector', dnn_hidden_units (16, 8)
  matrix      cross_num 3, 'matrix', dnn_hidden_units (16, 8)
  cross_only  cross_num 2, 'vector', dnn_hidden_units ()
Embeddings (also the linear model's) and the head's parameters are overwritten with values of a visible size (embeddings
N(0, 1), weights and kernels N(0, 1) n_in^-1/2, biases 0.3 N(0, 1)): at the default init_std = 1e-4 every gradient rounds away.
Recorded per case (arrays only; fp32 unless stated):

  X [B, columns], labels [B]                 the input matrix in feature_index order, the labels
  matrix                                     0 / 1
  keys, shapes                               state_dict() keys of the head's entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  emb [B,F,D], dense [B,1], linear_logit [B,1]
                                             the looked-up embeddings in field order, the dense values, linear_model's output
  y_pred [B,1], loss                         the probabilities; the summed BCE
  reg_loss [1]                               get_regularization_loss() over the entries DCN.__init__ itself appended (the
                                             model's last three regularization_weight entries)
  grad/<key>, grad/emb                       the loss's gradients: every recorded parameter, and the looked-up embeddings
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

import deepctr_torch.layers as shim_layers  # noqa: E402  (shim)
from deepctr_torch.inputs import DenseFeat, SparseFeat  # noqa: E402  (shim)

D, B, NUM_DOMAINS = 4, 24, 3
HEAD_PREFIXES = ("out.", "dnn.", "dnn_linear.", "crossnet.")
CASES = {
    "vector": dict(cross=2, form="vector", dnn=(16, 8)),
    "matrix": dict(cross=3, form="matrix", dnn=(16, 8)),
    "cross_only": dict(cross=2, form="vector", dnn=()),
}


class PlainDNN(nn.Module):
    """deepctr's DNN as main.py configures it: Linear layers N(0, init_std), relu after each, no dropout, no batch-norm.
    Unlike deepctr's, it accepts an empty hidden_units."""

    def __init__(self, inputs_dim, hidden_units, activation='relu', l2_reg=0, dropout_rate=0, use_bn=False, init_std=0.0001,
                 device='cpu'):
        super().__init__()
        assert activation == 'relu' and dropout_rate == 0 and not use_bn
        units = [inputs_dim] + list(hidden_units)
        self.linears = nn.ModuleList([nn.Linear(units[i], units[i + 1]) for i in range(len(units) - 1)])
        for name, tensor in self.linears.named_parameters():
            if 'weight' in name:
                nn.init.normal_(tensor, mean=0, std=init_std)

    def forward(self, x):
        for lin in self.linears:
            x = torch.relu(lin(x))
        return x


class StandInCrossNet(nn.Module):
    """The cross network as deepctr-torch 0.2.9 defines it (parameters `kernels`, `bias`)."""

    def __init__(self, in_features, layer_num=2, parameterization='vector', seed=1024, device='cpu'):
        super().__init__()
        if parameterization not in ('vector', 'matrix'):
            raise ValueError("parameterization should be 'vector' or 'matrix'")
        self.layer_num, self.parameterization = layer_num, parameterization
        self.kernels = nn.Parameter(torch.empty(layer_num, in_features, 1 if parameterization == 'vector' else in_features))
        self.bias = nn.Parameter(torch.empty(layer_num, in_features, 1))
        for i in range(layer_num):
            nn.init.xavier_normal_(self.kernels[i])
        for i in range(layer_num):
            nn.init.zeros_(self.bias[i])

    def forward(self, inputs):
        x_0 = inputs.unsqueeze(2)
        x_l = x_0
        for i in range(self.layer_num):
            if self.parameterization == 'vector':
                xl_w = torch.tensordot(x_l, self.kernels[i], dims=([1], [0]))
                x_l = torch.matmul(x_0, xl_w) + self.bias[i] + x_l
            else:
                x_l = x_0 * (torch.matmul(self.kernels[i], x_l) + self.bias[i]) + x_l
        return torch.squeeze(x_l, dim=2)


shim_layers.CrossNet = StandInCrossNet
shim_layers.DNN = PlainDNN

import models.dcn as dcn  # noqa: E402  (the reference)


def run_case(name, outdir):
    cfg = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    vocab = {"dom": NUM_DOMAINS + 1, "f0": 7, "f1": 5, "f2": 9}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    torch.manual_seed(11)
    model = dcn.DCN(cols, cols, cross_num=cfg["cross"], cross_parameterization=cfg["form"], dnn_hidden_units=cfg["dnn"],
                    init_std=0.0001, device='cpu', flag="x", domain_column="dom", num_domains=NUM_DOMAINS,
                    meta_dnn_hidden_units=(D, 8, D))
    X = np.zeros((B, len(cols)), dtype=np.float32)
    for name_, (lo, hi) in model.feature_index.items():
        X[:, lo] = rng.randn(B) if name_ == "price" else rng.randint(0, vocab[name_], B)
    labels = (rng.rand(B) > 0.5).astype(np.float32)
    keys = [k for k in model.state_dict() if k.startswith(HEAD_PREFIXES)]
    params = dict(model.named_parameters())
    with torch.no_grad():
        for emb in list(model.embedding_dict.values()) + list(model.linear_model.embedding_dict.values()):
            emb.weight.copy_(torch.from_numpy(rng.randn(*emb.weight.shape).astype(np.float32)))
        model.linear_model.weight.copy_(torch.from_numpy(rng.randn(*model.linear_model.weight.shape).astype(np.float32)))
        for k in keys:
            p = params[k]
            if k.endswith("weight") or k == "crossnet.kernels":      # (kernels [L, N, .]: N = shape[1] too)
                v = rng.randn(*p.shape) * p.shape[1] ** -0.5
            else:
                v = 0.3 * rng.randn(*p.shape)
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    out = dict(X=X, labels=labels, matrix=np.array(int(cfg["form"] == "matrix")), keys=np.array(keys),
               shapes=np.array([str(tuple(sd[k].shape)) for k in keys]))
    for k in keys:
        out[f"param/{k}"] = sd[k].numpy().copy()
    kept = {}
    lookup = model.input_from_feature_columns

    def keeping_lookup(*a, **k):
        sparse, dense = lookup(*a, **k)
        for e in sparse:
            e.retain_grad()
        kept["sparse"], kept["dense"] = sparse, dense
        return sparse, dense

    model.input_from_feature_columns = keeping_lookup
    model.linear_model.register_forward_hook(lambda mod, args, res: kept.__setitem__("linear_logit", res.detach().clone()))
    Xt, y = torch.from_numpy(X), torch.from_numpy(labels)
    model.train()
    y_pred = model(Xt)
    loss = F.binary_cross_entropy(y_pred.squeeze(1), y, reduction='sum')
    loss.backward()
    # the entries DCN.__init__ appended: the DNN's weights (l2_reg_dnn = 0), dnn_linear.weight, crossnet.kernels
    every = model.regularization_weight
    own = every[-3:]
    assert own[1][0][0] is model.dnn_linear.weight and own[2][0][0] is model.crossnet.kernels
    model.regularization_weight = own
    out["reg_loss"] = model.get_regularization_loss().detach().numpy().copy()
    model.regularization_weight = every
    out["emb"] = torch.cat(kept["sparse"], dim=1).detach().numpy().copy()
    out["grad/emb"] = torch.cat([e.grad for e in kept["sparse"]], dim=1).numpy().copy()
    out["dense"] = torch.cat(kept["dense"], dim=-1).detach().numpy().copy()
    out["linear_logit"] = kept["linear_logit"].numpy().copy()
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = loss.detach().numpy().copy()
    for k in keys:
        out[f"grad/{k}"] = params[k].grad.numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "dcn")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
