"""Generate tests/golden/pnn/*.npz by running the REFERENCE's own PNN.forward (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_pnn_golden.py          # writes tests/golden/pnn/*.npz

The reference (read-only, never copied) is imported exactly as tools/gen_fibinet_golden.py imports it, with the stand-in packages
of oracle/shims/ on sys.path.  models/pnn.py takes `InnerProductLayer`, `OutterProductLayer`, `DNN` and `concat_fun` from
deepctr_torch.layers and `combined_dnn_input` from deepctr_torch.inputs; the shims have no InnerProductLayer or
OutterProductLayer, and a `DNN` and a `combined_dnn_input` that raise, and deepctr-torch itself is not part of the reference
tree.  So BEFORE the import this script assigns stand-ins of its own to the shim modules: a DNN of Linear layers N(0, init_std)
with relu between them (no dropout, no batch-norm: what main.py configures), deepctr's combined_dnn_input, and
InnerProductLayer and OutterProductLayer written from deepctr-torch 0.2.9's definition, with deepctr's parameter name
(`kernel`), shapes and xavier-uniform initialisation.

What the fixtures pin, and what they do not.  They pin the reference's WIRING: what goes into the two product layers (the
embeddings of ALL sparse fields, the domain column included), the order of the DNN input (the flattened embeddings, the inner
products, the outer products, the dense values), that there is no linear model, `dnn_linear`, `out`, the state_dict key names
and their order, and which parameters PNN regularises itself: the DNN's weights and dnn_linear.weight with l2_reg_dnn
(`reg_loss` over the entries PNN.__init__ appended, `n_own_reg` how many those are).  The layers' ARITHMETIC comes from the
stand-ins below, not from deepctr's code: the fixtures hold the product code and tests/pnn_reference.py to that definition as
written here.

Cases (D = 4; columns: the domain column, three sparse fields, one dense field, so F = 4, P = 6; B = 24; flag "x";
dnn_hidden_units (16, 8); l2_reg_dnn = 1e-3):  inner (use_inner), mat, vec, num (use_outter with that kernel), both (use_inner and
use_outter with 'mat').  Embeddings and the head's parameters are overwritten with values of a visible size (embeddings N(0, 1),
the kernel N(0, 1) D^-1/2, weights N(0, 1) n_in^-1/2, biases 0.3 N(0, 1)): at the default init_std = 1e-4 every gradient rounds
away.
Recorded per case (arrays only; fp32 unless stated):

  X [B, columns], labels [B]                 the input matrix in feature_index order, the labels
  use_inner, use_outter, kernel_type         the case's configuration;  l2_reg_dnn  its regularisation factor
  keys, shapes                               state_dict() keys of the head's entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  emb [B,F,D], dense [B,1]                   the looked-up embeddings in field order, the dense values
  y_pred [B,1], loss                         the probabilities; the summed BCE
  reg_loss [1], n_own_reg                    get_regularization_loss() over the entries PNN.__init__ itself appended, and how
                                             many those are (2: the DNN's weights, dnn_linear.weight)
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

import deepctr_torch.inputs as shim_inputs  # noqa: E402  (shim)
import deepctr_torch.layers as shim_layers  # noqa: E402  (shim)
from deepctr_torch.inputs import DenseFeat, SparseFeat  # noqa: E402  (shim)

D, B, NUM_DOMAINS, L2_REG_DNN = 4, 24, 3, 1e-3
HEAD_PREFIXES = ("out.", "innerproduct.", "outterproduct.", "dnn.", "dnn_linear.")
CASES = {"inner": (True, False, "mat"), "mat": (False, True, "mat"), "vec": (False, True, "vec"), "num": (False, True, "num"),
         "both": (True, True, "mat")}


class PlainDNN(nn.Module):
    """deepctr's DNN as main.py configures it: Linear layers N(0, init_std), relu after each, no dropout, no batch-norm."""

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


def _gathers(embed_list):
    """deepctr's p, q: the pairs' first and second pieces, i < j in the order of its double loop, each [B, P, D]."""
    row, col = [], []
    num_inputs = len(embed_list)
    for i in range(num_inputs - 1):
        for j in range(i + 1, num_inputs):
            row.append(i)
            col.append(j)
    return torch.cat([embed_list[idx] for idx in row], dim=1), torch.cat([embed_list[idx] for idx in col], dim=1)


class StandInInner(nn.Module):
    """The inner product layer as deepctr-torch 0.2.9 defines it (no parameters)."""

    def __init__(self, reduce_sum=True, device='cpu'):
        super().__init__()
        self.reduce_sum = reduce_sum

    def forward(self, inputs):
        p, q = _gathers(inputs)
        inner_product = p * q
        if self.reduce_sum:
            inner_product = torch.sum(inner_product, dim=2, keepdim=True)
        return inner_product


class StandInOuter(nn.Module):
    """The outer product layer as deepctr-torch 0.2.9 defines it (parameter `kernel`, xavier-uniform)."""

    def __init__(self, field_size, embedding_size, kernel_type='mat', seed=1024, device='cpu'):
        super().__init__()
        self.kernel_type = kernel_type
        num_pairs = int(field_size * (field_size - 1) / 2)
        if self.kernel_type == 'mat':
            self.kernel = nn.Parameter(torch.Tensor(embedding_size, num_pairs, embedding_size))
        elif self.kernel_type == 'vec':
            self.kernel = nn.Parameter(torch.Tensor(num_pairs, embedding_size))
        elif self.kernel_type == 'num':
            self.kernel = nn.Parameter(torch.Tensor(num_pairs, 1))
        nn.init.xavier_uniform_(self.kernel)

    def forward(self, inputs):
        p, q = _gathers(inputs)
        if self.kernel_type == 'mat':
            p = p.unsqueeze(dim=1)
            kp = torch.sum(torch.mul(torch.transpose(torch.sum(torch.mul(p, self.kernel), dim=-1), 2, 1), q), dim=-1)
        else:
            k = torch.unsqueeze(self.kernel, 0)
            kp = torch.sum(p * q * k, dim=-1)
        return kp


def combined_dnn_input(sparse_embedding_list, dense_value_list):
    """deepctr's: the pieces side by side, flattened, then the dense values."""
    parts = []
    if len(sparse_embedding_list) > 0:
        parts.append(torch.flatten(torch.cat(sparse_embedding_list, dim=-1), start_dim=1))
    if len(dense_value_list) > 0:
        parts.append(torch.flatten(torch.cat(dense_value_list, dim=-1), start_dim=1))
    if not parts:
        raise NotImplementedError
    return shim_layers.concat_fun(parts)


shim_layers.InnerProductLayer = StandInInner
shim_layers.OutterProductLayer = StandInOuter
shim_layers.DNN = PlainDNN
shim_inputs.combined_dnn_input = combined_dnn_input      # (the shim's raises: off the SATrans path)

import models.pnn as pnn  # noqa: E402  (the reference)


def run_case(name, outdir):
    use_inner, use_outter, kernel_type = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    vocab = {"dom": NUM_DOMAINS + 1, "f0": 7, "f1": 5, "f2": 9}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    torch.manual_seed(11)
    model = pnn.PNN(cols, dnn_hidden_units=(16, 8), l2_reg_dnn=L2_REG_DNN, init_std=0.0001, use_inner=use_inner,
                    use_outter=use_outter, kernel_type=kernel_type, device='cpu', flag="x", domain_column="dom",
                    num_domains=NUM_DOMAINS, meta_dnn_hidden_units=(D, 8, D))
    n_base = 2      # BaseModel's own entries: the embeddings, the (empty) linear model
    own = model.regularization_weight[n_base:]
    X = np.zeros((B, len(cols)), dtype=np.float32)
    for name_, (lo, hi) in model.feature_index.items():
        X[:, lo] = rng.randn(B) if name_ == "price" else rng.randint(0, vocab[name_], B)
    labels = (rng.rand(B) > 0.5).astype(np.float32)
    keys = [k for k in model.state_dict() if k.startswith(HEAD_PREFIXES)]
    params = dict(model.named_parameters())
    with torch.no_grad():
        for emb in model.embedding_dict.values():
            emb.weight.copy_(torch.from_numpy(rng.randn(*emb.weight.shape).astype(np.float32)))
        for k in keys:
            p = params[k]
            if k == "outterproduct.kernel":
                v = rng.randn(*p.shape) * D ** -0.5
            elif k.endswith("weight"):
                v = rng.randn(*p.shape) * p.shape[1] ** -0.5
            else:
                v = 0.3 * rng.randn(*p.shape)
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    out = dict(X=X, labels=labels, use_inner=np.array(use_inner), use_outter=np.array(use_outter), kernel_type=np.array(kernel_type),
               l2_reg_dnn=np.array(L2_REG_DNN), keys=np.array(keys), shapes=np.array([str(tuple(sd[k].shape)) for k in keys]),
               n_own_reg=np.array(len(own)))
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
    Xt, y = torch.from_numpy(X), torch.from_numpy(labels)
    model.train()
    y_pred = model(Xt)
    loss = F.binary_cross_entropy(y_pred.squeeze(1), y, reduction='sum')
    loss.backward()
    every = model.regularization_weight
    model.regularization_weight = own      # the entries PNN.__init__ appended
    out["reg_loss"] = model.get_regularization_loss().detach().numpy().copy()
    model.regularization_weight = every
    out["emb"] = torch.cat(kept["sparse"], dim=1).detach().numpy().copy()
    out["grad/emb"] = torch.cat([e.grad for e in kept["sparse"]], dim=1).numpy().copy()
    out["dense"] = torch.cat(kept["dense"], dim=-1).detach().numpy().copy()
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = loss.detach().numpy().copy()
    for k in keys:
        out[f"grad/{k}"] = params[k].grad.numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB, own regularisation entries {len(own)}, "
          f"reg_loss {float(out['reg_loss'][0]):.4g}")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "pnn")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
