"""Generate tests/golden/fibinet/*.npz by running the REFERENCE's own FiBiNET.forward (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_fibinet_golden.py          # writes tests/golden/fibinet/*.npz

The reference (read-only, never copied) is imported exactly as tools/gen_dcn_golden.py imports it, with the stand-in packages of
oracle/shims/ on sys.path.  models/fibinet.py takes `SENETLayer`, `BilinearInteraction` and `DNN` from deepctr_torch.layers and
`combined_dnn_input` from deepctr_torch.inputs; the shims have no SENETLayer or BilinearInteraction, and a `DNN` and a
`combined_dnn_input` that raise, and deepctr-torch itself is not part of the reference tree.  So BEFORE the import this script
assigns stand-ins of its own to the shim modules: a DNN of Linear layers N(0, init_std) with relu between them (no dropout, no
batch-norm: what main.py configures), deepctr's combined_dnn_input, and SENETLayer and BilinearInteraction written from
deepctr-torch 0.2.9's definition, with deepctr's parameter names (`excitation.{0,2}.weight`, `bilinear.weight` /
`bilinear.{i}.weight`) and torch's default Linear initialisation.

What the fixtures pin, and what they do not.  They pin the reference's WIRING: what goes into the SENet layer and the bilinear
interaction (the embeddings of ALL sparse fields, the domain column included), that the SAME Bilinear module runs on the SENet
output and on the raw embeddings, the order of the DNN input (SENet block, raw block, dense values), `dnn_linear`, `out`, the
state_dict key names and their order, and which parameters FiBiNET regularises: NONE of its own - fibinet.py never calls
add_regularization_weight, so `reg_loss` over the entries FiBiNET.__init__ appended is zero and `n_own_reg` records that it
appended no entry.  The layers' ARITHMETIC comes from the stand-ins below, not from deepctr's code: the fixtures hold the
product code and tests/fibinet_reference.py to that definition as written here.

Cases (D = 4; columns: the domain column, three sparse fields, one dense field, so F = 4, P = 6, DNN input 49 wide; B = 24; flag
"x"; reduction_ratio 3, so R = 1; dnn_hidden_units (16, 8)):  interaction, each, all - the three bilinear types.
Embeddings (also the linear model's) and the head's parameters are overwritten with values of a visible size (embeddings
N(0, 1), weights N(0, 1) n_in^-1/2 - the excitation's |N(0, 1)| n_in^-1/2 so that its relus stay open - biases 0.3 N(0, 1)):
at the default init_std = 1e-4 every gradient rounds away.
Recorded per case (arrays only; fp32 unless stated):

  X [B, columns], labels [B]                 the input matrix in feature_index order, the labels
  bilinear_type                              the type's name
  keys, shapes                               state_dict() keys of the head's entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  emb [B,F,D], dense [B,1], linear_logit [B,1]
                                             the looked-up embeddings in field order, the dense values, linear_model's output
  y_pred [B,1], loss                         the probabilities; the summed BCE
  reg_loss [1], n_own_reg                    get_regularization_loss() over the entries FiBiNET.__init__ itself appended, and
                                             how many those are (0)
  grad/<key>, grad/emb                       the loss's gradients: every recorded parameter (an unused 'each' weight: zeros,
                                             where the reference leaves None), and the looked-up embeddings
"""
from __future__ import annotations

import itertools
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

D, B, NUM_DOMAINS = 4, 24, 3
HEAD_PREFIXES = ("out.", "SE.", "Bilinear.", "dnn.", "dnn_linear.")
CASES = ("interaction", "each", "all")


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


class StandInSENET(nn.Module):
    """The SENET layer as deepctr-torch 0.2.9 defines it (parameters `excitation.0.weight`, `excitation.2.weight`)."""

    def __init__(self, filed_size, reduction_ratio=3, seed=1024, device='cpu'):
        super().__init__()
        self.seed = seed
        self.filed_size = filed_size
        self.reduction_size = max(1, filed_size // reduction_ratio)
        self.excitation = nn.Sequential(nn.Linear(self.filed_size, self.reduction_size, bias=False), nn.ReLU(),
                                        nn.Linear(self.reduction_size, self.filed_size, bias=False), nn.ReLU())

    def forward(self, inputs):
        if len(inputs.shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(inputs.shape)))
        Z = torch.mean(inputs, dim=-1, out=None)
        A = self.excitation(Z)
        return torch.mul(inputs, torch.unsqueeze(A, dim=2))


class StandInBilinear(nn.Module):
    """The bilinear interaction as deepctr-torch 0.2.9 defines it (parameters `bilinear.weight` or `bilinear.{i}.weight`)."""

    def __init__(self, filed_size, embedding_size, bilinear_type="interaction", seed=1024, device='cpu'):
        super().__init__()
        self.bilinear_type = bilinear_type
        self.seed = seed
        self.bilinear = nn.ModuleList()
        if self.bilinear_type == "all":
            self.bilinear = nn.Linear(embedding_size, embedding_size, bias=False)
        elif self.bilinear_type == "each":
            for _ in range(filed_size):
                self.bilinear.append(nn.Linear(embedding_size, embedding_size, bias=False))
        elif self.bilinear_type == "interaction":
            for _, _ in itertools.combinations(range(filed_size), 2):
                self.bilinear.append(nn.Linear(embedding_size, embedding_size, bias=False))
        else:
            raise NotImplementedError

    def forward(self, inputs):
        if len(inputs.shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(inputs.shape)))
        inputs = torch.split(inputs, 1, dim=1)
        if self.bilinear_type == "all":
            p = [torch.mul(self.bilinear(v_i), v_j) for v_i, v_j in itertools.combinations(inputs, 2)]
        elif self.bilinear_type == "each":
            p = [torch.mul(self.bilinear[i](inputs[i]), inputs[j]) for i, j in itertools.combinations(range(len(inputs)), 2)]
        elif self.bilinear_type == "interaction":
            p = [torch.mul(bilinear(v[0]), v[1]) for v, bilinear in zip(itertools.combinations(inputs, 2), self.bilinear)]
        else:
            raise NotImplementedError
        return torch.cat(p, dim=1)


def combined_dnn_input(sparse_embedding_list, dense_value_list):
    """deepctr's: the [B, 1, D] pieces side by side, flattened, then the dense values."""
    parts = []
    if len(sparse_embedding_list) > 0:
        parts.append(torch.flatten(torch.cat(sparse_embedding_list, dim=-1), start_dim=1))
    if len(dense_value_list) > 0:
        parts.append(torch.flatten(torch.cat(dense_value_list, dim=-1), start_dim=1))
    if not parts:
        raise NotImplementedError
    return shim_layers.concat_fun(parts)


shim_layers.SENETLayer = StandInSENET
shim_layers.BilinearInteraction = StandInBilinear
shim_layers.DNN = PlainDNN
shim_inputs.combined_dnn_input = combined_dnn_input      # (the shim's raises: off the SATrans path)

import models.fibinet as fibinet  # noqa: E402  (the reference)


def run_case(name, outdir):
    rng = np.random.RandomState(sum(map(ord, name)))
    vocab = {"dom": NUM_DOMAINS + 1, "f0": 7, "f1": 5, "f2": 9}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    torch.manual_seed(11)
    model = fibinet.FiBiNET(cols, cols, bilinear_type=name, reduction_ratio=3, dnn_hidden_units=(16, 8), init_std=0.0001,
                            device='cpu', flag="x", domain_column="dom", num_domains=NUM_DOMAINS, meta_dnn_hidden_units=(D, 8, D))
    n_base = 2      # BaseModel's own entries: the embeddings, the linear model
    n_own = len(model.regularization_weight) - n_base
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
            if k.startswith("SE."):
                v = np.abs(rng.randn(*p.shape)) * p.shape[1] ** -0.5
            elif k.endswith("weight"):
                v = rng.randn(*p.shape) * p.shape[1] ** -0.5
            else:
                v = 0.3 * rng.randn(*p.shape)
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    out = dict(X=X, labels=labels, bilinear_type=np.array(name), keys=np.array(keys),
               shapes=np.array([str(tuple(sd[k].shape)) for k in keys]), n_own_reg=np.array(n_own))
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
    every = model.regularization_weight
    model.regularization_weight = every[n_base:]      # the entries FiBiNET.__init__ appended
    out["reg_loss"] = model.get_regularization_loss().detach().numpy().copy()
    model.regularization_weight = every
    out["emb"] = torch.cat(kept["sparse"], dim=1).detach().numpy().copy()
    out["grad/emb"] = torch.cat([e.grad for e in kept["sparse"]], dim=1).numpy().copy()
    out["dense"] = torch.cat(kept["dense"], dim=-1).detach().numpy().copy()
    out["linear_logit"] = kept["linear_logit"].numpy().copy()
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = loss.detach().numpy().copy()
    for k in keys:
        grad = params[k].grad
        out[f"grad/{k}"] = (torch.zeros_like(params[k]) if grad is None else grad).numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB, own regularisation entries {n_own}")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "fibinet")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
