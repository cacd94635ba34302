"""Generate tests/golden/cin/*.npz by running the REFERENCE's own xDeepFM.forward (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_cin_golden.py          # writes tests/golden/cin/*.npz

The reference (read-only, never copied) is imported exactly as oracle/gen_golden.py imports it, with the stand-in packages of
oracle/shims/ on sys.path.  models/xdeepfm.py takes `DNN` and `CIN` from deepctr_torch.layers; the shims have no `CIN` and their
`DNN` raises (both are off the SATrans path), and deepctr-torch itself is not part of the reference tree.  So BEFORE the import
this script assigns two stand-ins of its own to deepctr_torch.layers: a DNN of Linear layers N(0, init_std) with relu between
them (no dropout, no batch-norm: what main.py configures), and a CIN written from deepctr-torch 0.2.9's definition - per layer
the outer product of the hidden block and the input along the fields, a Conv1d(H M, O, 1), relu, the split - with deepctr's
parameter names.  After the import it replaces `combined_dnn_input` of models.xdeepfm with the flatten-and-concatenate.

What the fixtures pin, and what they do not.  They pin the reference's WIRING: which tensor goes into the CIN (the looked-up
embeddings of ALL sparse fields, the domain column included, concatenated along dim 1), the three logits and their sum, `out`,
the state_dict key names and their order.  The CIN ARITHMETIC comes from the stand-in below, not from deepctr's code: the
fixtures hold the product code and tests/cin_reference.py to that definition as written here.

Cases (D = 4; columns: the domain column, three sparse fields, one dense field; B = 24; flag "x"):
  plain     cin_layer_size (8, 6), cin_split_half=True, dnn_hidden_units (16, 8)
  nosplit   cin_layer_size (6, 5), cin_split_half=False, dnn_hidden_units (16, 8)
  cin_only  cin_layer_size (8, 6), cin_split_half=True, dnn_hidden_units ()
Embeddings (also the linear model's) and the head's parameters are overwritten with values of a visible size (embeddings
N(0, 1), weights N(0, 1) n_in^-1/2, biases 0.3 N(0, 1)): at the default init_std = 1e-4 every gradient rounds away.  Recorded
per case (arrays only; fp32 unless stated):

  X [B, columns], labels [B]                 the input matrix in feature_index order, the labels
  split_half                                 0 / 1
  keys, shapes                               state_dict() keys of the head's entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  emb [B,F,D], dense [B,1], linear_logit [B,1]
                                             the looked-up embeddings in field order, the dense values, linear_model's output
  y_pred [B,1], loss                         the probabilities; the summed BCE
  grad/<key>, grad/emb                       its gradients: every recorded parameter, and the looked-up embeddings (both
                                             paths: through the CIN and through the DNN)
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
HEAD_PREFIXES = ("out.", "dnn.", "dnn_linear.", "cin.", "cin_linear.")
CASES = {
    "plain": dict(cin=(8, 6), split=True, dnn=(16, 8)),
    "nosplit": dict(cin=(6, 5), split=False, dnn=(16, 8)),
    "cin_only": dict(cin=(8, 6), split=True, dnn=()),
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


class StandInCIN(nn.Module):
    """The compressed interaction network as deepctr-torch 0.2.9 defines it (parameters `conv1ds.{i}.{weight,bias}`)."""

    def __init__(self, field_size, layer_size=(128, 128), activation='relu', split_half=True, l2_reg=1e-5, seed=1024, device='cpu'):
        super().__init__()
        assert activation == 'relu' and len(layer_size) > 0
        self.layer_size, self.split_half = tuple(layer_size), split_half
        self.field_nums = [field_size]
        self.conv1ds = nn.ModuleList()
        for i, size in enumerate(self.layer_size):
            self.conv1ds.append(nn.Conv1d(self.field_nums[-1] * self.field_nums[0], size, 1))
            if split_half and i != len(self.layer_size) - 1 and size % 2 > 0:
                raise ValueError("layer_size must be even number except for the last layer when split_half=True")
            self.field_nums.append(size // 2 if split_half else size)

    def forward(self, inputs):
        batch, dim = inputs.shape[0], inputs.shape[-1]
        hidden, final = inputs, []
        for i, size in enumerate(self.layer_size):
            x = torch.einsum('bhd,bmd->bhmd', hidden, inputs).reshape(batch, hidden.shape[1] * inputs.shape[1], dim)
            x = torch.relu(self.conv1ds[i](x))
            if self.split_half and i != len(self.layer_size) - 1:
                hidden, direct = torch.split(x, 2 * [size // 2], 1)
            else:
                hidden = direct = x
            final.append(direct)
        return torch.sum(torch.cat(final, dim=1), -1)


shim_layers.CIN = StandInCIN
shim_layers.DNN = PlainDNN

import models.xdeepfm as xdeepfm  # noqa: E402  (the reference)


def combined_dnn_input(sparse_embedding_list, dense_value_list):
    parts = []
    if sparse_embedding_list:
        parts.append(torch.flatten(torch.cat(sparse_embedding_list, dim=-1), start_dim=1))
    if dense_value_list:
        parts.append(torch.flatten(torch.cat(dense_value_list, dim=-1), start_dim=1))
    return torch.cat(parts, dim=-1)


xdeepfm.combined_dnn_input = combined_dnn_input


def run_case(name, outdir):
    cfg = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    vocab = {"dom": NUM_DOMAINS + 1, "f0": 7, "f1": 5, "f2": 9}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    torch.manual_seed(11)
    model = xdeepfm.xDeepFM(cols, cols, dnn_hidden_units=cfg["dnn"], cin_layer_size=cfg["cin"], cin_split_half=cfg["split"],
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
            v = rng.randn(*p.shape) * p.shape[1] ** -0.5 if k.endswith("weight") else 0.3 * rng.randn(*p.shape)
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    out = dict(X=X, labels=labels, split_half=np.array(int(cfg["split"])), keys=np.array(keys),
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
    model.linear_model.register_forward_hook(lambda mod, args, res: kept.__setitem__("linear_logit", res))
    Xt, y = torch.from_numpy(X), torch.from_numpy(labels)
    model.train()
    y_pred = model(Xt)
    loss = F.binary_cross_entropy(y_pred.squeeze(1), y, reduction='sum')
    loss.backward()
    out["emb"] = torch.cat(kept["sparse"], dim=1).detach().numpy().copy()
    out["grad/emb"] = torch.cat([e.grad for e in kept["sparse"]], dim=1).numpy().copy()
    out["dense"] = torch.cat(kept["dense"], dim=-1).detach().numpy().copy()
    out["linear_logit"] = kept["linear_logit"].detach().numpy().copy()
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = loss.detach().numpy().copy()
    for k in keys:
        out[f"grad/{k}"] = params[k].grad.numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "cin")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
