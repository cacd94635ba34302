"""Generate tests/golden/autoint/*.npz by running the REFERENCE's own AutoInt.forward (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_autoint_golden.py          # writes tests/golden/autoint/*.npz

The reference (read-only, never copied) is imported exactly as tools/gen_fm_golden.py imports it, with the stand-in packages of
oracle/shims/ on sys.path.  models/autoint.py takes `DNN`, `concat_fun` and `InteractingLayer` from deepctr_torch.layers and
`combined_dnn_input` from deepctr_torch.inputs; the shims have no InteractingLayer, and a `DNN` and a `combined_dnn_input` that
raise, and deepctr-torch itself is not part of the reference tree.  So BEFORE the import this script assigns stand-ins to the
shim modules: the plain DNN and the combined_dnn_input of tools/gen_pnn_golden.py (Linear layers N(0, init_std) with relu between
them; deepctr's concatenation), and InteractingLayer written here from deepctr-torch 0.2.9's definition, with deepctr's
parameter names (W_Query, W_key, W_Value, W_Res), creation order and initialisation (every parameter N(0, 0.05)).

What the fixtures pin, and what they do not.  They pin the reference's WIRING: what enters the interacting stack (the embeddings
of ALL sparse fields, the domain column included), what the DNN reads (the flattened embeddings, then the dense values), the
concatenation order for dnn_linear (att_output, then deep_out), that dnn_linear has no bias and the linear model is NOT added
(`logit = 0`, autoint.py:89-90), `out`, the state_dict key names and their order.  The layer's ARITHMETIC comes from the stand-in
below, not from deepctr's code: the fixtures hold the product code and tests/autoint_reference.py to that definition as written
here.

D = 4 is outside the HIP kernels' shapes (D in {16, 32, 64}), so the fixtures are reproduced by the restatement
tests/autoint_reference.py on the CPU (tests/test_autoint_cpu.py::test_restatement_reproduces_every_fixture), as the fm and pnn
ones are; what ties the restatement to the kernels is tests/test_autoint_gpu.py (test_layer_matches_the_restatement and
test_head_matches_the_restatement, over the sweep of autoint_reference.SWEEP).

Cases (D = 4; columns: the domain column, three sparse fields, one dense field, so F = 4; B = 24; flag "x"):  autoint (3 layers,
2 heads, dnn_hidden_units (16, 8)), autoint_nodnn (dnn_hidden_units ()), autoint_nores (att_res=False, 1 layer, (16, 8)).
Embeddings and the head's parameters are overwritten with values of a visible size (embeddings N(0, 1), matrices N(0, 1)
n_in^-1/2, biases 0.3 N(0, 1)): at the default init_std = 1e-4 every gradient rounds away.
Recorded per case (arrays only; fp32 unless stated):

  X [B, columns], labels [B]                 the input matrix in feature_index order, the labels
  att_layer_num, att_head_num, att_res       the case's constructor arguments
  keys, shapes                               state_dict() keys of the head's entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  emb [B,F,D], dense [B,1]                   the looked-up embeddings in field order, the dense values
  y_pred [B,1], loss                         the probabilities; the summed BCE
  grad/<key>, grad/emb                       the loss's gradients: every recorded parameter, and the looked-up embeddings
  normalized_att_scores [H,B,F,F]            the last interacting layer's attribute after the forward
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_pnn_golden as PG  # noqa: E402,F401  (the shims and the reference on sys.path; its DNN and combined_dnn_input assigned)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import deepctr_torch.layers as shim_layers  # noqa: E402  (shim)
from deepctr_torch.inputs import DenseFeat, SparseFeat  # noqa: E402  (shim)

D, B, NUM_DOMAINS = 4, 24, 3
HEAD_PREFIXES = ("out.", "dnn.", "dnn_linear.", "int_layers.")
CASES = {"autoint": dict(att_layer_num=3, att_head_num=2, att_res=True, dnn_hidden_units=(16, 8)),
         "autoint_nodnn": dict(att_layer_num=3, att_head_num=2, att_res=True, dnn_hidden_units=()),
         "autoint_nores": dict(att_layer_num=1, att_head_num=2, att_res=False, dnn_hidden_units=(16, 8))}


class StandInInteractingLayer(nn.Module):
    """InteractingLayer as deepctr-torch 0.2.9 defines it."""

    def __init__(self, embedding_size, head_num=2, use_res=True, scaling=False, seed=1024, device='cpu'):
        super().__init__()
        if head_num <= 0:
            raise ValueError('head_num must be a int > 0')
        if embedding_size % head_num != 0:
            raise ValueError('embedding_size is not an integer multiple of head_num!')
        self.att_embedding_size = embedding_size // head_num
        self.head_num = head_num
        self.use_res = use_res
        self.scaling = scaling
        self.seed = seed
        self.W_Query = nn.Parameter(torch.Tensor(embedding_size, embedding_size))
        self.W_key = nn.Parameter(torch.Tensor(embedding_size, embedding_size))
        self.W_Value = nn.Parameter(torch.Tensor(embedding_size, embedding_size))
        if self.use_res:
            self.W_Res = nn.Parameter(torch.Tensor(embedding_size, embedding_size))
        for tensor in self.parameters():
            nn.init.normal_(tensor, mean=0.0, std=0.05)
        self.to(device)

    def forward(self, inputs):
        if len(inputs.shape) != 3:
            raise ValueError("Unexpected inputs dimensions %d, expect to be 3 dimensions" % (len(inputs.shape)))
        querys = torch.tensordot(inputs, self.W_Query, dims=([-1], [0]))
        keys = torch.tensordot(inputs, self.W_key, dims=([-1], [0]))
        values = torch.tensordot(inputs, self.W_Value, dims=([-1], [0]))
        querys = torch.stack(torch.split(querys, self.att_embedding_size, dim=2))
        keys = torch.stack(torch.split(keys, self.att_embedding_size, dim=2))
        values = torch.stack(torch.split(values, self.att_embedding_size, dim=2))
        inner_product = torch.einsum('bnik,bnjk->bnij', querys, keys)
        if self.scaling:
            inner_product /= self.att_embedding_size ** 0.5
        self.normalized_att_scores = F.softmax(inner_product, dim=-1)
        result = torch.matmul(self.normalized_att_scores, values)
        result = torch.cat(torch.split(result, 1, ), dim=-1)
        result = torch.squeeze(result, dim=0)
        if self.use_res:
            result += torch.tensordot(inputs, self.W_Res, dims=([-1], [0]))
        result = F.relu(result)
        return result


shim_layers.InteractingLayer = StandInInteractingLayer

import models.autoint as autoint  # noqa: E402  (the reference)


def run_case(name, outdir):
    kw = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    vocab = {"dom": NUM_DOMAINS + 1, "f0": 7, "f1": 5, "f2": 9}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    torch.manual_seed(11)
    model = autoint.AutoInt(cols, cols, init_std=0.0001, device='cpu', flag="x", domain_column="dom", num_domains=NUM_DOMAINS,
                            meta_dnn_hidden_units=(D, 8, D), **kw)
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
            v = rng.randn(*p.shape) * p.shape[-1 if k.startswith("dnn") else 0] ** -0.5 if p.dim() == 2 else 0.3 * rng.randn(*p.shape)
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    out = dict(X=X, labels=labels, keys=np.array(keys), shapes=np.array([str(tuple(sd[k].shape)) for k in keys]),
               att_layer_num=np.array(kw["att_layer_num"]), att_head_num=np.array(kw["att_head_num"]),
               att_res=np.array(kw["att_res"]))
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
    out["emb"] = torch.cat(kept["sparse"], dim=1).detach().numpy().copy()
    out["grad/emb"] = torch.cat([e.grad for e in kept["sparse"]], dim=1).numpy().copy()
    out["dense"] = torch.cat(kept["dense"], dim=-1).detach().numpy().copy()
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = loss.detach().numpy().copy()
    out["normalized_att_scores"] = model.int_layers[-1].normalized_att_scores.detach().numpy().copy()
    for k in keys:
        out[f"grad/{k}"] = params[k].grad.numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB, keys {keys}")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "autoint")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
