"""Generate tests/golden/fm/*.npz by running the REFERENCE's own DeepFM.forward, NFM.forward and AFM.forward (CPU; build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_fm_golden.py          # writes tests/golden/fm/*.npz

The reference (read-only, never copied) is imported exactly as tools/gen_pnn_golden.py imports it, with the stand-in packages of
oracle/shims/ on sys.path.  models/deepfm.py, nfm.py and afm.py take `FM`, `BiInteractionPooling`, `AFMLayer`, `DNN` and
`concat_fun` from deepctr_torch.layers and `combined_dnn_input` from deepctr_torch.inputs; the shims have no FM,
BiInteractionPooling or AFMLayer, and a `DNN` and a `combined_dnn_input` that raise, and deepctr-torch itself is not part of the
reference tree.  So BEFORE the import this script assigns stand-ins to the shim modules: the plain DNN and the
combined_dnn_input of tools/gen_pnn_golden.py (Linear layers N(0, init_std) with relu between them; deepctr's concatenation),
and FM, BiInteractionPooling and AFMLayer written here from deepctr-torch 0.2.9's definitions, with deepctr's parameter names
(attention_W, attention_b, projection_h, projection_p), shapes, creation order and initialisation.

What the fixtures pin, and what they do not.  They pin the reference's WIRING: what goes into the interaction layer (the
embeddings of ALL sparse fields, the domain column included, as a list of pieces for AFM and as a tensor for FM and the
pooling), what the DNN reads (DeepFM: the flattened embeddings then the dense values; NFM: the pooled row then the dense values),
that the linear model's logit is added, `dnn_linear`, `out`, the state_dict key names and their order, and which parameters each
model regularises itself (`reg_loss` over the entries its __init__ appended, `n_own_reg` how many those are).  The layers'
ARITHMETIC comes from the stand-ins below, not from deepctr's code: the fixtures hold the product code and
tests/fm_reference.py to that definition as written here.

Cases (D = 4; columns: the domain column, three sparse fields, one dense field, so F = 4, P = 6; B = 24; flag "x"; l2_reg_dnn =
l2_reg_att = 1e-3):  deepfm (dnn_hidden_units (16, 8)), deepfm_nodnn (dnn_hidden_units ()), nfm ((16, 8)), afm
(attention_factor 3), afm_wide (attention_factor 5, wider than D).  Embeddings, the linear model and the head's parameters are
overwritten with values of a visible size (embeddings N(0, 1), the linear model 0.3 N(0, 1), matrices N(0, 1) n_in^-1/2,
biases 0.3 N(0, 1)): at the default init_std = 1e-4 every gradient rounds away.
Recorded per case (arrays only; fp32 unless stated):

  X [B, columns], labels [B]                 the input matrix in feature_index order, the labels
  kind, l2                                   "deepfm" / "nfm" / "afm"; the case's own regularisation factor
  keys, shapes                               state_dict() keys of the head's entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  emb [B,F,D], dense [B,1]                   the looked-up embeddings in field order, the dense values
  linear_logit [B,1]                         what the reference's linear_model(X) returned
  y_pred [B,1], loss                         the probabilities; the summed BCE
  reg_loss [1], n_own_reg                    get_regularization_loss() over the entries the model's __init__ itself appended,
                                             and how many those are (deepfm, nfm: 2; deepfm_nodnn: 0; afm: 1)
  grad/<key>, grad/emb                       the loss's gradients: every recorded parameter, and the looked-up embeddings
  normalized_att_score [B,P,1]               AFM only: the layer's attribute after the forward
"""
from __future__ import annotations

import itertools
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

D, B, NUM_DOMAINS, L2 = 4, 24, 3, 1e-3
HEAD_PREFIXES = ("out.", "fm.", "bi_pooling.", "dnn.", "dnn_linear.")
CASES = {"deepfm": ("deepfm", dict(dnn_hidden_units=(16, 8))), "deepfm_nodnn": ("deepfm", dict(dnn_hidden_units=())),
         "nfm": ("nfm", dict(dnn_hidden_units=(16, 8))), "afm": ("afm", dict(attention_factor=3)),
         "afm_wide": ("afm", dict(attention_factor=5))}


class StandInFM(nn.Module):
    """FM as deepctr-torch 0.2.9 defines it (no parameters)."""

    def forward(self, inputs):
        fm_input = inputs
        square_of_sum = torch.pow(torch.sum(fm_input, dim=1, keepdim=True), 2)
        sum_of_square = torch.sum(fm_input * fm_input, dim=1, keepdim=True)
        cross_term = square_of_sum - sum_of_square
        return 0.5 * torch.sum(cross_term, dim=2, keepdim=False)


class StandInBiPooling(nn.Module):
    """BiInteractionPooling as deepctr-torch 0.2.9 defines it (no parameters)."""

    def forward(self, inputs):
        concated_embeds_value = inputs
        square_of_sum = torch.pow(torch.sum(concated_embeds_value, dim=1, keepdim=True), 2)
        sum_of_square = torch.sum(concated_embeds_value * concated_embeds_value, dim=1, keepdim=True)
        return 0.5 * (square_of_sum - sum_of_square)


class StandInAFM(nn.Module):
    """AFMLayer as deepctr-torch 0.2.9 defines it."""

    def __init__(self, in_features, attention_factor=4, l2_reg_w=0, dropout_rate=0, seed=1024, device='cpu'):
        super().__init__()
        self.attention_factor, self.l2_reg_w, self.dropout_rate, self.seed = attention_factor, l2_reg_w, dropout_rate, seed
        embedding_size = in_features
        self.attention_W = nn.Parameter(torch.Tensor(embedding_size, self.attention_factor))
        self.attention_b = nn.Parameter(torch.Tensor(self.attention_factor))
        self.projection_h = nn.Parameter(torch.Tensor(self.attention_factor, 1))
        self.projection_p = nn.Parameter(torch.Tensor(embedding_size, 1))
        for tensor in [self.attention_W, self.projection_h, self.projection_p]:
            nn.init.xavier_normal_(tensor, )
        for tensor in [self.attention_b]:
            nn.init.zeros_(tensor, )
        self.dropout = nn.Dropout(dropout_rate)
        self.to(device)

    def forward(self, inputs):
        embeds_vec_list = inputs
        row, col = [], []
        for r, c in itertools.combinations(embeds_vec_list, 2):
            row.append(r)
            col.append(c)
        p = torch.cat(row, dim=1)
        q = torch.cat(col, dim=1)
        bi_interaction = p * q
        attention_temp = F.relu(torch.tensordot(bi_interaction, self.attention_W, dims=([-1], [0])) + self.attention_b)
        self.normalized_att_score = F.softmax(torch.tensordot(attention_temp, self.projection_h, dims=([-1], [0])), dim=1)
        attention_output = torch.sum(self.normalized_att_score * bi_interaction, dim=1)
        attention_output = self.dropout(attention_output)
        return torch.tensordot(attention_output, self.projection_p, dims=([-1], [0]))


shim_layers.FM = StandInFM
shim_layers.BiInteractionPooling = StandInBiPooling
shim_layers.AFMLayer = StandInAFM

import models.afm as afm  # noqa: E402  (the reference)
import models.deepfm as deepfm  # noqa: E402
import models.nfm as nfm  # noqa: E402


def run_case(name, outdir):
    kind, kw = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    vocab = {"dom": NUM_DOMAINS + 1, "f0": 7, "f1": 5, "f2": 9}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    common = dict(init_std=0.0001, device='cpu', flag="x", domain_column="dom", num_domains=NUM_DOMAINS,
                  meta_dnn_hidden_units=(D, 8, D))
    torch.manual_seed(11)
    if kind == "deepfm":
        model = deepfm.DeepFM(cols, cols, l2_reg_dnn=L2, **kw, **common)
    elif kind == "nfm":
        model = nfm.NFM(cols, cols, l2_reg_dnn=L2, **kw, **common)
    else:
        model = afm.AFM(cols, cols, l2_reg_att=L2, **kw, **common)
    n_base = 2      # BaseModel's own entries: the embeddings, the linear model
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
        for p in model.linear_model.parameters():
            p.copy_(torch.from_numpy((0.3 * rng.randn(*p.shape)).astype(np.float32)))
        for k in keys:
            p = params[k]
            v = rng.randn(*p.shape) * p.shape[-1 if k.startswith("dnn") else 0] ** -0.5 if p.dim() == 2 else 0.3 * rng.randn(*p.shape)
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    out = dict(X=X, labels=labels, kind=np.array(kind), l2=np.array(L2), keys=np.array(keys),
               shapes=np.array([str(tuple(sd[k].shape)) for k in keys]), n_own_reg=np.array(len(own)))
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
    model.linear_model.register_forward_hook(lambda mod, args, res: kept.__setitem__("lin", res.detach().clone()))
    Xt, y = torch.from_numpy(X), torch.from_numpy(labels)
    model.train()
    y_pred = model(Xt)
    loss = F.binary_cross_entropy(y_pred.squeeze(1), y, reduction='sum')
    loss.backward()
    every = model.regularization_weight
    model.regularization_weight = own      # the entries the model's own __init__ appended
    out["reg_loss"] = model.get_regularization_loss().detach().numpy().copy()
    model.regularization_weight = every
    out["emb"] = torch.cat(kept["sparse"], dim=1).detach().numpy().copy()
    out["grad/emb"] = torch.cat([e.grad for e in kept["sparse"]], dim=1).numpy().copy()
    out["dense"] = torch.cat(kept["dense"], dim=-1).detach().numpy().copy()
    out["linear_logit"] = kept["lin"].numpy().copy()
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = loss.detach().numpy().copy()
    if kind == "afm":
        out["normalized_att_score"] = model.fm.normalized_att_score.detach().numpy().copy()
    for k in keys:
        out[f"grad/{k}"] = params[k].grad.numpy().copy()
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB, keys {keys}, own regularisation entries {len(own)}, "
          f"reg_loss {float(out['reg_loss'][0]):.4g}")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "fm")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
