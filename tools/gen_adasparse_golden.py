"""Generate tests/golden/adasparse/*.npz by running the REFERENCE's own AdaSparse.forward (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_adasparse_golden.py          # writes tests/golden/adasparse/*.npz

The reference (read-only, never copied) is imported exactly as oracle/gen_golden.py imports it, with the stand-in packages of
oracle/shims/ on sys.path.  models/adasparse.py imports `deepctr_torch.layers.activation`, a submodule the shims do not have:
this script registers a stand-in module under that name in sys.modules, whose `activation_layer` is the shim's own.  After the
import it replaces `combined_dnn_input` of models.adasparse with a flatten-and-concatenate that keeps the `dnn_input` tensor,
so that its gradient is recorded.

Cases (D = 4 = domain_emb_dim; columns: the domain column, two sparse fields, one dense field; B = 24):
  plain      widths (16, 8), the reference's constants alpha = 1, beta = 2, epsilon = 0.25
  one_layer  widths (8,)
  scaled     widths (16, 8), alpha = 0.5, beta = 1.5, epsilon = 0.4
Embeddings are N(0, 1).  The head's parameters are overwritten with values of a visible size (weights N(0, 1) n_in^-1/2,
biases 0.3 N(0, 1)); the pruners' weights are then doubled and their biases shifted by -1: at the default initialisation
nothing is ever pruned.  Recorded per case (arrays only; fp32 unless stated):

  X [B, columns], labels [B]                 the input matrix in feature_index order (column 0 of `dom_ids` below), the labels
  dom_ids [B], dom_cols [2], consts [3]      the domain ids; the columns [lo, hi) of dnn_input that hold the domain embedding;
                                             alpha, beta, epsilon
  keys, shapes                               state_dict() keys of the head's entries and their shapes (in order)
  param/<key>                                the values those entries are set to
  dnn_input [B,C], domain_emb [B,D]          what the pruned DNN receives
  z/<l> [B, n_l]                             the output of pruners.<l> (a forward hook)
  y_pred [B,1], loss                         the probabilities; the summed BCE
  grad/<key>, grad/dnn_input, grad/domain_table [rows, D]
                                             its gradients: every recorded parameter, `dnn_input`, and the domain column's
                                             embedding table (both paths: through dnn_input and through domain_emb)
"""
from __future__ import annotations

import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from oracle import gen_golden as G  # noqa: E402,F401  (puts the shims and the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import deepctr_torch.layers as shim_layers  # noqa: E402  (shim)
from deepctr_torch.inputs import DenseFeat, SparseFeat  # noqa: E402  (shim)

_activation = types.ModuleType("deepctr_torch.layers.activation")
_activation.activation_layer = shim_layers.activation_layer
sys.modules["deepctr_torch.layers.activation"] = _activation

import models.adasparse as adasparse  # noqa: E402  (the reference)

D, B, NUM_DOMAINS = 4, 24, 3
HEAD_PREFIXES = ("out.", "dnn.", "dnn_linear.")
CASES = {
    "plain": dict(widths=(16, 8), consts=(1, 2.0, 0.25)),
    "one_layer": dict(widths=(8,), consts=(1, 2.0, 0.25)),
    "scaled": dict(widths=(16, 8), consts=(0.5, 1.5, 0.4)),
}
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


adasparse.combined_dnn_input = combined_dnn_input


def run_case(name, outdir):
    cfg = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    vocab = {"dom": NUM_DOMAINS, "f0": 7, "f1": 5}
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    torch.manual_seed(11)
    model = adasparse.AdaSparse(cols, cols, dnn_hidden_units=cfg["widths"], init_std=0.0001, device='cpu', flag="x",
                                domain_column="dom", num_domains=NUM_DOMAINS, domain_emb_dim=D)
    model.dnn.alpha, model.dnn.beta, model.dnn.epsilon = cfg["consts"]
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
            v = rng.randn(*p.shape) * p.shape[1] ** -0.5 if k.endswith("weight") else 0.3 * rng.randn(*p.shape)
            if k.startswith("dnn.pruners."):
                v = 2.0 * v if k.endswith("weight") else v - 1.0
            p.copy_(torch.from_numpy(np.asarray(v, dtype=np.float32)))
    sd = model.state_dict()
    dom_col = model.feature_index["dom"][0]
    out = dict(X=X, labels=labels, dom_ids=X[:, dom_col].astype(np.int64), consts=np.asarray(cfg["consts"], dtype=np.float32),
               keys=np.array(keys), shapes=np.array([str(tuple(sd[k].shape)) for k in keys]))
    for k in keys:
        out[f"param/{k}"] = sd[k].numpy().copy()
    zs = {}
    hooks = [m.register_forward_hook(lambda mod, inp, res, l=l: zs.__setitem__(l, res.detach().numpy().copy()))
             for l, m in enumerate(model.dnn.pruners)]
    table = model.embedding_dict["dom"]
    Xt, y = torch.from_numpy(X), torch.from_numpy(labels)
    model.train()
    y_pred = model(Xt)
    loss = F.binary_cross_entropy(y_pred.squeeze(1), y, reduction='sum')
    loss.backward()
    for h in hooks:
        h.remove()
    dnn_input = KEPT["dnn_input"]
    # the domain embedding as the DNN received it: the table's rows of the ids (what forward() squeezes out of the lookup)
    domain_emb = table.weight.detach()[torch.from_numpy(out["dom_ids"])]
    names = [c.name for c in cols if isinstance(c, SparseFeat)]
    lo = names.index("dom") * D
    assert torch.equal(dnn_input.detach()[:, lo:lo + D], domain_emb)
    out["dom_cols"] = np.array([lo, lo + D])
    out["dnn_input"] = dnn_input.detach().numpy().copy()
    out["domain_emb"] = domain_emb.numpy().copy()
    for l, z in zs.items():
        out[f"z/{l}"] = z
    out["y_pred"] = y_pred.detach().numpy().copy()
    out["loss"] = loss.detach().numpy().copy()
    out["grad/dnn_input"] = dnn_input.grad.numpy().copy()
    out["grad/domain_table"] = table.weight.grad.numpy().copy()
    for k in keys:
        out[f"grad/{k}"] = params[k].grad.numpy().copy()
    thr = np.log(cfg["consts"][2] / (cfg["consts"][1] - cfg["consts"][2])) / cfg["consts"][0]
    shares = [float((z <= thr).mean()) for z in zs.values()]
    margin = min(float(np.abs(z - thr).min()) for z in zs.values())
    path = os.path.join(outdir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB; pruned shares {shares}, "
          f"smallest |z - threshold| {margin:.3f} (threshold {thr:.3f})")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "adasparse")   # (a directory of their own: tests/helpers.py lists golden/*.npz)
    os.makedirs(outdir, exist_ok=True)
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, outdir)
