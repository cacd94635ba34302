"""Generate tests/golden/models/{wdl,deepfm,dcn_vector,dcn_matrix,mmoe,star}.npz and the ten of MORE_CASES by running the
REFERENCE's own model classes through their own compile() / fit() / predict() (CPU; build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_models_golden.py          # writes tests/golden/models/*.npz
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_models_golden.py esmm ple # only these cases

The reference (read-only, never copied) is imported exactly as oracle/gen_golden.py imports it, with the stand-in packages of
oracle/shims/ on sys.path.  deepctr's `DNN`, `combined_dnn_input`, `FM` and `CrossNet` are off the SATrans path and absent from the
shims; the stand-ins the earlier generators define (tools/gen_esmm_golden.py, gen_fm_golden.py, gen_dcn_golden.py,
gen_star_golden.py, gen_mmoe_golden.py) are imported from them and assigned to the reference's modules here.

Case shape: D = 16; columns dom (3 scenarios; ids start at 1 for mmoe and star, so that the offset is exercised), user (50), item
(37), cate (4), one dense `price`; hidden units (16, 8) (mmoe: experts (16, 8), gates (8,), towers (8,)); 96 rows as three batches
of 32, every batch holding at least two rows of every scenario (asserted); l2_reg_embedding = l2_reg_linear = 1e-5, Adam lr 1e-3,
shuffle=False, 2 epochs: six Adam steps.  wdl, deepfm and dcn are built without `domain_column`, which would only add the
reference's unused meta modules.  The ten further cases (MORE_CASES) keep that shape with small case-specific sizes: xdeepfm CIN
(8, 8); afm attention factor 4; autoint two interacting layers of two heads; pnn inner and 'mat' outer products; adasparse
domain_emb_dim = D over `dom` (ids from 0); sharedbottom and ple towers (8,), ple gates (8,), ids from 1; esmm two scenarios,
ids from 1, built without `flag` (its constructor has none).  Their layers come from the earlier generators too
(gen_cin_golden.py, gen_fm_golden.py, gen_autoint_golden.py, gen_fibinet_golden.py, gen_pnn_golden.py, gen_adasparse_golden.py).  All parameters are overwritten with values of a visible size.  Recorded per case (arrays only):

  x/<name>, y                      the model input by column, the labels
  keys                             the reference's state_dict() key list, in order
  signature                        the constructor's parameters as "name=repr(default)" ("name" without one), in order
  init/<key>                       the whole initial state, tables included
  pred0                            predict() from the initial state (eval mode)
  loss0, reg0                      the first batch's summed loss and get_regularization_loss() at the initial state (train mode)
  fit/loss, fit/pred               History['loss'] and predict() of the reference's own compile / fit / predict
  fit_perm/loss, fit_perm/pred     the same run from the same initial state with the rows inside each batch permuted (predict on
                                   the unpermuted x): the same mathematics in another summation order, the reference against itself
"""
from __future__ import annotations

import contextlib
import inspect
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import gen_golden as G  # noqa: E402,F401  (puts the shims and the reference on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import gen_dcn_golden as DG  # noqa: E402  (PlainDNN, StandInCrossNet; imports the reference's dcn)
import gen_fm_golden as FG  # noqa: E402  (StandInFM; imports the reference's deepfm)
import gen_star_golden as SG  # noqa: E402  (TowerDNN, combined_dnn_input; imports the reference's star)
import gen_esmm_golden as EG  # noqa: E402,F401  (imports the reference's wdl)
import gen_mmoe_golden as MG  # noqa: E402,F401  (imports the reference's mmoe)
import gen_cin_golden as CG  # noqa: E402  (StandInCIN; imports the reference's xdeepfm)
import gen_autoint_golden as AG  # noqa: E402  (StandInInteractingLayer; imports the reference's autoint)
import gen_fibinet_golden as BG  # noqa: E402  (StandInSENET, StandInBilinear; imports the reference's fibinet)
import gen_pnn_golden as PG  # noqa: E402  (StandInInner, StandInOuter; imports the reference's pnn)
import gen_adasparse_golden as SPG  # noqa: E402,F401  (imports the reference's adasparse)
from deepctr_torch.inputs import DenseFeat, SparseFeat  # noqa: E402  (shim)
import models.dcn as dcn  # noqa: E402  (the reference)
import models.deepfm as deepfm  # noqa: E402
import models.mmoe as mmoe  # noqa: E402
import models.star as star  # noqa: E402
import models.wdl as wdl  # noqa: E402
import models.adasparse as adasparse  # noqa: E402
import models.afm as afm  # noqa: E402
import models.autoint as autoint  # noqa: E402
import models.esmm as esmm  # noqa: E402
import models.fibinet as fibinet  # noqa: E402
import models.nfm as nfm  # noqa: E402
import models.ple as ple  # noqa: E402
import models.pnn as pnn  # noqa: E402
import models.sharedbottom as sharedbottom  # noqa: E402
import models.xdeepfm as xdeepfm  # noqa: E402

for module in (wdl, deepfm, dcn, mmoe):
    module.DNN = DG.PlainDNN
    module.combined_dnn_input = SG.combined_dnn_input
deepfm.FM = FG.StandInFM
dcn.CrossNet = DG.StandInCrossNet
star.DNN = SG.TowerDNN
star.combined_dnn_input = SG.combined_dnn_input
for module in (xdeepfm, nfm, autoint, fibinet, pnn, sharedbottom, ple, esmm):
    module.DNN = DG.PlainDNN
for module in (xdeepfm, nfm, fibinet, pnn, adasparse, sharedbottom, ple, esmm):
    module.combined_dnn_input = SG.combined_dnn_input
xdeepfm.CIN = CG.StandInCIN
nfm.BiInteractionPooling = FG.StandInBiPooling
afm.AFMLayer, afm.FM = FG.StandInAFM, FG.StandInFM
autoint.InteractingLayer = AG.StandInInteractingLayer
fibinet.SENETLayer, fibinet.BilinearInteraction = BG.StandInSENET, BG.StandInBilinear
pnn.InnerProductLayer, pnn.OutterProductLayer = PG.StandInInner, PG.StandInOuter

D, ROWS, BATCH, S, UNITS, L2, LR, EPOCHS = 16, 96, 32, 3, (16, 8), 1e-5, 1e-3, 2
VOCAB = {"dom": S, "user": 50, "item": 37, "cate": 4}
CASES = ("wdl", "deepfm", "dcn_vector", "dcn_matrix", "mmoe", "star")
MORE_CASES = ("xdeepfm", "nfm", "afm", "autoint", "fibinet", "pnn", "adasparse", "sharedbottom", "ple", "esmm")
MULTI_TASK = ("mmoe", "sharedbottom", "ple", "esmm")
FROM_ONE = MULTI_TASK + ("star",)                      # scenario ids start at 1


def build(name, cols, offset):
    common = dict(l2_reg_embedding=L2, seed=7, device="cpu", flag="")
    if name == "wdl":
        return wdl.WDL, dict(linear_feature_columns=cols, dnn_feature_columns=cols, dnn_hidden_units=UNITS, l2_reg_linear=L2, **common)
    if name == "deepfm":
        return deepfm.DeepFM, dict(linear_feature_columns=cols, dnn_feature_columns=cols, dnn_hidden_units=UNITS, l2_reg_linear=L2,
                                   **common)
    if name.startswith("dcn"):
        return dcn.DCN, dict(linear_feature_columns=cols, dnn_feature_columns=cols, dnn_hidden_units=UNITS, l2_reg_linear=L2,
                             cross_parameterization=name.split("_")[1], **common)
    if name == "mmoe":
        return mmoe.MMOE, dict(dnn_feature_columns=cols, expert_dnn_hidden_units=UNITS, gate_dnn_hidden_units=(8,),
                               tower_dnn_hidden_units=(8,), l2_reg_linear=L2, task_types=["binary"] * S,
                               task_names=["ctr%d" % i for i in range(S)], domain_column="dom", **common)
    both = dict(linear_feature_columns=cols, dnn_feature_columns=cols)
    tasks = dict(task_types=["binary"] * scenarios(name), task_names=["ctr%d" % i for i in range(scenarios(name))], domain_column="dom")
    if name == "xdeepfm":
        return xdeepfm.xDeepFM, dict(dnn_hidden_units=UNITS, cin_layer_size=(8, 8), l2_reg_linear=L2, **both, **common)
    if name == "nfm":
        return nfm.NFM, dict(dnn_hidden_units=UNITS, l2_reg_linear=L2, **both, **common)
    if name == "afm":
        return afm.AFM, dict(attention_factor=4, l2_reg_linear=L2, **both, **common)
    if name == "autoint":
        return autoint.AutoInt, dict(att_layer_num=2, att_head_num=2, dnn_hidden_units=UNITS, **both, **common)
    if name == "fibinet":
        return fibinet.FiBiNET, dict(dnn_hidden_units=UNITS, l2_reg_linear=L2, **both, **common)
    if name == "pnn":
        return pnn.PNN, dict(dnn_feature_columns=cols, dnn_hidden_units=UNITS, use_inner=True, use_outter=True, **common)
    if name == "adasparse":
        return adasparse.AdaSparse, dict(dnn_hidden_units=UNITS, l2_reg_linear=L2, domain_column="dom", num_domains=S, domain_emb_dim=D,
                                         **both, **common)
    if name == "sharedbottom":
        return sharedbottom.SharedBottom, dict(dnn_feature_columns=cols, bottom_dnn_hidden_units=UNITS, tower_dnn_hidden_units=(8,),
                                               l2_reg_linear=L2, **tasks, **common)
    if name == "ple":
        return ple.PLE, dict(dnn_feature_columns=cols, expert_dnn_hidden_units=UNITS, gate_dnn_hidden_units=(8,),
                             tower_dnn_hidden_units=(8,), l2_reg_linear=L2, **tasks, **common)
    if name == "esmm":
        common.pop("flag")
        return esmm.ESMM, dict(dnn_feature_columns=cols, tower_dnn_hidden_units=UNITS, l2_reg_linear=L2, **tasks, **common)
    return star.Star_Net, dict(linear_feature_columns=cols, dnn_feature_columns=cols, domain_column="dom", num_domains=S,
                               domain_id_as_feature=True, dnn_hidden_units=UNITS, use_domain_dnn=True, use_domain_bn=True, **common)


def scenarios(name):
    return 2 if name == "esmm" else S


def visible(rng, key, shape):
    """A value of a visible size for the state entry `key` (None: keep what the constructor left, e.g. running statistics)."""
    if "running_" in key or "num_batches" in key:
        return None
    if key.startswith("embedding_dict."):
        return 0.5 * rng.randn(*shape)
    if key.startswith("linear_model."):
        return 0.3 * rng.randn(*shape)
    if key.endswith("shared_bn_weight") or (key.startswith("bns.") and key.endswith("weight")):
        return 1.0 + 0.2 * rng.randn(*shape)
    if key.startswith("cin.conv1ds.") and len(shape) == 3:      # [out, in, 1]
        return rng.randn(*shape) * shape[1] ** -0.5
    if len(shape) >= 2 and "bias" not in key:
        return rng.randn(*shape) * shape[-1] ** -0.5
    return 0.3 * rng.randn(*shape)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*args, **kwargs)


def run_case(name, outdir):
    rng = np.random.RandomState(sum(map(ord, name)) + 5)
    offset = 1 if name in FROM_ONE else 0
    S = scenarios(name)
    vocab = dict(VOCAB, dom=S + offset)
    cols = [SparseFeat(k, v, embedding_dim=D) for k, v in vocab.items()] + [DenseFeat("price", 1)]
    x = {}
    dom = np.concatenate([rng.permutation(np.arange(BATCH) % S) for _ in range(ROWS // BATCH)]) + offset
    for b in range(ROWS // BATCH):
        counts = np.bincount(dom[b * BATCH:(b + 1) * BATCH] - offset, minlength=S)
        assert counts.min() >= 2, (name, b, counts)
    x["dom"] = dom.astype(np.int64)
    for k in ("user", "item", "cate"):
        x[k] = rng.randint(0, vocab[k], ROWS).astype(np.int64)
    x["price"] = rng.rand(ROWS).astype(np.float32)
    y = (rng.rand(ROWS) < 0.35).astype(np.float32)
    cls, kwargs = build(name, cols, offset)
    loss_arg = ["binary_crossentropy"] * S if name in MULTI_TASK else "binary_crossentropy"

    def fresh(init=None):
        model = cls(**kwargs)
        if init is None:
            init = OrderedInit(model)
        with torch.no_grad():
            sd = model.state_dict()
            for k, v in init.items():
                sd[k].copy_(torch.from_numpy(v))
        return model, init

    def OrderedInit(model):
        init = {}
        for k, v in model.state_dict().items():
            val = visible(rng, k, tuple(v.shape))
            init[k] = v.numpy().copy() if val is None else np.asarray(val, dtype=v.numpy().dtype)
        return init

    def feed(order=None):
        return {k: (v if order is None else v[order]).copy() for k, v in x.items()}

    def run_fit(init, order):
        model, _ = fresh(init)
        model.compile(torch.optim.Adam(model.parameters(), lr=LR), loss_arg, metrics=["binary_crossentropy", "auc"])
        labels = y if order is None else y[order]
        hist = quiet(model.fit, x=feed(order), y=labels.copy(), batch_size=BATCH, epochs=EPOCHS, verbose=0, shuffle=False)
        pred = quiet(model.predict, feed(), BATCH)
        return np.asarray(hist.history["loss"], dtype=np.float64), np.asarray(pred, dtype=np.float64)

    model, init = fresh()
    sig = inspect.signature(cls.__init__)
    out = {"y": y, "keys": np.array(list(model.state_dict())),
           "signature": np.array([p if v.default is inspect.Parameter.empty else f"{p}={v.default!r}"
                                  for p, v in sig.parameters.items() if p != "self"])}
    for k, v in x.items():
        out[f"x/{k}"] = v
    for k, v in init.items():
        out[f"init/{k}"] = v
    model.domain_id_offset = offset                      # (star.py reads it; the reference's fit sets it from x)
    model.compile(torch.optim.Adam(model.parameters(), lr=LR), loss_arg, metrics=["binary_crossentropy", "auc"])
    out["pred0"] = np.asarray(quiet(model.predict, feed(), BATCH), dtype=np.float64)
    model.train()
    X0 = torch.from_numpy(np.stack([x[k][:BATCH].astype(np.float32) for k in model.feature_index], axis=1))
    y0 = torch.from_numpy(y[:BATCH])
    y_pred = model(X0)
    if name in MULTI_TASK:
        ids = torch.from_numpy(dom[:BATCH])
        loss0 = sum(F.binary_cross_entropy(y_pred[:, i][ids == i + offset], y0[ids == i + offset], reduction='sum') for i in range(S))
    else:
        loss0 = F.binary_cross_entropy(y_pred.squeeze(), y0, reduction='sum')
    out["loss0"] = np.asarray(loss0.item(), dtype=np.float64)
    out["reg0"] = np.asarray(model.get_regularization_loss().item(), dtype=np.float64)
    out["fit/loss"], out["fit/pred"] = run_fit(init, None)
    order = np.concatenate([b * BATCH + rng.permutation(BATCH) for b in range(ROWS // BATCH)])
    out["fit_perm/loss"], out["fit_perm/pred"] = run_fit(init, order)
    path = os.path.join(outdir, f"{name}.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    dl = np.abs(out["fit_perm/loss"] / out["fit/loss"] - 1).max()
    dp = np.abs(out["fit_perm/pred"] - out["fit/pred"]).max()
    print(f"{name}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} KB, loss {out['fit/loss']}, reg0 {out['reg0']:.6f}, "
          f"loss0 {out['loss0']:.6f}, perm: loss rel {dl:.2e}, pred {dp:.2e}")


if __name__ == "__main__":
    outdir = os.path.join(ROOT, "tests", "golden", "models")
    for case in (sys.argv[1:] or list(CASES + MORE_CASES)):
        run_case(case, outdir)
