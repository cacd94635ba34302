"""The ten further sibling model classes on the GPU (satrans_amd/models.py) against the reference's own compile / fit / predict,
recorded in tests/golden/models/ (tools/gen_models_golden.py, MORE_CASES).  The tests and bounds are tests/test_models_gpu.py's:
2e-5 relative for the forward, the first loss and the regulariser; History loss rtol 2e-5 and predictions atol 5e-4 over two
epochs of fit - the reference alone stays within a quarter of them (test_models_more_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

import satrans_amd as S
from satrans_amd import PointLoss, RoutedPointLoss, TableAdam
from tests import models_more_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def fresh(name, **extra):
    model = M.build(name, DEV, **extra)
    model.load_state_dict(M.init_state(name))
    return model


def device_batches(model, name):
    x, y = M.inputs(name)
    X = torch.from_numpy(np.stack([np.asarray(x[k], dtype=np.float32) for k in model.feature_index], axis=1)).to(DEV)
    return X, torch.from_numpy(y).to(DEV)


@functools.lru_cache(maxsize=None)
def fitted(name, lazy=True):
    """The model's own compile / fit / predict from the recorded initial state -> (state, History loss, predict, table moments)."""
    model = fresh(name)
    model._table_adam_options = dict(lazy=lazy)
    model.compile(torch.optim.Adam(model.parameters(), lr=M.LR), M.loss_arg(name), metrics=["binary_crossentropy", "auc"])
    x, y = M.inputs(name)
    hist = model.fit(x, y, batch_size=M.BATCH, epochs=M.EPOCHS, verbose=0, shuffle=False)
    pred = model.predict(x, M.BATCH)
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return state, list(hist.history["loss"]), pred, model._table_opt.state_dict()


@functools.lru_cache(maxsize=None)
def written_out(name, lazy=True):
    """The same training as a loop written out here over the model's modules, PointLoss (ESMM: RoutedPointLoss over the head's
    two probabilities), TableAdam and torch.optim.Adam."""
    model = fresh(name)
    tables = [model.embedding] + ([model.linear_model] if model._linear_in_forward else [])
    topt = TableAdam(tables, lr=M.LR, l2_reg_embedding=M.L2, l2_reg_linear=model.l2_reg_linear, lazy=lazy, track_regularizer=True)
    taken = {id(p) for mod in tables for p in mod.parameters()}
    dopt = torch.optim.Adam([p for p in model.parameters() if id(p) not in taken], lr=M.LR)
    point, routed = PointLoss("binary_crossentropy"), RoutedPointLoss("binary_crossentropy", "regression")
    X, y = device_batches(model, name)
    model.domain_id_offset = M.offset_of(name)
    dom = model.feature_index["dom"][0]
    losses = []
    for _ in range(M.EPOCHS):
        model.train()
        epoch = torch.zeros((), dtype=torch.float64, device=DEV)
        topt.zero_regularization_sum()
        for lo in range(0, M.ROWS, M.BATCH):
            Xb, yb = X[lo:lo + M.BATCH], y[lo:lo + M.BATCH]
            if name == "esmm":
                loss, _ = routed(model.head(model._dnn_input(Xb)), Xb[:, dom].long() - M.offset_of(name), yb)
            else:
                loss, _ = point(model._logit(Xb), yb)
            total = loss + model.regularization_loss() + model.aux_loss
            dopt.zero_grad(set_to_none=True)
            total.backward()
            topt.step()
            dopt.step()
            epoch += total.detach().sum()
        topt.flush()
        epoch = epoch + topt.regularization_sum()
        losses.append(float(epoch.item()) / M.ROWS)
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return state, losses, topt.state_dict()


def same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def same_moments(a, b):
    for k, v in b["state"].items():
        assert torch.equal(a["state"][k]["exp_avg"], v["exp_avg"]) and torch.equal(a["state"][k]["exp_avg_sq"], v["exp_avg_sq"]), k


@pytest.mark.parametrize("name", M.CASES)
def test_forward_loss_and_regulariser(name):
    c = M.load(name)
    model = fresh(name)
    model.compile(torch.optim.Adam(model.parameters(), lr=M.LR), M.loss_arg(name))
    x, y = M.inputs(name)
    pred = model.predict(x, M.BATCH)
    assert pred.dtype == np.float64 and pred.shape == c["pred0"].shape
    err = float(np.abs(pred - c["pred0"]).max())
    print(f"{name}: pred0 err {err:.3e} (rel {err / float(np.abs(c['pred0']).max()):.3e})")
    assert err <= M.FWD_RTOL * float(np.abs(c["pred0"]).max())
    # one training step on the first batch: its loss, and the regulariser's value at the initial state (the head's from torch,
    # the tables' from the optimizer's partial sums once every row has taken the step)
    X, yd = device_batches(model, name)
    model.train()
    head_reg = float(model.regularization_loss().detach())
    total, _ = model.train_step(X[:M.BATCH], yd[:M.BATCH])
    model._table_opt.flush()
    reg = head_reg + float(model._table_opt.regularization_sum())
    loss = float(total) - head_reg
    print(f"{name}: loss0 {loss:.7f} / {float(c['loss0']):.7f} (rel {abs(loss / float(c['loss0']) - 1):.3e})  "
          f"reg0 {reg:.8f} / {float(c['reg0']):.8f} (rel {abs(reg / float(c['reg0']) - 1):.3e})")
    assert abs(loss - float(c["loss0"])) <= M.FWD_RTOL * abs(float(c["loss0"]))
    assert abs(reg - float(c["reg0"])) <= M.FWD_RTOL * abs(float(c["reg0"]))


@pytest.mark.parametrize("name", M.CASES)
def test_fit_and_predict_reproduce_the_reference(name):
    c = M.load(name)
    _, hist, pred, _ = fitted(name)
    print(f"{name}: History loss rel {float(np.abs(np.asarray(hist) / c['fit/loss'] - 1).max()):.3e}  "
          f"pred err {float(np.abs(pred - c['fit/pred']).max()):.3e}")
    assert pred.shape == c["fit/pred"].shape
    np.testing.assert_allclose(hist, c["fit/loss"], rtol=M.LOSS_RTOL, atol=0)
    np.testing.assert_allclose(pred, c["fit/pred"], rtol=0, atol=M.PRED_ATOL)


@pytest.mark.parametrize("lazy", (True, False))
@pytest.mark.parametrize("name", M.CASES)
def test_the_harness_adds_nothing(name, lazy):
    """fit equals, bit for bit, the loop written out above - with the lazy TableAdam and with the streaming one."""
    state, hist, _, moments = fitted(name, lazy)
    want_state, want_hist, want_moments = written_out(name, lazy)
    same_state(state, want_state)
    assert hist == want_hist
    assert moments["step"] == want_moments["step"] == M.EPOCHS * (M.ROWS // M.BATCH)
    same_moments(moments, want_moments)


@pytest.mark.parametrize("name", M.CASES)
def test_lazy_and_streaming_runs_leave_the_same_bits(name):
    lazy_state, lazy_hist, lazy_moments = written_out(name, True)
    stream_state, stream_hist, stream_moments = written_out(name, False)
    same_state(lazy_state, stream_state)
    for k, v in stream_moments["state"].items():
        assert torch.equal(lazy_moments["state"][k]["exp_avg"], v["exp_avg"]), k
    np.testing.assert_allclose(lazy_hist, stream_hist, rtol=1e-9, atol=0)      # (the regulariser is ~1e-4 of the loss)


@pytest.mark.parametrize("name", ("xdeepfm", "esmm"))
def test_evaluate_against_sklearn(name):
    from sklearn.metrics import log_loss, roc_auc_score
    model = fresh(name)
    model.compile("adam", M.loss_arg(name), metrics=["binary_crossentropy", "auc"])
    x, y = M.inputs(name)
    pred = model.predict(x, 40)                            # a ragged last batch
    assert pred.shape == ((M.ROWS, 1) if name not in M.MULTI_TASK else (M.ROWS,))
    got = model.evaluate(x, y, 40)
    assert got["auc"] == pytest.approx(roc_auc_score(y, pred.reshape(-1)), abs=1e-12)
    assert got["binary_crossentropy"] == pytest.approx(log_loss(y, pred.reshape(-1)), rel=1e-6)
    rep = model.evaluate_domains(x, y, 40, "dom")
    assert np.array_equal(rep["pred"], pred)
    for i in np.unique(x["dom"]):
        sel = x["dom"] == i
        assert rep["domain_auc"][int(i)] == pytest.approx(roc_auc_score(y[sel], pred.reshape(-1)[sel]), abs=1e-12)


def test_esmm_rows_of_no_task_predict_zero_and_take_no_loss():
    """An id that is neither task's (here offset + 2): predict leaves 0 and the step's loss is that of the other rows, as
    mtl_basemodel.py:268-269 and :376-378 have it."""
    model = fresh("esmm")
    model.compile("adam", M.loss_arg("esmm"))
    x, y = M.inputs("esmm")
    pred = model.predict(x, M.BATCH)
    odd = np.arange(M.ROWS) % 7 == 3
    x2 = dict(x, dom=np.where(odd, 3, x["dom"]))
    cols = M.columns("esmm")
    assert cols[0].vocabulary_size == 3                    # ids 0..2: a table one row taller takes id 3
    cols[0] = S.SparseFeat("dom", 4, embedding_dim=M.D)
    wide = S.ESMM(cols, tower_dnn_hidden_units=M.UNITS, l2_reg_linear=M.L2, l2_reg_embedding=M.L2, seed=7, device=DEV,
                  task_types=["binary"] * 2, task_names=["ctr0", "ctr1"], domain_column="dom")
    init = M.init_state("esmm")
    init["embedding_dict.dom.weight"] = torch.cat([init["embedding_dict.dom.weight"], torch.zeros(1, M.D)])
    wide.load_state_dict(init)
    wide.compile("adam", M.loss_arg("esmm"))
    pred2 = wide.predict(x2, M.BATCH)
    assert wide.domain_id_offset == 1
    assert np.array_equal(pred2[~odd], pred[~odd]) and bool((pred2[odd] == 0).all())
    X, yd = device_batches(wide, "esmm")
    X2 = X.clone()
    X2[:, wide.feature_index["dom"][0]] = torch.from_numpy(x2["dom"].astype(np.float32)).to(DEV)
    wide.eval()
    keep = torch.from_numpy(~odd[:M.BATCH]).to(DEV)
    with torch.no_grad():
        total, _ = wide._loss_and_pred(X2[:M.BATCH], yd[:M.BATCH])
        want, _ = wide._loss_and_pred(X[:M.BATCH][keep], yd[:M.BATCH][keep])
    assert abs(float(total) - float(want)) <= 1e-12 * abs(float(want))


@pytest.mark.parametrize("name", ("adasparse", "esmm"))
def test_sgd_takes_the_dense_route(name):
    import warnings
    model = fresh(name)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        model.compile(torch.optim.SGD(model.parameters(), lr=0.005), M.loss_arg(name))
    assert len(seen) == 1 and "slow route" in str(seen[0].message) and model._table_opt is None
    x, y = M.inputs(name)
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    hist = model.fit(x, y, batch_size=M.BATCH, epochs=2, verbose=0, shuffle=False).history["loss"]
    c = M.load(name)
    # the same model from the same state with the regulariser as torch terms: the first epoch's loss is the reference's but
    # for what three small steps of either optimizer move (the reference's own two epochs differ by under 4 %)
    assert np.isfinite(hist).all() and abs(hist[0] - c["fit/loss"][0]) < 0.05 * c["fit/loss"][0]
    after = model.state_dict()
    assert not torch.equal(after["embedding_dict.user.weight"].cpu(), before["embedding_dict.user.weight"])
    assert np.isfinite(model.predict(x, M.BATCH)).all()


def test_esmm_verbose_metrics_and_validation(capsys):
    model = fresh("esmm")
    model.compile("adam", M.loss_arg("esmm"), metrics=["binary_crossentropy", "auc"])
    x, y = M.inputs("esmm")
    logs = model.fit(x, y, batch_size=M.BATCH, epochs=1, verbose=2, shuffle=True, validation_split=0.25).history
    assert set(logs) == {"loss", "binary_crossentropy", "auc", "val_binary_crossentropy", "val_auc"}
    assert all(np.isfinite(v[0]) for v in logs.values()) and 0.0 <= logs["auc"][0] <= 1.0
    assert "Epoch 1/1" in capsys.readouterr().out
