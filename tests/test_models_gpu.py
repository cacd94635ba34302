"""The sibling model classes on the GPU (satrans_amd/models.py) against the reference's own compile / fit / predict, recorded in
tests/golden/models/ (tools/gen_models_golden.py).  Bounds: the sibling forward bound of DESIGN.md §4 (2e-5 relative) for the
forward, the loss and the regulariser; for two epochs of fit the bounds tests/test_gpu_parity.py holds the SATrans fit to over
eight Adam steps (History loss rtol 2e-5, predictions atol 5e-4) - the reference alone stays within a quarter of them
(test_models_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

from satrans_amd import PointLoss, TableAdam
from tests import models_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def fresh(name, offset=None, **extra):
    model = M.build(name, DEV, offset, **extra)
    init = M.init_state(name)
    if offset is not None and offset != M.offset_of(name):      # the scenario tables without the unused rows below the offset
        lo = M.offset_of(name) - offset
        init = {k: (v[lo:lo + M.SCENARIOS + offset] if k.endswith("embedding_dict.dom.weight") else v) for k, v in init.items()}
    model.load_state_dict(init)
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
def written_out(name, lazy=True, track=True):
    """The same training as a loop written out here over the model's modules, PointLoss, TableAdam and torch.optim.Adam."""
    model = fresh(name)
    tables = [model.embedding] + ([model.linear_model] if model._linear_in_forward else [])
    topt = TableAdam(tables, lr=M.LR, l2_reg_embedding=M.L2, l2_reg_linear=model.l2_reg_linear, lazy=lazy, track_regularizer=track)
    taken = {id(p) for mod in tables for p in mod.parameters()}
    dopt = torch.optim.Adam([p for p in model.parameters() if id(p) not in taken], lr=M.LR)
    point = PointLoss("binary_crossentropy")
    X, y = device_batches(model, name)
    model.domain_id_offset = M.offset_of(name)
    losses, table_reg = [], []
    for _ in range(M.EPOCHS):
        model.train()
        epoch = torch.zeros((), dtype=torch.float64, device=DEV)
        if track:
            topt.zero_regularization_sum()
        for lo in range(0, M.ROWS, M.BATCH):
            logit = model._logit(X[lo:lo + M.BATCH])
            loss, _ = point(logit, y[lo:lo + M.BATCH])
            total = loss + model.regularization_loss() + model.aux_loss
            dopt.zero_grad(set_to_none=True)
            total.backward()
            topt.step()
            dopt.step()
            epoch += total.detach().sum()
        topt.flush()
        if track:
            table_reg.append(float(topt.regularization_sum().item()))
            epoch = epoch + topt.regularization_sum()
        losses.append(float(epoch.item()) / M.ROWS)
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return state, losses, table_reg, topt.state_dict()


def same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("name", M.CASES)
def test_forward_loss_and_regulariser(name):
    c = M.load(name)
    model = fresh(name)
    model.compile(torch.optim.Adam(model.parameters(), lr=M.LR), M.loss_arg(name))
    x, y = M.inputs(name)
    pred = model.predict(x, M.BATCH)
    assert pred.dtype == np.float64 and pred.shape == c["pred0"].shape
    err = float(np.abs(pred - c["pred0"]).max())
    print(f"{name}: pred0 err {err:.3e}")
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
    print(f"{name}: loss0 {loss:.7f} / {float(c['loss0']):.7f}  reg0 {reg:.8f} / {float(c['reg0']):.8f}")
    assert abs(loss - float(c["loss0"])) <= M.FWD_RTOL * abs(float(c["loss0"]))
    assert abs(reg - float(c["reg0"])) <= M.FWD_RTOL * abs(float(c["reg0"]))


@pytest.mark.parametrize("name", M.CASES)
def test_fit_and_predict_reproduce_the_reference(name):
    c = M.load(name)
    _, hist, pred, _ = fitted(name)
    print(f"{name}: History loss {hist} / {c['fit/loss'].tolist()}  pred err {float(np.abs(pred - c['fit/pred']).max()):.3e}")
    assert pred.shape == c["fit/pred"].shape
    np.testing.assert_allclose(hist, c["fit/loss"], rtol=M.LOSS_RTOL, atol=0)
    np.testing.assert_allclose(pred, c["fit/pred"], rtol=0, atol=M.PRED_ATOL)


@pytest.mark.parametrize("lazy", (True, False))
@pytest.mark.parametrize("name", M.CASES)
def test_the_harness_adds_nothing(name, lazy):
    """fit equals, bit for bit, the loop written out above - with the lazy TableAdam and with the streaming one, which shows the
    flushes in front of epoch end, predict and state_dict."""
    state, hist, _, moments = fitted(name, lazy)
    want_state, want_hist, _, want_moments = written_out(name, lazy)
    same_state(state, want_state)
    assert hist == want_hist
    assert moments["step"] == want_moments["step"] == M.EPOCHS * (M.ROWS // M.BATCH)
    for k, v in want_moments["state"].items():
        assert torch.equal(moments["state"][k]["exp_avg"], v["exp_avg"]) and torch.equal(moments["state"][k]["exp_avg_sq"], v["exp_avg_sq"]), k


@pytest.mark.parametrize("name", M.CASES)
def test_lazy_and_streaming_runs_leave_the_same_bits(name):
    lazy_state, lazy_hist, _, lazy_moments = written_out(name, True)
    stream_state, stream_hist, _, stream_moments = written_out(name, False)
    same_state(lazy_state, stream_state)
    for k, v in stream_moments["state"].items():
        assert torch.equal(lazy_moments["state"][k]["exp_avg"], v["exp_avg"]), k
    np.testing.assert_allclose(lazy_hist, stream_hist, rtol=1e-9, atol=0)      # (the regulariser is ~1e-4 of the loss)


@pytest.mark.parametrize("name", M.CASES)
def test_regulariser_total_of_the_lazy_and_the_streaming_run(name):
    """After flush() the tables' regulariser total of an epoch agrees between the lazy and the streaming run to 1e-9 relative: at
    most ~10^6 double additions of 2^-53 each, in another grouping.  That premise needs the replay to form every postponed p^2 in
    double, as the step kernels do: TableAdam(track_regularizer=True) runs satrans_embed_lazy_replay_reg64 / _flush_reg64 for it
    (with the engine's replay, which adds an element's postponed p^2 in fp32, the totals differed by up to 1.56e-9)."""
    _, _, lazy_reg, _ = written_out(name, True)
    _, _, stream_reg, _ = written_out(name, False)
    assert len(lazy_reg) == len(stream_reg) == M.EPOCHS
    for a, b in zip(lazy_reg, stream_reg):
        print(f"{name}: table regulariser total lazy {a!r} streaming {b!r} rel {abs(a - b) / abs(b):.3e}")
    for a, b in zip(lazy_reg, stream_reg):
        assert abs(a - b) <= 1e-9 * abs(b)


@pytest.mark.parametrize("name", ("deepfm", "star"))
def test_tracking_the_regulariser_changes_no_table_and_no_moment(name):
    state, _, _, moments = written_out(name, True, True)
    plain_state, _, _, plain_moments = written_out(name, True, False)
    same_state(state, plain_state)
    for k, v in plain_moments["state"].items():
        assert torch.equal(moments["state"][k]["exp_avg"], v["exp_avg"]) and torch.equal(moments["state"][k]["exp_avg_sq"], v["exp_avg_sq"]), k


@pytest.mark.parametrize("name", ("wdl", "mmoe", "star"))
def test_evaluate_against_sklearn(name):
    from sklearn.metrics import log_loss, roc_auc_score
    model = fresh(name)
    model.compile("adam", M.loss_arg(name), metrics=["binary_crossentropy", "auc"])
    x, y = M.inputs(name)
    pred = model.predict(x, 40)                            # a ragged last batch
    assert pred.shape == ((M.ROWS, 1) if name != "mmoe" else (M.ROWS,))
    got = model.evaluate(x, y, 40)
    assert got["auc"] == pytest.approx(roc_auc_score(y, pred.reshape(-1)), abs=1e-12)
    assert got["binary_crossentropy"] == pytest.approx(log_loss(y, pred.reshape(-1)), rel=1e-6)
    rep = model.evaluate_domains(x, y, 40, "dom")
    assert np.array_equal(rep["pred"], pred)
    assert rep["auc"] == pytest.approx(roc_auc_score(y, pred.reshape(-1)), abs=1e-12)
    for i in np.unique(x["dom"]):
        sel = x["dom"] == i
        assert rep["domain_auc"][int(i)] == pytest.approx(roc_auc_score(y[sel], pred.reshape(-1)[sel]), abs=1e-12)


@pytest.mark.parametrize("name", ("deepfm", "mmoe"))
def test_an_id_outside_its_table_raises_and_the_next_fit_runs(name):
    model = fresh(name)
    model.compile("adam", M.loss_arg(name))
    x, y = M.inputs(name)
    bad = dict(x, user=np.where(np.arange(M.ROWS) == 5, 50, x["user"]))
    with pytest.raises(IndexError):
        model.fit(bad, y, batch_size=M.BATCH, epochs=1, verbose=0, shuffle=False)
    hist = model.fit(x, y, batch_size=M.BATCH, epochs=1, verbose=0, shuffle=False)
    assert np.isfinite(hist.history["loss"]).all() and np.isfinite(model.predict(x, M.BATCH)).all()


@pytest.mark.parametrize("name", ("mmoe", "star"))
def test_scenario_ids_from_zero_and_from_one(name):
    """The fixtures' ids start at 1 (domain_id_offset = 1); the same rows with ids from 0 and tables without the unused row
    predict the same bits and train to the same loss but for the regulariser of the row that is gone."""
    x, y = M.inputs(name)
    x0 = dict(x, dom=x["dom"] - 1)
    one, zero = fresh(name), fresh(name, offset=0)
    for m in (one, zero):
        m.compile("adam", M.loss_arg(name))
    p1, p0 = one.predict(x, M.BATCH), zero.predict(x0, M.BATCH)
    assert one.domain_id_offset == 1 and zero.domain_id_offset == 0
    assert np.array_equal(p1, p0)
    h0 = zero.fit(x0, y, batch_size=M.BATCH, epochs=1, verbose=0, shuffle=False).history["loss"][0]
    h1 = fitted(name)[1][0]
    print(f"{name}: epoch loss with ids from 0: {h0!r}, from 1: {h1!r}")
    assert np.isfinite(h0) and abs(h0 - h1) <= 1e-3 * abs(h1)      # (the 0-based tables lack one regularised, never gathered row)


def test_verbose_metrics_and_validation(capsys):
    model = fresh("deepfm")
    model.compile("adam", "binary_crossentropy", metrics=["binary_crossentropy", "auc"])
    x, y = M.inputs("deepfm")
    hist = model.fit(x, y, batch_size=M.BATCH, epochs=1, verbose=2, shuffle=True, validation_split=0.25)
    logs = hist.history
    assert set(logs) == {"loss", "binary_crossentropy", "auc", "val_binary_crossentropy", "val_auc"}
    assert all(np.isfinite(v[0]) for v in logs.values()) and 0.0 <= logs["auc"][0] <= 1.0
    assert "Epoch 1/1" in capsys.readouterr().out
