"""The sibling model classes without a GPU (satrans_amd/models.py): the recorded reference against itself, constructor signatures and
state_dict keys against the recorded lists, compile()'s parsing and errors, and what is refused."""
import inspect
import warnings

import numpy as np
import pytest
import torch

import satrans_amd as S
from satrans_amd.optim import TableAdam
from tests import models_cases as M


@pytest.mark.parametrize("name", M.CASES)
def test_the_reference_agrees_with_itself_well_inside_the_gpu_bounds(name):
    """fit_perm/*: the reference's own run with the rows inside each batch permuted - the same mathematics, another summation
    order - must stay within a quarter of what the GPU test asks of the HIP route."""
    c = M.load(name)
    assert c["fit/loss"].shape == (M.EPOCHS,) and c["fit/pred"].shape[0] == M.ROWS
    np.testing.assert_allclose(c["fit_perm/loss"], c["fit/loss"], rtol=0.25 * M.LOSS_RTOL, atol=0)
    np.testing.assert_allclose(c["fit_perm/pred"], c["fit/pred"], rtol=0, atol=0.25 * M.PRED_ATOL)


@pytest.mark.parametrize("name", M.CASES)
def test_constructor_signature_is_the_references(name):
    sig = inspect.signature(M.CLASSES[name].__init__)
    mine = [p if v.default is inspect.Parameter.empty else f"{p}={v.default!r}" for p, v in sig.parameters.items() if p != "self"]
    assert mine == list(M.load(name)["signature"])


@pytest.mark.parametrize("name", M.CASES)
def test_state_dict_keys_and_order_are_the_references(name):
    model = M.build(name)
    want = list(M.load(name)["keys"])
    assert list(model.state_dict()) == want
    init = M.init_state(name)
    model.load_state_dict(init)                           # a reference checkpoint loads
    sd = model.state_dict()
    for k in want:
        assert torch.equal(sd[k], init[k]), k
    # the reference's unused meta modules (created whenever domain_column is given) are skipped
    model.load_state_dict(dict(init, **{"domain_embeddings.weight": torch.zeros(4, M.D), "meta_net.x": torch.zeros(1)}))
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: v for k, v in init.items() if k != "out.bias" and k != "out.0.bias"})


def test_compile_parses_adam_and_splits_the_parameters():
    model = M.build("deepfm")
    model.compile(torch.optim.Adam(model.parameters(), lr=3e-3, betas=(0.8, 0.9), eps=1e-6), "binary_crossentropy", metrics=["auc", "mse"])
    assert isinstance(model._table_opt, TableAdam) and model._table_opt.track_regularizer
    assert model._table_opt.param_groups[0]["lr"] == 3e-3 and model._table_opt.betas == (0.8, 0.9) and model._table_opt.eps == 1e-6
    g = model._dense_opt.param_groups[0]
    assert isinstance(model._dense_opt, torch.optim.Adam) and (g["lr"], g["betas"], g["eps"]) == (3e-3, (0.8, 0.9), 1e-6)
    tables = {id(p) for p in list(model.embedding.parameters()) + list(model.linear_model.parameters())}
    dense = {id(p) for p in g["params"]}
    assert not (tables & dense) and (tables | dense) == {id(p) for p in model.parameters()}
    assert model.metrics_names == ["loss", "auc", "mse"] and list(model.metrics) == ["auc", "mse"] and model.loss_func == "binary_crossentropy"
    model.compile("adam", "mse")                          # again: the earlier TableAdam lets go of the tables
    assert model._table_opt.param_groups[0]["lr"] == 1e-3 and model.loss_func == "mse"


def test_compile_keeps_a_linear_model_outside_the_logit_with_the_head():
    model = M.build("wdl")                                # wdl.py leaves linear_model out of the logit
    model.compile("adam", "binary_crossentropy")
    dense = {id(p) for p in model._dense_opt.param_groups[0]["params"]}
    assert all(id(p) in dense for p in model.linear_model.parameters())
    assert [type(rec.mod).__name__ for rec in model._table_opt._adopted] == ["FeatureEmbedding"]
    reg = float(model.regularization_loss().detach())
    want = sum(float((M.L2 * p.double() ** 2).sum()) for p in model.linear_model.parameters())
    assert reg == pytest.approx(want, rel=1e-5)


def test_compile_list_of_losses():
    model = M.build("mmoe")
    model.compile("adam", ["binary_crossentropy"] * 3)
    assert model.loss_func == "binary_crossentropy"
    with pytest.raises(NotImplementedError):
        model.compile("adam", ["binary_crossentropy", "mse", "binary_crossentropy"])
    with pytest.raises(ValueError):
        model.compile("adam", ["binary_crossentropy"] * 2)
    with pytest.raises(NotImplementedError):
        model.compile("adam", "hinge")
    with pytest.raises(NotImplementedError):
        model.compile("lbfgs", "mse")
    with pytest.raises(NotImplementedError):
        model.compile(torch.optim.Adam(model.parameters(), weight_decay=0.1), "mse")


@pytest.mark.parametrize("kind", ("sgd", "adagrad", "rmsprop"))
def test_other_optimizers_take_the_dense_route_with_one_warning(kind):
    model = M.build("dcn_vector")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        model.compile(kind, "binary_crossentropy")
    assert len(seen) == 1 and "slow route" in str(seen[0].message)
    assert model._table_opt is None and type(model._dense_opt).__name__.lower() == kind
    assert len(model._dense_opt.param_groups[0]["params"]) == len(list(model.parameters()))
    inst = torch.optim.SGD(model.parameters(), lr=0.25)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        model.compile(inst, "binary_crossentropy")
    assert model._dense_opt is not inst and model._dense_opt.param_groups[0]["lr"] == 0.25
    assert getattr(model.embedding, "_table_opt", None) is None


def test_what_is_not_built_is_refused():
    cols = M.columns("wdl")
    for cls in (S.WDL, S.DeepFM, S.DCN):
        with pytest.raises(NotImplementedError, match="metatrans"):
            cls(cols, cols, flag="metatrans_x")
    with pytest.raises(NotImplementedError, match="metatrans"):
        M.build("mmoe", flag="metatrans")
    with pytest.raises(NotImplementedError, match="metatrans"):
        M.build("star", flag="metatrans")
    with pytest.raises(NotImplementedError):              # the heads' own refusals, at construction
        S.WDL(cols, cols, dnn_activation="prelu", flag="")
    with pytest.raises(NotImplementedError):
        S.WDL(cols, cols, dnn_use_bn=True, flag="")
    with pytest.raises(NotImplementedError):
        S.DeepFM(cols, cols, dnn_use_bn=True, flag="")
    with pytest.raises(NotImplementedError):
        S.DCN(cols, cols, dnn_dropout=0.5, flag="")
    with pytest.raises(NotImplementedError):
        M.build("mmoe", dnn_dropout=0.5)
    with pytest.raises(NotImplementedError):
        S.Star_Net(cols, cols, "dom", 3, True, use_domain_dnn=False, flag="")
    model = M.build("wdl")
    model.compile("adam", "binary_crossentropy")
    x, y = M.inputs("wdl")
    with pytest.raises(NotImplementedError, match="valid_cnt_per_epoch"):
        model.fit(x, y, batch_size=32, valid_cnt_per_epoch=2)
    with pytest.raises(NotImplementedError):
        S.WDL(cols, cols, gpus=[0], flag="")


def test_table_adam_tracking_is_off_by_default_and_guarded():
    model = M.build("deepfm")
    opt = TableAdam([model.embedding, model.linear_model])
    assert opt.track_regularizer is False
    with pytest.raises(RuntimeError, match="track_regularizer"):
        opt.regularization_sum()
    other = M.build("deepfm")
    with pytest.raises(NotImplementedError, match="linear_lazy"):
        TableAdam([other.embedding, other.linear_model], track_regularizer=True, linear_lazy=True)


def test_exports():
    for name in ("HeadModel", "WDL", "DeepFM", "DCN", "MMOE", "Star_Net", "PointLoss"):
        assert name in S.__all__ and hasattr(S, name)
    assert not issubclass(S.HeadModel, S.BaseModel)
