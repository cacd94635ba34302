"""The ten further sibling model classes without a GPU (satrans_amd/models.py: xDeepFM, NFM, AFM, AutoInt, FiBiNET, PNN, AdaSparse,
SharedBottom, PLE, ESMM): the recorded reference against itself, constructor signatures and state_dict keys against the recorded
lists, and what is refused."""
import inspect

import numpy as np
import pytest
import torch

import satrans_amd as S
from tests import models_more_cases as M


@pytest.mark.parametrize("name", M.CASES)
def test_the_reference_agrees_with_itself_well_inside_the_gpu_bounds(name):
    c = M.load(name)
    assert c["fit/loss"].shape == (M.EPOCHS,) and c["fit/pred"].shape[0] == M.ROWS
    np.testing.assert_allclose(c["fit_perm/loss"], c["fit/loss"], rtol=0.25 * M.LOSS_RTOL, atol=0)
    np.testing.assert_allclose(c["fit_perm/pred"], c["fit/pred"], rtol=0, atol=0.25 * M.PRED_ATOL)
    ids, dom = c["x/dom"], set(range(M.offset_of(name), M.offset_of(name) + M.scenarios(name)))
    for lo in range(0, M.ROWS, M.BATCH):                  # every batch holds at least two rows of every scenario
        counts = {i: int((ids[lo:lo + M.BATCH] == i).sum()) for i in dom}
        assert set(ids[lo:lo + M.BATCH].tolist()) == dom and min(counts.values()) >= 2


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
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: v for k, v in init.items() if k != "out.bias" and k != "out.0.bias"})


@pytest.mark.parametrize("name", [n for n in M.CASES if n != "esmm"])
@pytest.mark.parametrize("word", ("metatrans", "usemetatrans", "usetrans"))
def test_the_transformation_flags_are_refused(name, word):
    with pytest.raises(NotImplementedError, match=word):
        M.build(name, flag=f"x_{word}_y")


def test_esmm_takes_two_binary_tasks_a_domain_column_and_no_flag():
    cols = M.columns("esmm")
    with pytest.raises(ValueError):
        S.ESMM(cols, task_types=["binary"] * 3, task_names=["a", "b", "c"], domain_column="dom")
    with pytest.raises(ValueError):
        S.ESMM(cols, task_types=["binary", "regression"], domain_column="dom")
    with pytest.raises(ValueError):
        S.ESMM(cols)                                      # no domain_column: nothing picks a row's task
    with pytest.raises(TypeError):
        S.ESMM(cols, domain_column="dom", flag="")
    with pytest.raises(NotImplementedError):
        M.build("esmm", dnn_use_bn=True)
    with pytest.raises(NotImplementedError):
        M.build("esmm", gpus=[0])
    model = M.build("esmm")
    assert model.num_tasks == 2 and not model.returns_column
    with pytest.raises(ValueError):
        model.compile("adam", ["binary_crossentropy"] * 3)
    with pytest.raises(NotImplementedError):
        model.compile("adam", ["binary_crossentropy", "mse"])
    model.compile("adam", ["binary_crossentropy"] * 2)
    assert model._routed.loss == "binary_crossentropy" and model._routed.task == "regression"


@pytest.mark.parametrize("name", ("sharedbottom", "ple"))
def test_the_multi_task_models_share_mmoes_checks(name):
    cols = M.columns(name)
    cls = M.CLASSES[name]
    with pytest.raises(ValueError):
        cls(cols, task_types=["binary"] * 3, task_names=["a", "b"], domain_column="dom", flag="")
    with pytest.raises(ValueError):
        cls(cols, task_types=["binary", "ranking"], domain_column="dom", flag="")
    with pytest.raises(NotImplementedError):
        cls(cols, task_types=["binary", "regression"], domain_column="dom", flag="")
    with pytest.raises(ValueError):
        cls(cols, flag="")                                # domain_column is required
    with pytest.raises(NotImplementedError, match="l2_reg_dnn"):
        M.build(name, l2_reg_dnn=1e-4)
    with pytest.raises(NotImplementedError):
        M.build(name, dnn_dropout=0.5)
    model = M.build(name)
    with pytest.raises(NotImplementedError):
        model.compile("adam", ["binary_crossentropy", "mse", "binary_crossentropy"])
    with pytest.raises(ValueError):
        model.compile("adam", ["binary_crossentropy"] * 2)


def test_what_the_heads_lack_is_refused_at_construction():
    for name, extra in (("xdeepfm", dict(l2_reg_dnn=1e-4)), ("xdeepfm", dict(l2_reg_cin=1e-4)), ("xdeepfm", dict(dnn_dropout=0.5)),
                        ("xdeepfm", dict(dnn_use_bn=True)), ("xdeepfm", dict(cin_activation="sigmoid")), ("nfm", dict(bi_dropout=0.5)),
                        ("nfm", dict(dnn_dropout=0.5)), ("nfm", dict(dnn_activation="prelu")), ("afm", dict(afm_dropout=0.5)),
                        ("autoint", dict(l2_reg_dnn=1e-4)), ("autoint", dict(dnn_use_bn=True)), ("autoint", dict(dnn_dropout=0.5)),
                        ("fibinet", dict(dnn_dropout=0.5)), ("fibinet", dict(dnn_activation="prelu")), ("pnn", dict(dnn_dropout=0.5)),
                        ("adasparse", dict(l2_reg_dnn=1e-4)), ("adasparse", dict(dnn_use_bn=True))):
        with pytest.raises(NotImplementedError):
            M.build(name, **extra)
    with pytest.raises(ValueError):
        M.build("pnn", kernel_type="cube")
    with pytest.raises(ValueError, match="domain_emb_dim"):
        M.build("adasparse", domain_emb_dim=32)
    with pytest.raises(ValueError):
        M.build("adasparse", domain_column=None)
    for name in ("xdeepfm", "ple", "esmm"):
        with pytest.raises(NotImplementedError):
            M.build(name, gpus=[0])
        model = M.build(name)
        model.compile("adam", M.loss_arg(name))
        x, y = M.inputs(name)
        with pytest.raises(NotImplementedError, match="valid_cnt_per_epoch"):
            model.fit(x, y, batch_size=32, valid_cnt_per_epoch=2)


def test_afm_without_attention_is_the_fm_term():
    cols = M.columns("afm")
    model = S.AFM(cols, cols, use_attention=False, flag="")
    assert list(model.state_dict())[-1] == "out.bias" and not any(k.startswith("fm.") for k in model.state_dict())


def test_linear_models_outside_the_logit_stay_with_the_head():
    for name in ("autoint", "adasparse"):
        model = M.build(name)
        model.compile("adam", "binary_crossentropy")
        dense = {id(p) for p in model._dense_opt.param_groups[0]["params"]}
        assert all(id(p) in dense for p in model.linear_model.parameters())
        assert [type(rec.mod).__name__ for rec in model._table_opt._adopted] == ["FeatureEmbedding"]
    assert M.build("autoint").l2_reg_linear == 0          # autoint.py:46


def test_exports():
    for name in ("xDeepFM", "NFM", "AFM", "AutoInt", "FiBiNET", "PNN", "AdaSparse", "SharedBottom", "PLE", "ESMM", "RoutedPointLoss"):
        assert name in S.__all__ and hasattr(S, name)
        assert name == "RoutedPointLoss" or issubclass(getattr(S, name), S.HeadModel)
