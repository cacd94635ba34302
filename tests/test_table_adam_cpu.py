"""TableAdam without a GPU: what the constructor refuses, the per-step constant table, the layout of a fresh state_dict, and
the premise of the GPU comparison with torch (the fp32 twin stays far inside the bound of the fp64 twin on the same draws)."""
import math

import numpy as np
import pytest
import torch

from tests import table_adam_reference as T


def modules(D=16):
    from satrans_amd import FeatureEmbedding, LinearModel
    from satrans_amd.inputs import build_input_features
    cols = T.columns(D)
    fi = build_input_features(cols)
    return FeatureEmbedding(cols, fi), LinearModel(cols, fi)


def test_constructor_refuses_what_is_not_built():
    from satrans_amd import TableAdam
    fe, lin = modules()
    for kw in (dict(weight_decay=1e-4), dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            TableAdam([fe, lin], **kw)
    with pytest.raises(ValueError, match="arith"):
        TableAdam([fe, lin], arith="quick")
    with pytest.raises(TypeError):
        TableAdam([torch.nn.Linear(2, 2)])
    with pytest.raises(ValueError, match="already adopted"):
        TableAdam([fe, fe])
    assert getattr(fe, "_table_opt", None) is None      # a refused constructor adopts nothing
    opt = TableAdam([fe, lin])
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1
    assert (opt.arith, opt.lazy, opt.flush_every) == ("fast", True, 32)
    assert {id(p) for p in opt.param_groups[0]["params"]} == {id(p) for m in (fe, lin) for p in m.parameters()}
    with pytest.raises(ValueError, match="already adopted"):
        TableAdam([fe])
    with pytest.raises(ValueError, match="already adopted"):
        TableAdam(lin)
    with pytest.raises(NotImplementedError, match="param group"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(1))]})
    with pytest.raises(NotImplementedError):
        opt.step(closure=lambda: 0.0)


def test_step_table_is_the_step_kernels_constants_including_a_rate_change():
    from satrans_amd.optim import StepTable
    b1, b2 = 0.9, 0.999
    tab = StepTable((b1, b2), cap=8)
    rates = [1e-3] * 5 + [5e-4] * 4 + [1e-4] * 30      # step s is taken with rates[s - 1]; past the first capacity too
    for s, lr in enumerate(rates, start=1):
        tab.note(s, lr)
    rows = tab.rows
    assert rows.shape[0] > len(rates) and rows.dtype == np.float64
    assert tuple(rows[0]) == (0.0, 1.0)
    for s, lr in enumerate(rates, start=1):
        assert rows[s, 0] == float(np.float32(lr / (1.0 - b1 ** s))), s
        assert rows[s, 1] == 1.0 / float(np.float32(math.sqrt(1.0 - b2 ** s))), s
    dev = tab.device(len(rates), "cpu")
    assert dev.dtype == torch.float64 and np.array_equal(dev.numpy(), tab.rows)
    tab.note(len(rates) + 1, 7e-4)                     # only the rows from the change on move
    assert np.array_equal(tab.rows[:len(rates) + 1], rows[:len(rates) + 1])
    assert np.array_equal(tab.device(len(rates) + 1, "cpu").numpy(), tab.rows)


def test_hparams_of_a_step_match_its_table_row():
    from satrans_amd import TableAdam
    fe, lin = modules()
    opt = TableAdam([fe, lin], lr=2e-3)
    for s in (1, 2, 7):
        opt.t = s
        opt._steps.note(s, 2e-3)
        h = opt.hparams(1e-5, "fast")
        assert float(h.lr_over_bc1) == opt._steps.rows[s, 0]
        assert 1.0 / float(h.bc2_sqrt) == opt._steps.rows[s, 1]


def test_fresh_state_dict_layout_and_round_trip():
    from satrans_amd import TableAdam
    fe, lin = modules()
    opt = TableAdam([fe, lin])
    sd = opt.state_dict()
    assert sd["kind"] == "adam" and sd["step"] == 0
    want = {f"0.{k}": tuple(v.shape) for k, v in fe.state_dict().items()}
    want.update({f"1.{k}": tuple(v.shape) for k, v in lin.state_dict().items()})
    assert "1.weight" in want and "0.embedding_dict.c.weight" in want and "0.embedding_dict.d.weight" not in want
    assert set(sd["state"]) == set(want)
    for k, st in sd["state"].items():
        assert set(st) == {"exp_avg", "exp_avg_sq"}
        for t in st.values():
            assert t.device.type == "cpu" and t.dtype == torch.float32 and tuple(t.shape) == want[k] and not bool(t.any())
    sd["step"] = 3
    sd["state"]["1.weight"]["exp_avg"].fill_(0.25)
    opt.load_state_dict(sd)
    again = opt.state_dict()
    assert again["step"] == 3 and bool((again["state"]["1.weight"]["exp_avg"] == 0.25).all())
    assert all(int(rec.last.min()) == 3 for rec in opt._adopted)
    bad = dict(sd, state={k: v for k, v in sd["state"].items() if k != "1.weight"})
    with pytest.raises(ValueError, match="1.weight"):
        opt.load_state_dict(bad)
    assert all(p.grad is None for p in opt.param_groups[0]["params"])


@pytest.mark.parametrize("l2", [0.0, 1e-5])
def test_fp32_twin_stays_far_inside_the_bound_of_the_fp64_twin(l2):
    """The premise of the GPU test against torch: on the very draws it uses, torch's own fp32 run of the nine steps differs from
    the fp64 run by less than 0.1 of 1e-4 max|p| + 5e-9 (measured 2.0e-3 on a like shape)."""
    L64, E64 = T.twin(16, l2, torch.float64)
    L32, E32 = T.twin(16, l2, torch.float32)
    ratio = max(T.worst_ratio(L32, L64), T.worst_ratio(E32, E64))
    print(f"[table_adam] fp32 twin against fp64 twin, l2 = {l2}: {ratio:.2e} of the bound")
    assert ratio < 0.1
    moved = max(float((E64[k].double() - T.draw(16)[4][k].double()).abs().max()) for k in E64)
    assert moved > 5 * T.LR      # the nine steps did move the tables
