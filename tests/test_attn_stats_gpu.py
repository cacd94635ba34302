"""Scenario-specific attention maps on the device (csrc/attn_stats.hip, predict's 'showattn', attention_statistics): against the
reference's branch on the golden attention taps, against an fp64 reduction of captured attention at scale, determinism, the
streamed input, batch-size independence, unchanged predictions, the bf16 setting and the configs[4] shape."""
import numpy as np
import pytest
import torch

import bench
from satrans_amd import attn_stats as AS
from tests.attn_stats_reference import reference_showattn
from tests.helpers import NATIVE_CASES, Case, build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", NATIVE_CASES)
def test_showattn_matches_the_reference_branch_on_the_golden_taps(name):
    c = Case(name)
    c.meta = dict(c.meta, flag=c.meta["flag"] + "-showattn")
    model = build_model(c, DEV)
    X, y = c.X.numpy(), c.y.numpy()
    col = c.meta["feature_names"].index(c.meta["domain"][0])
    dom = X[:, col]
    pred = model.predict(X, 64, y, dom)
    want = c.arrays("out")
    np.testing.assert_allclose(pred[:, 0], want["prob"].reshape(-1), rtol=0, atol=2e-6)
    S, L = c.meta["num_domains_list"][0], c.meta["L"]
    atts = [[want[f"att{l}"][:, lo:lo + 64] for l in range(L)] for lo in range(0, X.shape[0], 64)]
    ref = reference_showattn(atts, y, dom, S, L)
    got = (model.attn_list_pos, model.attn_list_neg, model.attn_list_all)
    assert model.inst_attn_dict == []
    for g, r in zip(got, ref):
        assert len(g) == L and all(len(row) == S for row in g)
        for l in range(L):
            for j in range(S):
                assert g[l][j].dtype == np.float32 and g[l][j].shape == r[l][j].shape
                np.testing.assert_allclose(g[l][j], r[l][j], rtol=0, atol=2e-6, equal_nan=True, err_msg=f"{name} l{l} j{j}")
    # the lists are reset on every call: a second call gives the same maps, not twice the sums
    model.predict(X, 64, y, dom)
    np.testing.assert_array_equal(model.attn_list_all[0][0], got[2][0][0])


def _captured_reduction(model, X, y, dom, batch_size, S):
    """fp64 torch reduction of capture_attention forwards: [L, S, 3, H, F, F] sums (pos, neg, all)."""
    bias = AS.scenario_bias(dom)
    keys = torch.from_numpy(AS.class_keys(dom, y, S, bias).astype(np.int64)).to(DEV)
    eng = model._require_engine()
    acc = torch.zeros(eng.L, 3 * S, eng.H, eng.F, eng.F, dtype=torch.float64, device=DEV)
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(DEV)
    model.eval()
    model.capture_attention = True
    try:
        for lo in range(0, X.shape[0], batch_size):
            hi = min(X.shape[0], lo + batch_size)
            model(Xd[lo:hi])
            k = keys[lo:hi]
            ok = k >= 0
            for l, layer in enumerate(model.domain_int_layers):
                a = layer.normalized_att_scores[:, ok].double().permute(1, 0, 2, 3)
                acc[l].index_add_(0, k[ok], a)
    finally:
        model.capture_attention = False
    r = acc.reshape(eng.L, S, 3, eng.H, eng.F, eng.F).cpu().numpy()
    return np.stack([r[:, :, 0], r[:, :, 1], r[:, :, 0] + r[:, :, 1] + r[:, :, 2]], axis=2)


def _aliccp_data(n, seed):
    cfg = bench.make_config("aliccp")
    X, y = bench.synth_batches(n, seed, cfg=cfg)
    rng = np.random.RandomState(seed + 1)
    y = (rng.rand(n) < 0.3).astype(np.float64)
    col = cfg["fields"].index(cfg["domain"])
    dom = X[:, col].astype(np.int64)
    return cfg, X, y, dom


def _check_against_capture(model, X, y, dom, bs, S, tol=1e-6):
    st = model.attention_statistics(X, y, dom, batch_size=bs)
    want = _captured_reduction(model, X, y, dom, bs, S)
    assert st["sum"].shape == want.shape and st["sum"].dtype == np.float64
    np.testing.assert_allclose(st["sum"] / np.maximum(st["count"], 1)[None, :, :, None, None, None],
                               want / np.maximum(st["count"], 1)[None, :, :, None, None, None], rtol=0, atol=tol)
    return st


def test_attention_statistics_at_scale_aliccp_shape():
    n, S = 20_480, 3
    cfg, X, y, dom = _aliccp_data(n, 5)
    # ids in the bias-1 convention (AliCCP's 1..3) with out-of-range ids, a label of 0.5 and a scenario without positives
    dom[:37] = 4
    y[40:90] = 0.5
    y[dom == 2] = np.where(y[dom == 2] == 1, 0, y[dom == 2])
    model = bench.build_model(DEV, 0.005, cfg=cfg)
    st = _check_against_capture(model, X, y, dom, 4096, S)
    assert st["bias"] == 1 and st["count"][1, 0] == 0 and np.isnan(st["mean"][:, 1, 0]).all()
    assert st["count"][:, 2].sum() == n - 37
    # deterministic: two runs, the same bits
    again = model.attention_statistics(X, y, dom, batch_size=4096)
    assert np.array_equal(st["sum"], again["sum"])
    # another batch size: the same statistics to rounding
    other = model.attention_statistics(X, y, dom, batch_size=8192)
    np.testing.assert_allclose(other["mean"], st["mean"], rtol=0, atol=1e-6, equal_nan=True)
    # the streamed input gives the bits of the resident one
    model.stream_input = True
    try:
        streamed = model.attention_statistics(X, y, dom, batch_size=4096)
    finally:
        model.stream_input = None
    assert np.array_equal(streamed["sum"], st["sum"])
    # the bias-0 convention: ids 0..2 (+ out-of-range 3)
    dom0 = dom - 1
    st0 = model.attention_statistics(X, y, dom0, batch_size=4096)
    assert st0["bias"] == 0 and np.array_equal(st0["sum"], st["sum"]) and np.array_equal(st0["count"], st["count"])


def test_showattn_predictions_are_those_without_it():
    n = 20_480
    cfg, X, y, dom = _aliccp_data(n, 9)
    shown = bench.build_model(DEV, 0.005, cfg=cfg)
    p0 = shown.predict(X, 4096, y)
    assert not hasattr(shown, "attn_list_all")
    shown.flag = cfg["flag"] + "-showattn"
    p1 = shown.predict(X, 4096, y)                      # domain ids from the model's scenario column
    assert np.array_equal(p0, p1)
    st = shown.attention_statistics(X, y, dom, batch_size=4096)
    np.testing.assert_array_equal(np.asarray(shown.attn_list_all, dtype=np.float32), st["mean"][:, :, 2].astype(np.float32))
    # evaluate() goes through predict(x, batch_size, y)
    shown.evaluate(X, y, batch_size=4096)
    np.testing.assert_array_equal(shown.attn_list_pos[2][0], st["mean"][2, 0, 0].astype(np.float32))


def test_showattn_needs_labels():
    cfg, X, y, dom = _aliccp_data(256, 3)
    model = bench.build_model(DEV, 0.005, cfg=cfg, flag=cfg["flag"] + "-showattn")
    with pytest.raises(ValueError):
        model.predict(X, 256)
    with pytest.raises(ValueError):
        model.attention_statistics(X, None)


def test_bf16_setting_gives_fp32_statistics():
    n = 8192
    cfg, X, y, dom = _aliccp_data(n, 11)
    model = bench.build_model(DEV, 0.005, cfg=cfg)
    st32 = model.attention_statistics(X, y, dom, batch_size=4096)
    model.set_forward_precision("bf16")
    st16 = model.attention_statistics(X, y, dom, batch_size=4096)
    assert np.array_equal(st16["sum"], st32["sum"])
    model.set_forward_precision("fp32")


def test_attention_statistics_configs4_shape():
    cfg = bench.make_config("c5", 20_000)
    n, S = 4096, 3
    X, _ = bench.synth_batches(n, 4, cfg=cfg)
    rng = np.random.RandomState(4)
    y = (rng.rand(n) < 0.3).astype(np.float64)
    dom = X[:, cfg["fields"].index(cfg["domain"])].astype(np.int64)
    model = bench.build_model(DEV, 0.005, cfg=cfg)
    eng = model._require_engine()
    assert eng.F == 64
    st = _check_against_capture(model, X, y, dom, 2048, S)
    assert st["sum"].shape == (cfg["L"], S, 3, cfg["H"], 64, 64)
    again = model.attention_statistics(X, y, dom, batch_size=2048)
    assert np.array_equal(st["sum"], again["sum"])
    assert eng._ws[2048]["generic"], "configs[4] runs the general path"
