"""Instance-level attention search on the device (csrc/attn_inst.hip, attention_instances, predict's 'instattn'): the kernels
through the C ABI against the numpy brute force - identical fp32 comparisons, so everything is compared EXACTLY -, the public API
against captured attention, the reference's own attention (golden taps) and the one pass that serves 'showattn' too."""
import ctypes
import os

import numpy as np
import pytest
import torch

from satrans_amd import attn_inst as AI
from satrans_amd import native
from tests.attn_inst_reference import MATCH_DTYPE, brute_force, clauses_of
from tests.helpers import Case, build_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- kernel level ---------------------------------------------------------------------------------------------------------
def _att(B, H, F, seed):
    """softmax of N(0, 1.5^2) scores: a few entries per row well above 1 / F, so that atoms fire."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.softmax(1.5 * torch.randn(H, B, F, F, generator=g, device=DEV), dim=-1).contiguous()


def _c_rules(rules):
    arr = (native.AttnRule * len(rules))()
    for r, rule in enumerate(rules):
        arr[r].n_clauses = len(rule)
        for c, clause in enumerate(rule):
            arr[r].n_atoms[c] = len(clause)
            for a, (q, k, t) in enumerate(clause):
                arr[r].atoms[c][a].q, arr[r].atoms[c][a].k, arr[r].atoms[c][a].thr = q, k, t
    return arr


class _List:
    """A device match list of `cap` entries, filled with a sentinel, and its total."""

    def __init__(self, cap, F, C=0, x_dtype=torch.float32):
        self.cap = cap
        self.records = torch.full((max(cap, 1), 2), -7, dtype=torch.int64, device=DEV)
        self.maps = torch.full((max(cap, 1), F, F), -7.0, device=DEV)
        self.pred = torch.full((max(cap, 1),), -7.0, device=DEV)
        self.rows = torch.full((max(cap, 1), max(C, 1)), -7, dtype=x_dtype, device=DEV)
        self.total = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.range = torch.zeros(2, dtype=torch.int64, device=DEV)

    def rec(self, n):
        return self.records[:n].cpu().numpy().view(MATCH_DTYPE).reshape(n)


def _match(att, rules, lst, eligible=None, first_index=0):
    lib = native.lib()
    H, B, F, _ = att.shape
    need = lib.satrans_attn_inst_workspace_bytes(B, H, F)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    native.check(lib.satrans_attn_inst_match(att.data_ptr(), B, H, F, _c_rules(rules), len(rules), native.ptr(eligible), first_index,
                                             lst.records.data_ptr(), lst.cap, lst.total.data_ptr(), lst.range.data_ptr(),
                                             ws.data_ptr(), need, native.stream_handle(DEV)), "satrans_attn_inst_match")


def _gather(att, lst, m0, m1, first_index, prob=None, x=None, use_range=False):
    lib = native.lib()
    H, B, F, _ = att.shape
    w = x.element_size() // 4 if x is not None else 0
    native.check(lib.satrans_attn_inst_gather(
        att.data_ptr(), B, H, F, lst.records.data_ptr(), m0, m1, lst.range.data_ptr() if use_range else None, first_index,
        lst.maps.data_ptr(), native.ptr(prob), lst.pred.data_ptr() if prob is not None else None,
        x.data_ptr() if x is not None else None, x.stride(0) * w if x is not None else 0, x.shape[1] * w if x is not None else 0,
        lst.rows.data_ptr() if x is not None else None, native.stream_handle(DEV)), "satrans_attn_inst_gather")


def _quantile_rules(att_h, F, rng):
    """Three rules with thresholds at quantiles of the atoms they name: a single atom, the reference's `A and (B or C)` shape
    (meta_basemodel.py:484) and a conjunction of a two-atom and a four-atom clause."""
    def atom(quant):
        q, k = int(rng.integers(0, F)), int(rng.integers(0, F))
        return (q, k, float(np.quantile(att_h[:, :, q, k], quant)))
    return [[[atom(0.8)]],
            [[atom(0.5)], [atom(0.7), atom(0.7)]],
            [[atom(0.4), atom(0.6)], [atom(0.6), atom(0.7), atom(0.8), atom(0.9)]]]


@pytest.mark.parametrize("B", [1, 63, 700, 8192])
@pytest.mark.parametrize("H", [1, 2, 4])
@pytest.mark.parametrize("F", [8, 15, 19, 23, 64])
def test_match_and_gather_equal_the_brute_force_exactly(F, H, B):
    rng = np.random.default_rng(1000 * F + 10 * H + B)
    att = _att(B, H, F, 17 * F + H + B)
    att_h = att.cpu().numpy()
    rules = _quantile_rules(att_h, F, rng)
    elig_h = rng.integers(0, 8, B).astype(np.uint8)
    elig_h[rng.random(B) < 0.2] = 0xFF
    first = 1_000_000_007
    want = brute_force(att_h, rules, elig_h, first)
    C = F + 3
    wide = torch.from_numpy(rng.integers(0, 1 << 23, (B, C + 2)).astype(np.float32)).to(DEV)
    x = wide[:, :C]                                                       # rows C + 2 apart: the stride is honoured
    prob = torch.from_numpy(rng.random(B).astype(np.float32)).to(DEV)
    cap = len(want) + 5
    lst = _List(cap, F, C)
    _match(att, rules, lst, torch.from_numpy(elig_h).to(DEV), first)
    _gather(att, lst, 0, cap, first, prob, x, use_range=True)
    torch.cuda.synchronize()
    print(f"F={F} H={H} B={B}: {len(want)} records of {B * H * 3} possible")
    assert int(lst.total.item()) == len(want)
    assert lst.range.tolist() == [0, len(want)]
    got = lst.rec(cap)
    assert np.array_equal(got[:len(want)], want)
    assert (lst.records[len(want):] == -7).all(), "nothing is written beyond the matches"
    b = want["index"] - first
    n = len(want)
    assert np.array_equal(lst.maps[:n].cpu().numpy().view(np.uint32), att_h[want["head"], b].view(np.uint32))
    assert np.array_equal(lst.pred[:n].cpu().numpy(), prob.cpu().numpy()[b])
    assert np.array_equal(lst.rows[:n].cpu().numpy(), x.cpu().numpy()[b])
    assert (lst.maps[n:] == -7).all() and (lst.pred[n:] == -7).all() and (lst.rows[n:] == -7).all()
    if B >= 63:
        assert 0 < n < B * H * 3, "the case exercises both outcomes"


def test_threshold_is_strict_and_a_nan_never_matches():
    B, H, F = 700, 4, 19
    att = _att(B, H, F, 3)
    att_h = att.cpu().numpy()
    h0, b0, q, k = 2, 345, 7, 5
    thr = float(att_h[h0, b0, q, k])                                      # exactly that pair's value
    below = float(np.nextafter(np.float32(thr), np.float32(0)))
    for t, expect in ((thr, False), (below, True)):
        rules = [[[(q, k, t)]]]
        want = brute_force(att_h, rules)
        lst = _List(len(want) + 1, F)
        _match(att, rules, lst)
        got = lst.rec(len(want))
        assert int(lst.total.item()) == len(want) and np.array_equal(got, want)
        assert (((got["index"] == b0) & (got["head"] == h0)).any()) == expect
    # NaN entries: in a single atom, in a conjunction, in one arm of a disjunction (the other arm still decides)
    att[:, ::3, q, k] = float("nan")
    att[1, :, 2, 2] = float("nan")
    att_h = att.cpu().numpy()
    rules = [[[(q, k, -1.0)]], [[(q, k, -1.0)], [(0, 0, -1.0)]], [[(q, k, 0.5), (2, 2, -1.0)]], [[(2, 2, 0.01)]]]
    want = brute_force(att_h, rules)
    lst = _List(len(want) + 1, F)
    _match(att, rules, lst)
    got = lst.rec(len(want))
    assert int(lst.total.item()) == len(want) and np.array_equal(got, want)
    assert not (got["index"][got["rule"] < 2] % 3 == 0).any()
    assert not ((got["rule"] == 3) & (got["head"] == 1)).any() and ((got["rule"] == 3) & (got["head"] == 0)).any()
    assert ((got["rule"] == 2) & (got["head"] != 1) & (got["index"] % 3 == 0)).any()


@pytest.mark.parametrize("B,H,F", [(63, 1, 15), (700, 4, 19), (8192, 2, 8)])
def test_no_match_every_pair_matching_and_several_rules_per_pair(B, H, F):
    att = _att(B, H, F, 11)
    att_h = att.cpu().numpy()
    # nothing: a threshold of 1 (a softmax entry never exceeds it), and an eligibility of 0 under rules that always hold
    always = [[[(0, 0, -1.0)]], [[(1, 2, -1.0)], [(3, 3, 2.0), (F - 1, F - 1, -0.5)]], [[(2, 1, -1.0)]]]
    for rules, elig in (([[[(1, 1, 1.0)]]], None), (always, torch.zeros(B, dtype=torch.uint8, device=DEV))):
        lst = _List(4, F)
        _match(att, rules, lst, elig)
        assert int(lst.total.item()) == 0 and lst.range.tolist() == [0, 0] and (lst.records == -7).all()
    # every pair, three rules each: B * H * 3 records in (sample, head, rule) order
    lst = _List(B * H * 3, F)
    _match(att, always, lst, first_index=5)
    got = lst.rec(B * H * 3)
    assert int(lst.total.item()) == B * H * 3
    assert np.array_equal(got["index"], np.repeat(np.arange(B), H * 3) + 5)
    assert np.array_equal(got["head"], np.tile(np.repeat(np.arange(H), 3), B))
    assert np.array_equal(got["rule"], np.tile(np.arange(3), B * H))
    assert np.array_equal(got, brute_force(att_h, always, None, 5))
    # rule bits: sample b may match rule (b % 3) only, 0xff every rule
    elig = (1 << (np.arange(B) % 3)).astype(np.uint8)
    elig[::7] = 0xFF
    lst = _List(B * H * 3, F)
    _match(att, always, lst, torch.from_numpy(elig).to(DEV))
    want = brute_force(att_h, always, elig)
    assert int(lst.total.item()) == len(want) and np.array_equal(lst.rec(len(want)), want)


def test_capacity_appending_across_calls_and_determinism():
    B, H, F = 8192, 4, 19
    att = _att(B, H, F, 23)
    att_h = att.cpu().numpy()
    rules = _quantile_rules(att_h, F, np.random.default_rng(2))
    want = brute_force(att_h, rules)
    total = len(want)
    assert total > 1000
    # a capacity below the total: the first `cap` records arrive, the total is exact, nothing is written past the list
    cap = total // 3
    lst = _List(cap + 64, F)
    lst.cap = cap
    _match(att, rules, lst)
    _gather(att, lst, 0, cap, 0, use_range=True)
    assert int(lst.total.item()) == total and lst.range.tolist() == [0, cap]
    assert np.array_equal(lst.rec(cap), want[:cap]) and (lst.records[cap:] == -7).all()
    assert np.array_equal(lst.maps[:cap].cpu().numpy().view(np.uint32), att_h[want["head"][:cap], want["index"][:cap]].view(np.uint32))
    assert (lst.maps[cap:] == -7).all()
    # a second call on the full list: nothing more is written, the total keeps counting
    _match(att, rules, lst, first_index=B)
    assert int(lst.total.item()) == 2 * total and lst.range.tolist() == [cap, cap] and np.array_equal(lst.rec(cap), want[:cap])
    # the batches of a pass appended one after the other give the list of the whole, whatever the cut - also across the capacity
    for cuts, cap2 in (((0, 1000, 1063, 5000, B), total + 3), ((0, 4096, B), total - 100), ((0, 1, 2, B), total)):
        parts = _List(cap2, F)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            sub = att[:, lo:hi].contiguous()
            before = int(parts.total.item())
            _match(sub, rules, parts, first_index=lo)
            _gather(sub, parts, 0, cap2, lo, use_range=True)
            assert parts.range.tolist() == [min(before, cap2), min(int(parts.total.item()), cap2)]
        n = min(total, cap2)
        assert int(parts.total.item()) == total and np.array_equal(parts.rec(n), want[:n])
        assert np.array_equal(parts.maps[:n].cpu().numpy().view(np.uint32),
                              att_h[want["head"][:n], want["index"][:n]].view(np.uint32))
    # two calls, the same bits
    a, b = _List(total, F), _List(total, F)
    _match(att, rules, a)
    _match(att, rules, b)
    _gather(att, a, 0, total, 0)
    _gather(att, b, 0, total, 0)
    assert torch.equal(a.records, b.records) and torch.equal(a.total, b.total) and torch.equal(a.maps, b.maps)


def test_gather_of_a_hand_built_list_skips_other_batches_and_copies_int64_rows():
    B, H, F, C = 700, 4, 23, 9
    att = _att(B, H, F, 31)
    att_h = att.cpu().numpy()
    ids = np.array([50, 1049, 1000, 1699, 1700, 999, 1000], dtype=np.int64)      # batch = [1000, 1700)
    rec = AI.hand_records(ids, H)
    bad_head = np.array([[1001, (-1 << 32) | 99]], dtype=np.int64)               # head 99, rule -1
    rec = np.concatenate([rec, bad_head])
    lst = _List(len(rec), F, C, torch.int64)
    lst.records.copy_(torch.from_numpy(rec))
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 1 << 40, (B, C))).to(DEV)
    prob = torch.rand(B, device=DEV)
    _gather(att, lst, 0, len(rec), 1000, prob, x)
    inside = np.repeat((ids >= 1000) & (ids < 1700), H)
    maps, rows, pred = lst.maps.cpu().numpy(), lst.rows.cpu().numpy(), lst.pred.cpu().numpy()
    for m in range(len(rec) - 1):
        if inside[m]:
            b = ids[m // H] - 1000
            assert np.array_equal(maps[m].view(np.uint32), att_h[m % H, b].view(np.uint32))
            assert np.array_equal(rows[m], x[b].cpu().numpy()) and pred[m] == float(prob[b])
        else:
            assert (maps[m] == -7).all() and (rows[m] == -7).all() and pred[m] == -7
    assert (maps[-1] == -7).all() and pred[-1] == -7


# ---- public API -----------------------------------------------------------------------------------------------------------
def _captured(model, X, batch_size, layer=0):
    """float32 [H, N, F, F] attention of `layer` and float64 [N] probabilities from capture_attention forwards."""
    Xd = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).to(DEV)
    model.eval()
    model.capture_attention = True
    atts, probs = [], []
    try:
        for lo in range(0, X.shape[0], batch_size):
            probs.append(model(Xd[lo:lo + batch_size]).cpu().numpy())
            atts.append(model.domain_int_layers[layer].normalized_att_scores.cpu().numpy())
    finally:
        model.capture_attention = False
    return np.concatenate(atts, axis=1), np.concatenate(probs).reshape(-1).astype(np.float64)


def _tiled(X, y, n, seed):
    """n rows drawn from the fixture's rows (its ids are the ones the tables hold)."""
    pick = np.random.default_rng(seed).integers(0, X.shape[0], n)
    return np.ascontiguousarray(X[pick]), np.ascontiguousarray(y[pick])


def _api_model(name):
    if name == "varlen":
        from tests import varlen_reference as VR
        model = VR.build(DEV, combiners=("mean", "max"), length=False)
        X, y = VR.batch(model, 700, seed=4)
        return model, X.numpy(), y.numpy().astype(np.float64)
    c = Case(name)
    model = build_model(c, DEV)
    X, y = _tiled(c.X.numpy(), c.y.numpy().reshape(-1), 700, 6)
    return model, X, y.astype(np.float64)


def _api_rules(model, att, y, X):
    """Rules at quantiles of the captured attention, by index and by name, with label and column filters."""
    names = AI.layer_field_names(model)
    F = len(names)
    qt = lambda q, k, quant: float(np.quantile(att[:, :, q, k], quant))
    feat = next(iter(model.feature_index))
    col = model.feature_index[feat][0]
    med = float(np.median(X[:, col]))
    return [AI.AttentionRule([(1, 2, qt(1, 2, 0.7))]),
            AI.AttentionRule([(names[F - 1], names[0], qt(F - 1, 0, 0.5)), [(0, F - 1, qt(0, F - 1, 0.6)), (2, names[1], qt(2, 1, 0.6))]],
                             label=1),
            AI.AttentionRule([(F - 1, F - 1, qt(F - 1, F - 1, 0.3))], where=[(feat, ">=", med)], label=0)]


def _api_brute(model, rules, att, X, y):
    elig = AI.eligibility(rules, X, y, model.feature_index)
    names = AI.layer_field_names(model)
    plain = []
    for r in rules:
        c = AI.resolve_rules([r], names)[0]
        plain.append([[(c.atoms[i][j].q, c.atoms[i][j].k, c.atoms[i][j].thr) for j in range(c.n_atoms[i])] for i in range(c.n_clauses)])
    return brute_force(att, plain, elig)


@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos", "small_gate", "varlen"])
def test_attention_instances_equal_the_brute_force_over_captured_attention(name):
    model, X, y = _api_model(name)
    N_ = X.shape[0]
    eng = model._require_engine()
    layer = 1 if name == "aliccp_sota" else 0
    att, prob = _captured(model, X, 256, layer)
    rules = _api_rules(model, att, y, X)
    want = _api_brute(model, rules, att, X, y)
    res = model.attention_instances(X, y, rules=rules, layer=layer, batch_size=256)
    print(f"{name}: {len(want)} matches of {N_ * eng.H * len(rules)} possible")
    assert res["total"] == len(want) and not res["truncated"]
    assert res["index"].dtype == np.int64 and res["head"].dtype == np.int32 and res["rule"].dtype == np.int32
    assert res["pred"].dtype == np.float64 and res["attention"].dtype == np.float32
    assert np.array_equal(res["index"], want["index"]) and np.array_equal(res["head"], want["head"])
    assert np.array_equal(res["rule"], want["rule"])
    assert res["attention"].shape == (len(want), eng.F, eng.F)
    assert np.array_equal(res["attention"].view(np.uint32), att[want["head"], want["index"]].view(np.uint32))
    assert np.array_equal(res["label"], y[want["index"]])
    assert np.array_equal(res["x"], X[want["index"]].astype(np.float32))
    # pred is predict()'s
    pred = model.predict(X, 256)
    assert np.array_equal(res["pred"], pred[want["index"], 0]) and np.array_equal(pred[:, 0], prob)
    if name != "small_gate":                                              # (its attention is the constant 1 / F: all or nothing)
        assert 0 < len(want) < N_ * eng.H * len(rules)
    # the same for every batch size
    for bs in (64, N_):
        other = model.attention_instances(X, y, rules=rules, layer=layer, batch_size=bs)
        for k in ("index", "head", "rule", "attention", "x", "label", "pred"):
            assert np.array_equal(other[k], res[k]), (bs, k)
        assert other["total"] == res["total"]
    # streamed input equals resident input
    model.stream_input = True
    try:
        streamed = model.attention_instances(X, y, rules=rules, layer=layer, batch_size=256)
    finally:
        model.stream_input = None
    for k in ("index", "head", "rule", "attention", "x", "label", "pred"):
        assert np.array_equal(streamed[k], res[k]), k
    # truncation: the first matches, the exact total
    if len(want) > 3:
        cut = model.attention_instances(X, y, rules=rules, layer=layer, batch_size=256, max_instances=len(want) // 2)
        assert cut["truncated"] and cut["total"] == len(want) and len(cut["index"]) == len(want) // 2
        assert np.array_equal(cut["attention"], res["attention"][:len(want) // 2])
        assert np.array_equal(cut["pred"], res["pred"][:len(want) // 2])
    # sample_ids: every head of the listed samples, in the given order
    ids = [N_ - 1, 0, 300, 299, 300, 64]
    picked = model.attention_instances(X, sample_ids=ids, layer=layer, batch_size=256)
    assert picked["total"] == len(ids) * eng.H and not picked["truncated"] and "label" not in picked
    assert np.array_equal(picked["index"], np.repeat(ids, eng.H)) and (picked["rule"] == -1).all()
    assert np.array_equal(picked["head"], np.tile(np.arange(eng.H), len(ids)))
    assert np.array_equal(picked["attention"].reshape(len(ids), eng.H, eng.F, eng.F).view(np.uint32),
                          att[:, ids].transpose(1, 0, 2, 3).view(np.uint32))
    assert np.array_equal(picked["pred"], prob[np.repeat(ids, eng.H)])
    with pytest.raises(ValueError):
        model.attention_instances(X, sample_ids=[N_])
    with pytest.raises(ValueError):
        model.attention_instances(X, y)
    with pytest.raises(ValueError):
        model.attention_instances(X, y, rules=rules, layer=eng.L)


def test_bf16_setting_gives_the_fp32_instances():
    model, X, y = _api_model("aliccp_sota")
    att, _ = _captured(model, X, 256)
    rules = _api_rules(model, att, y, X)
    a = model.attention_instances(X, y, rules=rules, batch_size=256)
    model.set_forward_precision("bf16")
    try:
        b = model.attention_instances(X, y, rules=rules, batch_size=256)
    finally:
        model.set_forward_precision("fp32")
    for k in ("index", "head", "rule", "attention", "pred"):
        assert np.array_equal(a[k], b[k]), k


# ---- against the reference's own numbers ----------------------------------------------------------------------------------
MIN_GAP = 2e-5          # ten times the 2e-6 attention bound of DESIGN section 4
GOLDEN_RULES = {        # case -> clauses of (q, k): every atom's threshold comes from the golden values of that atom
    "aliccp_sota": [[(7, 7)]],
    "alimama_sota_pos": [[(9, 9), (9, 8), (9, 1)]],
    "small_onlyemb": [[(0, 0), (3, 4)], [(0, 0), (1, 5)]],
    "small_d64": [[(1, 1), (0, 3)]],
    "small_multidomain": [[(5, 3), (5, 0), (0, 3)]],
}


def _gap_threshold(values, quant=0.9):
    """(threshold, gap): the midpoint and width of the widest gap between consecutive sorted values within 5 % of the sample
    around the `quant` quantile."""
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    n = len(v)
    c = int(quant * (n - 1))
    lo, hi = max(0, c - n // 20), min(n - 1, c + n // 20)
    gaps = np.diff(v[lo:hi + 1])
    i = int(np.argmax(gaps))
    return 0.5 * (v[lo + i] + v[lo + i + 1]), float(gaps[i])


@pytest.mark.parametrize("name", sorted(GOLDEN_RULES))
def test_match_set_equals_the_one_of_the_golden_attention(name):
    """The golden files hold the reference's `normalized_att_scores`.  Every atom's threshold sits in the middle of a gap of the
    golden values of at least 2e-5 - a condition on the fixture alone, asserted here - so the device's attention, within 2e-6
    of the golden, falls on the same side for every pair and the match set must equal the golden's exactly.  small_gate,
    small_bilinear and small_none cannot serve: their golden attention is the constant 1 / F (a spread of 0: no gap at all),
    small_k / small_q / small_query spread over 6e-7 only."""
    c = Case(name)
    gold = c.arrays("out")["att0"]
    rule, gaps = [], []
    for clause in GOLDEN_RULES[name]:
        atoms = []
        for q, k in clause:
            thr, gap = _gap_threshold(gold[:, :, q, k])
            gaps.append(gap)
            thr32 = float(np.float32(thr))
            assert abs(thr32 - thr) < 1e-7
            atoms.append((q, k, thr32))
        rule.append(atoms)
    print(f"{name}: gaps {gaps}")
    assert min(gaps) >= MIN_GAP, (name, gaps)
    want = brute_force(gold, [rule])
    assert 0 < len(want) < gold.shape[0] * gold.shape[1]
    model = build_model(c, DEV)
    res = model.attention_instances(c.X.numpy(), rules=[AI.AttentionRule(rule)], batch_size=32)
    assert res["total"] == len(want)
    assert np.array_equal(res["index"], want["index"]) and np.array_equal(res["head"], want["head"])
    np.testing.assert_allclose(res["attention"], gold[want["head"], want["index"]], rtol=0, atol=2e-6)
    np.testing.assert_allclose(res["pred"], c.arrays("out")["prob"].reshape(-1)[want["index"]], rtol=0, atol=2e-6)


# ---- one pass serving both ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["aliccp_sota", "alimama_sota_pos"])
def test_predict_with_instattn_is_one_pass_with_showattn(name, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    c = Case(name)
    model = build_model(c, DEV)
    X, y = _tiled(c.X.numpy(), c.y.numpy().reshape(-1).astype(np.float64), 700, 8)
    dom = X[:, c.meta["feature_names"].index(c.meta["domain"][0])]
    att, _ = _captured(model, X, 256)
    rules = _api_rules(model, att, y, X)
    base = c.meta["flag"]
    model.flag = base + "-showattn"
    p0 = model.predict(X, 256, y, dom)
    shown = [np.asarray(v) for v in (model.attn_list_pos, model.attn_list_neg, model.attn_list_all)]
    assert model.inst_attn_dict == []
    model.flag = base + "-showattn-instattn"
    with pytest.raises(ValueError, match="instattn_rules"):
        model.predict(X, 256, y, dom)
    model.instattn_rules = rules
    model.test_visual_ids = [699, 5, 300, 5, 100000]
    p1 = model.predict(X, 256, y, dom)
    assert np.array_equal(p0, p1)
    for a, b in zip(shown, (model.attn_list_pos, model.attn_list_neg, model.attn_list_all)):
        assert np.array_equal(a.view(np.uint32), np.asarray(b).view(np.uint32))          # bitwise (NaN maps included)
    # inst_attn_dict: the [H, F, F] maps of the visual ids in sample order
    assert len(model.inst_attn_dict) == 3
    for got, i in zip(model.inst_attn_dict, (5, 300, 699)):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), att[:, i].view(np.uint32))
    # the file parses back to attention_instances' result
    path = f"./inst_attn_{model.flag}.txt"
    assert os.path.exists(path)
    back = AI.read_instances(path)
    res = model.attention_instances(X, y, rules=rules, batch_size=64)
    assert res["total"] > 0 and len(back["index"]) == res["total"]
    for k in ("index", "head", "rule", "pred", "label"):
        assert np.array_equal(back[k], res[k]), k
    assert np.array_equal(back["attention"].view(np.uint32), res["attention"].reshape(res["total"], -1).view(np.uint32))
    assert np.array_equal(back["x"], res["x"].astype(np.float64))
    for k in ("index", "head", "rule", "attention", "pred"):
        assert np.array_equal(model.inst_attn_matches[k], res[k]), k
    # 'showattn' alone with visual ids: the maps, no file
    os.remove(path)
    model.flag = base + "-showattn"
    model.predict(X, 256, y, dom)
    assert len(model.inst_attn_dict) == 3 and not os.path.exists(path)
