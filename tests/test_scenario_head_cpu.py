"""csrc/scenario.hip and csrc/head.hip without a GPU: the fp64 restatements of tests/scenario_head_reference.py against the
oracle's own functions on model-shaped examples, the chain lengths and the cases of the GPU tests, and the premise of their
bounds (torch's fp32 CPU evaluation of the same operations on the same seeded inputs stays within HALF of every bound)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import satrans_oracle as O
from tests import scenario_head_reference as R

U = R.U


# ---- the restatements are the oracle's functions ------------------------------------------------------------------------------
def _spec(n_cols, flag, L, D, dense=(), sparse=()):
    names = [f"dom{c}" for c in range(n_cols)]
    return O.PathSpec(sparse=list(sparse), dense=list(dense), domain_cols=list(range(n_cols)), embedding_dim=D, head_num=1,
                      layer_num=L, flag=flag, multi_domain_sparse=[(n, c) for c, n in enumerate(names)] if n_cols > 1 else [])


def _close(a, b, tol=1e-13):
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("name", list(R.CHAIN_CASES))
def test_scenario_restatement_equals_the_oracle(name):
    """inputs_fwd + table_fwd on one row per id tuple equal O.scenario_embedding / O.scenario_encoder / O.scenario_vectors of
    a model with those tables, for every case of the chain test (one and several scenario columns, with and without 'pos')."""
    d = R.draw_chain(name)
    S, D, C, pos = d["S"], d["D"], d["C"], d["pos"]
    index = d["index"] if d["index"] is not None else torch.arange(S, dtype=torch.int32).unsqueeze(0)
    X = index.T.double()                                                   # one row per scenario / id tuple
    P = {"domain_map_dnn_Q.linears.0.weight": d["W"].double(), "domain_map_dnn_Q.linears.0.bias": d["bias"].double(),
         "domain_embeddings.weight": d["tables"][0].double()}
    for c in range(C):
        P[f"domain_embedding_dict.dom{c}.weight"] = d["tables"][c].double()
    if pos:
        P["layerid_embeddings.weight"], P["qkvid_embeddings.weight"] = d["lay"].double(), d["role"].double()
    spec = _spec(C, "pos" if pos else "sota", d["L"], D)
    E = R.inputs_fwd([t.double() for t in d["tables"]], d["index"], S, d["lay"].double() if pos else None,
                     d["role"][:2].double() if pos else None)
    tab = R.table_fwd(E, P["domain_map_dnn_Q.linears.0.weight"], P["domain_map_dnn_Q.linears.0.bias"])
    assert torch.equal(torch.relu(E[:S, :D]), O.scenario_embedding(P, X, spec))
    vecs = O.scenario_vectors(P, X, spec)
    if not pos:
        assert E.shape == (S, D)
        assert torch.equal(tab, O.scenario_encoder(P, O.scenario_embedding(P, X, spec), spec))
        assert torch.equal(tab, vecs[0][0]) and vecs[0][0] is vecs[0][1]
        return
    assert len(vecs) == d["L"] and E.shape == (2 * d["L"] * S, 2 * D)
    for l in range(d["L"]):
        for r in range(2):
            lr = 2 * l + r
            assert torch.equal(tab[lr * S:(lr + 1) * S], vecs[l][r]), (l, r)


def test_table_and_relu_restatements_equal_the_oracle():
    """The plain form (one scenario column, no positions: emb straight into the encoder) and 'onlyemb' (relu alone)."""
    emb, W, bias, _ = R.draw_table((37, 20, 257))
    X = torch.arange(37).double().unsqueeze(1)
    P = {"domain_embeddings.weight": emb.double(), "domain_map_dnn_Q.linears.0.weight": W.double(),
         "domain_map_dnn_Q.linears.0.bias": bias.double()}
    want = O.scenario_vectors(P, X, _spec(1, "sota", 2, 20))[1][2]
    assert torch.equal(R.table_fwd(emb.double(), W.double(), bias.double()), want)
    assert torch.equal(torch.relu(emb.double()), O.scenario_vectors(P, X, _spec(1, "onlyemb", 1, 20))[0][0])
    assert bool((emb == 0).any()) and bool((emb < 0).any()) and bool(torch.signbit(emb[emb == 0]).any())


def test_head_restatement_equals_the_tail_of_the_oracle_forward():
    """O.forward of a model without layers IS its tail: gather, flatten, dense columns, Linear, sigmoid."""
    g = torch.Generator().manual_seed(3)
    B, Fn, D = 9, 5, 4
    vocab = 6
    sparse = [(f"f{i}", i) for i in range(Fn)]
    dense = [(Fn + 1, Fn + 2), (Fn, Fn + 1)]                               # dense columns in another order than X's
    X = torch.cat([torch.randint(0, vocab, (B, Fn), generator=g).double(), torch.randn(B, 2, generator=g).double(),
                   torch.randint(0, 3, (B, 1), generator=g).double()], dim=1)
    P = {f"embedding_dict.f{i}.weight": torch.randn(vocab, D, generator=g).double() for i in range(Fn)}
    P.update({"domain_embeddings.weight": torch.randn(3, D, generator=g).double(),
              "domain_map_dnn_Q.linears.0.weight": torch.randn(7, D, generator=g).double(),
              "domain_map_dnn_Q.linears.0.bias": torch.randn(7, generator=g).double(),
              "dnn_linear.weight": torch.randn(1, Fn * D + 2, generator=g).double(), "dnn_linear.bias": torch.randn(1, generator=g).double()})
    spec = O.PathSpec(sparse=sparse, dense=dense, domain_cols=[Fn + 2], embedding_dim=D, head_num=1, layer_num=0)
    want_p, want_z = O.forward(P, X, spec)
    a = O.gather_fields(P, X, spec).flatten(1)
    p, z, flat = R.head_forward(a, X[:, Fn:Fn + 2], torch.tensor([1, 0], dtype=torch.int32), P["dnn_linear.weight"][0], P["dnn_linear.bias"])
    assert torch.equal(z, want_z.squeeze(-1)) and torch.equal(p, want_p.squeeze(-1))
    assert torch.equal(flat[:, Fn * D:], O.dense_block(X, spec))
    p0, z0, _ = R.head_forward(a, None, None, P["dnn_linear.weight"][0, :Fn * D], P["dnn_linear.bias"])
    assert torch.equal(z0, F.linear(a, P["dnn_linear.weight"][:, :Fn * D], P["dnn_linear.bias"]).squeeze(-1))


@pytest.mark.parametrize("kind", [R.BCE, R.MSE, R.MAE], ids=lambda k: R.LOSS_NAMES[k])
def test_loss_pieces_equal_torch(kind):
    """The per-sample formulas of head.hip:54-66 add up to O.bce_sum / F.mse_loss / F.l1_loss(reduction='sum') and their
    dlogit is autograd's through p = sigmoid(z), in fp64, with 0 / 1 and fractional labels and |z| up to 14."""
    g = torch.Generator().manual_seed(5 + kind)
    z = (torch.rand(64, generator=g).double() * 28 - 14).requires_grad_(True)
    t = (torch.rand(64, generator=g) < 0.5).double()
    if kind != R.BCE:
        t[1::2] = torch.rand(32, generator=g).double()
    p = torch.sigmoid(z)
    want = {R.BCE: O.bce_sum, R.MSE: lambda a, b: F.mse_loss(a, b, reduction="sum"),
            R.MAE: lambda a, b: F.l1_loss(a, b, reduction="sum")}[kind](p, t)
    want.backward()
    loss, dl = R.loss_pieces(p.detach(), t, kind)
    want = want.detach()
    assert abs(float(loss.sum() - want)) <= 1e-13 * float(want)
    assert float((dl - z.grad).abs().max()) <= 1e-13
    assert float(R.torch_loss(p.detach(), t, kind)) == float(want)


def test_fed_probability_form_is_autograd_through_sigmoid():
    """torch_loss_and_dlogit, fed torch's own fp32 p = sigmoid(z), gives autograd's d loss / d z bit for bit - saturated z
    included, where p rounds to 1.0 / 0.0, the loss clamps at 100 and the gradient is exactly 0."""
    z = torch.tensor([0.3, -2.0, 7.5, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0, 20.0, -20.0, 90.0, -90.0], requires_grad=True)
    t = torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0])
    p = torch.sigmoid(z)
    loss = F.binary_cross_entropy(p, t, reduction="sum")
    loss.backward()
    got_loss, got_dl = R.torch_loss_and_dlogit(p.detach(), t)
    assert torch.equal(got_loss, loss.detach()) and torch.equal(got_dl, z.grad)
    per = F.binary_cross_entropy(p.detach(), t, reduction="none")
    assert per[3] == 100.0 and per[5] == 100.0 and per[6] == 100.0 and per[7] == 0.0 and per[8] == 0.0
    p = p.detach()
    assert bool((z.grad[[3, 5, 6, 7, 8, 9, 11, 12]] == 0).all()) and float(p[5]) == 1.0 and float(p[6]) == 0.0


# ---- chain lengths and cases -------------------------------------------------------------------------------------------------
def test_chain_lengths():
    assert [R.n_tab(De) for De in (1, 32, 36, 256)] == [7, 7, 8, 14]
    assert [R.n_g_emb(P) for P in (1, 255, 257, 2080)] == [41, 41, 42, 49]
    assert R.n_logit(4, 0) == 11 and R.n_logit(260, 1) == 16 and R.n_logit(736, 65) == 21
    assert R.n_head_sum(1) == 25 and R.n_head_sum(131) == 26 and R.n_head_sum(269) == 27
    assert float(R.sum_bound(3, torch.tensor(2.0))) == 10 * U


def test_cases_hold_what_they_claim():
    S_, De_, P_ = zip(*R.TABLE_CASES)
    assert set(S_) == {1, 3, 37, 240} and set(De_) == {1, 4, 20, 32, 36, 64, 256}
    assert set(P_) == {1, 7, 8, 9, 31, 33, 255, 257, 2080}
    assert {(1, 1, 1), (240, 256, 33), (3, 32, 2080), (37, 20, 257)} <= set(R.TABLE_CASES)
    assert len(set(R.TABLE_CASES)) == len(R.TABLE_CASES) and 18 <= len(R.TABLE_CASES) <= 24
    for v in set(De_):
        assert len({c[0] for c in R.TABLE_CASES if c[1] == v}) >= 3 and len({c[2] for c in R.TABLE_CASES if c[1] == v}) >= 3
    for v in set(P_):
        assert len({c[1] for c in R.TABLE_CASES if c[2] == v}) >= 2
    B_, FD_, nd_, kind_ = zip(*R.HEAD_CASES)
    assert set(B_) == {1, 7, 8, 9, 131, 269} and set(FD_) == {4, 252, 256, 260, 736} and {0, 1, 2, 65} <= set(nd_)
    assert all(kind_.count(k) >= 3 for k in (R.BCE, R.MSE, R.MAE)) and 14 <= len(R.HEAD_CASES) <= 20
    assert R.ceil_div(131, 8) == 17 and R.ceil_div(269, 8) == 34 and R.REDUCE_GROUPS == 16
    assert any((fd + nd + 2) % 32 == 0 for _, fd, nd, _ in R.HEAD_CASES) and any((fd + nd + 2) % 32 == 1 for _, fd, nd, _ in R.HEAD_CASES)
    for case in R.HEAD_CASES:
        d = R.draw_head(case)
        assert float(d["w"][0]) == 1.0 and set(d["y"][0::2].tolist()) <= {0.0, 1.0}
        if case[3] != R.BCE and case[0] > 1:
            assert bool(((d["y"] > 0) & (d["y"] < 1)).any())
        if case[2]:
            cols = d["cols"].long()
            assert d["stride"] >= int(cols.max()) + 4 and len(set(cols.tolist())) == case[2]
            assert case[2] == 1 or not bool((cols[1:] > cols[:-1]).all())
            assert bool((d["dense"] == 7777.0).any())
    names = R.CHAIN_CASES
    assert names["c2_pos_l3_d4"]["L"] > 0 and len(names["c2_pos_l3_d4"]["sizes"]) == 2
    assert {len(c["rows"]) for c in names.values()} == {1, 2, 3, 8}
    for name in names:
        d = R.draw_chain(name)
        E = R.inputs_fwd([t.double() for t in d["tables"]], d["index"], d["S"], d["lay"].double() if d["pos"] else None,
                         d["role"][:2].double() if d["pos"] else None)
        assert bool((E == 0).any()) and bool((E < 0).any()) and E.shape == (d["LR"] * d["S"], d["De"])
    d = R.draw_chain("c2")
    assert d["rows"][0] > 3 and int(d["index"][0].max()) == 2                                     # a table row no scenario names
    assert d["index"].shape == (2, 12) and d["index"][1].tolist() == [0, 1, 2, 3] * 3             # the last column runs fastest
    assert R.draw_chain("c1_pos_l1_d4")["rows"][0] > 3
    for mixed in (False, True):
        d, rows = R.draw_saturated(mixed)
        _, z, _ = R.head_forward(d["a"], d["dense"], d["cols"], d["w"], d["bias"])                # fp32: the rows are exact
        assert d["B"] == (9 if mixed else 12)
        for b, (zb, tb) in rows.items():
            assert float(z[b]) == zb and float(d["y"][b]) == tb
        assert {zb for zb, _ in rows.values()} == set(R.SATURATED_Z)


def test_bounds_are_fatal_to_a_dropped_term():
    """One term of the sum missing is hundreds of bounds away: the head logit at FD = 252 and the last p of a sub-slice of g_emb."""
    d = R.draw_head((7, 252, 2, R.BCE))
    _, z, flat = R.head_forward(d["a"].double(), d["dense"].double(), d["cols"], d["w"].double(), d["bias"].double())
    lb = R.logit_bound(flat, d["w"].double(), d["bias"].double(), 252, 2)
    short = z - flat[:, 100] * d["w"].double()[100]
    assert R.ratio(short, z, lb) > 300
    emb, W, bias, g_tab = R.draw_table((3, 32, 2080))
    want, bound = R.table_reference(emb, W, bias, g_tab)
    short = want["g_emb"] - (g_tab.double()[:, 64:65] @ W.double()[64:65]) * (emb > 0)
    assert R.ratio(short, want["g_emb"], bound["g_emb"]) > 300


# ---- the premise of the GPU bounds -------------------------------------------------------------------------------------------
HALF = 0.5


def _report(tag, worst):
    print(f"[scenario_head] premise {tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    for k, v in worst.items():
        assert v <= HALF, (tag, k, v)


def _upd(worst, key, got, want, bound):
    worst[key] = max(worst.get(key, 0.0), R.ratio(got, want, bound))


def test_premise_of_the_gpu_bounds():
    """On the GPU tests' own seeded inputs torch's fp32 CPU evaluation of the same operations (autograd for the backward)
    stays within half of every bound the kernels are held to; the worst err / bound per quantity is printed."""
    worst = {}
    for case in R.TABLE_CASES:
        emb, W, bias, g_tab = R.draw_table(case)
        want, bound = R.table_reference(emb, W, bias, g_tab)
        e, w, b = (t.clone().requires_grad_(True) for t in (emb, W, bias))
        tab = R.table_fwd(e, w, b)
        (tab * g_tab).sum().backward()
        for k, got in (("tab", tab.detach()), ("g_emb", e.grad), ("g_W", w.grad), ("g_bias", b.grad)):
            _upd(worst, k, got, want[k], bound[k])
        assert bool((e.grad[emb <= 0] == 0).all())
    _report("table", worst)

    worst = {}
    for name in R.CHAIN_CASES:
        d = R.draw_chain(name)
        pos = d["pos"]
        role = d["role"][:2] if pos else None
        want, bound = R.chain_reference(d["tables"], d["index"], d["S"], d["lay"], role, d["W"], d["bias"], d["g_tab"])
        assert R.kink_free(want["E"], bound["E"])
        T = [t.clone().requires_grad_(True) for t in d["tables"]]
        la, ro = (d["lay"].clone().requires_grad_(True), role.clone().requires_grad_(True)) if pos else (None, None)
        w, b = d["W"].clone().requires_grad_(True), d["bias"].clone().requires_grad_(True)
        E = R.inputs_fwd(T, d["index"], d["S"], la, ro)
        E.retain_grad()
        tab = R.table_fwd(E, w, b)
        (tab * d["g_tab"]).sum().backward()
        got = {"E": E.detach(), "tab": tab.detach(), "g_E": E.grad, "g_W": w.grad, "g_bias": b.grad}
        if pos:
            got["g_lay"], got["g_role"] = la.grad, ro.grad
        for k, v in got.items():
            _upd(worst, k, v, want[k], bound[k])
        for c, t in enumerate(T):
            _upd(worst, "g_tables", t.grad if t.grad is not None else torch.zeros_like(t), want["g_tables"][c], bound["g_tables"][c])
        # inputs_bwd alone, on a random g_E
        want1, bound1 = R.inputs_bwd_reference(d["g_E"], d["index"], d["C"], d["S"], d["D"], d["L"], pos, d["rows"])
        T = [torch.zeros_like(t).requires_grad_(True) for t in d["tables"]]
        la, ro = (torch.zeros_like(d["lay"]).requires_grad_(True), torch.zeros_like(role).requires_grad_(True)) if pos else (None, None)
        (R.inputs_fwd(T, d["index"], d["S"], la, ro) * d["g_E"]).sum().backward()
        for c, t in enumerate(T):
            _upd(worst, "alone g_tables", t.grad if t.grad is not None else torch.zeros_like(t), want1["g_tables"][c], bound1["g_tables"][c])
        if pos:
            _upd(worst, "alone g_lay", la.grad, want1["g_lay"], bound1["g_lay"])
            _upd(worst, "alone g_role", ro.grad, want1["g_role"], bound1["g_role"])
    _report("inputs and chain", worst)

    worst = {}
    for case in R.HEAD_CASES:
        d = R.draw_head(case)
        kind, w64, b64 = d["kind"], d["w"].double(), d["bias"].double()
        p64, z64, flat64 = R.head_forward(d["a"].double(), None if d["dense"] is None else d["dense"].double(), d["cols"], w64, b64)
        assert float(z64.abs().max()) <= R.Z_MAX
        lb = R.logit_bound(flat64, w64, b64, d["FD"], d["n_dense"])
        p32, z32, flat32 = R.head_forward(d["a"], d["dense"], d["cols"], d["w"], d["bias"])
        _upd(worst, "logit", z32, z64, lb)
        _upd(worst, "prob", p32, p64, R.prob_bound(lb))
        want, bound = R.head_stage2(p32, d["y"], flat64, w64, kind)
        loss32, dl32 = R.loss_pieces(p32, d["y"], kind)
        loss64, _ = R.loss_pieces(p32.double(), d["y"].double(), kind)
        _upd(worst, f"{R.LOSS_NAMES[kind]} dlogit", dl32, want["dlogit"], bound["dlogit"])
        _upd(worst, f"{R.LOSS_NAMES[kind]} loss", loss32, loss64, R.LOSS_REL * (1 + loss64.abs()))
        _upd(worst, "loss_sum", loss32.sum(), want["loss_sum"], bound["loss_sum"])
        _upd(worst, "g_b", dl32.sum(), want["g_b"], bound["g_b"])
        _upd(worst, "g_w", dl32 @ flat32, want["g_w"], bound["g_w"])
        da = dl32.unsqueeze(1) * d["w"][:d["FD"]]
        _upd(worst, "da", da, dl32.double().unsqueeze(1) * w64[:d["FD"]], 8 * U * (dl32.double().unsqueeze(1) * w64[:d["FD"]]).abs() + 1e-45)
        if kind == R.MAE:
            assert not bool(((p64 - d["y"].double()).abs() <= R.prob_bound(lb)).any())
    _report("head", worst)
