"""satrans_amd.layers.AdaSparseHead and PrunedDNN (csrc/adasparse.hip behind torch.autograd.Function) against the fp64
restatement tests/adasparse_reference.py on the same seeded inputs; that restatement is pinned to the reference's own
AdaSparse.forward by the recorded runs of tests/test_adasparse_cpu.py.

Bounds (the sibling bounds), all element-wise: logits and saved factors within 2e-5 max|.|; gradients within
1e-4 max|g| + 5e-9.  tests/test_adasparse_cpu.py::test_premise_of_the_gpu_bounds pins their margin.  R.draw keeps every unit
of the fp64 forward further than the output bound from relu's kink and from the pruning threshold."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import adasparse_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, CHUNK = native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adasparse")
check_close = functools.partial(helpers.check_close, "adasparse-parity")


def make_head(C, E, P, consts=R.DEFAULTS):
    """An AdaSparseHead of the shapes of P holding its values."""
    from satrans_amd import AdaSparseHead
    mod = AdaSparseHead(C, tuple(w.shape[0] for w in P["lin_w"]), domain_emb_dim=E)
    mod.load_state_dict({k: v.clone() for k, v in R.state_from_params(P).items()})
    mod.dnn.alpha, mod.dnn.beta, mod.dnn.epsilon = consts
    return mod.to(DEV)


def run(mod, x, e, w):
    """logit, {gradients keyed as R.flat keys them, "x", "emb"}, the pruned factors - all on the host."""
    mod.zero_grad(set_to_none=True)
    xg, eg = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    y = mod(xg, eg)
    (y * w.to(DEV)).sum().backward()
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in mod.named_parameters()}, len(mod.dnn.hidden_units), dtype=torch.float32))
    g["x"], g["emb"] = xg.grad.cpu(), eg.grad.cpu()
    return y.detach().cpu(), g, [p.cpu() for p in mod.last_pi]


def run_ref(x, e, P, w, consts=R.DEFAULTS):
    y, cache = R.forward(x.double(), e.double(), R.double(P), consts)
    return y, cache, R.flat(R.backward(w.double(), cache))


def check_all(got, ref, msg):
    (y, g, pis), (y_ref, cache, g_ref) = got, ref
    assert y.shape == (y_ref.shape[0], 1)
    check_close(y, y_ref, 2e-5, msg)
    assert len(pis) == len(cache.pis)
    for l, (pi, want) in enumerate(zip(pis, cache.pis)):
        assert pi.shape == want.shape
        assert torch.equal(pi == 0, want == 0), f"{msg}: layer {l} prunes other units"
        check_close(pi, want, 2e-5, msg, f"pi[{l}]")
    assert sorted(g) == sorted(g_ref)
    for k in g_ref:
        check_close(g[k], g_ref[k], 1e-4, f"{msg} {k}", what="grad", floor=5e-9)


@pytest.mark.parametrize("case", R.SWEEP, ids=lambda c: f"C{c[0]}-E{c[1]}")
def test_shape_sweep_against_the_restatement(case):
    """(C, E) = (1, 1); (33, 4): the x / embedding seam inside a contraction step; (64, 32): the seam on a step's edge and a
    whole embedding-only step; (609, 32).  One to three layers, widths off the 64-column tile, B one row past a weight-gradient
    chunk plus a row tile.  Logit, pruned factors (the same units cut), dx, demb, every parameter gradient."""
    C, E, _ = case
    x, e, w, P = R.sweep_draw(case, CHUNK + TILE + 1)
    check_all(run(make_head(C, E, P), x, e, w), run_ref(x, e, P, w), f"sweep {case}")


def test_batch_smaller_than_a_tile():
    B, C, E = 5, 20, 6
    x, e, w, P = R.draw(B, C, E, (24, 8), 5)
    check_all(run(make_head(C, E, P), x, e, w), run_ref(x, e, P, w), "B < tile")


def test_many_tiles_and_chunks():
    B, C, E = 3 * CHUNK + 7, 100, 12
    x, e, w, P = R.draw(B, C, E, (80, 40), 77)
    check_all(run(make_head(C, E, P), x, e, w), run_ref(x, e, P, w), "many tiles")


def test_everything_pruned_in_the_last_layer():
    """Pruner bias -20 in the last layer: the logit equals out.bias exactly and every gradient but out.bias's is exactly zero."""
    B, C, E = 70, 33, 4
    x, e, w, P = R.draw(B, C, E, (48, 32), 21, tweak=lambda P: P["prn_b"][1].fill_(-20.0))
    y, g, pis = run(make_head(C, E, P), x, e, w)
    assert float(pis[1].abs().max()) == 0.0 and float(pis[0].abs().max()) > 0.0
    assert torch.equal(y, P["out_bias"].expand(B, 1))
    for k, t in g.items():
        if k == "out_bias":
            check_close(t, w.double().sum().reshape(1), 1e-4, "all pruned out_bias", what="grad", floor=5e-9)
        else:
            assert float(t.abs().max()) == 0.0, k


def test_nothing_pruned():
    """Pruner bias +20 everywhere: every factor is beta up to rounding, and parity holds as in the sweep."""
    B, C, E = 70, 33, 4
    x, e, w, P = R.draw(B, C, E, (48, 32), 22, tweak=lambda P: [b.fill_(20.0) for b in P["prn_b"]])
    ref = run_ref(x, e, P, w)
    assert all(bool((pi != 0).all()) for pi in ref[1].pis)
    check_all(run(make_head(C, E, P), x, e, w), ref, "nothing pruned")


def test_one_column_pruned_for_all_rows():
    """Unit 7 of layer 0 pruned for every row: its row of linears.0.weight.grad and pruners.0.weight.grad and both bias entries
    are exactly zero; its neighbours' are not."""
    B, C, E = 130, 33, 4
    x, e, w, P = R.draw(B, C, E, (48, 32), 23, tweak=lambda P: P["prn_b"][0][7].fill_(-20.0))
    ref = run_ref(x, e, P, w)
    got = run(make_head(C, E, P), x, e, w)
    check_all(got, ref, "one column pruned")
    g = got[1]
    assert float(got[2][0][:, 7].abs().max()) == 0.0
    for k in ("lin_w[0]", "prn_w[0]", "lin_b[0]", "prn_b[0]"):
        assert float(g[k][7].abs().max()) == 0.0, k
        assert float(g[k][6].abs().max()) > 0.0 and float(g[k][8].abs().max()) > 0.0, k


def test_non_default_constants():
    consts = (0.5, 1.5, 0.4)
    B, C, E = 130, 33, 4
    x, e, w, P = R.draw(B, C, E, (48, 32), 24, consts=consts)
    check_all(run(make_head(C, E, P, consts), x, e, w), run_ref(x, e, P, w, consts), "scaled constants")


@pytest.mark.parametrize("name", ["plain", "one_layer", "scaled"])
def test_reference_fixtures_on_the_gpu(name):
    """The reference's own recorded AdaSparse run: its parameters, dnn_input and domain_emb in, sigmoid(logit) and the gradients
    of the summed BCE out, against what it recorded (an fp32 run: the bounds above, both sides fp32)."""
    from satrans_amd import AdaSparseHead
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    x, e = torch.from_numpy(fx["dnn_input"]), torch.from_numpy(fx["domain_emb"])
    L = sum(k.startswith("dnn.linears.") and k.endswith(".weight") for k in state)
    widths = tuple(state[f"dnn.linears.{l}.weight"].shape[0] for l in range(L))
    head = AdaSparseHead(x.shape[1], widths, domain_emb_dim=e.shape[1])
    head.load_state_dict(state)
    head.dnn.alpha, head.dnn.beta, head.dnn.epsilon = (float(v) for v in fx["consts"])
    head = head.to(DEV)
    xg, eg = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    y = torch.sigmoid(head(xg, eg))
    F.binary_cross_entropy(y.squeeze(1), torch.from_numpy(fx["labels"]).to(DEV), reduction='sum').backward()
    check_close(y.detach().cpu(), torch.from_numpy(fx["y_pred"]), 2e-5, f"fixture {name}")
    for k, p in head.named_parameters():
        check_close(p.grad.cpu(), torch.from_numpy(fx[f"grad/{k}"]), 1e-4, f"fixture {name} {k}", what="grad", floor=5e-9)
    check_close(xg.grad.cpu(), torch.from_numpy(fx["grad/dnn_input"]), 1e-4, f"fixture {name} dnn_input", what="grad", floor=5e-9)
    lo, hi = (int(v) for v in fx["dom_cols"])
    table = torch.zeros(fx["grad/domain_table"].shape, dtype=torch.float64)
    table.index_add_(0, torch.from_numpy(fx["dom_ids"]), (xg.grad[:, lo:hi] + eg.grad).cpu().double())
    check_close(table, torch.from_numpy(fx["grad/domain_table"]), 1e-4, f"fixture {name} domain table", what="grad", floor=5e-9)


def test_domain_emb_gathered_from_a_table():
    """domain_emb = table[ids] with the table requiring grad, S = 3 rows shared by all the batch's rows: autograd scatters demb
    back, and the table's gradient matches the restatement's demb summed per id."""
    B, C, E, S = 200, 33, 4, 3
    ids = torch.arange(B) % S
    x, e, w, P = R.draw(B, C, E, (48, 32), 25, emb_of=lambda emb: emb[:S][ids])
    assert torch.equal(e, e[:S][ids])
    table = e[:S].clone().to(DEV).requires_grad_(True)
    y = make_head(C, E, P)(x.to(DEV), table[ids.to(DEV)])
    (y * w.to(DEV)).sum().backward()
    y_ref, _, g_ref = run_ref(x, e, P, w)
    check_close(y.detach().cpu(), y_ref, 2e-5, "gathered table")
    want = torch.zeros(S, E, dtype=torch.float64).index_add_(0, ids, g_ref["emb"])
    check_close(table.grad.cpu(), want, 1e-4, "gathered table", what="grad", floor=5e-9)


def test_rows_alone_equal_rows_in_the_batch_bit_for_bit():
    C, E = 64, 32
    B = CHUNK + TILE + 1
    x, e, w, P = R.draw(B, C, E, (80, 24, 24), 26)
    rows = torch.arange(B)[torch.randperm(B, generator=torch.Generator().manual_seed(1))[:TILE + 9]].sort().values
    y_m, g_m, _ = run(make_head(C, E, P), x, e, w)
    y_a, g_a, _ = run(make_head(C, E, P), x[rows], e[rows], w[rows])
    assert torch.equal(y_a, y_m[rows])
    assert torch.equal(g_a["x"], g_m["x"][rows]) and torch.equal(g_a["emb"], g_m["emb"][rows])
    assert float(g_a["emb"].abs().max()) > 0.0


def test_two_runs_agree_bit_for_bit():
    C, E = 100, 12
    x, e, w, P = R.draw(CHUNK + TILE + 1, C, E, (80, 24), 11)
    (y0, g0, p0), (y1, g1, p1) = (run(make_head(C, E, P), x, e, w) for _ in range(2))
    assert torch.equal(y0, y1) and all(torch.equal(a, b) for a, b in zip(p0, p1))
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_pruned_dnn_alone():
    """PrunedDNN without the logit layer: h_L, last_pi, and the gradients of an arbitrary upstream [B, n_L]."""
    from satrans_amd import PrunedDNN
    B, C, E, widths = 130, 33, 4, (48, 32)
    x, e, _, P = R.draw(B, C, E, widths, 27)
    up = torch.randn(B, widths[-1], generator=torch.Generator().manual_seed(3))
    dnn = PrunedDNN(C, widths, domain_emb_dim=E)
    dnn.load_state_dict({k[len("dnn."):]: v.clone() for k, v in R.state_from_params(P).items() if k.startswith("dnn.")})
    dnn = dnn.to(DEV)
    xg, eg = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    h = dnn(xg, eg)
    (h * up.to(DEV)).sum().backward()
    h_ref, cache = R.forward(x.double(), e.double(), R.double(P), head=False)
    g_ref = R.flat(R.backward(up.double(), cache, head=False))
    assert h.shape == (B, widths[-1])
    check_close(h.detach().cpu(), h_ref, 2e-5, "PrunedDNN")
    for l, pi in enumerate(dnn.last_pi):
        assert torch.equal(pi.cpu() == 0, cache.pis[l] == 0)
        check_close(pi.cpu(), cache.pis[l], 2e-5, "PrunedDNN", f"pi[{l}]")
    sd = {"dnn." + k: p.grad.cpu() for k, p in dnn.named_parameters()}
    sd.update({"dnn_linear.weight": torch.zeros(1, widths[-1]), "out.bias": torch.zeros(1)})
    g = R.flat(R.params_from_state(sd, len(widths), dtype=torch.float32))
    g["x"], g["emb"] = xg.grad.cpu(), eg.grad.cpu()
    assert sorted(g_ref) == sorted(k for k in g if k not in R.SINGLES)
    for k in g_ref:
        check_close(g[k], g_ref[k], 1e-4, f"PrunedDNN {k}", what="grad", floor=5e-9)


def test_errors():
    from satrans_amd import AdaSparseHead
    B, C, E = 37, 20, 6
    x, e, w, P = R.draw(B, C, E, (16, 8), 9)
    head = make_head(C, E, P)
    head(x.to(DEV), e.to(DEV))
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        AdaSparseHead(C, (16, 8), domain_emb_dim=E)(x, e)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        head(x.to(DEV), e)
    with pytest.raises(TypeError, match="float32"):
        head(x.to(DEV).double(), e.to(DEV))
    with pytest.raises(TypeError, match="float32"):
        head(x.to(DEV), e.to(DEV).double())
    with pytest.raises(ValueError):
        head(x[:, :5].to(DEV), e.to(DEV))                 # wrong C
    with pytest.raises(ValueError):
        head(x.to(DEV), e[:, :5].to(DEV))                 # wrong E
    with pytest.raises(ValueError):
        head(x.to(DEV), e[:-1].to(DEV))                   # B mismatch
    with pytest.raises(ValueError):
        head(x.to(DEV), e[:, 0].to(DEV))                  # not [B, E]
    head.dnn.beta = 0.0
    with pytest.raises(ValueError, match="beta"):
        head(x.to(DEV), e.to(DEV))


def test_training_lowers_the_loss():
    """Twenty Adam steps on a fixed batch lower the summed BCE."""
    B, C, E = 256, 33, 4
    x, e, _, P = R.draw(B, C, E, (48, 32), 31)
    target = (torch.rand(B, generator=torch.Generator().manual_seed(5)) > 0.5).float().to(DEV)
    head = make_head(C, E, P)
    opt = torch.optim.Adam(head.parameters(), lr=1e-2)
    xd, ed = x.to(DEV), e.to(DEV)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = F.binary_cross_entropy_with_logits(head(xd, ed).squeeze(1), target, reduction='sum')
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print(f"[adasparse] training: summed BCE {losses[0]:.3f} -> {losses[-1]:.3f}")
    assert losses[-1] < losses[0]
