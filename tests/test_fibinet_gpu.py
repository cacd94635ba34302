"""satrans_amd.layers.SENETLayer, BilinearInteraction and FiBiNETHead (csrc/fibinet.hip behind torch.autograd.Function) against the
fp64 restatement tests/fibinet_reference.py on the same seeded inputs; that restatement is deepctr's LITERAL form (the kernels use
the factored a_i a_j (W e_i * e_j)) and is pinned to autograd and to the recorded runs of the reference's own FiBiNET.forward by
tests/test_fibinet_cpu.py.

Bounds (the sibling bounds), all element-wise: results within 2e-5 max|.|; gradients within 1e-4 max|g| + 5e-9.
tests/test_fibinet_cpu.py::test_premise_of_the_gpu_bounds pins their margin.  Measured on the MI355X over the sweep: at most
3.3e-6 max|.| on results and 2.6e-6 max|g| on gradients; the recorded runs of the reference are reproduced to 3.4e-6."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import fibinet_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fibinet")
check_close = functools.partial(helpers.check_close, "fibinet-parity")


def make_head(case, P):
    """A FiBiNETHead of the case's shapes holding P's values."""
    from satrans_amd import FiBiNETHead
    B, Fn, D, kind, ratio, dnn, dense_dim = case
    head = FiBiNETHead(Fn, D, dense_dim, kind, ratio, dnn)
    head.load_state_dict({k: v.clone() for k, v in R.state_from_params(P, Fn, kind).items()})
    return head.to(DEV)


def run(head, case, emb, dense, up):
    """logit, the gradients under the restatement's names (R.flat), the saved buffer - all on the host."""
    Fn, kind = case[1], case[3]
    head.zero_grad(set_to_none=True)
    eg = emb.to(DEV).requires_grad_(True)
    dg = None if dense is None else dense.to(DEV).requires_grad_(True)
    y = head(eg, dg)
    saved = y.grad_fn.saved_tensors[1]
    (y * up.to(DEV)).sum().backward()
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in head.named_parameters()}, Fn, kind, torch.float32))
    g["emb"] = eg.grad.cpu()
    if dg is not None:
        g["dense"] = dg.grad.cpu()
    return y.detach().cpu(), g, saved.cpu()


@functools.lru_cache(maxsize=None)
def drawn(case):
    """The seeded draw of a case and its fp64 logit, gradients and cache: computed once, shared, never written to."""
    emb, dense, up, P = R.sweep_draw(case)
    y, cache = R.forward(emb.double(), None if dense is None else dense.double(), R.double(P), case[3])
    return emb, dense, up, P, y, R.flat(R.backward(up.double(), cache)), cache


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_shape_sweep_against_the_restatement(case):
    """The logit, every parameter gradient, demb and ddense over the shapes of R.SWEEP (what each is there for is written
    beside it), and the DNN input the forward leaves in `saved`."""
    B, Fn, D, kind, ratio, dnn, dense_dim = case
    emb, dense, up, P, want_y, want, cache = drawn(case)
    head = make_head(case, P)
    y, g, saved = run(head, case, emb, dense, up)
    d = native.FiBiNETDesc()
    d.B, d.F, d.D, d.type, d.R, d.dense_dim, d.n_dnn = B, Fn, D, native.BILINEAR_TYPES[kind], max(1, Fn // ratio), dense_dim, len(dnn)
    for l, w in enumerate(dnn):
        d.width[l] = w
    assert y.shape == (B, 1) and saved.numel() == native.lib().satrans_fibinet_saved_floats(ctypes.byref(d))
    tag = f"sweep {R.case_id(case)}"
    check_close(y, want_y, 2e-5, tag)
    R_ = max(1, Fn // ratio)
    x0 = -(-(B * (Fn + R_)) // 4) * 4
    check_close(saved[:B * Fn].reshape(B, Fn), R.gates(cache), 2e-5, f"{tag} gates")
    check_close(saved[x0:x0 + cache.X.numel()].reshape(cache.X.shape), cache.X, 2e-5, f"{tag} dnn input")
    assert sorted(g) == sorted(want)
    for k in want:
        check_close(g[k], want[k], 1e-4, f"{tag} {k}", what="grad", floor=5e-9)
    if kind == "each":
        assert float(g["bil"][Fn - 1].abs().max()) == 0.0      # the unused weight: a zero gradient


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_layers_alone_against_the_restatement(case):
    """SENETLayer and BilinearInteraction as modules of their own: outputs, input gradients and parameter gradients; and
    BilinearInteraction(SENETLayer(x)) beside BilinearInteraction(x) gives the head's DNN input."""
    from satrans_amd import BilinearInteraction, SENETLayer
    B, Fn, D, kind, ratio, dnn, dense_dim = case
    emb, dense, _, P, _, _, cache = drawn(case)
    tag = f"layers {R.case_id(case)}"
    g = torch.Generator().manual_seed(B + Fn)
    n_pairs = Fn * (Fn - 1) // 2
    up_v, up_o = torch.randn(B, Fn, D, generator=g), torch.randn(B, n_pairs, D, generator=g)
    se = SENETLayer(Fn, ratio)
    se.load_state_dict({"excitation.0.weight": P["w1"].clone(), "excitation.2.weight": P["w2"].clone()})
    bi = BilinearInteraction(Fn, D, kind)
    bi.load_state_dict({k: P["bil"][i].clone() for i, k in enumerate(R.bilinear_keys(Fn, kind, ""))})
    se, bi = se.to(DEV), bi.to(DEV)
    Pd = R.double(P)
    # SENet
    x = emb.to(DEV).requires_grad_(True)
    v = se(x)
    (v * up_v.to(DEV)).sum().backward()
    want_v, mid = R.senet(emb.double(), Pd["w1"], Pd["w2"])
    want_dx, want_dw1, want_dw2 = R.senet_backward(up_v.double(), emb.double(), Pd["w1"], Pd["w2"], mid)
    check_close(v.detach().cpu(), want_v, 2e-5, f"{tag} senet")
    check_close(x.grad.cpu(), want_dx, 1e-4, f"{tag} senet dx", what="grad", floor=5e-9)
    check_close(se.excitation[0].weight.grad.cpu(), want_dw1, 1e-4, f"{tag} senet dw1", what="grad", floor=5e-9)
    check_close(se.excitation[2].weight.grad.cpu(), want_dw2, 1e-4, f"{tag} senet dw2", what="grad", floor=5e-9)
    # bilinear
    x = emb.to(DEV).requires_grad_(True)
    out = bi(x)
    (out * up_o.to(DEV)).sum().backward()
    want_dx, want_dw = R.bilinear_backward(up_o.double(), emb.double(), Pd["bil"], kind)
    check_close(out.detach().cpu(), R.bilinear(emb.double(), Pd["bil"], kind), 2e-5, f"{tag} bilinear")
    check_close(x.grad.cpu(), want_dx, 1e-4, f"{tag} bilinear dx", what="grad", floor=5e-9)
    got_dw = torch.stack([w.grad.cpu() for w in bi.weights()])
    check_close(got_dw, want_dw, 1e-4, f"{tag} bilinear dw", what="grad", floor=5e-9)
    # composed: the head's DNN input
    with torch.no_grad():
        both = torch.cat((bi(se(x)), out), dim=1).flatten(1).cpu()
    check_close(both, cache.X[:, :2 * n_pairs * D], 2e-5, f"{tag} composed")


@pytest.mark.parametrize("case", R.ALONE, ids=R.case_id)
def test_a_sample_alone_equals_the_batch_bit_for_bit(case):
    """A sample alone (B = 1) == the same sample inside the batch: its logit and its demb row.  Samples from the first, a
    middle and the last row tile and chunk; and a slice of the batch, which moves every sample to another place of its tile."""
    B = case[0]
    emb, dense, up, P = drawn(case)[:4]
    head = make_head(case, P)
    y, g, _ = run(head, case, emb, dense, up)
    assert float(g["emb"].abs().max()) > 0.0
    for b in (0, 1, B // 2, B - 1):
        y1, g1, _ = run(head, case, emb[b:b + 1], None if dense is None else dense[b:b + 1], up[b:b + 1])
        assert torch.equal(y1[0], y[b]), b
        assert torch.equal(g1["emb"][0], g["emb"][b]), b
    lo = B // 3
    y2, g2, _ = run(head, case, emb[lo:], None if dense is None else dense[lo:], up[lo:])
    assert torch.equal(y2, y[lo:]) and torch.equal(g2["emb"], g["emb"][lo:])


@pytest.mark.parametrize("case", (R.SWEEP[2], R.SWEEP[4]), ids=R.case_id)
def test_two_runs_agree_bit_for_bit(case):
    emb, dense, up, P = drawn(case)[:4]
    (y0, g0, s0), (y1, g1, s1) = (run(make_head(case, P), case, emb, dense, up) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(s0, s1) and float(s0.abs().max()) > 0.0
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]) and float(g0[k].abs().max()) > 0.0, k


@pytest.mark.parametrize("name", R.TYPES)
def test_reference_fixtures_on_the_gpu(name):
    """The reference's own recorded FiBiNET run: its parameters, emb, dense and linear_logit in; sigmoid(logit), the summed BCE,
    every parameter gradient, grad/emb and the regularisation loss out.  Both sides are fp32 runs of contractions at most 49
    long: the fixtures' bound 2e-5 max|.| of tests/test_fibinet_cpu.py."""
    from satrans_amd import FiBiNETHead
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    emb, dense, lin, labels = (torch.from_numpy(fx[k]) for k in ("emb", "dense", "linear_logit", "labels"))
    head = FiBiNETHead(emb.shape[1], emb.shape[2], dense.shape[1], str(fx["bilinear_type"]), 3, (16, 8))
    assert list(head.state_dict()) == list(fx["keys"])
    head.load_state_dict(state)
    head = head.to(DEV)
    eg = emb.to(DEV).requires_grad_(True)
    y = torch.sigmoid(head(eg, dense.to(DEV), lin.to(DEV)))
    loss = F.binary_cross_entropy(y.squeeze(1), labels.to(DEV), reduction='sum')
    loss.backward()
    check_close(y.detach().cpu(), torch.from_numpy(fx["y_pred"]), 2e-5, f"fixture {name}")
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    for k, p in head.named_parameters():
        check_close(p.grad.cpu(), torch.from_numpy(fx[f"grad/{k}"]), 2e-5, f"fixture {name} {k}", what="fixture grad")
    check_close(eg.grad.cpu(), torch.from_numpy(fx["grad/emb"]), 2e-5, f"fixture {name} emb", what="fixture grad")
    reg = head.regularization_loss()
    assert reg.shape == (1,) and torch.equal(reg.detach().cpu(), torch.from_numpy(fx["reg_loss"]))


def test_errors_and_odd_inputs():
    from satrans_amd import BilinearInteraction, FiBiNETHead, SENETLayer
    x = torch.randn(6, 4, 8)
    head = FiBiNETHead(4, 8, 0, 'each', 2, (16,), init_std=0.3).to(DEV)
    assert head(x.to(DEV)).shape == (6, 1)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        FiBiNETHead(4, 8)(x)
    with pytest.raises(TypeError, match="float32"):
        head(x.to(DEV).double())
    with pytest.raises(ValueError):
        head(x[:, :3].to(DEV))
    with pytest.raises(NotImplementedError, match="FIBINET_MAX_DIM"):
        SENETLayer(4).to(DEV)(torch.randn(2, 4, native.FIBINET_MAX_DIM + 1, device=DEV))
    xt = x.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)      # a non-contiguous input is made contiguous
    assert not xt.is_contiguous()
    for mod in (head, SENETLayer(4).to(DEV), BilinearInteraction(4, 8, 'all').to(DEV)):
        assert torch.equal(mod(xt), mod(x.to(DEV)))
    lin = torch.randn(6, 1, device=DEV)
    assert torch.equal(head(x.to(DEV), None, lin), lin + head(x.to(DEV)))


def test_metatransformation_feeds_the_head():
    """The reference's `metatrans` flag: MetaTransformation -> FiBiNETHead; one backward reaches the scenario embeddings, the
    embedding block, the excitation and the bilinear weights."""
    from satrans_amd import FiBiNETHead, MetaTransformation
    B, M, D, S = 40, 5, 16, 3      # (the MetaNet kernels take D in {16, 32, 64, 128})
    torch.manual_seed(6)
    meta = MetaTransformation(D, S, (D, 16, D), init_std=0.3).to(DEV)
    head = FiBiNETHead(M, D, 2, 'interaction', 2, (16, 8), init_std=0.3)
    with torch.no_grad():
        for w in (head.SE.excitation[0].weight, head.SE.excitation[2].weight):
            w.abs_()      # open gates
    head = head.to(DEV)
    g = torch.Generator().manual_seed(9)
    emb = (torch.randn(B, M, D, generator=g) + 0.5).to(DEV).requires_grad_(True)
    dense, lin = torch.randn(B, 2, generator=g).to(DEV), torch.randn(B, 1, generator=g).to(DEV)
    ids = torch.randint(0, S + 1, (B,), generator=g).to(DEV)
    target = (torch.rand(B, generator=g) > 0.5).float().to(DEV)
    logit = head(meta(ids, emb), dense, lin)
    assert logit.shape == (B, 1)
    F.binary_cross_entropy(torch.sigmoid(logit.squeeze(1)), target, reduction='sum').backward()
    for name, t in (("domain_embeddings.weight", meta.domain_embeddings.weight.grad), ("emb", emb.grad),
                    ("SE.excitation.0.weight", head.SE.excitation[0].weight.grad),
                    ("Bilinear.bilinear.0.weight", head.Bilinear.bilinear[0].weight.grad),
                    ("dnn.linears.0.weight", head.dnn.linears[0].weight.grad)):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0.0, name
