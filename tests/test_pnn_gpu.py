"""satrans_amd.layers.InnerProductLayer, OutterProductLayer and PNNHead (csrc/pnn.hip behind torch.autograd.Function) against the
fp64 restatement tests/pnn_reference.py on the same seeded inputs; that restatement is deepctr's LITERAL form (the gathered
[B, P, D] tensors, the [B, D, P, D] product of 'mat'; the kernels form neither) and is pinned to autograd and to the recorded runs of
the reference's own PNN.forward by tests/test_pnn_cpu.py.

Bounds (the sibling bounds), all element-wise: results within 2e-5 max|.|; gradients within 1e-4 max|g| + 5e-9.
tests/test_pnn_cpu.py::test_premise_of_the_gpu_bounds pins their margin.  Measured on the MI355X over the sweep: at most
1.3e-6 max|.| on results and 1.1e-6 max|g| on gradients; the recorded runs of the reference are reproduced to 2.0e-6."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import pnn_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnn")
check_close = functools.partial(helpers.check_close, "pnn-parity")


def make_head(case, P):
    """A PNNHead of the case's shapes holding P's values."""
    from satrans_amd import PNNHead
    B, Fn, D, use_inner, use_outter, kind, dnn, dense_dim = case
    head = PNNHead(Fn, D, dense_dim, dnn, use_inner, use_outter, kind)
    head.load_state_dict({k: v.clone() for k, v in R.state_from_params(P).items()})
    return head.to(DEV)


def run(head, emb, dense, up):
    """logit, the gradients under the restatement's names (R.flat), the saved buffer - all on the host."""
    head.zero_grad(set_to_none=True)
    eg = emb.to(DEV).requires_grad_(True)
    dg = None if dense is None else dense.to(DEV).requires_grad_(True)
    y = head(eg, dg)
    saved = y.grad_fn.saved_tensors[1]
    (y * up.to(DEV)).sum().backward()
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in head.named_parameters()}, torch.float32))
    g["emb"] = eg.grad.cpu()
    if dg is not None:
        g["dense"] = dg.grad.cpu()
    return y.detach().cpu(), g, saved.cpu()


@functools.lru_cache(maxsize=None)
def drawn(case):
    """The seeded draw of a case and its fp64 logit, gradients and cache: computed once, shared, never written to."""
    emb, dense, up, P = R.sweep_draw(case)
    y, cache = R.forward(emb.double(), None if dense is None else dense.double(), R.double(P), case[3:6])
    return emb, dense, up, P, y, R.flat(R.backward(up.double(), cache)), cache


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_shape_sweep_against_the_restatement(case):
    """The logit, every parameter gradient, demb and ddense over the shapes of R.SWEEP (what each is there for is written
    beside it), and the DNN input the forward leaves in `saved`, block by block: a misplaced ip / op column cannot hide behind
    the linear block's scale."""
    B, Fn, D, use_inner, use_outter, kind, dnn, dense_dim = case
    emb, dense, up, P, want_y, want, cache = drawn(case)
    head = make_head(case, P)
    y, g, saved = run(head, emb, dense, up)
    d = native.PNNDesc()
    d.B, d.F, d.D, d.use_inner, d.use_outer, d.kernel_type = B, Fn, D, use_inner, use_outter, native.PNN_KERNEL_TYPES[kind]
    d.dense_dim, d.n_dnn = dense_dim, len(dnn)
    for l, w in enumerate(dnn):
        d.width[l] = w
    assert y.shape == (B, 1) and saved.numel() == native.lib().satrans_pnn_saved_floats(ctypes.byref(d))
    tag = f"sweep {R.case_id(case)}"
    check_close(y, want_y, 2e-5, tag)
    x = saved[:cache.X.numel()].reshape(cache.X.shape)
    where = R.blocks(Fn, D, case[3:6], dense_dim)
    assert sum(w for _, w in where.values()) == cache.X.shape[1]
    assert ("inner" in where) == bool(use_inner) and ("outer" in where) == bool(use_outter)
    for name, (at, width) in where.items():
        check_close(x[:, at:at + width], cache.X[:, at:at + width], 2e-5, f"{tag} dnn input, {name} block")
    assert sorted(g) == sorted(want)
    for k in want:
        check_close(g[k], want[k], 1e-4, f"{tag} {k}", what="grad", floor=5e-9)


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_layers_alone_against_the_restatement(case):
    """InnerProductLayer and OutterProductLayer as modules of their own (both, whatever the case's head uses): outputs, input
    gradients and dkernel; and cat(flatten(e), ip, op, dense) of the layers gives the head's DNN input."""
    from satrans_amd import InnerProductLayer, OutterProductLayer
    B, Fn, D, use_inner, use_outter, kind, dnn, dense_dim = case
    emb, dense, _, P, _, _, cache = drawn(case)
    tag = f"layers {R.case_id(case)}"
    g = torch.Generator().manual_seed(B + Fn)
    n_pairs = Fn * (Fn - 1) // 2
    up_i, up_o = torch.randn(B, n_pairs, 1, generator=g), torch.randn(B, n_pairs, generator=g)
    kernel = P["kernel"] if use_outter else torch.randn(*R.kernel_shape(Fn, D, kind), generator=g) * D ** -0.5
    # inner, fed deepctr's list of pieces
    x = emb.to(DEV).requires_grad_(True)
    ip = InnerProductLayer()(list(torch.split(x, 1, dim=1)))
    assert ip.shape == (B, n_pairs, 1)
    (ip * up_i.to(DEV)).sum().backward()
    check_close(ip.detach().cpu(), R.inner(emb.double()), 2e-5, f"{tag} inner")
    check_close(x.grad.cpu(), R.inner_backward(up_i[:, :, 0].double(), emb.double()), 1e-4, f"{tag} inner dx", what="grad", floor=5e-9)
    # outer, fed the tensor
    layer = OutterProductLayer(Fn, D, kind)
    layer.load_state_dict({"kernel": kernel.clone()})
    layer = layer.to(DEV)
    x = emb.to(DEV).requires_grad_(True)
    op = layer(x)
    assert op.shape == (B, n_pairs)
    (op * up_o.to(DEV)).sum().backward()
    want_dx, want_dk = R.outer_backward(up_o.double(), emb.double(), kernel.double(), kind)
    check_close(op.detach().cpu(), R.outer(emb.double(), kernel.double(), kind), 2e-5, f"{tag} outer")
    check_close(x.grad.cpu(), want_dx, 1e-4, f"{tag} outer dx", what="grad", floor=5e-9)
    check_close(layer.kernel.grad.cpu(), want_dk, 1e-4, f"{tag} outer dkernel", what="grad", floor=5e-9)
    # composed: the head's DNN input
    parts = [emb.flatten(1)] + ([ip.detach().cpu().flatten(1)] if use_inner else []) + ([op.detach().cpu()] if use_outter else [])
    both = torch.cat(parts + ([] if dense is None else [dense]), dim=1)
    assert both.shape == cache.X.shape
    for name, (at, width) in R.blocks(Fn, D, case[3:6], dense_dim).items():
        check_close(both[:, at:at + width], cache.X[:, at:at + width], 2e-5, f"{tag} composed, {name} block")
    if use_inner and use_outter:      # the same bits as the head's own DNN input
        saved = run(make_head(case, P), emb, dense, torch.ones(B, 1))[2]
        assert torch.equal(saved[:both.numel()].reshape(both.shape)[:, :Fn * D], both[:, :Fn * D])
        if kind == "mat":
            assert torch.equal(saved[:both.numel()].reshape(both.shape), both)


@pytest.mark.parametrize("case", R.ALONE, ids=R.case_id)
def test_a_sample_alone_equals_the_batch_bit_for_bit(case):
    """A sample alone (B = 1) == the same sample inside the batch: its logit and its demb row.  Samples from the first, a
    middle and the last row tile and chunk; and a slice of the batch, which moves every sample to another place of its tile."""
    B = case[0]
    emb, dense, up, P = drawn(case)[:4]
    head = make_head(case, P)
    y, g, _ = run(head, emb, dense, up)
    assert float(g["emb"].abs().max()) > 0.0
    for b in (0, 1, B // 2, B - 1):
        y1, g1, _ = run(head, emb[b:b + 1], None if dense is None else dense[b:b + 1], up[b:b + 1])
        assert torch.equal(y1[0], y[b]), b
        assert torch.equal(g1["emb"][0], g["emb"][b]), b
    lo = B // 3
    y2, g2, _ = run(head, emb[lo:], None if dense is None else dense[lo:], up[lo:])
    assert torch.equal(y2, y[lo:]) and torch.equal(g2["emb"], g["emb"][lo:])


@pytest.mark.parametrize("case", R.TWICE, ids=R.case_id)
def test_two_runs_agree_bit_for_bit(case):
    emb, dense, up, P = drawn(case)[:4]
    (y0, g0, s0), (y1, g1, s1) = (run(make_head(case, P), emb, dense, up) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(s0, s1) and float(s0.abs().max()) > 0.0
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]) and float(g0[k].abs().max()) > 0.0, k


@pytest.mark.parametrize("name", R.FIXTURES)
def test_reference_fixtures_on_the_gpu(name):
    """The reference's own recorded PNN run: its parameters, emb and dense in; sigmoid(logit), the summed BCE, every parameter
    gradient, grad/emb and the regularisation loss out.  Both sides are fp32 runs of contractions at most 29 long: the
    fixtures' bound 2e-5 max|.| of tests/test_pnn_cpu.py."""
    from satrans_amd import PNNHead
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    use_inner, use_outter, kind = R.FIXTURE_CONFIG[name]
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    emb, dense, labels = (torch.from_numpy(fx[k]) for k in ("emb", "dense", "labels"))
    head = PNNHead(emb.shape[1], emb.shape[2], dense.shape[1], (16, 8), use_inner, use_outter, kind, l2_reg_dnn=float(fx["l2_reg_dnn"]))
    assert list(head.state_dict()) == list(fx["keys"])
    head.load_state_dict(state)
    head = head.to(DEV)
    eg = emb.to(DEV).requires_grad_(True)
    y = torch.sigmoid(head(eg, dense.to(DEV)))
    loss = F.binary_cross_entropy(y.squeeze(1), labels.to(DEV), reduction='sum')
    loss.backward()
    check_close(y.detach().cpu(), torch.from_numpy(fx["y_pred"]), 2e-5, f"fixture {name}", what="fixture y")
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    for k, p in head.named_parameters():
        check_close(p.grad.cpu(), torch.from_numpy(fx[f"grad/{k}"]), 2e-5, f"fixture {name} {k}", what="fixture grad")
    check_close(eg.grad.cpu(), torch.from_numpy(fx["grad/emb"]), 2e-5, f"fixture {name} emb", what="fixture grad")
    reg = head.regularization_loss()
    assert reg.shape == (1,) and float(fx["reg_loss"][0]) > 0.0
    check_close(reg.detach().cpu(), torch.from_numpy(fx["reg_loss"]), 1e-6, f"fixture {name} reg_loss", what="fixture reg")


def test_errors_and_odd_inputs():
    from satrans_amd import InnerProductLayer, OutterProductLayer, PNNHead
    x = torch.randn(6, 4, 8)
    head = PNNHead(4, 8, 0, (16,), True, True, 'mat', init_std=0.3).to(DEV)
    assert head(x.to(DEV)).shape == (6, 1)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        PNNHead(4, 8)(x)                                  # a CPU tensor
    with pytest.raises(TypeError, match="float32"):
        head(x.to(DEV).double())
    with pytest.raises(ValueError):
        head(x[:, :3].to(DEV))                            # wrong emb shape
    with pytest.raises(ValueError):
        head(x.to(DEV), torch.randn(6, 1, device=DEV))    # dense columns unexpected
    with pytest.raises(ValueError):
        PNNHead(4, 8, 2).to(DEV)(x.to(DEV), torch.randn(6, 3, device=DEV))      # wrong dense width
    with pytest.raises(NotImplementedError, match="PNN_MAX_DIM"):
        InnerProductLayer()(torch.randn(2, 4, native.PNN_MAX_DIM + 1, device=DEV))
    xt = x.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)      # a non-contiguous input is handled: made contiguous
    assert not xt.is_contiguous()
    for mod in (head, InnerProductLayer(), OutterProductLayer(4, 8, 'vec').to(DEV)):
        assert torch.equal(mod(xt), mod(x.to(DEV)))


def test_metatransformation_feeds_the_head():
    """The reference's `metatrans` flag: MetaTransformation -> PNNHead; one backward reaches the scenario embeddings, the
    embedding block, the outer product's kernel and the DNN."""
    from satrans_amd import MetaTransformation, PNNHead
    B, M, D, S = 40, 5, 16, 3      # (the MetaNet kernels take D in {16, 32, 64, 128})
    torch.manual_seed(6)
    meta = MetaTransformation(D, S, (D, 16, D), init_std=0.3).to(DEV)
    head = PNNHead(M, D, 2, (16, 8), True, True, 'mat', init_std=0.3).to(DEV)
    g = torch.Generator().manual_seed(9)
    emb = (torch.randn(B, M, D, generator=g) + 0.5).to(DEV).requires_grad_(True)
    dense = torch.randn(B, 2, generator=g).to(DEV)
    ids = torch.randint(0, S + 1, (B,), generator=g).to(DEV)
    target = (torch.rand(B, generator=g) > 0.5).float().to(DEV)
    logit = head(meta(ids, emb), dense)
    assert logit.shape == (B, 1)
    F.binary_cross_entropy(torch.sigmoid(logit.squeeze(1)), target, reduction='sum').backward()
    for name, t in (("domain_embeddings.weight", meta.domain_embeddings.weight.grad), ("emb", emb.grad),
                    ("outterproduct.kernel", head.outterproduct.kernel.grad),
                    ("dnn.linears.0.weight", head.dnn.linears[0].weight.grad)):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0.0, name
