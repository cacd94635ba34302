"""satrans_amd.layers.FM, BiInteractionPooling, AFMLayer, DeepFMHead, NFMHead and AFMHead (csrc/fm.hip behind
torch.autograd.Function) against the fp64 restatement tests/fm_reference.py on the same seeded inputs; that restatement is
deepctr's LITERAL form (the gathered [B, P, D] tensors, tensordot, softmax over dim 1; the kernels form none of them) and is
pinned to autograd and to the recorded runs of the reference's own DeepFM, NFM and AFM forward by tests/test_fm_cpu.py.

Bounds (the sibling bounds), all element-wise: results, the saved DNN input and normalized_att_score within 2e-5
max|.|; gradients within 1e-4 max|g| + 5e-9.  tests/test_fm_cpu.py::test_premise_of_the_gpu_bounds pins their margin.
Measured on the MI355X over the sweeps: at most 5.9e-7 max|.| on results (the attention output at B131-F19-D32-A8) and 1.7e-6
max|g| on gradients (d projection_h at B9-F64-D8-A4); the recorded runs of the reference are reproduced to 7.1e-7."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from satrans_amd import native
from tests import fm_reference as R
from tests import helpers

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fm")
check_close = functools.partial(helpers.check_close, "fm-parity")


def make_head(kind, case, P):
    """The head of a case's shapes holding P's values: case = (B, F, D, A) for "afm", a HEAD_SWEEP entry otherwise."""
    from satrans_amd import AFMHead, DeepFMHead, NFMHead
    if kind == "afm":
        head = AFMHead(case[2], case[3])
    elif kind == "deepfm":
        head = DeepFMHead(case[2], case[3], case[5], case[6], case[4])
    else:
        head = NFMHead(case[3], case[5], case[4])
    head.load_state_dict({k: v.clone() for k, v in R.state_from_params(P).items()})
    return head.to(DEV)


def run(kind, head, emb, dense, lin, up):
    """logit, the gradients under the restatement's names (R.flat), the saved buffer - all on the host."""
    head.zero_grad(set_to_none=True)
    eg = emb.to(DEV).requires_grad_(True)
    dg = None if dense is None else dense.to(DEV).requires_grad_(True)
    lg = lin.to(DEV).requires_grad_(True)
    y = head(eg, lg) if kind == "afm" else head(eg, dg, lg)
    saved = y.grad_fn.saved_tensors[1]
    (y * up.to(DEV)).sum().backward()
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in head.named_parameters()}, torch.float32))
    g["emb"], g["lin_logit"] = eg.grad.cpu(), lg.grad.cpu()
    if dg is not None and dg.grad is not None:
        g["dense"] = dg.grad.cpu()
    return y.detach().cpu(), g, saved.cpu()


@functools.lru_cache(maxsize=None)
def afm_drawn(case):
    """The seeded draw of an AFM case and its fp64 logit, gradients and cache: computed once, shared, never written to."""
    emb, lin, up, P, _ = R.afm_draw(case)
    y, cache = R.forward("afm", emb.double(), None, lin.double(), R.double(P))
    return emb, lin, up, P, y, R.flat(R.backward(up.double(), cache)), cache


@functools.lru_cache(maxsize=None)
def head_drawn(case):
    emb, dense, lin, up, P, _ = R.head_draw(case)
    y, cache = R.forward(case[0], emb.double(), None if dense is None else dense.double(), lin.double(), R.double(P), case[6])
    return emb, dense, lin, up, P, y, R.flat(R.backward(up.double(), cache)), cache


@pytest.mark.parametrize("case", R.AFM_SWEEP, ids=R.afm_id)
def test_afm_sweep_against_the_restatement(case):
    """AFMHead over the shapes of R.AFM_SWEEP (what each is there for is written beside it): the logit, normalized_att_score,
    the attention output in `saved`, the four parameter gradients, d out.bias, demb and dlinear_logit.  With one pair the softmax
    is the constant 1: d attention_W, d attention_b and d projection_h are exactly zero."""
    B, Fn, D, A = case
    emb, lin, up, P, want_y, want, cache = afm_drawn(case)
    head = make_head("afm", case, P)
    y, g, saved = run("afm", head, emb, None, lin, up)
    n_pairs = Fn * (Fn - 1) // 2
    d = native.AFMDesc()
    d.B, d.F, d.D, d.A = case
    assert y.shape == (B, 1) and saved.numel() == B * (n_pairs + D) == native.lib().satrans_afm_saved_floats(ctypes.byref(d))
    tag = f"afm {R.afm_id(case)}"
    check_close(y, want_y, 2e-5, tag)
    score = head.fm.normalized_att_score
    assert score.shape == (B, n_pairs, 1) and not score.requires_grad
    check_close(score.cpu(), cache.afm.a, 2e-5, f"{tag} normalized_att_score")
    check_close(saved[B * n_pairs:].reshape(B, D), cache.afm.ao, 2e-5, f"{tag} attention output")
    assert sorted(g) == sorted(want)
    for k in want:
        if Fn == 2 and k in ("W", "b", "h"):
            assert float(want[k].abs().max()) == 0.0 and float(g[k].abs().max()) == 0.0, k
            assert torch.equal(score.cpu(), torch.ones(B, 1, 1))
            continue
        check_close(g[k], want[k], 1e-4, f"{tag} {k}", what="grad", floor=5e-9)


@pytest.mark.parametrize("case", R.HEAD_SWEEP, ids=R.head_id)
def test_head_sweep_against_the_restatement(case):
    """DeepFMHead and NFMHead over R.HEAD_SWEEP: the logit, every parameter gradient, demb, ddense, dlinear_logit, and the DNN
    input the forward leaves in `saved`, block by block."""
    kind, B, Fn, D, dnn, dense_dim, use_fm = case
    emb, dense, lin, up, P, want_y, want, cache = head_drawn(case)
    head = make_head(kind, case, P)
    y, g, saved = run(kind, head, emb, dense, lin, up)
    d = native.FMHeadDesc()
    d.B, d.F, d.D, d.kind, d.use_fm = B, Fn, D, native.FMHEAD_NFM if kind == "nfm" else native.FMHEAD_DEEPFM, int(use_fm)
    d.dense_dim, d.n_dnn = dense_dim, len(dnn)
    for l, w in enumerate(dnn):
        d.width[l] = w
    assert y.shape == (B, 1) and saved.numel() == native.lib().satrans_fmhead_saved_floats(ctypes.byref(d))
    tag = f"head {R.head_id(case)}"
    check_close(y, want_y, 2e-5, tag)
    if dnn:
        x = saved[:cache.X.numel()].reshape(cache.X.shape)
        where = R.blocks(kind, Fn, D, dense_dim)
        assert sum(w for _, w in where.values()) == cache.X.shape[1]
        for name, (at, width) in where.items():
            check_close(x[:, at:at + width], cache.X[:, at:at + width], 2e-5, f"{tag} dnn input, {name} block")
    else:
        assert saved.numel() == 0
    assert sorted(g) == sorted(want)
    for k in want:
        check_close(g[k], want[k], 1e-4, f"{tag} {k}", what="grad", floor=5e-9)
    assert torch.equal(g["lin_logit"], up)


@pytest.mark.parametrize("case", R.AFM_SWEEP, ids=R.afm_id)
def test_layers_alone_against_the_restatement(case):
    """FM, BiInteractionPooling and AFMLayer as modules of their own, once fed deepctr's list of pieces and once the tensor:
    outputs and input gradients (AFMLayer: the parameter gradients too); and composed from the layers, linear_logit + layer +
    out.bias is the head's logit."""
    from satrans_amd import FM, AFMLayer, BiInteractionPooling
    B, Fn, D, A = case
    emb, lin, up, P, want_y, want, cache = afm_drawn(case)
    tag = f"layers {R.afm_id(case)}"
    g = torch.Generator().manual_seed(B + Fn)
    up_b = torch.randn(B, 1, D, generator=g)
    e64 = emb.double()
    results = {}
    for feed in ("pieces", "tensor"):
        give = (lambda x: list(torch.split(x, 1, dim=1))) if feed == "pieces" else (lambda x: x)      # noqa: E731
        x = emb.to(DEV).requires_grad_(True)
        out = FM()(give(x))
        assert out.shape == (B, 1)
        (out * up.to(DEV)).sum().backward()
        check_close(out.detach().cpu(), R.fm(e64), 2e-5, f"{tag} fm ({feed})")
        check_close(x.grad.cpu(), R.fm_backward(up.double(), e64), 1e-4, f"{tag} fm dx ({feed})", what="grad", floor=5e-9)
        x = emb.to(DEV).requires_grad_(True)
        out = BiInteractionPooling()(give(x))
        assert out.shape == (B, 1, D)
        (out * up_b.to(DEV)).sum().backward()
        check_close(out.detach().cpu(), R.bipool(e64), 2e-5, f"{tag} bipool ({feed})")
        check_close(x.grad.cpu(), R.bipool_backward(up_b.double(), e64), 1e-4, f"{tag} bipool dx ({feed})", what="grad", floor=5e-9)
        layer = AFMLayer(D, A)
        layer.load_state_dict({k[3:]: v.clone() for k, v in R.state_from_params(P).items() if k.startswith("fm.")})
        layer = layer.to(DEV)
        x = emb.to(DEV).requires_grad_(True)
        out = layer(give(x))
        assert out.shape == (B, 1)
        (out * up.to(DEV)).sum().backward()
        check_close(out.detach().cpu(), R.afm(e64, R.double(P))[0], 2e-5, f"{tag} afm ({feed})")
        check_close(layer.normalized_att_score.cpu(), cache.afm.a, 2e-5, f"{tag} afm score ({feed})")
        check_close(x.grad.cpu(), want["emb"], 1e-4, f"{tag} afm dx ({feed})", what="grad", floor=5e-9)
        if Fn > 2:
            for name, p in (("W", layer.attention_W), ("b", layer.attention_b), ("h", layer.projection_h), ("p", layer.projection_p)):
                check_close(p.grad.cpu(), want[name], 1e-4, f"{tag} afm d{name} ({feed})", what="grad", floor=5e-9)
        results[feed] = (out.detach().cpu(), x.grad.cpu())
    assert torch.equal(results["pieces"][0], results["tensor"][0]) and torch.equal(results["pieces"][1], results["tensor"][1])
    check_close(lin + results["tensor"][0] + P["out_bias"], want_y, 2e-5, f"{tag} composed")


@pytest.mark.parametrize("case", R.HEAD_SWEEP, ids=R.head_id)
def test_composed_from_the_layers_equals_the_head(case):
    """linear_logit + FM(emb) + dnn_linear(dnn(...)) + out.bias built from the layers and torch's Linear gives the head's logit,
    and the pooled row of BiInteractionPooling is bit for bit the head's DNN input block."""
    from satrans_amd import FM, BiInteractionPooling
    kind, B, Fn, D, dnn, dense_dim, use_fm = case
    emb, dense, lin, up, P, want_y, _, cache = head_drawn(case)
    head = make_head(kind, case, P)
    y, _, saved = run(kind, head, emb, dense, lin, up)
    with torch.no_grad():
        x = emb.to(DEV)
        logit = lin.to(DEV) + head.out.bias
        if kind == "deepfm" and use_fm:
            logit = logit + FM()(x)
        if dnn:
            first = BiInteractionPooling()(x)[:, 0, :] if kind == "nfm" else x.flatten(1)
            if kind == "nfm":
                assert torch.equal(first.cpu(), saved[:cache.X.numel()].reshape(cache.X.shape)[:, :D])
            h = first if dense is None else torch.cat([first, dense.to(DEV)], dim=1)
            for l in head.dnn.linears:
                h = torch.relu(l(h))
            logit = logit + head.dnn_linear(h)
    check_close(logit.cpu(), want_y, 2e-5, f"composed {R.head_id(case)}")
    check_close(logit.cpu(), y.double(), 2e-5, f"composed against the head {R.head_id(case)}")


def alone_equals_batch(kind, case, emb, dense, lin, up, P):
    B = emb.shape[0]
    head = make_head(kind, case, P)
    y, g, _ = run(kind, head, emb, dense, lin, up)
    assert float(g["emb"].abs().max()) > 0.0
    for b in (0, 1, B // 2, B - 1):
        y1, g1, _ = run(kind, head, emb[b:b + 1], None if dense is None else dense[b:b + 1], lin[b:b + 1], up[b:b + 1])
        assert torch.equal(y1[0], y[b]), b
        assert torch.equal(g1["emb"][0], g["emb"][b]), b
    lo = B // 3
    y2, g2, _ = run(kind, head, emb[lo:], None if dense is None else dense[lo:], lin[lo:], up[lo:])
    assert torch.equal(y2, y[lo:]) and torch.equal(g2["emb"], g["emb"][lo:])


@pytest.mark.parametrize("case", R.AFM_ALONE, ids=R.afm_id)
def test_afm_sample_alone_equals_the_batch_bit_for_bit(case):
    """A sample alone (B = 1) == the same sample inside the batch: its logit and its demb row; and a slice of the batch, which
    moves every sample to another place of its pass."""
    emb, lin, up, P = afm_drawn(case)[:4]
    alone_equals_batch("afm", case, emb, None, lin, up, P)


@pytest.mark.parametrize("case", R.HEAD_ALONE, ids=R.head_id)
def test_head_sample_alone_equals_the_batch_bit_for_bit(case):
    emb, dense, lin, up, P = head_drawn(case)[:5]
    alone_equals_batch(case[0], case, emb, dense, lin, up, P)


@pytest.mark.parametrize("which", ["afm-2", "afm-7", "afm-6", "head-0", "head-5", "head-3"])
def test_two_runs_agree_bit_for_bit(which):
    kind, n = which.split("-")
    if kind == "afm":
        case = R.AFM_SWEEP[int(n)]
        emb, lin, up, P = afm_drawn(case)[:4]
        dense = None
    else:
        case = R.HEAD_SWEEP[int(n)]
        kind = case[0]
        emb, dense, lin, up, P = head_drawn(case)[:5]
    (y0, g0, s0), (y1, g1, s1) = (run(kind, make_head(kind, case, P), emb, dense, lin, up) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]) and float(g0[k].abs().max()) > 0.0, k


@pytest.mark.parametrize("name", R.FIXTURES)
def test_reference_fixtures_on_the_gpu(name):
    """The reference's own recorded DeepFM / NFM / AFM run: its parameters, emb, dense and linear_logit in; sigmoid(logit), the
    summed BCE, every parameter gradient, grad/emb, normalized_att_score and the regularisation loss out."""
    from satrans_amd import AFMHead, DeepFMHead, NFMHead
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    kind, l2 = R.FIXTURE_KIND[name], float(fx["l2"])
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    emb, dense, lin, labels = (torch.from_numpy(fx[k]) for k in ("emb", "dense", "linear_logit", "labels"))
    if kind == "afm":
        head = AFMHead(emb.shape[2], state["fm.attention_W"].shape[1], l2_reg_att=l2)
    elif kind == "nfm":
        head = NFMHead(emb.shape[2], dense.shape[1], (16, 8), l2_reg_dnn=l2)
    else:
        head = DeepFMHead(emb.shape[1], emb.shape[2], dense.shape[1], True, () if name == "deepfm_nodnn" else (16, 8), l2_reg_dnn=l2)
    assert list(head.state_dict()) == list(fx["keys"])
    head.load_state_dict(state)
    head = head.to(DEV)
    eg = emb.to(DEV).requires_grad_(True)
    logit = head(eg, lin.to(DEV)) if kind == "afm" else head(eg, dense.to(DEV), lin.to(DEV))
    y = torch.sigmoid(logit)
    loss = F.binary_cross_entropy(y.squeeze(1), labels.to(DEV), reduction='sum')
    loss.backward()
    check_close(y.detach().cpu(), torch.from_numpy(fx["y_pred"]), 2e-5, f"fixture {name}", what="fixture y")
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    for k, p in head.named_parameters():
        check_close(p.grad.cpu(), torch.from_numpy(fx[f"grad/{k}"]), 2e-5, f"fixture {name} {k}", what="fixture grad")
    check_close(eg.grad.cpu(), torch.from_numpy(fx["grad/emb"]), 2e-5, f"fixture {name} emb", what="fixture grad")
    if kind == "afm":
        check_close(head.fm.normalized_att_score.cpu(), torch.from_numpy(fx["normalized_att_score"]), 2e-5,
                    f"fixture {name} normalized_att_score", what="fixture y")
    reg = head.regularization_loss()
    assert reg.shape == (1,)
    check_close(reg.detach().cpu(), torch.from_numpy(fx["reg_loss"]), 1e-6, f"fixture {name} reg_loss", what="fixture reg")


def test_errors_and_odd_inputs():
    from satrans_amd import FM, AFMHead, AFMLayer, BiInteractionPooling, DeepFMHead, NFMHead
    torch.manual_seed(3)
    x = torch.randn(6, 4, 8)
    deepfm = DeepFMHead(4, 8, 0, True, (16,), init_std=0.3).to(DEV)
    nfm = NFMHead(8, 0, (16,), init_std=0.3).to(DEV)
    afm = AFMHead(8, 4).to(DEV)
    for head in (deepfm, nfm, afm):
        assert head(x.to(DEV)).shape == (6, 1)                      # no linear_logit, no dense
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        AFMHead(8)(x)                                               # a CPU tensor
    for head in (deepfm, nfm, afm):
        with pytest.raises(TypeError, match="float32"):
            head(x.to(DEV).double())
    with pytest.raises(ValueError):
        deepfm(x[:, :3].to(DEV))                                    # wrong field count
    with pytest.raises(ValueError):
        nfm(x.to(DEV), torch.randn(6, 1, device=DEV))               # dense columns unexpected
    with pytest.raises(ValueError):
        afm(x.to(DEV), torch.randn(6, 2, device=DEV))               # linear_logit of another shape
    with pytest.raises(ValueError):
        AFMLayer(5).to(DEV)(x.to(DEV))                              # another embedding size
    with pytest.raises(NotImplementedError, match="FM_MAX_DIM"):
        FM()(torch.randn(2, 4, native.FM_MAX_DIM + 1, device=DEV))
    with pytest.raises(NotImplementedError, match="FM_MAX_FIELDS"):
        BiInteractionPooling()(torch.randn(2, native.FM_MAX_FIELDS + 1, 4, device=DEV))
    xt = x.to(DEV).transpose(0, 1).contiguous().transpose(0, 1)      # a non-contiguous input is handled: made contiguous
    assert not xt.is_contiguous()
    lin = torch.randn(6, 2, device=DEV)[:, :1]                       # a non-contiguous linear_logit too
    assert not lin.is_contiguous()
    for mod in (deepfm, nfm, afm, FM(), BiInteractionPooling(), afm.fm):
        assert torch.equal(mod(xt), mod(x.to(DEV)))
    assert torch.equal(afm(xt, lin), afm(x.to(DEV), lin.contiguous()))
    assert torch.equal(deepfm(xt, None, lin), deepfm(x.to(DEV), None, lin.contiguous()))
    assert torch.equal(afm(list(torch.split(x.to(DEV), 1, dim=1))), afm(x.to(DEV)))      # deepctr's list of pieces


@pytest.mark.parametrize("kind", ["afm", "nfm", "deepfm"])
def test_metatransformation_feeds_the_head(kind):
    """The reference's `metatrans` flag: MetaTransformation -> the head; one backward reaches the scenario embeddings, the
    embedding block and the head's parameters."""
    from satrans_amd import AFMHead, DeepFMHead, MetaTransformation, NFMHead
    B, M, D, S = 40, 5, 16, 3      # (the MetaNet kernels take D in {16, 32, 64, 128})
    torch.manual_seed(6)
    meta = MetaTransformation(D, S, (D, 16, D), init_std=0.3).to(DEV)
    head = {"afm": lambda: AFMHead(D, 8), "nfm": lambda: NFMHead(D, 2, (16, 8), init_std=0.3),
            "deepfm": lambda: DeepFMHead(M, D, 2, True, (16, 8), init_std=0.3)}[kind]().to(DEV)
    g = torch.Generator().manual_seed(9)
    emb = (torch.randn(B, M, D, generator=g) + 0.5).to(DEV).requires_grad_(True)
    dense = torch.randn(B, 2, generator=g).to(DEV)
    lin = torch.randn(B, 1, generator=g).to(DEV)
    ids = torch.randint(0, S + 1, (B,), generator=g).to(DEV)
    target = (torch.rand(B, generator=g) > 0.5).float().to(DEV)
    x = meta(ids, emb)
    logit = head(x, lin) if kind == "afm" else head(x, dense, lin)
    assert logit.shape == (B, 1)
    F.binary_cross_entropy(torch.sigmoid(logit.squeeze(1)), target, reduction='sum').backward()
    first = head.fm.attention_W if kind == "afm" else head.dnn.linears[0].weight
    for name, t in (("domain_embeddings.weight", meta.domain_embeddings.weight.grad), ("emb", emb.grad), ("head", first.grad),
                    ("out.bias", head.out.bias.grad)):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0.0, name
