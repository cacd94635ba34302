"""satrans_amd.layers.InteractingLayer and AutoIntHead (csrc/autoint.hip behind torch.autograd.Function) against the fp64
restatement tests/autoint_reference.py on the same seeded inputs; that restatement is deepctr's LITERAL form (tensordot, split /
stack over the heads, the einsum, softmax over the last dim, cat, relu) and is pinned to autograd and to the recorded runs of the
reference's own AutoInt.forward by tests/test_autoint_cpu.py.

Bounds (the sibling bounds), all element-wise: results and normalized_att_scores within 2e-5 max|.|; gradients
within 1e-4 max|g| + 5e-9.  tests/test_autoint_cpu.py::test_premise_of_the_gpu_bounds pins their margin and that no relu of a
draw sits near its kink.  The figures measured on the MI355X are in DESIGN.md §3.17."""
import ctypes
import functools

import pytest
import torch

from satrans_amd import native
from tests import autoint_reference as R
from tests import helpers

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
check_close = functools.partial(helpers.check_close, "autoint-parity")
LAYER_CASES = R.SWEEP + [R.WALK]
HEAD_CASES = [(c, R.HEAD_EXTRAS[i]) for i, c in enumerate(R.SWEEP)]


def head_id(cx):
    c, (dnn, dense_dim) = cx
    return f"{R.case_id(c)}-dnn{'x'.join(map(str, dnn)) or 'none'}-dense{dense_dim}"


def flags_of(use_res, scaling):
    return (0 if use_res else native.NO_RES) | (0 if scaling else 128)


def make_layer(case, W):
    from satrans_amd import InteractingLayer
    _, _, D, H, _, use_res, scaling = case
    layer = InteractingLayer(D, H, use_res, scaling)
    layer.load_state_dict({k: v.clone() for k, v in W.items()})
    return layer.to(DEV)


def make_head(case, dnn, dense_dim, P):
    from satrans_amd import AutoIntHead
    _, Fn, D, H, L, use_res, scaling = case
    head = AutoIntHead(Fn, D, dense_dim, L, H, use_res, dnn)
    head.load_state_dict({k: v.clone() for k, v in R.state_from_params(P).items()})
    for layer in head.int_layers:
        layer.scaling = scaling
    return head.to(DEV)


@functools.lru_cache(maxsize=None)
def layer_drawn(case):
    """The seeded draw of a case, its first layer alone in fp64: y, the scores, dx and the weight gradients under up_y.
    Computed once, shared, never written to."""
    emb, _, up_y, _, P, _ = R.draw(case)
    W = P["int"][0]
    y, cache = R.layer_forward(emb.double(), {k: v.double() for k, v in W.items()}, case[3], case[6])
    dx, g = R.layer_backward(up_y.double(), cache)
    return emb, up_y, W, y, cache.p, dx, g


@functools.lru_cache(maxsize=None)
def head_drawn(case, dnn, dense_dim):
    emb, dense, up_y, up, P, _ = R.draw(case, dnn, dense_dim)
    y, cache = R.forward(emb.double(), None if dense is None or not dnn else dense.double(), R.double(P), case[3], case[6])
    return emb, dense, up_y, up, P, y, R.flat(R.backward(up.double(), cache)), cache


def run_layer(layer, emb, up_y):
    """y, dx, the weight gradients by name, the saved statistics - all on the host."""
    layer.zero_grad(set_to_none=True)
    x = emb.detach().to(DEV).requires_grad_(True)
    y = layer(x)
    saved = y.grad_fn.saved_tensors[2]
    (y * up_y.to(DEV)).sum().backward()
    return y.detach().cpu(), x.grad.cpu(), {k: p.grad.cpu() for k, p in layer.named_parameters()}, saved.cpu()


def run_head(head, emb, dense, up):
    """logit, the gradients under the restatement's names (R.flat), the saved buffer - all on the host."""
    head.zero_grad(set_to_none=True)
    eg = emb.detach().to(DEV).requires_grad_(True)
    dg = None if dense is None else dense.detach().to(DEV).requires_grad_(True)
    y = head(eg, dg)
    saved = y.grad_fn.saved_tensors[1]
    (y * up.to(DEV)).sum().backward()
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in head.named_parameters()}, torch.float32))
    g["emb"] = eg.grad.cpu()
    if dg is not None and dg.grad is not None:
        g["dense"] = dg.grad.cpu()
    return y.detach().cpu(), g, saved.cpu()


@pytest.mark.parametrize("case", LAYER_CASES, ids=R.case_id)
def test_layer_matches_the_restatement(case):
    """InteractingLayer alone over the sweep (each case's first layer) and over the WALK case, whose workgroups each walk
    several passes: y, normalized_att_scores under capture_attention, dx, the weight gradients, and the size of what is saved."""
    B, Fn, D, H, _, use_res, scaling = case
    emb, up_y, W, want_y, want_p, want_dx, want_g = layer_drawn(case)
    layer = make_layer(case, W)
    assert layer.normalized_att_scores is None
    y, dx, g, saved = run_layer(layer, emb, up_y)
    assert layer.normalized_att_scores is None      # (deepctr fills it on every forward; here the switch does)
    d = native.InteractingDesc()
    d.B, d.F, d.D, d.H, d.flags = B, Fn, D, H, flags_of(use_res, scaling)
    assert saved.numel() == native.lib().satrans_interacting_saved_floats(ctypes.byref(d)) <= 2 * B * H * Fn + 4
    tag = f"layer {R.case_id(case)}"
    assert y.shape == (B, Fn, D)
    check_close(y, want_y, 2e-5, tag)
    check_close(dx, want_dx, 1e-4, f"{tag} dx", what="grad", floor=5e-9)
    assert sorted(g) == sorted(want_g)
    for k in want_g:
        check_close(g[k], want_g[k], 1e-4, f"{tag} {k}", what="grad", floor=5e-9)
    layer.capture_attention = True
    y2 = layer(emb.to(DEV))
    att = layer.normalized_att_scores
    assert att.shape == (H, B, Fn, Fn) and not att.requires_grad
    check_close(att.cpu(), want_p, 2e-5, f"{tag} normalized_att_scores")
    assert torch.equal(y2.detach().cpu(), y)      # (capturing changes no bit of y)


@pytest.mark.parametrize("cx", HEAD_CASES, ids=head_id)
def test_head_matches_the_restatement(cx):
    """The stack and AutoIntHead over the sweep, DNN widths (16, 8) and () and dense_dim 0 and 1 spread over the cases: the
    logit, every parameter gradient, demb, ddense, the last layer's scores, and the size of what is saved."""
    case, (dnn, dense_dim) = cx
    B, Fn, D, H, L, use_res, scaling = case
    emb, dense, _, up, P, want_y, want, cache = head_drawn(case, dnn, dense_dim)
    head = make_head(case, dnn, dense_dim, P)
    head.int_layers[-1].capture_attention = True
    y, g, saved = run_head(head, emb, dense, up)
    ld = Fn * D + dense_dim
    assert saved.numel() == L * B * Fn * D + L * 2 * B * H * Fn + (B * ld + B * sum(dnn) if dnn else 0)
    tag = f"head {head_id(cx)}"
    assert y.shape == (B, 1)
    check_close(y, want_y, 2e-5, tag)
    check_close(head.int_layers[-1].normalized_att_scores.cpu(), cache.layers[-1].p, 2e-5, f"{tag} normalized_att_scores")
    assert all(layer.normalized_att_scores is None for layer in head.int_layers[:-1])
    stack = saved[(L - 1) * B * Fn * D:L * B * Fn * D].reshape(B, Fn * D)
    check_close(stack, cache.att, 2e-5, f"{tag} att_output")
    assert sorted(g) == sorted(want)
    for k in want:
        check_close(g[k], want[k], 1e-4, f"{tag} {k}", what="grad", floor=5e-9)


@pytest.mark.parametrize("cx", [HEAD_CASES[2], HEAD_CASES[4], HEAD_CASES[7]], ids=head_id)
def test_head_is_the_composition_of_its_layers(cx):
    """The head's logit equals dnn_linear([flatten(stack(emb)) | dnn(...)]) + out.bias formed from its own int_layers called one
    by one (the DNN in fp64 torch from the head's parameters), within the result bound."""
    case, (dnn, dense_dim) = cx
    emb, dense, _, up, P, want_y, _, _ = head_drawn(case, dnn, dense_dim)
    head = make_head(case, dnn, dense_dim, P)
    with torch.no_grad():
        y = head(emb.to(DEV), None if dense is None else dense.to(DEV)).cpu()
        x = emb.to(DEV)
        for layer in head.int_layers:
            x = layer(x)
        stack_out = torch.flatten(x, start_dim=1).cpu().double()
        if dnn:
            h = torch.flatten(emb, start_dim=1).double()
            if dense is not None:
                h = torch.cat([h, dense.double()], dim=-1)
            for lin in head.dnn.linears:
                h = torch.relu(h @ lin.weight.cpu().double().T + lin.bias.cpu().double())
            stack_out = torch.cat([stack_out, h], dim=-1)
        composed = stack_out @ head.dnn_linear.weight.cpu().double().T + head.out.bias.cpu().double()
    check_close(y, composed, 2e-5, f"composition {head_id(cx)}")


@pytest.mark.parametrize("case", R.ALONE, ids=R.case_id)
def test_a_sample_alone_gives_the_bits_it_gives_in_the_batch(case):
    """Forward y of the first layer and the head's logit: sample b alone (B = 1) and inside the batch, bit for bit, for the
    first sample, one in the middle of a workgroup's group and the last (the tail group)."""
    i = R.SWEEP.index(case)
    dnn, dense_dim = R.HEAD_EXTRAS[i]
    emb, dense, _, _, P, _, _, _ = head_drawn(case, dnn, dense_dim)
    layer = make_layer(case, P["int"][0])
    head = make_head(case, dnn, dense_dim, P)
    B = case[0]
    with torch.no_grad():
        x = emb.to(DEV)
        dn = None if dense is None else dense.to(DEV)
        y_all, logit_all = layer(x), head(x, dn)
        for b in (0, B // 2 + 1, B - 1):
            assert torch.equal(layer(x[b:b + 1]), y_all[b:b + 1]), b
            assert torch.equal(head(x[b:b + 1], None if dn is None else dn[b:b + 1]), logit_all[b:b + 1]), b


@pytest.mark.parametrize("cx", [HEAD_CASES[2], HEAD_CASES[6], HEAD_CASES[7]], ids=head_id)
def test_two_runs_give_the_same_bits(cx):
    """Forward + backward twice: every gradient and the saved buffer bit for bit, for the head and for a layer alone (and the
    WALK case: several passes per workgroup, the ordered reduce over 512 partials)."""
    case, (dnn, dense_dim) = cx
    emb, dense, up_y, up, P, _, _, _ = head_drawn(case, dnn, dense_dim)
    head = make_head(case, dnn, dense_dim, P)
    y1, g1, s1 = run_head(head, emb, dense, up)
    y2, g2, s2 = run_head(head, emb, dense, up)
    assert torch.equal(y1, y2) and torch.equal(s1, s2) and sorted(g1) == sorted(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for c in (case, R.WALK):
        e, u, W = layer_drawn(c)[:3]
        layer = make_layer(c, W)
        a, b = run_layer(layer, e, u), run_layer(layer, e, u)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
        for k in a[2]:
            assert torch.equal(a[2][k], b[2][k]), k


def test_unsupported_shapes_raise_and_do_not_launch():
    """D = 24, d_head = 4, F = 65: NativeError from the size query, before any launch (a following launch on the same stream
    works and no error is pending)."""
    from satrans_amd import AutoIntHead, InteractingLayer
    for B, Fn, D, H in ((4, 5, 24, 2), (4, 5, 16, 4), (4, 65, 32, 2)):
        x = torch.randn(B, Fn, D, device=DEV)
        with pytest.raises(native.NativeError, match="not supported"):
            InteractingLayer(D, H).to(DEV)(x)
        with pytest.raises(native.NativeError, match="not supported"):
            AutoIntHead(Fn, D, 0, 1, H, True, ()).to(DEV)(x)
    torch.cuda.synchronize()
    y = InteractingLayer(16, 2).to(DEV)(torch.randn(4, 5, 16, device=DEV))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
