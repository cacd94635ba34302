"""satrans_amd.layers.CrossNet and DCNHead (csrc/cross.hip behind torch.autograd.Function) against the fp64 restatement
tests/cross_reference.py on the same seeded inputs; that restatement is pinned to autograd of deepctr's tensordot / matmul form
and to the recorded runs of the reference's own DCN.forward by tests/test_cross_cpu.py.

Bounds (the sibling bounds), all element-wise: results within 2e-5 max|.|; gradients within 1e-4 max|g| + 5e-9.
tests/test_cross_cpu.py::test_premise_of_the_gpu_bounds pins their margin."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import cross_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dcn")
check_close = functools.partial(helpers.check_close, "cross-parity")


def make_net(N, P, matrix):
    """A CrossNet of the shapes of P holding its values."""
    from satrans_amd import CrossNet
    mod = CrossNet(N, P["kernels"].shape[0], "matrix" if matrix else "vector")
    mod.load_state_dict({k: v.clone() for k, v in R.state_from_params(P).items()})
    return mod.to(DEV)


def run(mod, x, up):
    """result, {"kernels", "bias", "x"} gradients in the restatement's shapes, the saved buffer - all on the host."""
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg)
    saved = y.grad_fn.saved_tensors[1]
    (y * up.to(DEV)).sum().backward()
    g = R.params_from_state({k: p.grad.cpu() for k, p in mod.named_parameters()}, dtype=torch.float32)
    g["x"] = xg.grad.cpu()
    return y.detach().cpu(), g, saved.cpu()


@functools.lru_cache(maxsize=None)
def drawn(case):
    """The seeded draw of a case and its fp64 result and gradients: computed once, shared, never written to."""
    x, up, P = R.sweep_draw(case)
    y, cache = R.forward(x.double(), R.double(P), case[3])
    return x, up, P, y, R.backward(up.double(), cache)


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_shape_sweep_against_the_restatement(case):
    """Results, dx0, dkernels and dbias over the shapes of R.SWEEP (what each is there for is written beside it)."""
    B, N, L, matrix = case
    x, up, P, want_y, want = drawn(case)
    mod = make_net(N, P, matrix)
    y, g, saved = run(mod, x, up)
    d = native.CrossDesc()
    d.B, d.N, d.L, d.matrix = B, N, L, int(matrix)
    assert y.shape == (B, N) and saved.numel() == native.lib().satrans_cross_saved_floats(ctypes.byref(d))
    if not matrix:
        assert saved.numel() == B * L      # the vector form keeps nothing that scales with N
    check_close(y, want_y, 2e-5, f"sweep {R.case_id(case)}")
    assert sorted(g) == sorted(want)
    for k in want:
        check_close(g[k], want[k], 1e-4, f"sweep {R.case_id(case)} {k}", what="grad", floor=5e-9)


@pytest.mark.parametrize("case", R.ALONE, ids=R.case_id)
def test_a_sample_alone_equals_the_batch_bit_for_bit(case):
    """A sample alone (B = 1) == the same sample inside the batch: its result row and its dx0 row.  Samples from the first, a
    middle and the last row tile and chunk."""
    B, N, L, matrix = case
    x, up, P = drawn(case)[:3]
    mod = make_net(N, P, matrix)
    y, g, _ = run(mod, x, up)
    assert float(g["x"].abs().max()) > 0.0
    for b in (0, 1, B // 2, B - 1):
        y1, g1, _ = run(mod, x[b:b + 1], up[b:b + 1])
        assert torch.equal(y1[0], y[b]), b
        assert torch.equal(g1["x"][0], g["x"][b]), b
    lo = B // 3      # and a slice of the batch, which moves every sample to another place of its tile
    y2, g2, _ = run(mod, x[lo:], up[lo:])
    assert torch.equal(y2, y[lo:]) and torch.equal(g2["x"], g["x"][lo:])


@pytest.mark.parametrize("matrix", (False, True), ids=("vector", "matrix"))
def test_two_runs_agree_bit_for_bit(matrix):
    case = R.SHAPES[1] + (matrix,)
    x, up, P = drawn(case)[:3]
    (y0, g0, s0), (y1, g1, s1) = (run(make_net(case[1], P, matrix), x, up) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(s0, s1) and float(s0.abs().max()) > 0.0
    for k in ("x", "kernels", "bias"):
        assert torch.equal(g0[k], g1[k]) and float(g0[k].abs().max()) > 0.0, k


def test_the_vector_form_does_not_keep_the_layer_inputs():
    """At B = 4096, N = 608, L = 8: the peak of torch's allocator over one forward plus backward, above what was allocated
    before, stays below L B N 4 bytes (79.7 MB) - the x_l alone that the torch form must keep.  The library needs the result,
    dy, dx, the test's own product and small partials: about 5 B N."""
    from satrans_amd import CrossNet
    B, N, L = 4096, 608, 8
    torch.manual_seed(5)
    mod = CrossNet(N, L).to(DEV)
    x = torch.randn(B, N, device=DEV, requires_grad=True)
    up = torch.randn(B, N, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    (mod(x) * up).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"[cross-memory] peak above the start: {peak / 1e6:.1f} MB")
    assert float(x.grad.abs().max()) > 0.0
    assert peak < L * B * N * 4


@pytest.mark.parametrize("name", ["vector", "matrix", "cross_only"])
def test_reference_fixtures_on_the_gpu(name):
    """The reference's own recorded DCN run: its parameters, emb, dense and linear_logit in; sigmoid(logit), the summed BCE,
    every parameter gradient, grad/emb and the regularisation loss out.  Both sides are fp32 runs of contractions at most 25
    long: the fixtures' bound 2e-5 max|.| of tests/test_cross_cpu.py."""
    from satrans_amd import DCNHead
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    dnn = tuple(state[f"dnn.linears.{l}.weight"].shape[0] for l in range(2)) if name != "cross_only" else ()
    emb, dense, lin, labels = (torch.from_numpy(fx[k]) for k in ("emb", "dense", "linear_logit", "labels"))
    head = DCNHead(emb.shape[1], emb.shape[2], dense.shape[1], state["crossnet.kernels"].shape[0],
                   "matrix" if int(fx["matrix"]) else "vector", dnn)
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
    assert reg.shape == (1,)
    check_close(reg.detach().cpu(), torch.from_numpy(fx["reg_loss"]), 2e-5, f"fixture {name} reg_loss", what="fixture reg")


def test_errors():
    from satrans_amd import CrossNet
    x = torch.randn(6, 8)
    net = CrossNet(8, 2).to(DEV)
    assert net(x.to(DEV)).shape == (6, 8)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        CrossNet(8, 2)(x)
    with pytest.raises(TypeError, match="float32"):
        net(x.to(DEV).double())
    with pytest.raises(ValueError):
        net(x[:, :7].to(DEV))
    with pytest.raises(ValueError):
        net(x[0].to(DEV))
    with pytest.raises(ValueError, match="parameterization should be 'vector' or 'matrix'"):
        CrossNet(8, 2, 'tensor')
    with pytest.raises(NotImplementedError, match="layers"):
        CrossNet(8, native.CROSS_MAX_LAYERS + 1)
    for form in ("vector", "matrix"):
        net = CrossNet(8, 2, form).to(DEV)
        y = net(x.to(DEV).t().contiguous().t())      # a non-contiguous input is made contiguous
        assert torch.equal(y, net(x.to(DEV)))
    xd = x.to(DEV)
    assert CrossNet(8, 0).to(DEV)(xd) is xd          # no layers: the input, no native call


class _Net(nn.Module):
    def __init__(self, D, H, M, L):
        super().__init__()
        from satrans_amd import CrossNet, SelfAttention_Layer
        self.att = SelfAttention_Layer(D, head_num=H)
        self.cross = CrossNet(M * D, L, 'matrix')
        self.lin = nn.Linear(M * D, 1)

    def forward(self, x):
        return torch.sigmoid(self.lin(self.cross(torch.flatten(self.att(x), start_dim=1)))).squeeze(1)


def test_composition_trains_like_the_restatement():
    """SelfAttention_Layer (evaluation mode) -> flatten -> CrossNet (matrix, L = 2) -> Linear -> sigmoid -> summed BCE, three
    Adam steps with lr = eps = 1e-2: autograd into the cross network and through it into the layer in front.  lr / eps <= 1, so
    an error of the gradient moves a parameter by at most as much (the argument of
    tests/test_sharedbottom_gpu.py::test_composition_trains_like_the_restatement applies unchanged): parameters within the
    gradient bound, and enough of them moved for that to mean something."""
    from oracle import satrans_oracle as O
    D, H, M, B, LR, EPS, STEPS, L = 16, 2, 3, 30, 1e-2, 1e-2, 3, 2
    torch.manual_seed(4)
    net = _Net(D, H, M, L)
    g = torch.Generator().manual_seed(8)
    _, _, P = R.draw(B, M * D, L, True, 12)
    net.cross.load_state_dict(R.state_from_params(P))
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.startswith("att.W_"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    x, target = torch.randn(B, M, D, generator=g), (torch.rand(B, generator=g) > 0.5).float()
    start = {k: v.detach().clone() for k, v in net.named_parameters()}
    # fp64 restatement
    leaves = {k: v.double().requires_grad_(True) for k, v in start.items()}
    att = {k[4:]: v for k, v in leaves.items() if k.startswith("att.")}
    opt = torch.optim.Adam([v for k, v in leaves.items() if k != "att.W_Out"], lr=LR, eps=EPS)
    for _ in range(STEPS):
        opt.zero_grad()
        Pl = {"kernels": leaves["cross.kernels"], "bias": leaves["cross.bias"].squeeze(-1)}
        h = O.selfattention_layer(att, x.double(), H)[0].flatten(1)
        out = R.forward(h, Pl, True)[0] @ leaves["lin.weight"].T + leaves["lin.bias"]
        F.binary_cross_entropy(torch.sigmoid(out.squeeze(1)), target.double(), reduction='sum').backward()
        opt.step()
    # the modules on the GPU
    net = net.to(DEV).train()
    net.att.eval()
    opt = torch.optim.Adam(net.parameters(), lr=LR, eps=EPS)
    for _ in range(STEPS):
        opt.zero_grad()
        F.binary_cross_entropy(net(x.to(DEV)), target.to(DEV), reduction='sum').backward()
        opt.step()
    moved = 0
    for k, p in net.named_parameters():
        want = leaves[k].detach()
        check_close(p.detach().cpu(), want, 1e-4, f"composition {k}", what="parameter", floor=5e-9)
        moved += float((want - start[k].double()).abs().max()) > 10 * (1e-4 * float(want.abs().max()) + 5e-9)
    assert moved >= 10, moved     # the check above is not satisfied by parameters that stood still


def test_metatransformation_feeds_the_head():
    """The reference's `metatrans` flag: MetaTransformation -> DCNHead; one backward reaches the scenario embeddings, the
    embedding block and the cross network's kernels."""
    from satrans_amd import DCNHead, MetaTransformation
    B, M, D, S = 40, 5, 16, 3      # (the MetaNet kernels take D in {16, 32, 64, 128})
    torch.manual_seed(6)
    meta = MetaTransformation(D, S, (D, 16, D), init_std=0.3).to(DEV)
    head = DCNHead(M, D, 2, 2, 'vector', (16, 8), init_std=0.3).to(DEV)
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(B, M, D, generator=g).to(DEV).requires_grad_(True)
    dense, lin = torch.randn(B, 2, generator=g).to(DEV), torch.randn(B, 1, generator=g).to(DEV)
    ids = torch.randint(0, S + 1, (B,), generator=g).to(DEV)
    target = (torch.rand(B, generator=g) > 0.5).float().to(DEV)
    logit = head(meta(ids, emb), dense, lin)
    assert logit.shape == (B, 1)
    F.binary_cross_entropy(torch.sigmoid(logit.squeeze(1)), target, reduction='sum').backward()
    for name, t in (("domain_embeddings.weight", meta.domain_embeddings.weight.grad), ("emb", emb.grad),
                    ("crossnet.kernels", head.crossnet.kernels.grad)):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0.0, name
