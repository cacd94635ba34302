"""satrans_amd.layers.CIN and XDeepFMHead (csrc/cin.hip behind torch.autograd.Function) against the fp64 restatement
tests/cin_reference.py on the same seeded inputs; that restatement is pinned to autograd of deepctr's einsum form and to the
recorded runs of the reference's own xDeepFM.forward by tests/test_cin_cpu.py.

Bounds (the sibling bounds), all element-wise: results within 2e-5 max|.|; gradients within 1e-4 max|g| + 5e-9.
tests/test_cin_cpu.py::test_premise_of_the_gpu_bounds pins their margin."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import cin_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cin")
check_close = functools.partial(helpers.check_close, "cin-parity")


def make_cin(M, P, split):
    """A CIN of the shapes of P holding its values."""
    from satrans_amd import CIN
    mod = CIN(M, tuple(w.shape[0] for w in P["w"]), split_half=split)
    mod.load_state_dict({k: v.clone() for k, v in R.state_from_params(P).items()})
    return mod.to(DEV)


def run(mod, x, up):
    """result, {gradients keyed as R.flat keys them, "x"}, the saved buffer - all on the host."""
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg)
    saved = y.grad_fn.saved_tensors[1]
    (y * up.to(DEV)).sum().backward()
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in mod.named_parameters()}, dtype=torch.float32))
    g["x"] = xg.grad.cpu()
    return y.detach().cpu(), g, saved.cpu()


@functools.lru_cache(maxsize=None)
def drawn(case):
    """The seeded draw of a case and its fp64 result and gradients: computed once, shared, never written to."""
    B, M, D, layers, split = case
    x, up, P = R.sweep_draw(case)
    y, cache = R.forward(x.double(), R.double(P), split)
    return x, up, P, y, R.flat(R.backward(up.double(), cache))


@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_shape_sweep_against_the_restatement(case):
    """Results, dX0 and every dW, db over the shapes of R.SWEEP (what each is there for is written beside it)."""
    B, M, D, layers, split = case
    x, up, P, want_y, want = drawn(case)
    y, g, saved = run(make_cin(M, P, split), x, up)
    assert y.shape == (B, R.featuremap_num(layers, split)) and saved.numel() == B * D * sum(layers)
    check_close(y, want_y, 2e-5, f"sweep {R.case_id(case)}")
    assert sorted(g) == sorted(want)
    for k in want:
        check_close(g[k], want[k], 1e-4, f"sweep {R.case_id(case)} {k}", what="grad", floor=5e-9)


@pytest.mark.parametrize("case", R.ALONE, ids=R.case_id)
def test_a_sample_alone_equals_the_batch_bit_for_bit(case):
    """A sample alone (B = 1) == the same sample inside the batch: its result row and its dX0 rows.  Samples from the first, a
    middle and the last row tile, at a D that straddles row tiles and at the AliCCP D."""
    B, M, D, layers, split = case
    x, up, P = drawn(case)[:3]
    mod = make_cin(M, P, split)
    y, g, _ = run(mod, x, up)
    assert float(g["x"].abs().max()) > 0.0
    for b in (0, 1, B // 2, B - 1):
        y1, g1, _ = run(mod, x[b:b + 1], up[b:b + 1])
        assert torch.equal(y1[0], y[b]), b
        assert torch.equal(g1["x"][0], g["x"][b]), b
    lo = B // 3      # and a slice of the batch, which moves every sample to another place of its tile
    y2, g2, _ = run(mod, x[lo:], up[lo:])
    assert torch.equal(y2, y[lo:]) and torch.equal(g2["x"], g["x"][lo:])


def test_two_runs_agree_bit_for_bit():
    case = R.SWEEP[1]
    x, up, P = drawn(case)[:3]
    (y0, g0, s0), (y1, g1, s1) = (run(make_cin(case[1], P, case[4]), x, up) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(s0, s1) and float(s0.abs().max()) > 0.0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_the_outer_product_is_not_materialised():
    """At B = 128, M = 19, D = 32, (256, 128), split: the peak of torch's allocator over one forward plus backward, above what
    was allocated before, stays below the byte size of layer 2's outer product [B, 2432, 32] fp32 (39.8 MB) - which the torch
    form holds at least twice.  The activations the backward needs are 6.3 MB."""
    from satrans_amd import CIN
    B, M, D = 128, 19, 32
    torch.manual_seed(5)
    mod = CIN(M, (256, 128), split_half=True).to(DEV)
    x = torch.randn(B, M, D, device=DEV, requires_grad=True)
    up = torch.randn(B, mod.featuremap_num, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    (mod(x) * up).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"[cin-memory] peak above the start: {peak / 1e6:.1f} MB")
    assert float(x.grad.abs().max()) > 0.0
    assert peak < B * 2432 * D * 4


@pytest.mark.parametrize("name", ["plain", "nosplit", "cin_only"])
def test_reference_fixtures_on_the_gpu(name):
    """The reference's own recorded xDeepFM run: its parameters, emb, dense and linear_logit in; sigmoid(logit), the summed
    BCE, every parameter gradient and grad/emb out.  Both sides are fp32 runs of contractions at most 33 long: the fixtures'
    bound 2e-5 max|.| of tests/test_cin_cpu.py."""
    from satrans_amd import XDeepFMHead
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    dnn = tuple(state[f"dnn.linears.{l}.weight"].shape[0] for l in range(2)) if name != "cin_only" else ()
    cin = tuple(state[f"cin.conv1ds.{i}.weight"].shape[0] for i in range(2))
    emb, dense, lin, labels = (torch.from_numpy(fx[k]) for k in ("emb", "dense", "linear_logit", "labels"))
    head = XDeepFMHead(emb.shape[1], emb.shape[2], dense.shape[1], dnn, cin, bool(fx["split_half"]))
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


def test_errors():
    from satrans_amd import CIN
    x = torch.randn(6, 4, 8)
    cin = CIN(4, (8, 6)).to(DEV)
    assert cin(x.to(DEV)).shape == (6, 10)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        CIN(4, (8, 6))(x)
    with pytest.raises(TypeError, match="float32"):
        cin(x.to(DEV).double())
    with pytest.raises(ValueError):
        cin(x[:, :3].to(DEV))
    with pytest.raises(ValueError):
        cin(x[0].to(DEV))
    with pytest.raises(NotImplementedError, match="relu"):
        CIN(4, (8, 6), activation='prelu')
    with pytest.raises(ValueError, match="even"):
        CIN(4, (7, 6), split_half=True)
    y = cin(x.to(DEV).transpose(0, 1).contiguous().transpose(0, 1))      # a non-contiguous input is made contiguous
    assert torch.equal(y, cin(x.to(DEV)))


class _Net(nn.Module):
    def __init__(self, D, H, M, layers):
        super().__init__()
        from satrans_amd import CIN, SelfAttention_Layer
        self.att = SelfAttention_Layer(D, head_num=H)
        self.cin = CIN(M, layers)
        self.lin = nn.Linear(self.cin.featuremap_num, 1)

    def forward(self, x):
        return torch.sigmoid(self.lin(self.cin(self.att(x)))).squeeze(1)


def test_composition_trains_like_the_restatement():
    """SelfAttention_Layer (evaluation mode) -> CIN -> Linear -> sigmoid -> summed BCE, three Adam steps with lr = eps = 1e-2:
    autograd into the CIN and through it into the layer in front.  lr / eps <= 1, so an error of the gradient moves a
    parameter by at most as much (the argument of tests/test_sharedbottom_gpu.py::test_composition_trains_like_the_restatement
    applies unchanged): parameters within the gradient bound, and enough of them moved for that to mean something."""
    from oracle import satrans_oracle as O
    D, H, M, B, LR, EPS, STEPS = 16, 2, 3, 30, 1e-2, 1e-2, 3
    layers = (8, 6)
    torch.manual_seed(4)
    net = _Net(D, H, M, layers)
    g = torch.Generator().manual_seed(8)
    _, _, P = R.draw(B, M, D, layers, True, 12)
    net.cin.load_state_dict(R.state_from_params(P))
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
        Pl = R.params_from_state({k[4:]: v for k, v in leaves.items() if k.startswith("cin.")})
        h = O.selfattention_layer(att, x.double(), H)[0]
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
    """The reference's `metatrans` flag: MetaTransformation -> XDeepFMHead; one backward reaches the scenario embeddings and
    the embedding block."""
    from satrans_amd import MetaTransformation, XDeepFMHead
    B, M, D, S = 40, 5, 16, 3      # (the MetaNet kernels take D in {16, 32, 64, 128})
    torch.manual_seed(6)
    meta = MetaTransformation(D, S, (D, 16, D), init_std=0.3).to(DEV)
    head = XDeepFMHead(M, D, 2, (16, 8), (8, 6), init_std=0.3).to(DEV)
    g = torch.Generator().manual_seed(9)
    emb = torch.randn(B, M, D, generator=g).to(DEV).requires_grad_(True)
    dense, lin = torch.randn(B, 2, generator=g).to(DEV), torch.randn(B, 1, generator=g).to(DEV)
    ids = torch.randint(0, S + 1, (B,), generator=g).to(DEV)
    target = (torch.rand(B, generator=g) > 0.5).float().to(DEV)
    logit = head(meta(ids, emb), dense, lin)
    assert logit.shape == (B, 1)
    F.binary_cross_entropy(torch.sigmoid(logit.squeeze(1)), target, reduction='sum').backward()
    for name, t in (("domain_embeddings.weight", meta.domain_embeddings.weight.grad), ("emb", emb.grad),
                    ("cin.conv1ds.1.weight", head.cin.conv1ds[1].weight.grad)):
        assert t is not None and bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0.0, name
