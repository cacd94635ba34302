"""satrans_amd.layers.PartitionedNorm / MDR_BatchNorm (csrc/pnorm.hip behind torch.autograd.Function) against the fp64
restatement tests/mdr_bn_reference.py on the same seeded inputs; that restatement is pinned to the reference's own
MDR_BatchNorm by the recorded runs of tests/test_mdr_bn_cpu.py.

Bounds (the sibling bounds), all element-wise: y within 2e-5 max|y|; gradients within 1e-4 max|g| + 5e-9; the
saved statistics and the buffers get the y bound relative to their own largest magnitude."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import mdr_bn_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = native.PNORM_ROW_CHUNK
S5, OFFSET = 5, 2
GRADS = ("x", "weight", "bias", "shared_weight", "shared_bias")
check_close = functools.partial(helpers.check_close, "mdr-bn-parity")


def check_grads(got, want, msg):
    assert set(got) == set(want)
    for k in GRADS:
        check_close(got[k], want[k], 1e-4, f"{msg} {k}", what="grad", floor=5e-9)


def ragged_ids(B):
    """The `ragged_ids` pattern of tests/test_siblings_gpu.py: interleaved ids over S = 5 with 0, 1 and 3 filled, 2 and 4 empty."""
    return torch.tensor([0, 1, 3, 3, 1, 0, 3] * (B // 7 + 1))[:B].clone()


def sweep_ids():
    """Scenario 3 runs one row past the kernel's row chunk, scenario 2 has exactly two rows, scenario 4 none."""
    B = next(b for b in range(1, 10 * CHUNK) if int((ragged_ids(b) == 3).sum()) == CHUNK + 1)
    ids = ragged_ids(B)
    ids[[0, 7 * (B // 14)]] = 2
    counts = [int((ids == s).sum()) for s in range(S5)]
    assert counts[3] == CHUNK + 1 and counts[2] == 2 and counts[4] == 0 and min(counts[0], counts[1]) > 2, counts
    return ids


def draw(B, C, S, seed, batches=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batches, B, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + 2 * torch.randn(C, generator=g)
    P = dict(weight=1 + 0.3 * torch.randn(S, C, generator=g), bias=0.3 * torch.randn(S, C, generator=g),
             shared_weight=1 + 0.3 * torch.randn(C, generator=g), shared_bias=0.3 * torch.randn(C, generator=g))
    return x, torch.randn(B, C, generator=g), P


def make_pn(C, S, P, momentum=0.1):
    from satrans_amd import PartitionedNorm
    mod = PartitionedNorm(C, S, momentum=momentum)
    with torch.no_grad():
        for s, bn in enumerate(mod.bns):
            bn.weight.copy_(P["weight"][s])
            bn.bias.copy_(P["bias"][s])
    return mod.to(DEV)


def ref_state(P, track=True):
    S, C = P["weight"].shape
    st = R.State.fresh(S, C, track=track)
    st.weight, st.bias = P["weight"].double(), P["bias"].double()
    return st


def run_pn(mod, x, ids, P, w, offset=0):
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    sw, sb = P["shared_weight"].to(DEV).requires_grad_(True), P["shared_bias"].to(DEV).requires_grad_(True)
    y = mod(xg, ids.to(DEV), sw, sb, offset)
    (y * w.to(DEV)).sum().backward()
    grads = dict(x=xg.grad.cpu(), weight=torch.stack([bn.weight.grad for bn in mod.bns]).cpu(),
                 bias=torch.stack([bn.bias.grad for bn in mod.bns]).cpu(), shared_weight=sw.grad.cpu(), shared_bias=sb.grad.cpu())
    return y.detach().cpu(), grads


def run_ref(st, x, sid, P, w, momentum, training):
    y, cache = R.forward(x.double(), sid, st, P["shared_weight"].double(), P["shared_bias"].double(), 1e-5, momentum, training)
    return y, cache, R.backward(w.double(), cache)


def buffers(mod):
    return (torch.stack([bn.running_mean for bn in mod.bns]).cpu(), torch.stack([bn.running_var for bn in mod.bns]).cpu(),
            [int(bn.num_batches_tracked) for bn in mod.bns])


@pytest.mark.parametrize("C", [1, 33, 64, 608, 1000])
def test_shape_sweep_against_the_restatement(C):
    """Below, at and beyond a channel tile and off the wave width; S = 5 interleaved with an empty scenario, a two-row one and a
    run one row past the row chunk; a non-zero id offset.  Training forward, saved statistics, backward, buffers and counters
    after 1 and 3 steps for momentum 0.1 and None; then the evaluation forward and backward on the updated buffers."""
    ids = sweep_ids()
    x, w, P = draw(ids.numel(), C, S5, 1000 + C)
    for momentum in (0.1, None):
        mod, st = make_pn(C, S5, P, momentum), ref_state(P)
        mod.train()
        for step in (1, 2, 3):
            msg = f"C={C} momentum={momentum} step {step}"
            y, g = run_pn(mod, x[step - 1], ids + OFFSET, P, w, OFFSET)
            y_ref, cache, g_ref = run_ref(st, x[step - 1], ids, P, w, momentum, True)
            check_close(y, y_ref, 2e-5, msg)
            check_grads(g, g_ref, msg)
            stats = mod.last_stats.cpu()
            assert stats.shape == (2, S5, C) and float(stats[:, 4].abs().max()) == 0.0
            check_close(stats[0], cache.mean, 2e-5, msg, "saved mean")
            check_close(stats[1], cache.invstd, 2e-5, msg, "saved invstd")
            if step in (1, 3):
                rm, rv, nbt = buffers(mod)
                check_close(rm, st.running_mean, 2e-5, msg, "running_mean")
                check_close(rv, st.running_var, 2e-5, msg, "running_var")
                assert nbt == st.num_batches_tracked == [step] * S5
                assert torch.equal(rm[4], torch.zeros(C)) and torch.equal(rv[4], torch.ones(C))
        mod.eval()
        y, g = run_pn(mod, x[0], ids + OFFSET, P, w, OFFSET)
        y_ref, cache, g_ref = run_ref(st, x[0], ids, P, w, momentum, False)
        check_close(y, y_ref, 2e-5, f"C={C} momentum={momentum} eval")
        check_grads(g, g_ref, f"C={C} momentum={momentum} eval")
        assert buffers(mod)[2] == [3] * S5


def test_walker_edges_empty_first_scenario_and_an_exact_chunk():
    """The walker's edges that the sweep skips: S = 4 with row counts [0, CHUNK, 0, 2] (the first scenario empty, a run of
    exactly one chunk - no short last chunk - and an empty scenario between two runs), interleaved, a non-zero id offset,
    C = 65 (one channel past a tile), training mode.  An empty scenario's saved statistics are exactly zero, its running
    buffers untouched, its parameter gradients exactly zero."""
    C, S, counts = 65, 4, [0, CHUNK, 0, 2]
    ids = torch.cat([torch.full((n,), s) for s, n in enumerate(counts)])
    ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(41))]
    assert [int((ids == s).sum()) for s in range(S)] == counts
    x, w, P = draw(ids.numel(), C, S, 42, batches=1)
    mod, st = make_pn(C, S, P).train(), ref_state(P)
    y, g = run_pn(mod, x[0], ids + OFFSET, P, w, OFFSET)
    y_ref, cache, g_ref = run_ref(st, x[0], ids, P, w, 0.1, True)
    check_close(y, y_ref, 2e-5, "walker edges")
    check_grads(g, g_ref, "walker edges")
    stats = mod.last_stats.cpu()
    check_close(stats[0], cache.mean, 2e-5, "walker edges", "saved mean")
    check_close(stats[1], cache.invstd, 2e-5, "walker edges", "saved invstd")
    rm, rv, nbt = buffers(mod)
    check_close(rm, st.running_mean, 2e-5, "walker edges", "running_mean")
    check_close(rv, st.running_var, 2e-5, "walker edges", "running_var")
    assert nbt == st.num_batches_tracked == [1] * S
    for s in (0, 2):
        assert float(stats[:, s].abs().max()) == 0.0, s
        assert torch.equal(rm[s], torch.zeros(C)) and torch.equal(rv[s], torch.ones(C)), s
        assert float(g["weight"][s].abs().max()) == 0.0 and float(g["bias"][s].abs().max()) == 0.0, s


def run_one(bn, x, sw, sb, w):
    bn.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    swg, sbg = sw.to(DEV).requires_grad_(True), sb.to(DEV).requires_grad_(True)
    y = bn(xg, swg, sbg)
    (y * w.to(DEV)).sum().backward()
    return y.detach().cpu(), dict(x=xg.grad.cpu(), weight=bn.weight.grad.cpu(), bias=bn.bias.grad.cpu(),
                                  shared_weight=swg.grad.cpu(), shared_bias=sbg.grad.cpu())


def make_one(C, P, s, **kw):
    from satrans_amd import MDR_BatchNorm
    bn = MDR_BatchNorm(C, **kw)
    with torch.no_grad():
        bn.weight.copy_(P["weight"][s])
        bn.bias.copy_(P["bias"][s])
    return bn.to(DEV)


def test_without_running_stats_the_batch_normalises_in_both_modes():
    """track_running_stats=False: no buffers, no counter; training and evaluation both use the batch's statistics."""
    C, n = 70, CHUNK + 9
    x, w, P = draw(n, C, 1, 77, batches=1)
    bn = make_one(C, P, 0, track_running_stats=False)
    sid = torch.zeros(n, dtype=torch.long)
    for training in (True, False):
        bn.train(training)
        y, g = run_one(bn, x[0], P["shared_weight"], P["shared_bias"], w)
        y_ref, _, g_ref = run_ref(ref_state(P, track=False), x[0], sid, P, w, 0.1, training)
        g_ref = {k: (v[0] if k in ("weight", "bias") else v) for k, v in g_ref.items()}
        check_close(y, y_ref, 2e-5, f"untracked training={training}")
        check_grads(g, g_ref, f"untracked training={training}")
        assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None


def test_conditioning_against_torch_fp32():
    """Rows of mean 100 and standard deviation 0.1 over two scenarios: the kernel's error against fp64 is at most 4x that of
    torch's fp32 CPU F.batch_norm on the same rows (two fp32 implementations differ by their summation order; E[x^2] - E[x]^2
    would be thousands of times off - tests/test_mdr_bn_cpu.py::test_conditioning_premise)."""
    x = R.conditioning_rows()
    n, C = x.shape
    ids = torch.tensor([0, 1] * (n // 2))
    P = dict(weight=torch.ones(2, C), bias=torch.zeros(2, C), shared_weight=torch.ones(C), shared_bias=torch.zeros(C))
    mod = make_pn(C, 2, P).train()
    with torch.no_grad():
        y = mod(x.to(DEV), ids.to(DEV), P["shared_weight"].to(DEV), P["shared_bias"].to(DEV)).cpu()
    y_ref, _ = R.forward(x.double(), ids, ref_state(P), P["shared_weight"].double(), P["shared_bias"].double())
    torch_err = 0.0
    for s in (0, 1):
        rows = ids == s
        y_torch = F.batch_norm(x[rows], None, None, None, None, True, 0.0, 1e-5)
        torch_err = max(torch_err, float((y_torch.double() - y_ref[rows]).abs().max()))
    err = float((y.double() - y_ref).abs().max())
    print(f"[mdr-bn-parity] conditioning: kernel error {err:.3e}, torch fp32 CPU error {torch_err:.3e}, ratio {err / torch_err:.3f}")
    assert err <= 4 * torch_err, (err, torch_err)


def test_many_chunks():
    """B = 20,000 rows, C = 608, S = 4: 150 and more chunks, ten channel tiles; training forward + backward."""
    B, C, S = 20000, 608, 4
    x, w, P = draw(B, C, S, 20000, batches=1)
    ids = torch.randint(0, S, (B,), generator=torch.Generator().manual_seed(5))
    mod, st = make_pn(C, S, P).train(), ref_state(P)
    y, g = run_pn(mod, x[0], ids, P, w)
    y_ref, _, g_ref = run_ref(st, x[0], ids, P, w, 0.1, True)
    check_close(y, y_ref, 2e-5, "many chunks")
    check_grads(g, g_ref, "many chunks")
    rm, rv, _ = buffers(mod)
    check_close(rm, st.running_mean, 2e-5, "many chunks", "running_mean")
    check_close(rv, st.running_var, 2e-5, "many chunks", "running_var")


def test_single_scenario_equals_the_partition_bit_for_bit():
    """MDR_BatchNorm on one scenario's rows == PartitionedNorm's result for that scenario: outputs, buffers and gradients.
    The shared gradients sum over scenarios, so they are compared on a batch that holds this scenario alone."""
    C, s = 33, 3
    ids = sweep_ids()
    x, w, P = draw(ids.numel(), C, S5, 3)
    rows = ids == s
    sw, sb = P["shared_weight"], P["shared_bias"]
    mixed, alone, one = make_pn(C, S5, P).train(), make_pn(C, S5, P).train(), make_one(C, P, s).train()
    y_m, g_m = run_pn(mixed, x[0], ids, P, w)
    y_a, g_a = run_pn(alone, x[0][rows], ids[rows], P, w[rows])
    y_1, g_1 = run_one(one, x[0][rows], sw, sb, w[rows])
    assert torch.equal(y_1, y_m[rows]) and torch.equal(y_1, y_a)
    assert torch.equal(g_1["x"], g_m["x"][rows]) and torch.equal(g_1["x"], g_a["x"])
    for k in ("weight", "bias"):
        assert torch.equal(g_1[k], g_m[k][s]) and torch.equal(g_1[k], g_a[k][s]), k
    for k in ("shared_weight", "shared_bias"):
        assert torch.equal(g_1[k], g_a[k]), k
    for mod in (mixed, alone):
        bn = mod.bns[s]
        assert torch.equal(one.running_mean, bn.running_mean) and torch.equal(one.running_var, bn.running_var)
        assert int(one.num_batches_tracked) == int(bn.num_batches_tracked) == 1
    assert torch.equal(one.last_stats[:, 0], mixed.last_stats[:, s])


def test_two_runs_agree_bit_for_bit():
    C = 100
    ids = sweep_ids()
    x, w, P = draw(ids.numel(), C, S5, 11, batches=1)
    runs = []
    for _ in range(2):
        mod = make_pn(C, S5, P).train()
        y, g = run_pn(mod, x[0], ids, P, w)
        runs.append((y, g, buffers(mod)))
    (y0, g0, b0), (y1, g1, b1) = runs
    assert torch.equal(y0, y1)
    for k in GRADS:
        assert torch.equal(g0[k], g1[k]), k
    assert torch.equal(b0[0], b1[0]) and torch.equal(b0[1], b1[1]) and b0[2] == b1[2]


def test_errors():
    from satrans_amd import MDR_BatchNorm, PartitionedNorm
    C, B = 20, 37
    x, w, P = draw(B, C, S5, 9, batches=1)
    ids = ragged_ids(B)
    ids[B // 3] = 2                                       # ONE row in scenario 2
    mod = make_pn(C, S5, P).train()
    sw, sb = P["shared_weight"].to(DEV), P["shared_bias"].to(DEV)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        mod(x[0].to(DEV), ids.to(DEV), sw, sb)
    rm, rv, nbt = buffers(mod)
    assert torch.equal(rm, torch.zeros(S5, C)) and torch.equal(rv, torch.ones(S5, C)) and nbt == [0] * S5
    mod.eval()                                            # the same batch in evaluation mode works
    y, g = run_pn(mod, x[0], ids, P, w)
    y_ref, _, g_ref = run_ref(ref_state(P), x[0], ids, P, w, 0.1, False)
    check_close(y, y_ref, 2e-5, "one-row scenario, eval")
    check_grads(g, g_ref, "one-row scenario, eval")
    assert buffers(mod)[2] == [0] * S5
    mod.train()
    for bad in (-1, S5):
        off = ragged_ids(B)
        off[5] = bad
        with pytest.raises(IndexError):
            mod(x[0].to(DEV), off.to(DEV), sw, sb)
    with pytest.raises(IndexError):                       # the offset moves the accepted range
        mod(x[0].to(DEV), ragged_ids(B).to(DEV), sw, sb, 1)
    assert buffers(mod)[2] == [0] * S5
    with pytest.raises(NotImplementedError, match="2-D"):
        mod(torch.zeros(4, C, 3, device=DEV), torch.zeros(4, device=DEV), sw, sb)
    with pytest.raises(NotImplementedError, match="2-D"):
        MDR_BatchNorm(C).to(DEV)(torch.zeros(4, C, 3, device=DEV), sw, sb)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        MDR_BatchNorm(C).to(DEV)(torch.zeros(1, C, device=DEV), sw, sb)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        PartitionedNorm(C, S5)(x[0], ids, P["shared_weight"], P["shared_bias"])
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        MDR_BatchNorm(C)(x[0], P["shared_weight"], P["shared_bias"])


class _Net(nn.Module):
    def __init__(self, D, H, Fn, S):
        super().__init__()
        from satrans_amd import PartitionedNorm, SelfAttention_Layer
        self.att = SelfAttention_Layer(D, head_num=H)
        self.pn = PartitionedNorm(Fn * D, S)
        self.shared_bn_weight = nn.Parameter(torch.ones(Fn * D))
        self.shared_bn_bias = nn.Parameter(torch.zeros(Fn * D))
        self.lin = nn.Linear(Fn * D, 1)

    def forward(self, x, ids):
        h = self.att(x).flatten(1)
        return self.lin(self.pn(h, ids, self.shared_bn_weight, self.shared_bn_bias)).squeeze(1)


def test_composition_trains_like_the_restatement():
    """SelfAttention_Layer -> flatten -> PartitionedNorm -> nn.Linear, two Adam steps: autograd through the stacked per-scenario
    parameters and back into each bns.{i}.  The attention layer is in evaluation mode (no dropout to replay).

    Adam with lr = eps = 1e-2.  An Adam step, lr * m / (sqrt(v) + eps), changes by at most lr / eps times an error of the
    gradient, so the gradient bound carries over to the parameters only for lr / eps <= 1.  It matters for one parameter here:
    the gradient of the attention's LayerNorm bias is zero analytically (the batch normalisation removes a per-channel
    constant; 1.6e-15 in fp64) and rounding residue in ANY fp32 run - 1.0e-6 in torch's own fp32 CPU run of this model, which
    with eps = 1e-3 (lr / eps = 10) lands 2.1x outside the bound, as the kernels did at 1.5x (1.38e-5 against 8.98e-6)."""
    from oracle import satrans_oracle as O
    D, H, Fn, S, B, LR, EPS = 16, 2, 3, 3, 30, 1e-2, 1e-2
    torch.manual_seed(4)
    net = _Net(D, H, Fn, S)
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.startswith("att.W_"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif k.startswith("pn.") or k.startswith("shared"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    x, target = torch.randn(B, Fn, D, generator=g), torch.randn(B, generator=g)
    ids = torch.tensor([0, 1, 2, 1, 0] * (B // 5))
    start = {k: v.detach().clone() for k, v in net.named_parameters()}
    # fp64 restatement
    leaves = {k: v.double().requires_grad_(True) for k, v in start.items()}
    att = {k[4:]: v for k, v in leaves.items() if k.startswith("att.")}
    st = R.State.fresh(S, Fn * D)
    opt = torch.optim.Adam([v for k, v in leaves.items() if k != "att.W_Out"], lr=LR, eps=EPS)
    for _ in range(2):
        opt.zero_grad()
        st.weight = torch.stack([leaves[f"pn.bns.{s}.weight"] for s in range(S)])
        st.bias = torch.stack([leaves[f"pn.bns.{s}.bias"] for s in range(S)])
        h = O.selfattention_layer(att, x.double(), H)[0].flatten(1)
        h, _ = R.forward(h, ids, st, leaves["shared_bn_weight"], leaves["shared_bn_bias"])
        out = F.linear(h, leaves["lin.weight"], leaves["lin.bias"]).squeeze(1)
        ((out - target.double()) ** 2).mean().backward()
        opt.step()
    # the modules on the GPU
    net = net.to(DEV).train()
    net.att.eval()
    opt = torch.optim.Adam(net.parameters(), lr=LR, eps=EPS)
    for _ in range(2):
        opt.zero_grad()
        ((net(x.to(DEV), ids.to(DEV)) - target.to(DEV)) ** 2).mean().backward()
        opt.step()
    moved = 0
    for k, p in net.named_parameters():
        want = leaves[k].detach()
        check_close(p.detach().cpu(), want, 1e-4, f"composition {k}", what="parameter", floor=5e-9)
        moved += float((want - start[k].double()).abs().max()) > 10 * (1e-4 * float(want.abs().max()) + 5e-9)
    assert moved >= 10, moved      # the check above is not satisfied by parameters that stood still
    rm, rv, nbt = buffers(net.pn)
    check_close(rm, st.running_mean, 2e-5, "composition", "running_mean")
    check_close(rv, st.running_var, 2e-5, "composition", "running_var")
    assert nbt == [2] * S
