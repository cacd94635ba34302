"""satrans_amd.layers.StarTowers / StarHead (csrc/star.hip behind torch.autograd.Function) against the fp64 restatement
tests/star_reference.py on the same seeded inputs; that restatement is pinned to the reference's own Star_Net.forward by the
recorded runs of tests/test_star_cpu.py.

Bounds (the sibling bounds), all element-wise: logit and saved hidden rows within 2e-5 max|.|; gradients within
1e-4 max|g| + 5e-9; buffers get the output bound relative to their own largest magnitude.
tests/test_star_cpu.py::test_premise_of_the_gpu_bounds pins their margin."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import mdr_bn_reference as BN
from tests import star_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, CHUNK = native.STAR_ROW_TILE, native.STAR_DW_ROW_CHUNK
S5, OFFSET = 5, 2
check_close = functools.partial(helpers.check_close, "star-parity")


def check_grads(got, want, msg):
    check_close(got["x"], want["x"], 1e-4, f"{msg} x", what="grad", floor=5e-9)
    for k in R.GROUPS:
        assert len(got[k]) == len(want[k])
        for l, (a, b) in enumerate(zip(got[k], want[k])):
            check_close(a, b, 1e-4, f"{msg} {k}[{l}]", what="grad", floor=5e-9)


def load_towers(mod, P):
    """Set a StarTowers / StarHead's tower parameters from the stacked form."""
    H = len(mod.hidden_units)
    with torch.no_grad():
        for l in range(H + 1):
            for s in range(mod.num_domains):
                lin = mod.domain_dnns[s].linears[l] if l < H else mod.domain_dnn_linears[s]
                lin.weight.copy_(P["w_dom"][l][s])
                lin.bias.copy_(P["b_dom"][l][s])
            lin = mod.shared_dnn.linears[l] if l < H else mod.shared_dnn_linear
            lin.weight.copy_(P["w_sh"][l])
            lin.bias.copy_(P["b_sh"][l])
    return mod


def make_towers(C, hidden, S, P):
    from satrans_amd import StarTowers
    return load_towers(StarTowers(C, hidden, S), P).to(DEV)


def tower_grads(mod):
    H, S = len(mod.hidden_units), mod.num_domains
    dom = [[mod.domain_dnns[s].linears[l] for s in range(S)] for l in range(H)] + [list(mod.domain_dnn_linears)]
    sh = list(mod.shared_dnn.linears) + [mod.shared_dnn_linear]
    return dict(w_dom=[torch.stack([m.weight.grad for m in layer]).cpu() for layer in dom],
                b_dom=[torch.stack([m.bias.grad for m in layer]).cpu() for layer in dom],
                w_sh=[m.weight.grad.cpu() for m in sh], b_sh=[m.bias.grad.cpu() for m in sh])


def run(mod, x, ids, w, offset=0):
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg, ids.to(DEV), offset)
    (y * w.to(DEV)).sum().backward()
    g = tower_grads(mod)
    g["x"] = xg.grad.cpu()
    return y.detach().cpu(), g


def run_ref(x, sid, P, w):
    y, cache = R.forward(x.double(), sid, R.double(P))
    return y, cache, R.backward(w.double(), cache)


@pytest.mark.parametrize("C,hidden", [(1, (16,)), (33, (48, 32)), (609, (256, 128)), (64, (16, 16, 16, 16))])
def test_shape_sweep_against_the_restatement(C, hidden):
    """K tails (1, 33, 609), widths off the 64-column tile, 1 to 4 hidden layers; S = 5 interleaved with a non-zero id offset:
    one scenario one row past the row tile, one one row past the weight-gradient chunk, one with a single row, one empty.
    Forward, saved hidden rows, every gradient; the empty scenario's parameter gradients are exactly zero."""
    ids = R.sweep_ids(TILE, CHUNK)
    x, w, P = R.draw(ids.numel(), C, hidden, S5, 1000 + C)
    mod = make_towers(C, hidden, S5, P)
    msg = f"C={C} hidden={hidden}"
    y, g = run(mod, x, ids + OFFSET, w, OFFSET)
    y_ref, cache, g_ref = run_ref(x, ids, P, w)
    assert y.shape == (ids.numel(), 1)
    check_close(y, y_ref, 2e-5, msg)
    assert len(mod.last_hidden) == len(hidden)
    for l, h in enumerate(mod.last_hidden):
        check_close(h.cpu(), cache.h[l + 1], 2e-5, f"{msg} hidden {l}", "hidden")
    check_grads(g, g_ref, msg)
    for k in ("w_dom", "b_dom"):
        for l, t in enumerate(g[k]):
            assert float(t[4].abs().max()) == 0.0, (k, l)
    assert float(g["b_dom"][-1][2].abs().max()) > 0.0      # the one-row scenario is not skipped


def test_walker_edges_empty_first_scenario_and_an_exact_chunk():
    """The walker's edges that the sweep skips: S = 4 with row counts [0, CHUNK, 0, TILE + 1] (the first scenario empty, a run
    of exactly one weight-gradient chunk = whole row tiles with no short last one, an empty scenario between two runs),
    interleaved, a non-zero id offset.  The empty scenarios' parameter gradients are exactly zero."""
    C, hidden, S, counts = 33, (48, 32), 4, [0, CHUNK, 0, TILE + 1]
    ids = torch.cat([torch.full((n,), s) for s, n in enumerate(counts)])
    ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(41))]
    assert [int((ids == s).sum()) for s in range(S)] == counts
    x, w, P = R.draw(ids.numel(), C, hidden, S, 42)
    mod = make_towers(C, hidden, S, P)
    y, g = run(mod, x, ids + OFFSET, w, OFFSET)
    y_ref, cache, g_ref = run_ref(x, ids, P, w)
    check_close(y, y_ref, 2e-5, "walker edges")
    for l, h in enumerate(mod.last_hidden):
        check_close(h.cpu(), cache.h[l + 1], 2e-5, f"walker edges hidden {l}", "hidden")
    check_grads(g, g_ref, "walker edges")
    for k in ("w_dom", "b_dom"):
        for l, t in enumerate(g[k]):
            assert float(t[0].abs().max()) == 0.0 and float(t[2].abs().max()) == 0.0, (k, l)
            assert float(t[1].abs().max()) > 0.0 and float(t[3].abs().max()) > 0.0, (k, l)


def test_batch_smaller_than_a_tile():
    B, C, hidden = 5, 20, (24, 8)
    x, w, P = R.draw(B, C, hidden, 3, 5)
    ids = torch.full((B,), 1)
    y, g = run(make_towers(C, hidden, 3, P), x, ids, w)
    y_ref, _, g_ref = run_ref(x, ids, P, w)
    check_close(y, y_ref, 2e-5, "B < tile")
    check_grads(g, g_ref, "B < tile")


def test_many_tiles():
    """B = 20,000 rows, C = 608, (256, 128), S = 4: 300 and more row tiles, 80 weight-gradient chunks; forward + backward.

    7.7 million hidden elements: in the plain draw the fp64 forward puts one pre-activation (row 9433, unit 95 of the second
    layer) at -1.2e-7 under a largest activation of 5.6, where fp32 rounding decides the side of relu's kink; the kernel's 1.9e-7
    there is inside the output bound 300 times over, and the other side moves that one row of dx by 3.4e-4 of max|dx| while
    every other row agrees to 5.2e-7.  So the rows whose fp64 pre-activations come within the output bound of zero are drawn
    again (R.redraw_rows_at_a_kink, decided by the fp64 forward alone); all 20,000 rows are then held to the bounds."""
    B, C, hidden, S = 20000, 608, (256, 128), 4
    x, w, P = R.draw(B, C, hidden, S, 20000)
    ids = torch.randint(0, S, (B,), generator=torch.Generator().manual_seed(5))
    x, redrawn = R.redraw_rows_at_a_kink(x, ids, P, 2e-5, 20001)
    assert 0 < redrawn < B // 10      # the bulk of the batch is the plain draw
    y, g = run(make_towers(C, hidden, S, P), x, ids, w)
    y_ref, _, g_ref = run_ref(x, ids, P, w)
    check_close(y, y_ref, 2e-5, "many tiles")
    check_grads(g, g_ref, "many tiles")


def test_single_scenario_equals_the_mix_bit_for_bit():
    """A scenario's rows alone (a one-scenario StarTowers; and the S = 5 module on a batch holding that scenario alone) ==
    the same rows inside the mixed batch: logits, dx rows and the scenario's parameter gradients.  The shared gradients sum
    over scenarios, so they are compared on the batch that holds this scenario alone."""
    C, hidden, s = 33, (48, 32), 3
    ids = R.sweep_ids(TILE, CHUNK)
    x, w, P = R.draw(ids.numel(), C, hidden, S5, 3)
    rows = ids == s
    P1 = {k: [t[s:s + 1] if k.endswith("dom") else t for t in v] for k, v in P.items()}
    y_m, g_m = run(make_towers(C, hidden, S5, P), x, ids, w)
    y_a, g_a = run(make_towers(C, hidden, S5, P), x[rows], ids[rows], w[rows])
    y_1, g_1 = run(make_towers(C, hidden, 1, P1), x[rows], torch.zeros(int(rows.sum()), dtype=torch.long), w[rows])
    assert torch.equal(y_1, y_m[rows]) and torch.equal(y_1, y_a)
    assert torch.equal(g_1["x"], g_m["x"][rows]) and torch.equal(g_1["x"], g_a["x"])
    for l in range(len(hidden) + 1):
        for k in ("w_dom", "b_dom"):
            assert torch.equal(g_1[k][l][0], g_m[k][l][s]) and torch.equal(g_1[k][l][0], g_a[k][l][s]), (k, l)
        for k in ("w_sh", "b_sh"):
            assert torch.equal(g_1[k][l], g_a[k][l]), (k, l)


def test_two_runs_agree_bit_for_bit():
    C, hidden = 100, (80, 24)
    ids = R.sweep_ids(TILE, CHUNK)
    x, w, P = R.draw(ids.numel(), C, hidden, S5, 11)
    (y0, g0), (y1, g1) = (run(make_towers(C, hidden, S5, P), x, ids, w) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(g0["x"], g1["x"])
    for k in R.GROUPS:
        for a, b in zip(g0[k], g1[k]):
            assert torch.equal(a, b), k


def draw_bn(C, S, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(weight=1 + 0.3 * torch.randn(S, C, generator=g), bias=0.3 * torch.randn(S, C, generator=g),
                shared_weight=1 + 0.3 * torch.randn(C, generator=g), shared_bias=0.3 * torch.randn(C, generator=g))


def make_head(C, hidden, S, P, Q, use_domain_bn=True):
    from satrans_amd import StarHead
    mod = load_towers(StarHead(C, hidden, S, use_domain_bn=use_domain_bn), P)
    with torch.no_grad():
        mod.shared_bn_weight.copy_(Q["shared_weight"])
        mod.shared_bn_bias.copy_(Q["shared_bias"])
        if use_domain_bn:
            for s, bn in enumerate(mod.bns):
                bn.weight.copy_(Q["weight"][s])
                bn.bias.copy_(Q["bias"][s])
    return mod.to(DEV)


def head_grads(mod, g):
    g["bn"] = dict(weight=torch.stack([bn.weight.grad for bn in mod.bns]).cpu(), bias=torch.stack([bn.bias.grad for bn in mod.bns]).cpu(),
                   shared_weight=mod.shared_bn_weight.grad.cpu(), shared_bias=mod.shared_bn_bias.grad.cpu())
    return g


def head_buffers(mod):
    return (torch.stack([bn.running_mean for bn in mod.bns]).cpu(), torch.stack([bn.running_var for bn in mod.bns]).cpu(),
            [int(bn.num_batches_tracked) for bn in mod.bns])


def bn_ids(B):
    """S = 5 interleaved, every filled scenario with at least two rows, scenario 4 empty."""
    return torch.tensor([0, 1, 3, 3, 1, 0, 3, 2] * (B // 8 + 1))[:B].clone()


def test_head_against_the_restatements():
    """StarHead = partitioned normalisation (tests/mdr_bn_reference.py) then the towers: two training steps (batch statistics,
    buffers, num_batches_tracked; the second with ids shifted by an offset), then evaluation on the updated buffers; gradients of
    the towers, bns.{s}.*, shared_bn_* and the input.  With use_domain_bn=False it is StarTowers bit for bit."""
    C, hidden, B = 70, (48, 32), 2 * TILE + 9
    ids = bn_ids(B)
    x, w, P = R.draw(B, C, hidden, S5, 21)
    x2 = torch.randn(B, C, generator=torch.Generator().manual_seed(22)) * 1.5 + 0.5
    Q = draw_bn(C, S5, 23)
    mod = make_head(C, hidden, S5, P, Q).train()
    st = BN.State.fresh(S5, C)
    st.weight, st.bias = Q["weight"].double(), Q["bias"].double()
    sw, sb = Q["shared_weight"].double(), Q["shared_bias"].double()
    for step, (xs, offset, training) in enumerate([(x, 0, True), (x2, OFFSET, True), (x, 0, False)]):
        mod.train(training)
        msg = f"head step {step} training={training}"
        y, g = run(mod, xs, ids + offset, w, offset)
        g = head_grads(mod, g)
        y_ref, caches = R.head_forward(xs.double(), ids, R.double(P), st, sw, sb, training=training)
        g_ref = R.head_backward(w.double(), caches)
        check_close(y, y_ref, 2e-5, msg)
        check_grads(g, g_ref, msg)
        for k in ("weight", "bias", "shared_weight", "shared_bias"):
            check_close(g["bn"][k], g_ref["bn"][k], 1e-4, f"{msg} bn {k}", what="grad", floor=5e-9)
        rm, rv, nbt = head_buffers(mod)
        check_close(rm, st.running_mean, 2e-5, msg, "running_mean")
        check_close(rv, st.running_var, 2e-5, msg, "running_var")
        assert nbt == st.num_batches_tracked == [min(step + 1, 2)] * S5
    plain = make_head(C, hidden, S5, P, Q, use_domain_bn=False)
    y_h, g_h = run(plain, x, ids, w)
    y_t, g_t = run(make_towers(C, hidden, S5, P), x, ids, w)
    assert torch.equal(y_h, y_t) and torch.equal(g_h["x"], g_t["x"])
    for k in R.GROUPS:
        for a, b in zip(g_h[k], g_t[k]):
            assert torch.equal(a, b), k
    assert plain.shared_bn_weight.grad is None


def test_errors():
    from satrans_amd import StarHead, StarTowers
    C, hidden, B = 20, (16, 8), 37
    x, w, P = R.draw(B, C, hidden, S5, 9)
    Q = draw_bn(C, S5, 10)
    ids = bn_ids(B)
    ids[ids == 2] = 0
    ids[B // 3] = 2                                       # ONE row in scenario 2
    head = make_head(C, hidden, S5, P, Q).train()
    fresh = (torch.zeros(S5, C), torch.ones(S5, C), [0] * S5)

    def untouched():
        rm, rv, nbt = head_buffers(head)
        return torch.equal(rm, fresh[0]) and torch.equal(rv, fresh[1]) and nbt == fresh[2]

    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        head(x.to(DEV), ids.to(DEV))
    assert untouched()
    for bad in (-1, S5):
        off = bn_ids(B)
        off[5] = bad
        with pytest.raises(IndexError):
            head(x.to(DEV), off.to(DEV))
        with pytest.raises(IndexError):
            make_towers(C, hidden, S5, P)(x.to(DEV), off.to(DEV))
    with pytest.raises(IndexError):                       # the offset moves the accepted range
        head(x.to(DEV), bn_ids(B).to(DEV), 1)
    assert untouched()
    head.eval()                                           # the same batch in evaluation mode works
    y, g = run(head, x, ids, w)
    st = BN.State.fresh(S5, C)
    st.weight, st.bias = Q["weight"].double(), Q["bias"].double()
    y_ref, caches = R.head_forward(x.double(), ids, R.double(P), st, Q["shared_weight"].double(), Q["shared_bias"].double(),
                                   training=False)
    check_close(y, y_ref, 2e-5, "one-row scenario, eval")
    check_grads(g, R.head_backward(w.double(), caches), "one-row scenario, eval")
    assert untouched()
    y, g = run(make_towers(C, hidden, S5, P), x, ids, w)      # ... and with the towers alone
    y_ref, _, g_ref = run_ref(x, ids, P, w)
    check_close(y, y_ref, 2e-5, "one-row scenario, towers")
    check_grads(g, g_ref, "one-row scenario, towers")
    for cls in (StarTowers, StarHead):
        with pytest.raises(native.NativeError, match="no CPU fallback"):
            cls(C, hidden, S5)(x, ids)
        with pytest.raises(TypeError, match="float32"):
            cls(C, hidden, S5).to(DEV)(x.to(DEV).double(), ids.to(DEV))
        with pytest.raises(ValueError):
            cls(C, hidden, S5).to(DEV)(x[:, :5].to(DEV), ids.to(DEV))


class _Net(nn.Module):
    def __init__(self, D, H, Fn, S, hidden):
        super().__init__()
        from satrans_amd import SelfAttention_Layer, StarHead
        self.att = SelfAttention_Layer(D, head_num=H)
        self.head = StarHead(Fn * D, hidden, S)

    def forward(self, x, ids):
        return self.head(self.att(x).flatten(1), ids).squeeze(1)


def test_composition_trains_like_the_restatement():
    """SelfAttention_Layer (evaluation mode) -> flatten -> StarHead -> BCE with logits, two Adam steps with lr = eps = 1e-2:
    autograd through the stacked per-scenario parameters and back into each module.  lr / eps <= 1, so an error of the gradient
    moves a parameter by at most as much (the argument of tests/test_mdr_bn_gpu.py::test_composition_trains_like_the_restatement
    applies unchanged): parameters within the gradient bound, buffers within the output bound."""
    from oracle import satrans_oracle as O
    D, H, Fn, S, B, LR, EPS, hidden = 16, 2, 3, 3, 30, 1e-2, 1e-2, (16, 8)
    torch.manual_seed(4)
    net = _Net(D, H, Fn, S, hidden)
    g = torch.Generator().manual_seed(8)
    _, _, P = R.draw(B, Fn * D, hidden, S, 12)
    load_towers(net.head, P)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.startswith("att.W_"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif k.startswith("head.bns.") or k.startswith("head.shared_bn"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    x, target = torch.randn(B, Fn, D, generator=g), (torch.rand(B, generator=g) > 0.5).float()
    ids = torch.tensor([0, 1, 2, 1, 0] * (B // 5))
    start = {k: v.detach().clone() for k, v in net.named_parameters()}
    # fp64 restatement
    leaves = {k: v.double().requires_grad_(True) for k, v in start.items()}
    att = {k[4:]: v for k, v in leaves.items() if k.startswith("att.")}
    st = BN.State.fresh(S, Fn * D)
    opt = torch.optim.Adam([v for k, v in leaves.items() if k != "att.W_Out"], lr=LR, eps=EPS)
    for _ in range(2):
        opt.zero_grad()
        st.weight = torch.stack([leaves[f"head.bns.{s}.weight"] for s in range(S)])
        st.bias = torch.stack([leaves[f"head.bns.{s}.bias"] for s in range(S)])
        Pl = R.params_from_state({k[5:]: v for k, v in leaves.items() if k.startswith("head.")}, S, len(hidden))
        h = O.selfattention_layer(att, x.double(), H)[0].flatten(1)
        out, _ = R.head_forward(h, ids, Pl, st, leaves["head.shared_bn_weight"], leaves["head.shared_bn_bias"])
        F.binary_cross_entropy_with_logits(out.squeeze(1), target.double()).backward()
        opt.step()
    # the modules on the GPU
    net = net.to(DEV).train()
    net.att.eval()
    opt = torch.optim.Adam(net.parameters(), lr=LR, eps=EPS)
    for _ in range(2):
        opt.zero_grad()
        F.binary_cross_entropy_with_logits(net(x.to(DEV), ids.to(DEV)), target.to(DEV)).backward()
        opt.step()
    moved = 0
    for k, p in net.named_parameters():
        want = leaves[k].detach()
        check_close(p.detach().cpu(), want, 1e-4, f"composition {k}", what="parameter", floor=5e-9)
        moved += float((want - start[k].double()).abs().max()) > 10 * (1e-4 * float(want.abs().max()) + 5e-9)
    assert moved >= 10, moved      # the check above is not satisfied by parameters that stood still
    rm, rv, nbt = head_buffers(net.head)
    check_close(rm, st.running_mean, 2e-5, "composition", "running_mean")
    check_close(rv, st.running_var, 2e-5, "composition", "running_var")
    assert nbt == [2] * S
