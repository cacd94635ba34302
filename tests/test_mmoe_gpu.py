"""satrans_amd.layers.MMoEHead (csrc/mmoe.hip behind torch.autograd.Function) against the fp64 restatement
tests/mmoe_reference.py on the same seeded inputs; that restatement is pinned to the reference's own MMOE.forward by the
recorded runs of tests/test_mmoe_cpu.py.

Bounds (the sibling bounds), all element-wise: logits, saved gates and mixtures within 2e-5 max|.|; gradients
within 1e-4 max|g| + 5e-9.  tests/test_mmoe_cpu.py::test_premise_of_the_gpu_bounds pins their margin."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import mmoe_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, CHUNK = native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK
check_close = functools.partial(helpers.check_close, "mmoe-parity")


def dims(P):
    return P["expert_w"][0].shape[0], P["out_bias"].shape[0], len(P["expert_w"]), len(P["gate_w"]), len(P["tower_w"])


def make_head(C, P):
    """An MMoEHead of the shapes of P holding its values."""
    from satrans_amd import MMoEHead
    E, T, _, _, _ = dims(P)
    units = lambda k: tuple(w.shape[1] for w in P[k])      # noqa: E731
    mod = MMoEHead(C, T, E, units("expert_w"), units("gate_w"), units("tower_w"))
    mod.load_state_dict({k: v.clone() for k, v in R.state_from_params(P).items()})
    return mod.to(DEV)


def run(mod, x, ids, w, offset=0):
    """logit, {gradients keyed as R.flat keys them, "x"}, gates, mixture - all on the host."""
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg, ids.to(DEV), offset)
    (y * w.to(DEV)).sum().backward()
    E, T, nx, ng, nt = mod.num_experts, mod.num_tasks, len(mod.expert_dnn_hidden_units), len(mod.gate_dnn_hidden_units), \
        len(mod.tower_dnn_hidden_units)
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in mod.named_parameters()}, E, T, nx, ng, nt, dtype=torch.float32))
    g["x"] = xg.grad.cpu()
    return y.detach().cpu(), g, mod.last_gates.cpu(), mod.last_mixture.cpu()


def run_ref(x, sid, P, w):
    y, cache = R.forward(x.double(), sid, R.double(P))
    return y, cache, R.flat(R.backward(w.double(), cache))


def check_all(got, ref, msg):
    (y, g, gates, mix), (y_ref, cache, g_ref) = got, ref
    assert y.shape == (y_ref.shape[0], 1)
    check_close(y, y_ref, 2e-5, msg)
    check_close(gates, cache.gates, 2e-5, msg, "gates")
    check_close(mix, cache.th[0], 2e-5, msg, "mixture")
    assert sorted(g) == sorted(g_ref)
    for k in g_ref:
        check_close(g[k], g_ref[k], 1e-4, f"{msg} {k}", what="grad", floor=5e-9)


def routed_keys(g):
    return [k for k in g if k.split("[")[0] in R.ROUTED]


def counted_ids(counts, seed):
    ids = torch.cat([torch.full((n,), s, dtype=torch.long) for s, n in enumerate(counts)])
    ids = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(seed))]
    assert [int((ids == s).sum()) for s in range(len(counts))] == list(counts)
    return ids


@pytest.mark.parametrize("case", R.SWEEP, ids=lambda c: f"C{c[0]}-E{c[1]}")
def test_shape_sweep_against_the_restatement(case):
    """C in {1, 33, 609}, E in {2, 3, 8}, 1 to 3 expert layers, 0 to 3 gate and tower layers, widths off the 64-column tile;
    T = 5 interleaved with a non-zero id offset: one task one row past the row tile, one one row past the weight-gradient chunk,
    one with a single row, one empty.  Logit, gates, mixture, every gradient; the empty task's parameter gradients are exactly
    zero, the one-row task's are not."""
    ids, x, w, P = R.sweep_draw(case, TILE, CHUNK)
    got = run(make_head(case[0], P), x, ids + R.SWEEP_OFFSET, w, R.SWEEP_OFFSET)
    check_all(got, run_ref(x, ids, P, w), f"sweep {case}")
    g = got[1]
    for k in routed_keys(g):
        assert float(g[k][4].abs().max()) == 0.0, k
        assert float(g[k][2].abs().max()) > 0.0, k      # the one-row task is not skipped


def test_walker_edges_empty_first_task_and_an_exact_chunk():
    """T = 4 with row counts [0, CHUNK, 0, TILE + 1]: the first task empty, a run of exactly one weight-gradient chunk, an
    empty task between two runs; interleaved, a non-zero id offset."""
    C, counts = 33, [0, CHUNK, 0, TILE + 1]
    ids = counted_ids(counts, 41)
    x, w, P = R.draw(ids.numel(), C, 4, 3, (48, 32), (8,), (64,), 42, sid=ids)
    got = run(make_head(C, P), x, ids + 2, w, 2)
    check_all(got, run_ref(x, ids, P, w), "walker edges")
    g = got[1]
    for k in routed_keys(g):
        assert float(g[k][0].abs().max()) == 0.0 and float(g[k][2].abs().max()) == 0.0, k
        assert float(g[k][1].abs().max()) > 0.0 and float(g[k][3].abs().max()) > 0.0, k


def test_batch_smaller_than_a_tile():
    B, C = 5, 20
    ids = torch.tensor([1, 1, 0, 1, 1])
    x, w, P = R.draw(B, C, 3, 2, (24, 8), (8,), (), 5, sid=ids)
    check_all(run(make_head(C, P), x, ids, w), run_ref(x, ids, P, w), "B < tile")


def test_many_tiles():
    """B = 3 CHUNK + 7 with T = 4 drawn at random: the experts' gradient chunks (cut in the caller's row order) and the routed
    chunks (cut from the start of a task's run) disagree about where they cut."""
    B, C, T = 3 * CHUNK + 7, 100, 4
    ids = torch.randint(0, T, (B,), generator=torch.Generator().manual_seed(5))
    x, w, P = R.draw(B, C, T, 3, (80, 40), (24,), (24,), 77, sid=ids)
    check_all(run(make_head(C, P), x, ids, w), run_ref(x, ids, P, w), "many tiles")


def test_a_task_alone_equals_the_mix_bit_for_bit():
    """A task's rows alone == the same rows inside the mixed batch: logits, dx rows and that task's gate, tower and out-bias
    gradients.  Alone twice: the same T = 5 module on a batch holding that task only, and a two-task module whose task 0 holds
    that task's parameters.  The experts' gradients sum over all rows and are not compared."""
    C, s = 33, 3
    ids = R.sweep_ids(TILE, CHUNK)
    x, w, P = R.draw(ids.numel(), C, 5, 3, (48, 32), (8,), (64,), 3)
    rows = ids == s
    P2 = {k: ([t[[s, 0]] for t in v] if isinstance(v, list) else v[[s, 0]]) if k in R.ROUTED else v for k, v in P.items()}
    y_m, g_m, _, _ = run(make_head(C, P), x, ids, w)
    y_a, g_a, _, _ = run(make_head(C, P), x[rows], ids[rows], w[rows])
    y_2, g_2, _, _ = run(make_head(C, P2), x[rows], torch.zeros(int(rows.sum()), dtype=torch.long), w[rows])
    assert torch.equal(y_a, y_m[rows]) and torch.equal(y_2, y_a)
    assert torch.equal(g_a["x"], g_m["x"][rows]) and torch.equal(g_2["x"], g_a["x"])
    for k in routed_keys(g_m):
        assert float(g_m[k][s].abs().max()) > 0.0, k
        assert torch.equal(g_a[k][s], g_m[k][s]) and torch.equal(g_2[k][0], g_m[k][s]), k


def test_two_runs_agree_bit_for_bit():
    C = 100
    ids = R.sweep_ids(TILE, CHUNK)
    x, w, P = R.draw(ids.numel(), C, 5, 3, (80, 24), (24,), (16,), 11)
    (y0, g0, ga0, m0), (y1, g1, ga1, m1) = (run(make_head(C, P), x, ids, w) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(ga0, ga1) and torch.equal(m0, m1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_errors():
    from satrans_amd import MMoEHead
    C, B, T = 20, 37, 5
    ids = torch.tensor([0, 1, 3, 3, 1, 0, 3, 2] * 5)[:B]
    x, w, P = R.draw(B, C, T, 3, (16, 8), (8,), (8,), 9)
    head = make_head(C, P)
    for bad in (-1, T):
        off = ids.clone()
        off[5] = bad
        with pytest.raises(IndexError):
            head(x.to(DEV), off.to(DEV))
    with pytest.raises(IndexError):                       # the offset moves the accepted range
        head(x.to(DEV), ids.to(DEV), 1)
    head(x.to(DEV), (ids + 1).to(DEV), 1)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        MMoEHead(C, T)(x, ids)
    with pytest.raises(TypeError, match="float32"):
        head(x.to(DEV).double(), ids.to(DEV))
    with pytest.raises(ValueError):
        head(x[:, :5].to(DEV), ids.to(DEV))
    with pytest.raises(ValueError):
        head(x.to(DEV), ids[:-1].to(DEV))


class _Net(nn.Module):
    def __init__(self, D, H, Fn, T, E, expert, gate, tower):
        super().__init__()
        from satrans_amd import MMoEHead, SelfAttention_Layer
        self.att = SelfAttention_Layer(D, head_num=H)
        self.head = MMoEHead(Fn * D, T, E, expert, gate, tower)

    def forward(self, x, ids):
        return self.head(self.att(x).flatten(1), ids).squeeze(1)


def test_composition_trains_like_the_restatement():
    """SelfAttention_Layer (evaluation mode) -> flatten -> MMoEHead -> BCE with logits, two Adam steps with lr = eps = 1e-2:
    autograd through the stacked per-task and per-expert parameters and back into each module.  lr / eps <= 1, so an error of
    the gradient moves a parameter by at most as much (the argument of
    tests/test_star_gpu.py::test_composition_trains_like_the_restatement applies unchanged): parameters within the gradient
    bound, and enough of them moved for that to mean something."""
    from oracle import satrans_oracle as O
    D, H, Fn, T, E, B, LR, EPS = 16, 2, 3, 3, 3, 30, 1e-2, 1e-2
    expert, gate, tower = (16, 8), (8,), (8,)
    torch.manual_seed(4)
    net = _Net(D, H, Fn, T, E, expert, gate, tower)
    g = torch.Generator().manual_seed(8)
    _, _, P = R.draw(B, Fn * D, T, E, expert, gate, tower, 12)
    net.head.load_state_dict(R.state_from_params(P))
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.startswith("att.W_"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    x, target = torch.randn(B, Fn, D, generator=g), (torch.rand(B, generator=g) > 0.5).float()
    ids = torch.tensor([0, 1, 2, 1, 0] * (B // 5))
    start = {k: v.detach().clone() for k, v in net.named_parameters()}
    # fp64 restatement
    leaves = {k: v.double().requires_grad_(True) for k, v in start.items()}
    att = {k[4:]: v for k, v in leaves.items() if k.startswith("att.")}
    opt = torch.optim.Adam([v for k, v in leaves.items() if k != "att.W_Out"], lr=LR, eps=EPS)
    for _ in range(2):
        opt.zero_grad()
        Pl = R.params_from_state({k[5:]: v for k, v in leaves.items() if k.startswith("head.")}, E, T, len(expert), len(gate),
                                 len(tower))
        h = O.selfattention_layer(att, x.double(), H)[0].flatten(1)
        out, _ = R.forward(h, ids, Pl)
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
