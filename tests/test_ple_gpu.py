"""satrans_amd.layers.PLEHead (csrc/ple.hip behind torch.autograd.Function) against the fp64 restatement
tests/ple_reference.py on the same seeded inputs; that restatement is pinned to the reference's own PLE.forward by the
recorded runs of tests/test_ple_cpu.py.

Bounds (the sibling bounds), all element-wise: logits, saved gates and mixtures within 2e-5 max|.|; gradients
within 1e-4 max|g| + 5e-9.  tests/test_ple_cpu.py::test_premise_of_the_gpu_bounds measures their margin on these inputs."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import ple_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, CHUNK = native.PLE_ROW_TILE, native.PLE_DW_ROW_CHUNK
check_close = functools.partial(helpers.check_close, "ple-parity")


def dims(mod):
    return (mod.num_tasks, mod.specific_expert_num, mod.shared_expert_num, mod.num_levels, len(mod.expert_dnn_hidden_units),
            len(mod.gate_dnn_hidden_units), len(mod.tower_dnn_hidden_units))


def make_head(C, P):
    """A PLEHead of the shapes of P holding its values; the parameters that take no part keep their initial values."""
    from satrans_amd import PLEHead
    T, ns, nsh, two = R.sizes(P)
    units = lambda k: tuple(w.shape[-2] for w in P[k])      # noqa: E731
    mod = PLEHead(C, T, nsh, ns, 2 if two else 1, units("spec_w"), units("gate_w"), units("tower_w"))
    values = {k: v.clone() for k, v in R.state_from_params(P).items()}
    missing = mod.load_state_dict(values, strict=False)
    assert not missing.unexpected_keys and sorted(missing.missing_keys) == sorted(R.dead_keys(*dims(mod)))
    return mod.to(DEV)


def run(mod, x, ids, w, offset=0):
    """logit, {gradients keyed as R.flat keys them, "x"}, gates, mixture - all on the host.  The parameters that take no part
    must have been left without a gradient."""
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg, ids.to(DEV), offset)
    (y * w.to(DEV)).sum().backward()
    dead = set(R.dead_keys(*dims(mod)))
    named = dict(mod.named_parameters())
    assert all((p.grad is None) == (k in dead) for k, p in named.items()), [k for k, p in named.items() if (p.grad is None) != (k in dead)]
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in named.items() if k not in dead}, *dims(mod), dtype=torch.float32))
    g["x"] = xg.grad.cpu()
    return y.detach().cpu(), g, mod.last_gates.cpu(), mod.last_mixture.cpu()


def run_ref(x, sid, P, w):
    return R.grads(x.double(), sid, P, w)


def check_all(got, ref, msg):
    (y, g, gates, mix), (y_ref, cache, g_ref) = got, ref
    assert y.shape == (y_ref.shape[0], 1)
    check_close(y, y_ref, 2e-5, msg)
    check_close(gates, cache.gates.detach(), 2e-5, msg, "gates")
    check_close(mix, cache.mixture.detach(), 2e-5, msg, "mixture")
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


@pytest.mark.parametrize("case", R.SWEEP, ids=lambda c: f"C{c[0]}-ns{c[1]}-nsh{c[2]}-L{c[3]}")
def test_shape_sweep_against_the_restatement(case):
    """C in {1, 33, 609}, one and two levels, ns and nsh from 1 to 4, 1 to 3 expert layers, 0 to 3 gate and tower layers, widths
    off the 64-column tile; T = 5 interleaved with a non-zero id offset: one task one row past the row tile, one one row past
    the weight-gradient chunk, one with a single row, one empty.  Logit, gates, mixture, every gradient; the empty task's routed
    gradients are exactly zero, the one-row task's are not; the parameters that take no part have no gradient (run)."""
    ids, x, w, P = R.sweep_draw(case, TILE, CHUNK)
    ns = case[1]
    got = run(make_head(case[0], P), x, ids + R.SWEEP_OFFSET, w, R.SWEEP_OFFSET)
    check_all(got, run_ref(x, ids, P, w), f"sweep {case}")
    g = got[1]
    for k in routed_keys(g):
        assert float(R.of_task(k, g[k], 4, ns).abs().max()) == 0.0, k
        assert float(R.of_task(k, g[k], 2, ns).abs().max()) > 0.0, k      # the one-row task is not skipped


def test_widest_shared_gate():
    """T = 31, ns = nsh = 2: 64 scores under the level-0 shared gate, every lane of its softmax in use; about 100 rows, so
    several tasks are empty."""
    T, C = 31, 33
    ids = torch.randint(0, T, (101,), generator=torch.Generator().manual_seed(6))
    ids[ids % 7 == 3] = 0
    assert sum(int((ids == t).sum()) == 0 for t in range(T)) >= 3
    x, w, P = R.draw(ids.numel(), C, T, 2, 2, 2, (16,), (), (), 64, sid=ids)
    assert P["sg0_final_w"].shape[0] == 64
    check_all(run(make_head(C, P), x, ids, w), run_ref(x, ids, P, w), "64 shared scores")


def test_walker_edges_empty_first_task_and_an_exact_chunk():
    """T = 4 with row counts [0, CHUNK, 0, TILE + 1]: the first task empty, a run of exactly one weight-gradient chunk, an
    empty task between two runs; interleaved, a non-zero id offset."""
    C, counts, ns = 33, [0, CHUNK, 0, TILE + 1], 2
    ids = counted_ids(counts, 41)
    x, w, P = R.draw(ids.numel(), C, 4, ns, 1, 2, (48, 32), (8,), (64,), 42, sid=ids)
    got = run(make_head(C, P), x, ids + 2, w, 2)
    check_all(got, run_ref(x, ids, P, w), "walker edges")
    g = got[1]
    for k in routed_keys(g):
        assert float(R.of_task(k, g[k], 0, ns).abs().max()) == 0.0 and float(R.of_task(k, g[k], 2, ns).abs().max()) == 0.0, k
        assert float(R.of_task(k, g[k], 1, ns).abs().max()) > 0.0 and float(R.of_task(k, g[k], 3, ns).abs().max()) > 0.0, k


@pytest.mark.parametrize("levels", [1, 2])
def test_batch_smaller_than_a_tile(levels):
    B, C = 5, 20
    ids = torch.tensor([1, 1, 0, 1, 1])
    x, w, P = R.draw(B, C, 3, 2, 1, levels, (24, 8), (8,), (), 5, sid=ids)
    check_all(run(make_head(C, P), x, ids, w), run_ref(x, ids, P, w), "B < tile")


def test_many_tiles():
    """B = 8 CHUNK + 7 with T = 4 drawn at random: the dense gradient chunks (cut in the caller's row order) and the routed chunks
    (cut from the start of a task's run) disagree about where they cut, and every task crosses several chunks."""
    B, C, T = 8 * CHUNK + 7, 100, 4
    ids = torch.randint(0, T, (B,), generator=torch.Generator().manual_seed(5))
    x, w, P = R.draw(B, C, T, 2, 1, 2, (80, 40), (24,), (24,), 77, sid=ids)
    check_all(run(make_head(C, P), x, ids, w), run_ref(x, ids, P, w), "many tiles")


@pytest.mark.parametrize("levels", [1, 2])
def test_a_task_alone_equals_the_mix_bit_for_bit(levels):
    """A task's rows alone (the same module on a batch holding that task only) == the same rows inside the mixed batch: logits,
    dx rows and that task's routed gradients - its gates on both levels, its last-level experts, its tower and out bias.  The
    dense gradients sum over all rows and are not compared."""
    C, s, ns = 33, 3, 2
    ids = R.sweep_ids(TILE, CHUNK)
    x, w, P = R.draw(ids.numel(), C, 5, ns, 1, levels, (48, 32), (8,), (64,), 3)
    rows = ids == s
    y_m, g_m, ga_m, m_m = run(make_head(C, P), x, ids, w)
    y_a, g_a, ga_a, m_a = run(make_head(C, P), x[rows], ids[rows], w[rows])
    assert torch.equal(y_a, y_m[rows]) and torch.equal(ga_a, ga_m[rows]) and torch.equal(m_a, m_m[rows])
    assert torch.equal(g_a["x"], g_m["x"][rows])
    keys = routed_keys(g_m)
    # two expert layers (weight, bias), per level the gate's hidden layer and final layer, the tower's, the out bias
    assert len(keys) == 2 * 2 + 3 * levels + 3 + 1
    for k in keys:
        assert float(R.of_task(k, g_m[k], s, ns).abs().max()) > 0.0, k
        assert torch.equal(R.of_task(k, g_a[k], s, ns), R.of_task(k, g_m[k], s, ns)), k


def test_two_runs_agree_bit_for_bit():
    C = 100
    ids = R.sweep_ids(TILE, CHUNK)
    x, w, P = R.draw(ids.numel(), C, 5, 2, 2, 2, (80, 24), (24,), (16,), 11)
    (y0, g0, ga0, m0), (y1, g1, ga1, m1) = (run(make_head(C, P), x, ids, w) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(ga0, ga1) and torch.equal(m0, m1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


def test_errors():
    from satrans_amd import PLEHead
    C, B, T = 20, 37, 5
    ids = torch.tensor([0, 1, 3, 3, 1, 0, 3, 2] * 5)[:B]
    x, w, P = R.draw(B, C, T, 1, 1, 2, (16, 8), (8,), (8,), 9)
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
        PLEHead(C, T)(x, ids)
    with pytest.raises(TypeError, match="float32"):
        head(x.to(DEV).double(), ids.to(DEV))
    with pytest.raises(ValueError):
        head(x[:, :5].to(DEV), ids.to(DEV))
    with pytest.raises(ValueError):
        head(x.to(DEV), ids[:-1].to(DEV))


class _Net(nn.Module):
    def __init__(self, D, H, Fn, T, ns, nsh, expert, gate, tower):
        super().__init__()
        from satrans_amd import PLEHead, SelfAttention_Layer
        self.att = SelfAttention_Layer(D, head_num=H)
        self.head = PLEHead(Fn * D, T, nsh, ns, 2, expert, gate, tower)

    def forward(self, x, ids):
        return self.head(self.att(x).flatten(1), ids).squeeze(1)


def test_composition_trains_like_the_restatement():
    """SelfAttention_Layer (evaluation mode) -> flatten -> PLEHead (two levels) -> BCE with logits, two Adam steps with
    lr = eps = 1e-2: autograd through the stacked parameters and back into each module.  lr / eps <= 1, so an error of the
    gradient moves a parameter by at most as much (the argument of
    tests/test_star_gpu.py::test_composition_trains_like_the_restatement applies unchanged): parameters within the gradient
    bound, and enough of them moved for that to mean something.  The parameters that take no part are not handed to Adam's
    update (no gradient) and stay where they were."""
    from oracle import satrans_oracle as O
    D, H, Fn, T, ns, nsh, B, LR, EPS = 16, 2, 3, 3, 2, 1, 30, 1e-2, 1e-2
    expert, gate, tower = (16, 8), (8,), (8,)
    cfg = (T, ns, nsh, 2, len(expert), len(gate), len(tower))
    torch.manual_seed(4)
    net = _Net(D, H, Fn, T, ns, nsh, expert, gate, tower)
    g = torch.Generator().manual_seed(8)
    _, _, P = R.draw(B, Fn * D, T, ns, nsh, 2, expert, gate, tower, 12)
    net.head.load_state_dict(R.state_from_params(P), strict=False)
    dead = {"head." + k for k in R.dead_keys(*cfg)}
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.startswith("att.W_"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    x, target = torch.randn(B, Fn, D, generator=g), (torch.rand(B, generator=g) > 0.5).float()
    ids = torch.tensor([0, 1, 2, 1, 0] * (B // 5))
    start = {k: v.detach().clone() for k, v in net.named_parameters()}
    # fp64 restatement
    leaves = {k: v.double().requires_grad_(True) for k, v in start.items() if k not in dead}
    att = {k[4:]: v for k, v in leaves.items() if k.startswith("att.")}
    opt = torch.optim.Adam([v for k, v in leaves.items() if k != "att.W_Out"], lr=LR, eps=EPS)
    for _ in range(2):
        opt.zero_grad()
        Pl = R.params_from_state({k[5:]: v for k, v in leaves.items() if k.startswith("head.")}, *cfg)
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
        if k in dead:
            assert torch.equal(p.detach().cpu(), start[k]), k
            continue
        want = leaves[k].detach()
        check_close(p.detach().cpu(), want, 1e-4, f"composition {k}", what="parameter", floor=5e-9)
        moved += float((want - start[k].double()).abs().max()) > 10 * (1e-4 * float(want.abs().max()) + 5e-9)
    assert moved >= 10, moved      # the check above is not satisfied by parameters that stood still
