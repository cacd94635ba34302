"""satrans_amd.layers.SharedBottomHead (csrc/sharedbottom.hip behind torch.autograd.Function) against the fp64 restatement
tests/sharedbottom_reference.py on the same seeded inputs; that restatement is pinned to the reference's own
SharedBottom.forward by the recorded runs of tests/test_sharedbottom_cpu.py.

Bounds (the sibling bounds), all element-wise: logits and the bottom's output within 2e-5 max|.|; gradients
within 1e-4 max|g| + 5e-9.  tests/test_sharedbottom_cpu.py::test_premise_of_the_gpu_bounds pins their margin."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from satrans_amd import native
from tests import helpers
from tests import sharedbottom_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE, CHUNK = native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sharedbottom")
check_close = functools.partial(helpers.check_close, "sharedbottom-parity")


def units(P):
    return tuple(w.shape[0] for w in P["bottom_w"]), tuple(w.shape[1] for w in P["tower_w"])


def make_head(C, P):
    """A SharedBottomHead of the shapes of P holding its values."""
    from satrans_amd import SharedBottomHead
    bottom, tower = units(P)
    mod = SharedBottomHead(C, P["out_bias"].shape[0], bottom, tower)
    mod.load_state_dict({k: v.clone() for k, v in R.state_from_params(P).items()})
    return mod.to(DEV)


def run(mod, x, ids, w, offset=0, saved=False):
    """logit, {gradients keyed as R.flat keys them, "x"}, the bottom's output (the whole saved buffer with saved=True) - all on
    the host."""
    mod.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    y = mod(xg, ids.to(DEV), offset)
    (y * w.to(DEV)).sum().backward()
    T, nb, nt = mod.num_tasks, len(mod.bottom_dnn_hidden_units), len(mod.tower_dnn_hidden_units)
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in mod.named_parameters()}, T, nb, nt, dtype=torch.float32))
    g["x"] = xg.grad.cpu()
    kept = mod.last_bottom._base if saved else mod.last_bottom
    return y.detach().cpu(), g, kept.cpu()


def run_ref(x, sid, P, w):
    y, cache = R.forward(x.double(), sid, R.double(P))
    return y, cache, R.flat(R.backward(w.double(), cache))


def check_all(got, ref, msg):
    (y, g, bottom), (y_ref, cache, g_ref) = got, ref
    assert y.shape == (y_ref.shape[0], 1)
    check_close(y, y_ref, 2e-5, msg)
    check_close(bottom, cache.th[0], 2e-5, msg, "last_bottom")
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


@pytest.mark.parametrize("case", R.SWEEP, ids=lambda c: f"C{c[0]}-b{len(c[1])}-t{'x'.join(map(str, c[2])) or 'none'}")
def test_shape_sweep_against_the_restatement(case):
    """C in {1, 33, 609}, 1 to 3 bottom layers, 0 to 3 tower layers, widths off the 64-column tile, the last tower width from
    {1, 16, 64, 65, 130}, one case without a tower layer over a 72-wide bottom; T = 5 interleaved with a non-zero id offset: one
    task one row past the row tile, one one row past the weight-gradient chunk, one with a single row, one empty.  Logit, the
    bottom's output, every gradient; the empty task's parameter gradients are exactly zero, the one-row task's are not."""
    ids, x, w, P = R.sweep_draw(case, TILE, CHUNK)
    got = run(make_head(case[0], P), x, ids + R.SWEEP_OFFSET, w, R.SWEEP_OFFSET)
    check_all(got, run_ref(x, ids, P, w), f"sweep {case}")
    g = got[1]
    assert routed_keys(g)
    for k in routed_keys(g):
        assert float(g[k][4].abs().max()) == 0.0, k
        assert float(g[k][2].abs().max()) > 0.0, k      # the one-row task is not skipped


def test_walker_edges_empty_first_task_and_an_exact_chunk():
    """T = 4 with row counts [0, CHUNK, 0, TILE + 1]: the first task empty, a run of exactly one weight-gradient chunk, an
    empty task between two runs; interleaved, a non-zero id offset."""
    C, counts = 33, [0, CHUNK, 0, TILE + 1]
    ids = counted_ids(counts, 41)
    x, w, P = R.draw(ids.numel(), C, 4, (48, 32), (24, 65), 42, sid=ids)
    got = run(make_head(C, P), x, ids + 2, w, 2)
    check_all(got, run_ref(x, ids, P, w), "walker edges")
    g = got[1]
    for k in routed_keys(g):
        assert float(g[k][0].abs().max()) == 0.0 and float(g[k][2].abs().max()) == 0.0, k
        assert float(g[k][1].abs().max()) > 0.0 and float(g[k][3].abs().max()) > 0.0, k


@pytest.mark.parametrize("tower", [(8,), ()], ids=["tower", "none"])
def test_batch_smaller_than_a_tile(tower):
    B, C = 5, 20
    ids = torch.tensor([1, 1, 0, 1, 1])
    x, w, P = R.draw(B, C, 3, (24, 8), tower, 5, sid=ids)
    check_all(run(make_head(C, P), x, ids, w), run_ref(x, ids, P, w), "B < tile")


def test_many_tiles():
    """B = 3 CHUNK + 7 with T = 4 drawn at random: the bottom's gradient chunks (cut in the caller's row order) and the routed
    chunks (cut from the start of a task's run) disagree about where they cut."""
    B, C, T = 3 * CHUNK + 7, 100, 4
    ids = torch.randint(0, T, (B,), generator=torch.Generator().manual_seed(5))
    x, w, P = R.draw(B, C, T, (80, 40), (24,), 77, sid=ids)
    check_all(run(make_head(C, P), x, ids, w), run_ref(x, ids, P, w), "many tiles")


@pytest.mark.parametrize("name", ["plain", "notower"])
def test_reference_fixtures_on_the_gpu(name):
    """The reference's own recorded SharedBottom run: its parameters and dnn_input in, sigmoid(logit) and the gradients of the
    masked summed BCE out, against the own-task column of the recorded y_pred and the recorded gradients.  Both sides are fp32
    runs of contractions at most 25 long: the fixtures' bound 2e-5 max|.| of tests/test_sharedbottom_cpu.py."""
    from satrans_amd import SharedBottomHead
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    state = {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}
    x, labels = torch.from_numpy(fx["dnn_input"]), torch.from_numpy(fx["labels"])
    ids, off, T = torch.from_numpy(fx["X"][:, 0]).long(), int(fx["offset"]), fx["y_pred"].shape[1]
    bottom = tuple(state[f"bottom_dnn.linears.{l}.weight"].shape[0] for l in range(2))
    tower = (state["tower_dnn.0.linears.0.weight"].shape[0],) if name == "plain" else ()
    head = SharedBottomHead(x.shape[1], T, bottom, tower)
    head.load_state_dict(state)
    head = head.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    y = torch.sigmoid(head(xg, ids.to(DEV), off))
    loss = F.binary_cross_entropy(y.squeeze(1), labels.to(DEV), reduction='sum')
    loss.backward()
    own = torch.from_numpy(fx["y_pred"]).gather(1, (ids - off).unsqueeze(1))
    check_close(y.detach().cpu(), own, 2e-5, f"fixture {name}")
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 2e-5 * abs(float(fx["loss"]))
    for k, p in head.named_parameters():
        want = torch.from_numpy(fx[f"grad/{k}"])
        if float(want.abs().max()) == 0.0:
            assert float(p.grad.abs().max()) == 0.0, k
        check_close(p.grad.cpu(), want, 2e-5, f"fixture {name} {k}", what="fixture grad")
    check_close(xg.grad.cpu(), torch.from_numpy(fx["grad/dnn_input"]), 2e-5, f"fixture {name} dnn_input", what="fixture grad")


def test_a_task_alone_equals_the_mix_bit_for_bit():
    """A task's rows alone == the same rows inside the mixed batch: logits, dx rows and that task's tower, final-layer and
    out-bias gradients.  Alone twice: the same T = 5 module on a batch holding that task only, and a two-task module whose task
    0 holds that task's parameters.  The bottom's gradients sum over all rows and are not compared.  With a last tower width of
    130 (the tail's chain crosses column tiles) and without a tower layer."""
    C, s = 33, 3
    ids = R.sweep_ids(TILE, CHUNK)
    rows = ids == s
    for bottom, tower in (((48, 32), (24, 130)), ((48, 72), ())):
        x, w, P = R.draw(ids.numel(), C, 5, bottom, tower, 3)
        P2 = {k: ([t[[s, 0]] for t in v] if isinstance(v, list) else v[[s, 0]]) if k in R.ROUTED else v for k, v in P.items()}
        y_m, g_m, _ = run(make_head(C, P), x, ids, w)
        y_a, g_a, _ = run(make_head(C, P), x[rows], ids[rows], w[rows])
        y_2, g_2, _ = run(make_head(C, P2), x[rows], torch.zeros(int(rows.sum()), dtype=torch.long), w[rows])
        assert torch.equal(y_a, y_m[rows]) and torch.equal(y_2, y_a)
        assert torch.equal(g_a["x"], g_m["x"][rows]) and torch.equal(g_2["x"], g_a["x"])
        assert routed_keys(g_m)
        for k in routed_keys(g_m):
            assert float(g_m[k][s].abs().max()) > 0.0, k
            assert torch.equal(g_a[k][s], g_m[k][s]) and torch.equal(g_2[k][0], g_m[k][s]), k


def test_two_runs_agree_bit_for_bit():
    C = 100
    ids = R.sweep_ids(TILE, CHUNK)
    x, w, P = R.draw(ids.numel(), C, 5, (80, 24), (16, 65), 11)
    (y0, g0, s0), (y1, g1, s1) = (run(make_head(C, P), x, ids, w, saved=True) for _ in range(2))
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k


@pytest.mark.parametrize("bottom,tower", [((48, 32), (24, 130)), ((48, 72), ()), ((40,), (16,)), ((24, 24), (16, 1))],
                         ids=["t24x130", "none", "t16", "t16x1"])
def test_fused_tail_equals_the_composed_forward_bit_for_bit(bottom, tower):
    """The fused tail (one launch) against the composed forward (the last tower layer and the final layer as launches of the
    shared tile product): logits, the whole saved buffer, and every gradient of the backward that follows."""
    C = 33
    ids = R.sweep_ids(TILE, CHUNK)
    x, w, P = R.draw(ids.numel(), C, 5, bottom, tower, 21)
    lib = native.lib()
    was = lib.satrans_sharedbottom_set_forward(0)
    try:
        y_f, g_f, s_f = run(make_head(C, P), x, ids, w, saved=True)
        assert lib.satrans_sharedbottom_set_forward(1) == 0
        y_c, g_c, s_c = run(make_head(C, P), x, ids, w, saved=True)
    finally:
        lib.satrans_sharedbottom_set_forward(was)
    assert s_f.numel() == ids.numel() * (sum(bottom) + sum(tower))
    assert torch.equal(y_f, y_c) and torch.equal(s_f, s_c)
    assert float(y_f.abs().max()) > 0.0
    for k in g_f:
        assert torch.equal(g_f[k], g_c[k]), k
    check_close(y_f, run_ref(x, ids, P, w)[0], 2e-5, f"fused tail {tower}")      # (and both are the head's logits)


def test_errors():
    from satrans_amd import SharedBottomHead
    C, B, T = 20, 37, 5
    ids = torch.tensor([0, 1, 3, 3, 1, 0, 3, 2] * 5)[:B]
    x, w, P = R.draw(B, C, T, (16, 8), (8,), 9)
    head = make_head(C, P)
    for bad in (-1, T):
        off = ids.clone()
        off[5] = bad
        with pytest.raises(IndexError):
            head(x.to(DEV), off.to(DEV))
    with pytest.raises(IndexError):                       # the offset moves the accepted range
        head(x.to(DEV), ids.to(DEV), 1)
    assert head(x.to(DEV), (ids + 1).to(DEV), 1).shape == (B, 1)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        SharedBottomHead(C, T)(x, ids)
    with pytest.raises(TypeError, match="float32"):
        head(x.to(DEV).double(), ids.to(DEV))
    with pytest.raises(ValueError):
        head(x[:, :5].to(DEV), ids.to(DEV))
    with pytest.raises(ValueError):
        head(x.to(DEV).unsqueeze(0), ids.to(DEV))
    with pytest.raises(ValueError):
        head(x.to(DEV), ids[:-1].to(DEV))


class _Net(nn.Module):
    def __init__(self, D, H, Fn, T, bottom, tower):
        super().__init__()
        from satrans_amd import SelfAttention_Layer, SharedBottomHead
        self.att = SelfAttention_Layer(D, head_num=H)
        self.head = SharedBottomHead(Fn * D, T, bottom, tower)

    def forward(self, x, ids):
        return torch.sigmoid(self.head(self.att(x).flatten(1), ids)).squeeze(1)


def test_composition_trains_like_the_restatement():
    """SelfAttention_Layer (evaluation mode) -> flatten -> SharedBottomHead -> sigmoid -> summed BCE, three Adam steps with
    lr = eps = 1e-2: autograd through the stacked per-task parameters and back into each module.  lr / eps <= 1, so an error of
    the gradient moves a parameter by at most as much (the argument of
    tests/test_star_gpu.py::test_composition_trains_like_the_restatement applies unchanged): parameters within the gradient
    bound, and enough of them moved for that to mean something."""
    from oracle import satrans_oracle as O
    D, H, Fn, T, B, LR, EPS, STEPS = 16, 2, 3, 3, 30, 1e-2, 1e-2, 3
    bottom, tower = (16, 8), (8,)
    torch.manual_seed(4)
    net = _Net(D, H, Fn, T, bottom, tower)
    g = torch.Generator().manual_seed(8)
    _, _, P = R.draw(B, Fn * D, T, bottom, tower, 12)
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
    for _ in range(STEPS):
        opt.zero_grad()
        Pl = R.params_from_state({k[5:]: v for k, v in leaves.items() if k.startswith("head.")}, T, len(bottom), len(tower))
        h = O.selfattention_layer(att, x.double(), H)[0].flatten(1)
        out, _ = R.forward(h, ids, Pl)
        F.binary_cross_entropy(torch.sigmoid(out.squeeze(1)), target.double(), reduction='sum').backward()
        opt.step()
    # the modules on the GPU
    net = net.to(DEV).train()
    net.att.eval()
    opt = torch.optim.Adam(net.parameters(), lr=LR, eps=EPS)
    for _ in range(STEPS):
        opt.zero_grad()
        F.binary_cross_entropy(net(x.to(DEV), ids.to(DEV)), target.to(DEV), reduction='sum').backward()
        opt.step()
    moved = 0
    for k, p in net.named_parameters():
        want = leaves[k].detach()
        check_close(p.detach().cpu(), want, 1e-4, f"composition {k}", what="parameter", floor=5e-9)
        moved += float((want - start[k].double()).abs().max()) > 10 * (1e-4 * float(want.abs().max()) + 5e-9)
    assert moved >= 10, moved      # the check above is not satisfied by parameters that stood still
