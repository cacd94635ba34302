"""satrans_amd.layers.ESMMHead and WDLHead (csrc/esmm.hip behind one torch.autograd.Function) against the fp64 restatement
tests/esmm_reference.py on the same seeded inputs, dropout included: the restatement is fed the masks of
oracle.satrans_oracle.dropout_keep with the head's (seed, step).  That restatement is pinned to the reference's own ESMM.forward
and WDL.forward by the recorded runs of tests/test_esmm_cpu.py.

Bounds (the sibling bounds), all element-wise: results and the saved hidden rows within 2e-5 max|.|; gradients
within 1e-4 max|g| + 5e-9.  tests/test_esmm_cpu.py::test_premise_of_the_gpu_bounds pins their margin.  Everything else here is
bit for bit."""
import ctypes
import functools

import pytest
import torch

from satrans_amd import native
from tests import esmm_reference as R
from tests import helpers

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
check_close = functools.partial(helpers.check_close, "esmm-parity")
HEADS = ((2, "esmm"), (1, "wdl"))
HEAD_IDS = [h for _, h in HEADS]
# (name, training, p, step): dropout off is evaluation mode; the two training runs are R.DROP_RUNS
MODES = (("off", False, 0.0, 0),) + tuple((f"p{p}", True, p, step) for p, step in R.DROP_RUNS)


@functools.lru_cache(maxsize=None)
def drawn(case, towers):
    x, dout, P, _ = R.draw(case, towers)
    return x, dout, P


def make_head(case, towers, P, p):
    from satrans_amd import ESMMHead, WDLHead
    head = (ESMMHead if towers == 2 else WDLHead)(case[1], case[2], dnn_dropout=p)
    head.load_state_dict({k: v.clone() for k, v in R.state_from_params(P).items()})
    head._clock.seed = R.DROP_SEED
    return head.to(DEV)


def run(head, towers, x, dout, training=False, step=0, offset=0):
    """out, {gradients keyed as R.flat keys them, "x"}, the saved hidden rows per layer - all on the host.  A training run is
    the head's forward number `step`."""
    head.train(training)
    head._clock.step = step - 1 if training else step
    head.drop_row_offset = offset
    head.zero_grad(set_to_none=True)
    xg = x.to(DEV).requires_grad_(True)
    y = head(xg)
    assert head._clock.step == step
    (y * dout.to(DEV)).sum().backward()
    g = R.flat(R.params_from_state({k: p.grad.cpu() for k, p in head.named_parameters()}, towers), xg.grad.cpu())
    return y.detach().cpu(), g, [h.cpu() for h in head.last_hidden]


@functools.lru_cache(maxsize=None)
def shipped(case, towers, mode, ctcvr_only=False):
    """The head's run of a case in a mode, in the library's default form of the tail (composed), and the restatement's.
    Cached: several tests read it."""
    _, training, p, step = mode
    x, dout, P = drawn(case, towers)
    if ctcvr_only:
        dout = dout.clone()
        dout[:, 0] = 0
    got = run(make_head(case, towers, P, p), towers, x, dout, training, step)
    masks = R.keep_masks(R.DROP_SEED, step, case[0], case[2], towers, p) if training and p else None
    y_ref, cache = R.forward(x.double(), R.double(P), masks, p if masks is not None else 0.0)
    dx, G = R.backward(dout.double(), cache)
    return got, (y_ref, cache, R.flat(G, dx))


def same_bits(a, b, msg):
    (ya, ga, ha), (yb, gb, hb) = a, b
    assert torch.equal(ya, yb), f"{msg}: out"
    assert sorted(ga) == sorted(gb)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), f"{msg}: {k}"
    for l, (u, v) in enumerate(zip(ha, hb)):
        assert torch.equal(u, v), f"{msg}: hidden rows of layer {l}"


@pytest.mark.parametrize("towers,head", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_against_the_restatement(case, mode, towers, head):
    """The output, every parameter gradient, dx and the hidden rows left in saved, without dropout and in training mode at
    p = 0.5 (scale exact) and p = 0.1.  For ESMM once with a random dout [B, 2] and once with dout[:, 0] = 0: the product rule
    alone, which must reach both towers.
    Largest ratios seen over the sweep on an MI355X: the output 4.5e-7 max|.| and the saved rows 1.0e-6 max|.| (bound 2e-5),
    gradients 1.5e-6 max|g| (bound 1e-4); the largest of each come from the B = 260, C = 608 case."""
    for ctcvr_only in ((False, True) if towers == 2 else (False,)):
        (y, g, hidden), (y_ref, cache, g_ref) = shipped(case, towers, mode, ctcvr_only)
        msg = f"{head} {R.case_id(case)} {mode[0]}{' dout[:, 0] = 0' if ctcvr_only else ''}"
        assert y.shape == (case[0], towers)
        check_close(y, y_ref, 2e-5, msg)
        for l, h in enumerate(hidden):
            check_close(h, torch.cat(cache["h"][l + 1], dim=1), 2e-5, msg, f"hidden[{l}]")
        assert sorted(g) == sorted(g_ref)
        for k in g_ref:
            check_close(g[k], g_ref[k], 1e-4, f"{msg} {k}", what="grad", floor=5e-9)
        if ctcvr_only:
            assert float(g["wf"][0].abs().max()) > 0 and float(g["wf"][1].abs().max()) > 0


@pytest.mark.parametrize("towers,head", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("mode", MODES[1:], ids=[m[0] for m in MODES[1:]])
@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_the_mask_is_the_oracles(case, mode, towers, head):
    """Where the fp64 pre-activation exceeds 1e-4, a saved element is zero exactly where dropout_keep(seed, step, layer, tower,
    row, column, p) drops and non-zero where it keeps."""
    _, _, p, step = mode
    (_, _, hidden), (_, cache, _) = shipped(case, towers, mode)
    masks = R.keep_masks(R.DROP_SEED, step, case[0], case[2], towers, p)
    seen = 0
    for l, h in enumerate(hidden):
        z = torch.cat(cache["z"][l], dim=1)
        keep = torch.cat(list(masks[l]), dim=1)
        live = z > 1e-4
        assert torch.equal((h != 0)[live], keep[live]), f"{head} {R.case_id(case)} {mode[0]}: layer {l}"
        assert not (h != 0)[z < -1e-4].any()
        seen += int(live.sum())
    assert seen > 0


@pytest.mark.parametrize("towers,head", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("mode", MODES[:2], ids=[m[0] for m in MODES[:2]])
@pytest.mark.parametrize("case", R.SWEEP, ids=R.case_id)
def test_fused_tail_equals_composed_bit_for_bit(case, mode, towers, head):
    """The composed form (the default, satrans_esmm_set_forward(1)) runs the last hidden layer and the final layer as two tile
    products and a pointwise kernel; satrans_esmm_set_forward(0) runs them as the one launch of the fused tail.  The same
    chains, so the same bits in the output, the saved rows and every gradient, with and without dropout."""
    _, training, p, step = mode
    x, dout, P = drawn(case, towers)
    lib = native.lib()
    composed = shipped(case, towers, mode)[0]
    was = lib.satrans_esmm_set_forward(0)
    try:
        assert was == 1      # the default is the composed form
        fused = run(make_head(case, towers, P, p), towers, x, dout, training, step)
    finally:
        lib.satrans_esmm_set_forward(was)
    same_bits(fused, composed, f"{head} {R.case_id(case)} {mode[0]}")


@pytest.mark.parametrize("towers,head", HEADS, ids=HEAD_IDS)
def test_train_eval_and_determinism_bit_for_bit(towers, head):
    case = R.SWEEP[2]
    x, dout, P = drawn(case, towers)
    dropping, plain = make_head(case, towers, P, 0.5), make_head(case, towers, P, 0.0)
    # eval() with dnn_dropout = 0.5 is a dnn_dropout = 0 head, and the clock does not move
    a = run(dropping, towers, x, dout, False, 7)
    assert dropping._clock.step == 7
    same_bits(a, run(plain, towers, x, dout, False, 0), "eval")
    same_bits(a, run(plain, towers, x, dout, True, 3), "training at p = 0")
    # two training calls at the same step are equal; successive ones differ
    b, c = run(dropping, towers, x, dout, True, 5), run(dropping, towers, x, dout, True, 5)
    same_bits(b, c, "the same step twice")
    assert not torch.equal(a[0], b[0])
    dropping.train(True)
    y1 = dropping(x.to(DEV)).detach().cpu()
    y2 = dropping(x.to(DEV)).detach().cpu()
    assert dropping._clock.step == 7 and not torch.equal(y1, y2)
    if towers == 2:
        assert torch.equal(dropping.last_cvr.cpu() * y2[:, :1], y2[:, 1:]) and not dropping.last_cvr.requires_grad
    assert torch.equal(y1, run(dropping, towers, x, dout, True, 6)[0])


@pytest.mark.parametrize("towers,head", HEADS, ids=HEAD_IDS)
@pytest.mark.parametrize("mode", MODES[:2], ids=[m[0] for m in MODES[:2]])
@pytest.mark.parametrize("case", R.SWEEP[1:], ids=R.case_id)
def test_a_sample_alone_equals_the_sample_in_the_batch(case, mode, towers, head):
    """Its output row and its dx row, for rows 0, 1, B // 2 and B - 1; with dropout on, drop_row_offset = b keeps its masks."""
    _, training, p, step = mode
    x, dout, P = drawn(case, towers)
    (y, g, _), _ = shipped(case, towers, mode)
    mod = make_head(case, towers, P, p)
    B = case[0]
    for b in sorted({0, 1, B // 2, B - 1}):
        y1, g1, _ = run(mod, towers, x[b:b + 1], dout[b:b + 1], training, step, offset=b)
        assert torch.equal(y1[0], y[b]), f"{head} {R.case_id(case)} {mode[0]}: out row {b}"
        assert torch.equal(g1["x"][0], g["x"][b]), f"{head} {R.case_id(case)} {mode[0]}: dx row {b}"


def test_unsupported_descriptors_return_before_any_launch():
    """Sizes beyond 2^31 workgroups are refused from the descriptor alone: the pointers (of a tiny buffer) are never followed."""
    lib = native.lib()
    tiny = torch.zeros(16, device=DEV)
    for towers in (1, 2):
        d = native.ESMMDesc()
        d.B, d.C, d.towers, d.n_dnn = 2 ** 31 - 1, 8, towers, 1
        d.width[0] = 2 ** 20
        d.x = d.final_w = d.out_bias = tiny.data_ptr()
        d.dnn_w[0] = d.dnn_b[0] = tiny.data_ptr()
        g = native.ESMMGrads()
        g.final_w = g.out_bias = tiny.data_ptr()
        g.dnn_w[0] = g.dnn_b[0] = tiny.data_ptr()
        s = native.stream_handle(torch.device(DEV))
        assert lib.satrans_esmm_fwd(ctypes.byref(d), tiny.data_ptr(), tiny.data_ptr(), s) == -2
        assert b"2^31 workgroups" in lib.satrans_last_error()
        assert lib.satrans_esmm_bwd(ctypes.byref(d), tiny.data_ptr(), tiny.data_ptr(), tiny.data_ptr(), tiny.data_ptr(),
                                    ctypes.byref(g), s) == -2
    torch.cuda.synchronize()
    assert float(tiny.abs().max()) == 0.0
