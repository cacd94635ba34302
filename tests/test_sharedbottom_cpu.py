"""The scenario-routed SharedBottom head without a GPU: the fp64 restatement against the reference's recorded SharedBottom
runs, its explicit backward against autograd of the unrouted form, the module's state, the C ABI's new symbols and their
argument validation, and the premise of the GPU bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from satrans_amd import native
from tests import sharedbottom_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sharedbottom")
CASES = {"plain": dict(bottom=(16, 8), tower=(8,)), "notower": dict(bottom=(16, 8), tower=())}
T = 3
SYMBOLS = ("satrans_sharedbottom_saved_floats", "satrans_sharedbottom_workspace_floats", "satrans_sharedbottom_fwd",
           "satrans_sharedbottom_bwd", "satrans_sharedbottom_set_forward")
TILE, CHUNK = native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK

# The recorded side is an fp32 run (unit roundoff u = 6e-8), the restatement fp64 on the same fp32 inputs.  A recorded
# element has passed at most 8 products (forward and backward; the MMoE fixtures' count, this head has fewer) whose
# contractions are at most 25 long (C = 13, widths <= 16, B <= 25 rows in a weight gradient): its rounding error is bounded by
# about 8 * 25 * u = 1.2e-5 of the largest magnitude in the worst case.  The bound is that figure rounded up, the one
# tests/test_mmoe_cpu.py uses; the deviations seen are printed.
BOUND = 2e-5


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def state_of(fx):
    return {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}


def dims(name):
    c = CASES[name]
    return T, len(c["bottom"]), len(c["tower"])


def replay(fx, name):
    """Own-task probabilities, loss and every gradient, recomputed by tests/sharedbottom_reference.py in fp64 (ROUTED)."""
    P = R.params_from_state(state_of(fx), *dims(name))
    x, labels = torch.from_numpy(fx["dnn_input"]).double(), torch.from_numpy(fx["labels"]).double()
    sid = torch.from_numpy(fx["X"][:, 0]).long() - int(fx["offset"])
    logit, cache = R.forward(x, sid, P)
    y = torch.sigmoid(logit).squeeze(1)
    loss = -(labels * torch.log(y) + (1 - labels) * torch.log(1 - y)).sum()
    g = R.backward((y - labels).unsqueeze(1), cache)      # d(summed BCE) / d(logit)
    grads = R.state_from_params({k: v for k, v in g.items() if k != "x"})
    grads["dnn_input"] = g["x"]
    return sid, y, loss, grads


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_every_fixture(name):
    """The ROUTED fp64 restatement against the reference's own unrouted fp32 SharedBottom.forward under the masked loss: each
    row's own-task probability, the loss, and the gradient of every head parameter and of dnn_input."""
    fx = load(name)
    sid, y, loss, grads = replay(fx, name)
    rec_y = torch.from_numpy(fx["y_pred"]).double().gather(1, sid.unsqueeze(1)).squeeze(1)
    worst = float((y - rec_y).abs().max() / rec_y.abs().max())
    assert worst <= BOUND, ("y", worst)
    assert abs(float(loss) - float(fx["loss"])) <= BOUND * abs(float(fx["loss"]))
    recorded = sorted(k[len("grad/"):] for k in fx if k.startswith("grad/"))
    assert recorded == sorted(grads)
    for k in recorded:
        rec = torch.from_numpy(fx[f"grad/{k}"]).double()
        scale = float(rec.abs().max())
        if scale == 0.0:
            assert float(grads[k].abs().max()) == 0.0, k
            continue
        dev = float((grads[k].reshape(rec.shape) - rec).abs().max() / scale)
        worst = max(worst, dev)
        assert dev <= BOUND, (k, dev)
    print(f"[sharedbottom] {name}: largest deviation {worst:.2e}")


def test_fixtures_hold_the_cases_they_claim_and_the_premise_of_routing():
    """`plain` has a task without rows, and the recorded gradients of that task's tower, final layer and out bias - taken by
    the reference through its UNROUTED forward, which ran that task's tower over every row - are exactly zero: a row
    contributes to its own task's parameters only.  The loss read through the own-task column alone equals the recorded one."""
    plain, notower = load("plain"), load("notower")
    counts = lambda fx: [int((fx["X"][:, 0] - int(fx["offset"]) == t).sum()) for t in range(T)]      # noqa: E731
    assert counts(plain)[1] == 0 and min(counts(plain)[0], counts(plain)[2]) > 1 and min(counts(notower)) > 1
    assert int(plain["offset"]) == 1 and plain["y_pred"].shape == (24, T) and notower["y_pred"].shape == (25, T)
    for k in plain:
        if k.startswith("grad/") and re.search(r"\.1\.", k) and not k.startswith("grad/bottom_dnn"):
            assert float(np.abs(plain[k]).max()) == 0.0, k
    assert float(np.abs(plain["grad/tower_dnn.0.linears.0.weight"]).max()) > 0.0
    assert float(np.abs(plain["grad/bottom_dnn.linears.1.weight"]).max()) > 0.0
    assert not any(k.startswith("param/tower_dnn.") for k in notower)
    assert any(k.startswith("param/tower_dnn.") for k in plain)
    for fx in (plain, notower):
        assert all(fx[k].dtype.kind in "fiU" for k in fx)
        ids, off = torch.from_numpy(fx["X"][:, 0]).long(), int(fx["offset"])
        loss = R.masked_loss(torch.from_numpy(fx["y_pred"]), torch.from_numpy(fx["labels"]), ids, off)
        assert abs(float(loss) - float(fx["loss"])) <= 1e-6 * abs(float(fx["loss"]))


def test_explicit_backward_equals_autograd_of_the_unrouted_form():
    """The restatement's routed backward is the derivative of the reference's unrouted form read one column per row (fp64
    autograd through R.torch_loop), with an empty task and a one-row task; with and without tower layers."""
    ids = R.sweep_ids(4, 9)
    for tower in ((3, 3), ()):
        x, w, P = R.draw(ids.numel(), 7, 5, (6, 5), tower, 1)
        P = {k: ([t.double().requires_grad_(True) for t in v] if isinstance(v, list) else v.double().requires_grad_(True))
             for k, v in P.items()}
        x = x.double().requires_grad_(True)
        own = R.torch_loop(x, P, sigmoid=False).gather(1, ids.unsqueeze(1))
        (own * w.double()).sum().backward()
        with torch.no_grad():
            logit, cache = R.forward(x, ids, P)
            mine = R.flat(R.backward(w.double(), cache))
        assert float((logit - own.detach()).abs().max()) <= 1e-12 * float(own.detach().abs().max())
        want = R.flat(P)
        assert sorted(want) + ["x"] == sorted(mine)
        assert float((mine["x"] - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
        for k, t in want.items():
            assert float((mine[k] - t.grad).abs().max()) <= 1e-12 * float(t.grad.abs().max()), k
            if k.split("[")[0] in R.ROUTED:
                assert float(mine[k][4].abs().max()) == 0.0 and float(t.grad[4].abs().max()) == 0.0, k


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_matches_the_reference(name):
    """Keys, order and shapes of state_dict() equal the reference SharedBottom's head entries, and the recorded values load."""
    from satrans_amd import SharedBottomHead
    fx, c = load(name), CASES[name]
    keys, shapes = [str(k) for k in fx["keys"]], [str(s) for s in fx["shapes"]]
    assert keys == R.keys_of(*dims(name))
    C = fx["dnn_input"].shape[1]
    head = SharedBottomHead(C, T, c["bottom"], c["tower"])
    sd = head.state_dict()
    assert list(sd) == keys
    assert [str(tuple(sd[k].shape)) for k in keys] == shapes
    values = state_of(fx)
    head.load_state_dict(values)      # strict
    for k, v in values.items():
        assert torch.equal(head.state_dict()[k], v), k
    P = R.params_from_state(values, *dims(name), dtype=torch.float32)
    back = R.state_from_params(P)
    assert sorted(back) == sorted(values) and all(torch.equal(back[k], values[k]) for k in values)
    fresh = SharedBottomHead(C, T, c["bottom"], c["tower"])
    assert float(fresh.bottom_dnn.linears[0].weight.detach().abs().max()) < 1e-3      # N(0, 1e-4)
    assert float(fresh.tower_dnn_final_layer[0].weight.detach().abs().max()) > 1e-3      # torch's default
    assert all(float(m.bias.detach().abs().max()) == 0.0 for m in fresh.out)


def test_module_refuses_what_is_not_built():
    from satrans_amd import SharedBottomHead
    with pytest.raises(NotImplementedError, match="relu"):
        SharedBottomHead(8, 2, dnn_activation="prelu")
    with pytest.raises(NotImplementedError, match="dropout"):
        SharedBottomHead(8, 2, dnn_dropout=0.1)
    with pytest.raises(NotImplementedError, match="batch-norm"):
        SharedBottomHead(8, 2, dnn_use_bn=True)
    with pytest.raises(NotImplementedError, match="bottom hidden layers"):
        SharedBottomHead(8, 2, bottom_dnn_hidden_units=())
    with pytest.raises(NotImplementedError, match="bottom hidden layers"):
        SharedBottomHead(8, 2, bottom_dnn_hidden_units=(4,) * 4)
    with pytest.raises(NotImplementedError, match="tower hidden layers"):
        SharedBottomHead(8, 2, tower_dnn_hidden_units=(4,) * 4)
    with pytest.raises(ValueError):
        SharedBottomHead(8, 1)
    with pytest.raises(ValueError):
        SharedBottomHead(0, 2)
    with pytest.raises(ValueError):
        SharedBottomHead(8, 2, tower_dnn_hidden_units=(4, 0))
    with pytest.raises(ValueError):
        SharedBottomHead(8, 2)(torch.zeros(3, 7), torch.zeros(3))
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        SharedBottomHead(8, 2)(torch.zeros(3, 8), torch.zeros(3))
    assert SharedBottomHead(8, 2, tower_dnn_hidden_units=()).tower_dnn_hidden_units == ()


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert "typedef struct satrans_sharedbottom_desc" in header and "typedef struct satrans_sharedbottom_grads" in header
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    H = native.MMOE_MAX_HIDDEN
    # B, C, T, two layer counts, reserved, two width arrays + x, order, seg + the parameter pointers
    assert ctypes.sizeof(native.SharedBottomDesc) == (6 + 2 * H) * 4 + (3 + 4 * H + 2) * 8
    assert ctypes.sizeof(native.SharedBottomGrads) == (4 * H + 2) * 8
    # the field order of the two mirrors is the header's
    for struct, cls in (("satrans_sharedbottom_desc", native.SharedBottomDesc), ("satrans_sharedbottom_grads", native.SharedBottomGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.split(None, 1)[1] if decl.split() else "")]
        names = [n for n in names if n not in ("float", "int32_t", "const")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def sb_desc(B, Cn, Tn, bottom, tower):
    d = native.SharedBottomDesc()
    d.B, d.C, d.T, d.n_bottom, d.n_tower = B, Cn, Tn, len(bottom), len(tower)
    for arr, units in ((d.bottom_width, bottom), (d.tower_width, tower)):
        for l, n in enumerate(units[:native.MMOE_MAX_HIDDEN]):
            arr[l] = n
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    assert lib.satrans_abi_version() == 7
    null = ctypes.POINTER(native.SharedBottomDesc)()
    assert lib.satrans_sharedbottom_saved_floats(null) == -1
    assert lib.satrans_sharedbottom_workspace_floats(null) == -1
    assert lib.satrans_sharedbottom_fwd(null, None, None, None) == -1
    assert b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_sharedbottom_bwd(null, None, None, None, None, None, None) == -1
    ok = (4, 8, 2, (16, 8), (8,))
    bad = []
    for at, values in ((0, (0, -1)), (1, (0, -8)), (2, (0, -2)), (3, ((), (4,) * 4, (16, 0), (-4,))), (4, ((4,) * 4, (0,), (8, -1)))):
        for v in values:
            bad.append(ok[:at] + (v,) + ok[at + 1:])
    for args in bad:
        d = sb_desc(*args)
        assert lib.satrans_sharedbottom_saved_floats(ctypes.byref(d)) == -1, args
        assert lib.satrans_sharedbottom_workspace_floats(ctypes.byref(d)) == -1, args
        assert lib.satrans_sharedbottom_fwd(ctypes.byref(d), None, None, None) == -1, args
        assert b"bad sizes" in lib.satrans_last_error(), args
        assert lib.satrans_sharedbottom_bwd(ctypes.byref(d), None, None, None, None, None, None) == -1, args
    B, Cn, Tn = 300, 70, 3
    chunks = -(-B // CHUNK)
    dw_slots = chunks + Tn
    d = sb_desc(B, Cn, Tn, (48, 32), (24, 16))
    assert lib.satrans_sharedbottom_saved_floats(ctypes.byref(d)) == B * (48 + 32 + 24 + 16)
    dense = chunks * max(48 * (Cn + 1), 32 * (48 + 1))
    routed = dw_slots * max(24 * (32 + 1), 16 * (24 + 1), 1 * (16 + 1))
    assert lib.satrans_sharedbottom_workspace_floats(ctypes.byref(d)) == 2 * B * 48 + max(dense, routed)
    d0 = sb_desc(B, Cn, Tn, (16,), ())      # no tower hidden layers
    assert lib.satrans_sharedbottom_saved_floats(ctypes.byref(d0)) == B * 16
    assert lib.satrans_sharedbottom_workspace_floats(ctypes.byref(d0)) == 2 * B * 16 + max(chunks * 16 * (Cn + 1), dw_slots * (16 + 1))
    for dd in (d, d0):
        assert lib.satrans_sharedbottom_fwd(ctypes.byref(dd), None, None, None) == -1      # sizes fine, pointers null
        assert b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_sharedbottom_bwd(ctypes.byref(dd), None, None, None, None, None, None) == -1
        assert b"null pointer" in lib.satrans_last_error()
    # the forward's mode: 0 or 1, returns the previous one, refuses anything else
    assert lib.satrans_sharedbottom_set_forward(2) == -1 and b"mode 2" in lib.satrans_last_error()
    was = lib.satrans_sharedbottom_set_forward(1)
    try:
        assert was in (0, 1) and lib.satrans_sharedbottom_set_forward(0) == 1 and lib.satrans_sharedbottom_set_forward(1) == 0
        assert lib.satrans_sharedbottom_saved_floats(ctypes.byref(d)) == B * (48 + 32 + 24 + 16)      # the same in both modes
    finally:
        lib.satrans_sharedbottom_set_forward(was)


@pytest.mark.parametrize("case", R.SWEEP, ids=lambda c: f"C{c[0]}-b{len(c[1])}-t{'x'.join(map(str, c[2])) or 'none'}")
def test_premise_of_the_gpu_bounds(case):
    """The GPU tests hold the kernels to 2e-5 max|.| on logits and the bottom's output and 1e-4 max|g| + 5e-9 on gradients
    (DESIGN.md §4).  On their seeded inputs torch's fp32 CPU run of the reference's UNROUTED loop, read one column per row,
    stays at least 10x inside those bounds against the fp64 restatement; and no hidden pre-activation of the fp64 forward lies
    within the output bound of relu's kink (R.draw draws such rows again; decided by the fp64 forward alone)."""
    ids, x, w, P = R.sweep_draw(case, TILE, CHUNK)
    want_y, cache = R.forward(x.double(), ids, R.double(P))
    want = R.flat(R.backward(w.double(), cache))
    assert R.kink_margin(cache) >= 2e-5
    for k in want:      # what the sweep asserts of the empty task and of the one-row task holds of the restatement
        if k.split("[")[0] in R.ROUTED:
            assert float(want[k][4].abs().max()) == 0.0 and float(want[k][2].abs().max()) > 0.0, k
    P32 = {k: ([t.clone().requires_grad_(True) for t in v] if isinstance(v, list) else v.clone().requires_grad_(True))
           for k, v in P.items()}
    x32 = x.clone().requires_grad_(True)
    y = R.torch_loop(x32, P32, sigmoid=False).gather(1, ids.unsqueeze(1))
    (y * w).sum().backward()
    dev_y = float((y.detach().double() - want_y).abs().max() / want_y.abs().max())
    worst = 0.0
    for k, t in [("x", x32)] + list(R.flat(P32).items()):
        scale = float(want[k].abs().max())
        err = float((t.grad.double() - want[k]).abs().max())
        worst = max(worst, err / max(scale, 1e-30))
        assert err <= (1e-4 * scale + 5e-9) / 10, k
    print(f"[sharedbottom] premise {case}: y {dev_y:.2e}, worst gradient {worst:.2e}, kink margin {R.kink_margin(cache):.2e}")
    assert dev_y <= 2e-5 / 10
