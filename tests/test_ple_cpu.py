"""The scenario-routed PLE head without a GPU: the fp64 restatement against the reference's recorded PLE runs, the routed form
against autograd of the unrouted one, the module's state, the C ABI's new symbols and their argument validation, and the
premise of the GPU bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from satrans_amd import native
from tests import ple_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ple")
CASES = {"two_level": dict(L=2, ns=1, nsh=1, expert=(16, 8), gate=(8,), tower=(8,)),
         "one_level": dict(L=1, ns=2, nsh=1, expert=(16, 8), gate=(), tower=()),
         "wide": dict(L=2, ns=2, nsh=2, expert=(16, 8), gate=(), tower=(8,))}
T = 3
SYMBOLS = ("satrans_ple_saved_floats", "satrans_ple_workspace_floats", "satrans_ple_fwd", "satrans_ple_bwd")
TILE, CHUNK = native.PLE_ROW_TILE, native.PLE_DW_ROW_CHUNK

# The recorded side is an fp32 run (unit roundoff u = 6e-8), the restatement fp64 on the same fp32 inputs.  A recorded element
# has passed at most 14 products (two levels of experts, gates and the tower, forward and backward) whose contractions are at
# most 25 long (C = 13, widths <= 16, B <= 25 rows in a weight gradient): its rounding error is bounded by about
# 14 * 25 * u = 2.1e-5 of the largest magnitude in the worst case.  The bound is that figure rounded up; the deviations seen
# are printed.  (For the scalar out.{t}.bias the magnitude is that of the summed terms: see the test.)
BOUND = 3e-5


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def state_of(fx):
    return {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}


def dims(name):
    c = CASES[name]
    return T, c["ns"], c["nsh"], c["L"], len(c["expert"]), len(c["gate"]), len(c["tower"])


def make_head(name, C):
    from satrans_amd import PLEHead
    c = CASES[name]
    return PLEHead(C, T, c["nsh"], c["ns"], c["L"], c["expert"], c["gate"], c["tower"])


def replay(fx, name):
    """Own-task probabilities, loss and every live gradient, recomputed by tests/ple_reference.py in fp64 (ROUTED, autograd)."""
    P = R.leaves(R.params_from_state(state_of(fx), *dims(name)))
    x = torch.from_numpy(fx["dnn_input"]).double().requires_grad_(True)
    labels = torch.from_numpy(fx["labels"]).double()
    sid = torch.from_numpy(fx["X"][:, 0]).long() - int(fx["offset"])
    logit, _ = R.forward(x, sid, P)
    y = torch.sigmoid(logit).squeeze(1)
    loss = -(labels * torch.log(y) + (1 - labels) * torch.log(1 - y)).sum()
    loss.backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)      # noqa: E731
    grads = R.state_from_params({k: ([zero(t) for t in v] if isinstance(v, list) else zero(v)) for k, v in P.items()})
    grads["dnn_input"] = x.grad
    terms = {f"out.{t}.bias": float((y.detach() - labels)[sid == t].abs().sum()) for t in range(T)}
    return sid, y.detach(), loss.detach(), grads, terms


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_reproduces_every_fixture(name):
    """The ROUTED fp64 restatement against the reference's own unrouted fp32 PLE.forward under the masked loss: each row's
    own-task probability, the loss, and the gradient of every head parameter and of dnn_input (the parameters the reference
    left without a gradient are recorded as zeros and are not in the restatement)."""
    fx = load(name)
    sid, y, loss, grads, terms = replay(fx, name)
    rec_y = torch.from_numpy(fx["y_pred"]).double().gather(1, sid.unsqueeze(1)).squeeze(1)
    worst = float((y - rec_y).abs().max() / rec_y.abs().max())
    assert worst <= BOUND, ("y", worst)
    assert abs(float(loss) - float(fx["loss"])) <= BOUND * abs(float(fx["loss"]))
    dead = {str(k) for k in fx["dead"]}
    recorded = sorted(k[len("grad/"):] for k in fx if k.startswith("grad/"))
    assert sorted(set(recorded) - dead) == sorted(grads)
    for k in grads:
        rec = torch.from_numpy(fx[f"grad/{k}"]).double()
        # out.{t}.bias is ONE sum, of y - label over the task's rows, whose terms cancel: its rounding error scales with the sum
        # of their magnitudes, not with the result (a tensor's largest element has no such cancellation to speak of)
        scale = terms.get(k, float(rec.abs().max()))
        if scale == 0.0:
            assert float(grads[k].abs().max()) == 0.0, k
            continue
        dev = float((grads[k].reshape(rec.shape) - rec).abs().max() / scale)
        worst = max(worst, dev)
        assert dev <= BOUND, (k, dev)
    print(f"[ple] {name}: largest deviation {worst:.2e}")


def test_fixtures_hold_the_cases_they_claim_and_the_premise_of_routing():
    """`two_level` has a task without rows.  The gradients the reference took through its UNROUTED forward say what is routed:
    that task's level-0 gate, its last-level experts and gate, its tower and out bias got exactly zero; its level-0 experts
    did not (the shared mixture reads them for every row).  And the parameters autograd left at None are the last level's
    shared gate and the surplus shared experts - the set the module keeps out of the kernels."""
    fx = {name: load(name) for name in CASES}
    counts = lambda f: [int((f["X"][:, 0] - int(f["offset"]) == t).sum()) for t in range(T)]      # noqa: E731
    two = fx["two_level"]
    assert counts(two)[1] == 0 and min(counts(two)[0], counts(two)[2]) > 1
    assert min(counts(fx["one_level"])) > 1 and min(counts(fx["wide"])) > 1
    assert all(int(f["offset"]) == 1 and f["y_pred"].shape[1] == T for f in fx.values())
    pat = re.compile(r"grad/((?:specific_gate_dnn|specific_gate_dnn_final_layer)\.\d|specific_experts\.1|tower_dnn|tower_dnn_final_layer|out)"
                     r"\.1\.(.*)")
    routed = [m for m in map(pat.fullmatch, two) if m]
    assert len(routed) == 2 * 2 + 2 + 4 + 2 + 1 + 1
    for m in routed:
        assert float(np.abs(two[m.group(0)]).max()) == 0.0, m.group(0)
        assert float(np.abs(two[f"grad/{m.group(1)}.0.{m.group(2)}"]).max()) > 0.0, m.group(0)      # task 0's are not
    for k in two:
        if k.startswith("grad/specific_experts.0.1."):
            assert float(np.abs(two[k]).max()) > 0.0, k
    for name, f in fx.items():
        assert [str(k) for k in f["keys"]] == R.keys_of(*dims(name))
        assert sorted(str(k) for k in f["dead"]) == sorted(R.dead_keys(*dims(name))), name
        head = make_head(name, f["dnn_input"].shape[1])
        handed = set(R.state_from_params(R.params_from_state(head.state_dict(), *dims(name))))
        assert set(head.state_dict()) - handed == {str(k) for k in f["dead"]}, name
        assert all(f[k].dtype.kind in "fiU" for k in f)
    assert any("shared_experts.0.0.1." in str(k) for k in fx["one_level"]["dead"])


@pytest.mark.parametrize("levels,ns,nsh,gate", [(2, 2, 1, (4,)), (1, 1, 1, ()), (2, 1, 1, ())])
def test_routed_form_equals_autograd_of_the_unrouted_form(levels, ns, nsh, gate):
    """The restatement's routed form has the derivative of the reference's unrouted form read one column per row (fp64 autograd
    through both), with an empty task and a one-row task; the empty task's routed gradients are zero in both."""
    ids = R.sweep_ids(4, 9)
    x, w, P = R.draw(ids.numel(), 7, 5, ns, nsh, levels, (6, 5), gate, (3, 3), 1)
    y0, _, g0 = R.grads(x.double(), ids, P, w, fn=lambda xl, Pl: R.torch_loop(xl, Pl, sigmoid=False).gather(1, ids.unsqueeze(1)))
    y1, _, g1 = R.grads(x.double(), ids, P, w)
    assert float((y1 - y0).abs().max()) <= 1e-12 * float(y0.abs().max())
    assert sorted(g0) == sorted(g1)
    for k in g0:
        assert float((g1[k] - g0[k]).abs().max()) <= 1e-12 * float(g0[k].abs().max()), k
        if k.split("[")[0] in R.ROUTED:
            assert float(R.of_task(k, g1[k], 4, ns).abs().max()) == 0.0 and float(R.of_task(k, g0[k], 4, ns).abs().max()) == 0.0, k
            assert float(R.of_task(k, g1[k], 2, ns).abs().max()) > 0.0, k


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_matches_the_reference(name):
    """Keys, order and shapes of state_dict() equal the reference PLE's head entries, and the recorded values load."""
    fx = load(name)
    keys, shapes = [str(k) for k in fx["keys"]], [str(s) for s in fx["shapes"]]
    C = fx["dnn_input"].shape[1]
    head = make_head(name, C)
    sd = head.state_dict()
    assert list(sd) == keys
    assert [str(tuple(sd[k].shape)) for k in keys] == shapes
    values = state_of(fx)
    head.load_state_dict(values)      # strict
    for k, v in values.items():
        assert torch.equal(head.state_dict()[k], v), k
    fresh = make_head(name, C)
    assert float(fresh.specific_experts[0][1][0].linears[0].weight.detach().abs().max()) < 1e-3      # N(0, 1e-4)
    assert float(fresh.specific_gate_dnn_final_layer[0][0].weight.detach().abs().max()) > 1e-3      # torch's default
    assert all(float(m.bias.detach().abs().max()) == 0.0 for m in fresh.out)


def test_module_refuses_what_is_not_built():
    from satrans_amd import PLEHead
    with pytest.raises(NotImplementedError, match="relu"):
        PLEHead(8, 2, dnn_activation="prelu")
    with pytest.raises(NotImplementedError, match="dropout"):
        PLEHead(8, 2, dnn_dropout=0.1)
    with pytest.raises(NotImplementedError, match="batch-norm"):
        PLEHead(8, 2, dnn_use_bn=True)
    for levels in (0, 3):
        with pytest.raises(NotImplementedError, match="num_levels"):
            PLEHead(8, 2, num_levels=levels)
    with pytest.raises(NotImplementedError, match="at most 8"):
        PLEHead(8, 2, shared_expert_num=4, specific_expert_num=5)
    with pytest.raises(NotImplementedError, match="at most 64"):
        PLEHead(8, 32, shared_expert_num=1, specific_expert_num=2)
    PLEHead(8, 32, shared_expert_num=1, specific_expert_num=2, num_levels=1, expert_dnn_hidden_units=(4,))      # no shared gate to run
    PLEHead(8, 31, shared_expert_num=2, specific_expert_num=2, expert_dnn_hidden_units=(4,))      # exactly 64
    with pytest.raises(NotImplementedError, match="expert hidden layers"):
        PLEHead(8, 2, expert_dnn_hidden_units=())
    with pytest.raises(NotImplementedError, match="expert hidden layers"):
        PLEHead(8, 2, expert_dnn_hidden_units=(4,) * 4)
    with pytest.raises(NotImplementedError, match="gate and tower"):
        PLEHead(8, 2, gate_dnn_hidden_units=(4,) * 4)
    with pytest.raises(NotImplementedError, match="gate and tower"):
        PLEHead(8, 2, tower_dnn_hidden_units=(4,) * 4)
    with pytest.raises(ValueError):
        PLEHead(8, 1)
    with pytest.raises(ValueError, match="IndexError in its forward"):
        PLEHead(8, 2, shared_expert_num=2, specific_expert_num=1)
    with pytest.raises(ValueError):
        PLEHead(8, 2, shared_expert_num=0)
    with pytest.raises(ValueError):
        PLEHead(0, 2)
    with pytest.raises(ValueError):
        PLEHead(8, 2, expert_dnn_hidden_units=(4, 0))
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        PLEHead(8, 2)(torch.zeros(3, 8), torch.zeros(3))


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
        assert hasattr(native.lib(), sym)
    assert "typedef struct satrans_ple_desc" in header and "typedef struct satrans_ple_grads" in header
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    for name in ("ROW_TILE", "DW_ROW_CHUNK", "MAX_OWN", "MAX_SHARED_SCORES", "MAX_HIDDEN"):
        assert int(re.search(r"#define SATRANS_PLE_%s (\d+)" % name, header).group(1)) == getattr(native, "PLE_" + name)
    assert (native.PLE_ROW_TILE, native.PLE_DW_ROW_CHUNK) == (native.MMOE_ROW_TILE, native.MMOE_DW_ROW_CHUNK)      # one set of kernels
    H = native.PLE_MAX_HIDDEN
    pointers = sum(H if per_layer else 1 for _, per_layer in native.PLE_POINTERS)
    # B, C, T, ns, nsh, levels, three layer counts, reserved, three width arrays, reserved2 + x, order, seg, task + the parameters
    assert ctypes.sizeof(native.PLEDesc) == (10 + 3 * H + 1) * 4 + (4 + pointers) * 8
    assert ctypes.sizeof(native.PLEGrads) == pointers * 8
    for struct, cls in (("satrans_ple_desc", native.PLEDesc), ("satrans_ple_grads", native.PLEGrads)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.split(None, 1)[1] if decl.split() else "")]
        names = [n for n in names if n not in ("float", "int32_t", "const")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


def ple_desc(B, Cn, Tn, ns, nsh, levels, expert, gate, tower):
    d = native.PLEDesc()
    d.B, d.C, d.T, d.ns, d.nsh, d.levels, d.n_expert, d.n_gate, d.n_tower = B, Cn, Tn, ns, nsh, levels, len(expert), len(gate), len(tower)
    for arr, units in ((d.expert_width, expert), (d.gate_width, gate), (d.tower_width, tower)):
        for l, n in enumerate(units[:native.PLE_MAX_HIDDEN]):
            arr[l] = n
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    null = ctypes.POINTER(native.PLEDesc)()
    assert lib.satrans_ple_saved_floats(null) == -1
    assert lib.satrans_ple_workspace_floats(null) == -1
    assert lib.satrans_ple_fwd(null, None, None, None) == -1
    assert b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_ple_bwd(null, None, None, None, None, None, None) == -1
    ok = (4, 8, 3, 2, 1, 2, (16, 8), (8,), (8,))
    bad = []
    for at, values, word in ((0, (0, -1), b"B="), (1, (0, -8), b"C="), (2, (0, -2, 32), b"T"), (3, (0, -1, 8), b"ns="),
                             (4, (0, -1, 7), b"nsh="), (5, (0, 3, -1), b"levels="),
                             (6, ((), (4,) * 4), b"expert"), (6, ((16, 0), (-4,)), b"expert_width"),
                             (7, ((4,) * 4,), b"gate"), (7, ((0,), (8, -1)), b"gate_width"),
                             (8, ((4,) * 4,), b"tower"), (8, ((0,), (8, -1)), b"tower_width")):
        for v in values:
            bad.append((ok[:at] + (v,) + ok[at + 1:], word))
    for args, word in bad:
        d = ple_desc(*args)
        assert lib.satrans_ple_saved_floats(ctypes.byref(d)) == -1, args
        assert lib.satrans_ple_workspace_floats(ctypes.byref(d)) == -1, args
        assert lib.satrans_ple_fwd(ctypes.byref(d), None, None, None) == -1, args
        err = lib.satrans_last_error()
        assert b"bad sizes" in err and word in err, (args, err)      # the message names the field
        assert lib.satrans_ple_bwd(ctypes.byref(d), None, None, None, None, None, None) == -1, args
    assert lib.satrans_ple_saved_floats(ctypes.byref(ple_desc(4, 8, 32, 2, 1, 1, (16,), (), ()))) > 0      # no shared gate with one level
    B, Cn, Tn, ns, nsh = 300, 70, 3, 2, 1
    Eo, E0 = ns + nsh, Tn * ns + nsh
    d = ple_desc(B, Cn, Tn, ns, nsh, 2, (48, 32), (8,), (24, 16))
    last = Eo + 32 + Eo + Eo * 48 + Eo * 32 + 8 + 24 + 16
    level0 = Eo + E0 + 32 + 32 + Eo + E0 + E0 * 48 + E0 * 32 + 8 + 8
    assert lib.satrans_ple_saved_floats(ctypes.byref(d)) == B * (last + level0)
    chunks = -(-B // CHUNK)
    dw_slots = chunks + Tn
    dense = chunks * max(E0 * 48 * (Cn + 1), E0 * 32 * (48 + 1), 8 * (Cn + 1), E0 * (8 + 1), nsh * 48 * (32 + 1), nsh * 32 * (48 + 1))
    routed = dw_slots * max(8 * (Cn + 1), Eo * (8 + 1), ns * 48 * (32 + 1), ns * 32 * (48 + 1), 8 * (32 + 1), 24 * (32 + 1),
                            16 * (24 + 1), 1 * (16 + 1))
    fixed = 2 * B * E0 * 48 + B * (32 + Eo + Eo + E0 + 32 + 32)      # two dz buffers, dm, three dscores, both level-0 dm
    assert lib.satrans_ple_workspace_floats(ctypes.byref(d)) == fixed + max(dense, routed)
    d1 = ple_desc(B, Cn, Tn, ns, nsh, 1, (16,), (), ())      # one level, no gate and no tower hidden layers
    assert lib.satrans_ple_saved_floats(ctypes.byref(d1)) == B * (Eo + 16 + Eo + Eo * 16)
    part = max(chunks * nsh * 16 * (Cn + 1), dw_slots * max(ns * 16 * (Cn + 1), Eo * Cn, 1 * (16 + 1)))
    assert lib.satrans_ple_workspace_floats(ctypes.byref(d1)) == 2 * B * Eo * 16 + B * (16 + Eo) + part
    for dd in (d, d1):
        assert lib.satrans_ple_fwd(ctypes.byref(dd), None, None, None) == -1      # sizes fine, pointers null
        assert b"null pointer" in lib.satrans_last_error()
        assert lib.satrans_ple_bwd(ctypes.byref(dd), None, None, None, None, None, None) == -1
        assert b"null pointer" in lib.satrans_last_error()


@pytest.mark.parametrize("case", R.SWEEP, ids=lambda c: f"C{c[0]}-ns{c[1]}-nsh{c[2]}-L{c[3]}")
def test_premise_of_the_gpu_bounds(case):
    """The GPU tests hold the kernels to 2e-5 max|.| on logits, gates and mixtures and 1e-4 max|g| + 5e-9 on gradients
    (DESIGN.md §4).  Two levels make the chains deeper than the MMoE head's, so this measures: on the GPU tests' seeded inputs
    torch's fp32 CPU run of the reference's UNROUTED loop, read one column per row, against the fp64 restatement must stay at
    least 10x inside those bounds (the margin tests/test_mmoe_cpu.py::test_premise_of_the_gpu_bounds asserts); and no hidden
    pre-activation of the fp64 forward lies within the output bound of relu's kink (R.draw draws such rows again; decided by
    the fp64 forward alone).  Each figure is printed before it is asserted."""
    ids, x, w, P = R.sweep_draw(case, TILE, CHUNK)
    want_y, cache, want = R.grads(x.double(), ids, P, w)
    margin = R.kink_margin(cache)
    own = lambda xl, Pl: R.torch_loop(xl, Pl, sigmoid=False).gather(1, ids.unsqueeze(1))      # noqa: E731
    y, _, got = R.grads(x, ids, P, w, fn=own)
    dev_y = float((y.double() - want_y).abs().max() / want_y.abs().max())
    devs = {k: float((got[k].double() - want[k]).abs().max()) for k in want}
    worst = max(devs[k] / max(float(want[k].abs().max()), 1e-30) for k in want)
    print(f"[ple] premise {case}: y {dev_y:.2e}, worst gradient {worst:.2e}, kink margin {margin:.2e}")
    assert margin >= 2e-5
    for k in want:
        assert devs[k] <= (1e-4 * float(want[k].abs().max()) + 5e-9) / 10, k
    assert dev_y <= 2e-5 / 10
