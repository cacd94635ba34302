"""STAR's towers without a GPU: the fp64 restatement against the reference's recorded Star_Net runs, its explicit backward
against autograd, the modules' state, the C ABI's new symbols and their argument validation, and the premise of the GPU bounds."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from satrans_amd import native
from tests import mdr_bn_reference as BN
from tests import star_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "star")
CASES = ("plain", "bn")
SYMBOLS = ("satrans_star_saved_floats", "satrans_star_workspace_floats", "satrans_star_fwd", "satrans_star_bwd")
S, HIDDEN = 3, (16, 8)

# Largest deviation of the fp64 restatement from a recorded array, relative to the array's largest magnitude, measured once
# over every array of both fixtures (see test_restatement_reproduces_every_fixture).  The recorded side is an fp32 run.
# `plain` stays below 3.2e-7 (gradients) and 8.1e-8 (y_pred).  Both maxima are `bn`, training mode: grad_train/bns.0.weight and
# y_train.  With the domain id as a feature (the reference's wiring) the four columns of its embedding are CONSTANT within a
# scenario, so their batch variance is zero and invstd = 1 / sqrt(eps) = 316 multiplies whatever x - mean the fp32 run leaves
# (the mean of n equal fp32 values need not equal them); fp64 on the same inputs leaves exactly zero.
MEASURED_DEVIATION = {"grad": 6.70e-5, "other": 2.27e-6}
BOUND = {k: 4 * v for k, v in MEASURED_DEVIATION.items()}


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def state_of(fx):
    return {k[len("param/"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("param/")}


def replay(fx, name):
    """Every recorded result of a fixture, recomputed by tests/star_reference.py in fp64 from the recorded fp32 inputs."""
    sd = state_of(fx)
    P = R.params_from_state(sd, S, len(HIDDEN))
    x, w = torch.from_numpy(fx["dnn_input"]).double(), torch.from_numpy(fx["w"]).double()
    sid = torch.from_numpy(fx["X"][:, 0]).long() - int(fx["offset"])
    out = {}
    st = BN.State.fresh(S, x.shape[1])
    if name == "bn":
        st.weight = torch.stack([sd[f"bns.{s}.weight"] for s in range(S)]).double()
        st.bias = torch.stack([sd[f"bns.{s}.bias"] for s in range(S)]).double()
    for mode in ("train", "eval"):
        if name == "bn":
            logit, caches = R.head_forward(x, sid, P, st, sd["shared_bn_weight"].double(), sd["shared_bn_bias"].double(),
                                           training=mode == "train")
        else:
            logit, caches = R.forward(x, sid, P)
        y = torch.sigmoid(logit)
        out[f"y_{mode}"] = y
        dlogit = w * y * (1 - y)      # the reference records gradients of sum(sigmoid(logit) * w)
        g = R.head_backward(dlogit, caches) if name == "bn" else R.backward(dlogit, caches)
        out[f"grad_{mode}/dnn_input"] = g["x"]
        for k, v in R.grads_by_key(g, S, len(HIDDEN)).items():
            out[f"grad_{mode}/{k}"] = v
        if mode == "train" and name == "bn":
            for s in range(S):
                out[f"buf/bns.{s}.running_mean"], out[f"buf/bns.{s}.running_var"] = st.running_mean[s].clone(), st.running_var[s].clone()
                out[f"buf/bns.{s}.num_batches_tracked"] = torch.tensor(st.num_batches_tracked[s])
    return out


def deviations(name):
    fx = load(name)
    got = replay(fx, name)
    recorded = [k for k in fx if k.split("/")[0] in ("y_train", "y_eval", "buf", "grad_train", "grad_eval")]
    assert sorted(recorded) == sorted(got), sorted(set(recorded) ^ set(got))
    for k in recorded:
        rec = torch.from_numpy(np.asarray(fx[k])).double()
        if k.endswith("num_batches_tracked"):
            assert torch.equal(got[k].double(), rec), k
            continue
        scale = float(rec.abs().max())
        if scale == 0.0:      # the empty scenario's gradients: exactly zero on both sides
            assert float(got[k].abs().max()) == 0.0, k
            continue
        yield k, float((got[k].reshape(rec.shape) - rec).abs().max() / scale)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_every_fixture(name):
    """tests/star_reference.py (fp64; the normalisation of tests/mdr_bn_reference.py in front for `bn`) against the reference's
    own fp32 Star_Net.forward cast up: y_pred in both modes, the buffers after the training step, and the gradients of
    sum(y_pred * w) with respect to every tower and normalisation parameter and dnn_input, in both modes.

    Measured once over both fixtures, relative to the recorded array's largest magnitude: 6.70e-5 over the gradients and 2.27e-6
    over outputs and buffers (both `bn` in training mode; the comment above MEASURED_DEVIATION says why), 3.2e-7 and 8.1e-8 in `plain`.  The bound is 4x the measured value, taken separately for gradients and
    for everything else."""
    worst = {"grad": (0.0, ""), "other": (0.0, "")}
    for k, dev in deviations(name):
        kind = "grad" if k.startswith("grad_") else "other"
        worst[kind] = max(worst[kind], (dev, k))
    print(f"[star] {name}: largest deviation {worst}")
    for kind, (dev, k) in worst.items():
        assert dev <= BOUND[kind], (k, dev)


def test_fixtures_hold_the_cases_they_claim():
    plain, bn = load("plain"), load("bn")
    counts = lambda fx: [int((fx["X"][:, 0] - int(fx["offset"]) == s).sum()) for s in range(S)]      # noqa: E731
    assert counts(plain)[1] == 0 and min(counts(plain)[0], counts(plain)[2]) > 1
    assert min(counts(bn)) >= 2
    assert int(plain["offset"]) == 1 and float(np.abs(plain["grad_train/domain_dnns.1.linears.0.weight"]).max()) == 0.0


def test_explicit_backward_equals_autograd():
    """The restatement's backward formulas are the derivative of its forward (fp64 autograd), with an empty scenario."""
    ids = R.sweep_ids(4, 9)
    x, w, P = R.draw(ids.numel(), 7, (6, 5), 5, 1)
    P = {k: [t.double().requires_grad_(True) for t in v] for k, v in P.items()}
    x = x.double().requires_grad_(True)
    logit, cache = R.forward(x, ids, P)
    (logit * w.double()).sum().backward()
    with torch.no_grad():
        mine = R.backward(w.double(), cache)
    assert float((mine["x"] - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    for k in R.GROUPS:
        for l, t in enumerate(P[k]):
            assert float((mine[k][l] - t.grad).abs().max()) <= 1e-12 * float(t.grad.abs().max()), (k, l)
        assert float(mine[k][0][4].abs().max()) == 0.0 if k.endswith("dom") else True


@pytest.mark.parametrize("name", CASES)
def test_state_dict_matches_the_reference(name):
    """Keys, order and shapes of state_dict() equal the reference Star_Net's tower entries, and the recorded values load."""
    from satrans_amd import StarHead, StarTowers
    fx = load(name)
    keys, shapes = [str(k) for k in fx["keys"]], [str(s) for s in fx["shapes"]]
    C = fx["dnn_input"].shape[1]
    head = StarHead(C, HIDDEN, S, use_domain_bn=name == "bn")
    sd = head.state_dict()
    assert list(sd) == keys
    assert [str(tuple(sd[k].shape)) for k in keys] == shapes
    values = state_of(fx)
    values.update({k[len("buf/"):]: torch.from_numpy(np.asarray(v)) for k, v in fx.items() if k.startswith("buf/")})
    head.load_state_dict(values)      # strict
    for k, v in values.items():
        assert torch.equal(head.state_dict()[k], v), k
    towers = StarTowers(C, HIDDEN, S)
    tower_keys = [k for k in keys if not k.startswith(("shared_bn_", "bns."))]
    assert list(towers.state_dict()) == tower_keys
    towers.load_state_dict({k: values[k] for k in tower_keys})
    fresh = StarTowers(C, HIDDEN, S)
    assert float(fresh.shared_dnn.linears[0].weight.detach().abs().max()) < 1e-3      # N(0, 1e-4)
    assert float(fresh.domain_dnns[2].linears[1].weight.detach().abs().max()) < 1e-3
    assert float(fresh.domain_dnn_linears[0].weight.detach().abs().max()) > 1e-3      # torch's default


def test_modules_refuse_what_is_not_built():
    from satrans_amd import StarHead, StarTowers
    for cls in (StarTowers, StarHead):
        with pytest.raises(NotImplementedError, match="relu"):
            cls(8, (16,), 2, activation="prelu")
        with pytest.raises(NotImplementedError, match="dropout"):
            cls(8, (16,), 2, dropout_rate=0.1)
        with pytest.raises(NotImplementedError, match="batch-norm"):
            cls(8, (16,), 2, use_bn=True)
        with pytest.raises(NotImplementedError, match="hidden layers"):
            cls(8, (16,) * 5, 2)
        with pytest.raises(NotImplementedError, match="hidden layers"):
            cls(8, (), 2)
        with pytest.raises(native.NativeError, match="no CPU fallback"):
            cls(8, (16,), 2)(torch.zeros(3, 8), torch.zeros(3))
    assert list(StarHead(8, (16,), 2, use_domain_bn=False).state_dict())[:3] == [
        "shared_bn_weight", "shared_bn_bias", "domain_dnns.0.linears.0.weight"]


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
    assert "typedef struct satrans_star_desc" in header
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    for name in ("ROW_TILE", "DW_ROW_CHUNK", "MAX_LAYERS"):
        assert int(re.search(r"#define SATRANS_STAR_%s (\d+)" % name, header).group(1)) == getattr(native, "STAR_" + name)
    # B, C, S, L, width[5], reserved + x, order, seg + four groups of five pointers
    assert ctypes.sizeof(native.StarDesc) == 10 * 4 + (3 + 4 * native.STAR_MAX_LAYERS) * 8


def star_desc(B, Cn, Sn, widths):
    d = native.StarDesc()
    d.B, d.C, d.S, d.L = B, Cn, Sn, len(widths)
    for l, n in enumerate(widths[:native.STAR_MAX_LAYERS]):
        d.width[l] = n
    return d


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    assert lib.satrans_abi_version() == 7
    null = ctypes.POINTER(native.StarDesc)()
    assert lib.satrans_star_saved_floats(null) == -1
    assert lib.satrans_star_workspace_floats(null) == -1
    assert lib.satrans_star_fwd(null, None, None, None) == -1
    assert b"null descriptor" in lib.satrans_last_error()
    assert lib.satrans_star_bwd(null, None, None, None, None, None, None, None, None, None) == -1
    bad = [(0, 8, 2, (16, 1)), (4, 0, 2, (16, 1)), (4, 8, 0, (16, 1)), (-1, 8, 2, (16, 1)), (4, -8, 2, (16, 1)), (4, 8, -2, (16, 1)),
           (4, 8, 2, (1,)), (4, 8, 2, (16, 0, 1)), (4, 8, 2, (16, -4, 1)), (4, 8, 2, (16, 16)), (4, 8, 2, (8, 8, 8, 8, 8, 1))]
    for B, Cn, Sn, widths in bad:
        d = star_desc(B, Cn, Sn, widths)
        assert lib.satrans_star_saved_floats(ctypes.byref(d)) == -1, (B, Cn, Sn, widths)
        assert lib.satrans_star_workspace_floats(ctypes.byref(d)) == -1, (B, Cn, Sn, widths)
        assert lib.satrans_star_fwd(ctypes.byref(d), None, None, None) == -1, (B, Cn, Sn, widths)
        assert b"bad sizes" in lib.satrans_last_error()
    d = star_desc(300, 70, 3, (48, 32, 1))
    assert lib.satrans_star_saved_floats(ctypes.byref(d)) == 300 * (48 + 32)
    dw_slots = -(-300 // native.STAR_DW_ROW_CHUNK) + 3
    assert lib.satrans_star_workspace_floats(ctypes.byref(d)) == 2 * 300 * 48 + dw_slots * max(48 * 71, 32 * 49, 1 * 33)
    assert lib.satrans_star_fwd(ctypes.byref(d), None, None, None) == -1      # sizes fine, pointers null
    assert b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_star_bwd(ctypes.byref(d), None, None, None, None, None, None, None, None, None) == -1
    assert b"null pointer" in lib.satrans_last_error()


@pytest.mark.parametrize("C,hidden", [(609, (256, 128)), (33, (48, 32)), (1, (16,))])
def test_premise_of_the_gpu_bounds(C, hidden):
    """The GPU tests hold the kernels to 2e-5 max|y| on outputs and 1e-4 max|g| + 5e-9 on gradients.  On their
    seeded inputs (S = 5, B = 300) torch's fp32 CPU run of the reference's loop stays at least 10x inside those bounds against
    the fp64 restatement, so fp32 arithmetic of the reference's kind is well within them (probed: at most 3.3e-7 on y and
    4.8e-7 on any gradient)."""
    B, S5 = 300, 5
    ids = torch.tensor([0, 1, 3, 3, 1, 0, 3] * (B // 7 + 1))[:B]
    x, w, P = R.draw(B, C, hidden, S5, 1000 + C)
    want_y, cache = R.forward(x.double(), ids, R.double(P))
    want = R.backward(w.double(), cache)
    P32 = {k: [t.clone().requires_grad_(True) for t in v] for k, v in P.items()}
    x32 = x.clone().requires_grad_(True)
    y = R.torch_loop(x32, ids, P32)
    (y * w).sum().backward()
    dev_y = float((y.detach().double() - want_y).abs().max() / want_y.abs().max())
    worst = 0.0
    pairs = [(x32.grad, want["x"])] + [(t.grad, want[k][l]) for k in R.GROUPS for l, t in enumerate(P32[k])]
    for got, ref in pairs:
        scale = float(ref.abs().max())
        err = float((got.double() - ref).abs().max())
        worst = max(worst, err / scale)
        assert err <= (1e-4 * scale + 5e-9) / 10
    print(f"[star] premise C={C} hidden={hidden}: y {dev_y:.2e}, worst gradient {worst:.2e}")
    assert dev_y <= 2e-5 / 10


def test_redrawn_rows_leave_no_pre_activation_at_relus_kink():
    """R.redraw_rows_at_a_kink (the inputs of tests/test_star_gpu.py::test_many_tiles): afterwards no hidden pre-activation of
    the fp64 forward lies within the margin of zero, every row that had one was drawn again and most rows were not, and the result depends on the seed
    alone.  The margin here is wide (1e-3) so that a small batch has such rows at all."""
    B, C, hidden, S, rel = 200, 33, (48, 32), 3, 1e-3
    x, _, P = R.draw(B, C, hidden, S, 77)
    ids = torch.randint(0, S, (B,), generator=torch.Generator().manual_seed(1))
    zs = R.hidden_pre_activations(x.double(), ids, R.double(P))
    near = torch.zeros(B, dtype=torch.bool)
    for z in zs:
        near |= (z.abs() < rel * float(torch.relu(z).max())).any(1)
    assert 0 < int(near.sum()) < B
    got, redrawn = R.redraw_rows_at_a_kink(x, ids, P, rel, 5)
    changed = (got != x).any(1)      # a later pass may draw further rows again: the margin follows the largest activation
    assert bool(changed[near].all()) and int(near.sum()) <= int(changed.sum()) <= redrawn < B
    for z in R.hidden_pre_activations(got.double(), ids, R.double(P)):
        assert float(z.abs().min()) >= rel * float(torch.relu(z).max())
    assert torch.equal(R.redraw_rows_at_a_kink(x, ids, P, rel, 5)[0], got)
    y, cache = R.forward(got.double(), ids, R.double(P))      # the same pre-activations as the forward the tests compare with
    for z, h in zip(R.hidden_pre_activations(got.double(), ids, R.double(P)), cache.h[1:]):
        assert torch.equal(torch.relu(z), h)
