"""Partitioned normalisation without a GPU: the fp64 restatement against the reference's recorded runs, the modules' state,
the C ABI's new symbols and their argument validation, and the premise of the GPU conditioning test."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from satrans_amd import native
from tests import mdr_bn_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mdr_bn")
CASES = ("even", "ragged")
SYMBOLS = ("satrans_pnorm_saved_floats", "satrans_pnorm_workspace_floats", "satrans_pnorm_fwd", "satrans_pnorm_bwd")
GRADS = ("x", "weight", "bias", "shared_weight", "shared_bias")

# Largest deviation of the fp64 restatement from a recorded array, relative to the array's largest magnitude, measured once
# over every array of both fixtures (see test_restatement_reproduces_every_fixture).  The recorded side is an fp32 run.
MEASURED_DEVIATION = {"grad": 1.97e-5, "other": 1.31e-6}
BOUND = {k: 4 * v for k, v in MEASURED_DEVIATION.items()}


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def replay(fx):
    """Every recorded result of a fixture, recomputed by tests/mdr_bn_reference.py in fp64 from the recorded fp32 inputs."""
    t = lambda k: torch.from_numpy(fx[k]).double()      # noqa: E731
    x, w, sw, sb = t("x"), t("w"), t("shared_weight"), t("shared_bias")
    sid = torch.from_numpy(fx["ids"]) - int(fx["offset"])
    out = {}
    for tag, momentum in (("m01", 0.1), ("cma", None)):
        st = R.State.fresh(*fx["weight"].shape)
        st.weight, st.bias = t("weight"), t("bias")
        for step in (1, 2, 3):
            y, cache = R.forward(x[step - 1], sid, st, sw, sb, 1e-5, momentum, training=True)
            if step == 1:
                out[f"{tag}/y1"] = y
                if tag == "m01":
                    out.update({f"grad_train/{k}": v for k, v in R.backward(w, cache).items()})
            if step in (1, 3):
                out[f"{tag}/buf{step}/running_mean"] = st.running_mean.clone()
                out[f"{tag}/buf{step}/running_var"] = st.running_var.clone()
                out[f"{tag}/buf{step}/nbt"] = torch.tensor(st.num_batches_tracked)
        y, cache = R.forward(x[0], sid, st, sw, sb, 1e-5, momentum, training=False)
        out[f"{tag}/y_eval"] = y
        if tag == "m01":
            out.update({f"grad_eval/{k}": v for k, v in R.backward(w, cache).items()})
    return out


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_every_fixture(name):
    """tests/mdr_bn_reference.py (fp64) against the reference's own fp32 run cast up: outputs in both modes, buffers and
    num_batches_tracked after 1 and 3 training steps for momentum 0.1 and None, all gradients of sum(y * w) in both modes.

    Measured once over both fixtures, relative to the recorded array's largest magnitude, the largest deviation is 1.97e-5
    (`ragged`, grad_train/x: the two-row scenario, whose dx is what n * dy - sum(dy) - xhat * sum(dy * xhat) leaves after
    cancelling to nearly zero, carries the recorded fp32 run's rounding; the next gradient is at 4.2e-7) and, over outputs and
    buffers, 1.31e-6 (`ragged`, y1: torch's fp32 CPU form x * a + (b - mean * a)).  `even` stays below 1.7e-7 throughout.
    The bound is 4x the measured value, taken separately for gradients and for everything else."""
    fx = load(name)
    got = replay(fx)
    recorded = [k for k in fx if k.split("/")[0] in ("m01", "cma", "grad_train", "grad_eval")]
    assert sorted(recorded) == sorted(got)
    for k in recorded:
        rec = torch.from_numpy(fx[k]).double()
        if k.endswith("/nbt"):
            assert torch.equal(got[k].double(), rec), k
            continue
        dev = float((got[k] - rec).abs().max() / rec.abs().max())
        assert dev <= BOUND["grad" if k.startswith("grad_") else "other"], (k, dev)


def test_explicit_backward_equals_autograd():
    """The restatement's backward formulas are the derivative of its forward (fp64 autograd), in both modes."""
    fx = load("ragged")
    t = lambda k: torch.from_numpy(fx[k]).double()      # noqa: E731
    sid = torch.from_numpy(fx["ids"]) - int(fx["offset"])
    for training in (True, False):
        st = R.State.fresh(*fx["weight"].shape)
        st.weight, st.bias = t("weight").requires_grad_(True), t("bias").requires_grad_(True)
        st.running_mean, st.running_var = t("m01/buf3/running_mean"), t("m01/buf3/running_var")
        x, sw, sb = t("x")[0].requires_grad_(True), t("shared_weight").requires_grad_(True), t("shared_bias").requires_grad_(True)
        y, cache = R.forward(x, sid, st, sw, sb, training=training)
        (y * t("w")).sum().backward()
        auto = dict(x=x.grad, weight=st.weight.grad, bias=st.bias.grad, shared_weight=sw.grad, shared_bias=sb.grad)
        with torch.no_grad():
            mine = R.backward(t("w"), cache)
        for k in GRADS:
            assert float((mine[k] - auto[k]).abs().max()) <= 1e-12 * float(auto[k].abs().max()), (training, k)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_matches_the_reference(name):
    """Keys, order, shapes, dtypes and initial values of state_dict(): a fresh MDR_BatchNorm and a fresh PartitionedNorm
    (`bns.{i}.*`, as in the reference's Star_Net)."""
    from satrans_amd import MDR_BatchNorm, PartitionedNorm
    fx = load(name)
    S, Cn = fx["weight"].shape
    for prefix, mod in (("init1/", MDR_BatchNorm(Cn)), ("init/", PartitionedNorm(Cn, S))):
        want = [k[len(prefix):] for k in fx if k.startswith(prefix)]
        sd = mod.state_dict()
        assert list(sd) == want
        for k in want:
            rec = fx[prefix + k]
            assert tuple(sd[k].shape) == rec.shape and sd[k].numpy().dtype == rec.dtype, k
            assert np.array_equal(sd[k].numpy(), rec), k
    one = MDR_BatchNorm(Cn, momentum=None, track_running_stats=False)
    assert one.running_mean is None and one.num_batches_tracked is None and list(one.state_dict()) == ["weight", "bias"]
    with pytest.raises(ValueError):
        MDR_BatchNorm(Cn, affine=False)


def test_modules_refuse_what_is_not_built_before_touching_a_device():
    from satrans_amd import MDR_BatchNorm, PartitionedNorm
    sw, sb = torch.ones(4), torch.zeros(4)
    with pytest.raises(NotImplementedError, match="2-D"):
        MDR_BatchNorm(4)(torch.zeros(2, 4, 3), sw, sb)
    with pytest.raises(NotImplementedError, match="2-D"):
        PartitionedNorm(4, 2)(torch.zeros(2, 4, 3), torch.zeros(2), sw, sb)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        MDR_BatchNorm(4)(torch.zeros(3, 4), sw, sb)
    with pytest.raises(native.NativeError, match="no CPU fallback"):
        PartitionedNorm(4, 2)(torch.zeros(3, 4), torch.zeros(3), sw, sb)


def test_abi_carries_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in native.SIGNATURES, sym
    assert "typedef struct satrans_pnorm_desc" in header
    assert int(re.search(r"#define SATRANS_ABI_VERSION (\d+)", header).group(1)) == 7 == native.ABI_VERSION
    assert int(re.search(r"#define SATRANS_PNORM_ROW_CHUNK (\d+)", header).group(1)) == native.PNORM_ROW_CHUNK
    # B, C, S, flags, eps, factor + nine pointers
    assert ctypes.sizeof(native.PNormDesc) == 6 * 4 + 9 * 8


def test_library_validates_descriptors_without_a_device():
    lib = native.lib()
    assert lib.satrans_abi_version() == 7
    null = ctypes.POINTER(native.PNormDesc)()
    assert lib.satrans_pnorm_saved_floats(null) == -1
    assert lib.satrans_pnorm_workspace_floats(null) == -1
    assert lib.satrans_pnorm_fwd(null, None, None, None, None) == -1
    assert b"null descriptor" in lib.satrans_last_error()
    for B, Cn, S in ((0, 8, 2), (4, 0, 2), (4, 8, 0), (-1, 8, 2), (4, -8, 2), (4, 8, -2)):
        d = native.PNormDesc()
        d.B, d.C, d.S, d.eps, d.factor = B, Cn, S, 1e-5, 0.1
        assert lib.satrans_pnorm_saved_floats(ctypes.byref(d)) == -1, (B, Cn, S)
        assert lib.satrans_pnorm_workspace_floats(ctypes.byref(d)) == -1, (B, Cn, S)
        assert lib.satrans_pnorm_fwd(ctypes.byref(d), None, None, None, None) == -1, (B, Cn, S)
        assert b"bad sizes" in lib.satrans_last_error()
    d = native.PNormDesc()
    d.B, d.C, d.S, d.eps, d.factor = 300, 70, 3, 1e-5, 0.1
    assert lib.satrans_pnorm_saved_floats(ctypes.byref(d)) == 2 * 3 * 70
    slots = -(-300 // native.PNORM_ROW_CHUNK) + 3
    assert lib.satrans_pnorm_workspace_floats(ctypes.byref(d)) == slots * 3 * 70 + 2 * 3 * 70
    assert lib.satrans_pnorm_fwd(ctypes.byref(d), None, None, None, None) == -1      # sizes fine, pointers null
    assert b"null pointer" in lib.satrans_last_error()
    assert lib.satrans_pnorm_bwd(ctypes.byref(d), None, None, None, None, None, None, None, None, None) == -1
    d.flags = 4
    assert lib.satrans_pnorm_saved_floats(ctypes.byref(d)) == -1


def test_conditioning_premise():
    """The inputs of the GPU conditioning test (mean 100, standard deviation 0.1, 300 rows) separate a sound variance from
    E[x^2] - E[x]^2 in fp32: torch's fp32 F.batch_norm stays within 1e-3 of the fp64 result, the naive form is off by at least
    100x torch's error (probed: 9e-5 against 0.36)."""
    x = R.conditioning_rows()
    assert x.shape == (300, 64) and x.dtype == torch.float32
    want = F.batch_norm(x.double(), None, None, None, None, True, 0.0, 1e-5)
    torch_err = float((F.batch_norm(x, None, None, None, None, True, 0.0, 1e-5).double() - want).abs().max())
    mean = x.mean(0)
    var = ((x * x).mean(0) - mean * mean).clamp_min(0)
    naive_err = float((((x - mean) / torch.sqrt(var + 1e-5)).double() - want).abs().max())
    print(f"torch fp32 error {torch_err:.3g}, naive fp32 error {naive_err:.3g}")
    assert torch_err <= 1e-3
    assert naive_err >= 100 * torch_err
