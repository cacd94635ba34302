"""satrans_point_loss without a GPU: the header and the binding carry the symbols, the library refuses bad arguments before any
launch, and the premise of the GPU test's bounds - torch's own fp32 form of the same composition stays far inside them."""
import os
import re

import pytest
import torch

from satrans_amd import native as N
from tests import point_loss_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 4096      # a non-null address: every call below is refused before anything reads it


def test_header_and_binding_carry_the_symbols():
    header = open(os.path.join(ROOT, "include", "satrans_hip.h")).read()
    for name in ("satrans_point_loss", "satrans_point_loss_partials"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in N.SIGNATURES
    assert re.search(r"#define SATRANS_PRED_SIGMOID 0\b", header) and re.search(r"#define SATRANS_PRED_LINEAR 1\b", header)
    assert len(N.SIGNATURES["satrans_point_loss"][1]) == 11
    from satrans_amd import layers
    assert layers.PRED_KINDS == {"binary": 0, "regression": 1} and layers.LOSS_KINDS == P.LOSS_KIND


def test_partials_count():
    lib = N.lib()
    assert [lib.satrans_point_loss_partials(b) for b in (-1, 0, 1, 256, 257, 8269)] == [0, 0, 1, 1, 2, 33]


@pytest.mark.parametrize("what, args", [
    ("B = 0", dict(B=0)), ("B < 0", dict(B=-3)), ("null z", dict(z=None)), ("null pred", dict(pred=None)),
    ("labels without a loss sum", dict(loss_sum=None)), ("prediction kind", dict(pred_kind=2)), ("prediction kind < 0", dict(pred_kind=-1)),
    ("loss kind", dict(loss_kind=3)), ("loss kind < 0", dict(loss_kind=-1)), ("stride", dict(z_stride=0)),
    ("several blocks without scratch", dict(B=257, partial=None)),
])
def test_bad_arguments_are_refused_before_any_launch(what, args):
    a = dict(z=PTR, z_stride=1, y=PTR, B=8, pred_kind=0, loss_kind=0, pred=PTR, dz=PTR, loss_sum=PTR, partial=PTR)
    a.update(args)
    lib = N.lib()
    rc = lib.satrans_point_loss(a["z"], a["z_stride"], a["y"], a["B"], a["pred_kind"], a["loss_kind"], a["pred"], a["dz"],
                                a["loss_sum"], a["partial"], None)
    assert rc == -1, what                                 # SATRANS_E_BADARG
    assert b"point_loss" in lib.satrans_last_error(), what


def test_point_loss_module_refuses_what_it_cannot_take():
    from satrans_amd import PointLoss
    with pytest.raises(NotImplementedError):
        PointLoss("hinge")
    with pytest.raises(ValueError):
        PointLoss("mse", task="ranking")
    with pytest.raises(N.NativeError):
        PointLoss()(torch.zeros(4, 1))                   # a CPU tensor: there is no fallback


@pytest.mark.parametrize("B", P.SIZES)
@pytest.mark.parametrize("loss", P.LOSSES)
@pytest.mark.parametrize("pred", ("sigmoid", "linear"))
def test_torch_fp32_stays_within_a_tenth_of_each_bound(B, loss, pred):
    """The bounds come from the sibling bounds, not from the kernel: torch's fp32 composition of the same draws
    must use at most a tenth of each (measured on the CPU for these shapes: at worst 0.005 of the gradient bound and 8.4e-8
    relative on the loss)."""
    z, y = P.draws(B, pred, loss)
    p64, l64, g64 = P.reference64(B, pred, loss)
    p32, l32, g32 = P.reference(z, y, pred, loss, torch.float32)
    assert float((p32.double() - p64).abs().max()) <= 0.1 * P.PRED_RTOL * float(p64.abs().max())
    assert abs(float(l32) - float(l64)) <= 0.1 * P.LOSS_RTOL * abs(float(l64)) + 1e-30
    assert float((g32.double() - g64).abs().max()) <= 0.1 * (P.GRAD_RTOL * float(g64.abs().max()) + P.GRAD_ATOL)
