"""satrans_point_loss on the GPU (csrc/point_loss.hip): bit-equality with the shipped head's prediction and gradient, the fp64
form of torch on the CPU within the sibling bounds of DESIGN.md §4, saturation, reproducibility, the optional outputs, and the
autograd wrapper PointLoss.  Draws and references: tests/point_loss_cases.py."""
import numpy as np
import pytest
import torch

from satrans_amd import PointLoss, native as N
from tests import point_loss_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = dict(dtype=torch.float64, device=DEV)
F32 = dict(dtype=torch.float32, device=DEV)


def stream():
    return torch.cuda.current_stream().cuda_stream


def column(z, stride):
    """z as column 0 of a [B, stride] block whose other columns hold something else."""
    block = torch.full((z.shape[0], stride), 7.5, **F32)
    block[:, 0] = z.to(DEV)
    return block


def point_loss(block, y, pred, loss, want_dz=True, loss_sum=None, with_y=True):
    lib, B = N.lib(), block.shape[0]
    out = torch.full((B,), -3.0, **F32)
    dz = torch.full((B,), -3.0, **F32)
    total = torch.zeros(1, **F64) if loss_sum is None else loss_sum
    part = torch.full((max(int(lib.satrans_point_loss_partials(B)), 1),), -3.0, **F64)
    N.check(lib.satrans_point_loss(block.data_ptr(), block.stride(0), y.data_ptr() if with_y else None, B, P.PRED_KIND[pred],
                                   P.LOSS_KIND[loss], out.data_ptr(), dz.data_ptr() if want_dz else None, total.data_ptr(),
                                   part.data_ptr(), stream()), "satrans_point_loss")
    return out, dz, total, part


def head_loss(z, y, loss):
    """satrans_head_loss over a = [B, 4] with z in column 0, w = (1, 0, 0, 0), bias 0 -> (prob, dlogit = da[:, 0])."""
    lib, B = N.lib(), z.shape[0]
    a = torch.zeros(B, 4, **F32)
    a[:, 0] = z
    w = torch.tensor([1.0, 0.0, 0.0, 0.0], **F32)
    bias, prob, da = torch.zeros(1, **F32), torch.empty(B, **F32), torch.empty(B, 4, **F32)
    g_w, g_b, total = torch.zeros(4, **F32), torch.zeros(1, **F32), torch.zeros(1, **F64)
    scratch = torch.empty(max(int(lib.satrans_head_scratch_floats(B, 4, 0)), 1), **F32)
    N.check(lib.satrans_head_loss(a.data_ptr(), None, 0, None, 0, B, 4, w.data_ptr(), bias.data_ptr(), prob.data_ptr(), None,
                                  y.data_ptr(), total.data_ptr(), da.data_ptr(), g_w.data_ptr(), g_b.data_ptr(), scratch.data_ptr(),
                                  P.LOSS_KIND[loss], stream()), "satrans_head_loss")
    return prob, da[:, 0].contiguous(), total


@pytest.mark.parametrize("B", P.SIZES)
@pytest.mark.parametrize("loss", P.LOSSES)
def test_prediction_and_gradient_are_the_shipped_heads_bits(B, loss):
    z, y = P.draws(B, "sigmoid", loss)
    zd, yd = z.to(DEV), y.to(DEV)
    prob, dlogit, head_total = head_loss(zd, yd, loss)
    for stride in (1, 3):
        pred, dz, total, _ = point_loss(column(z, stride), yd, "sigmoid", loss)
        assert torch.equal(pred, prob), stride
        assert torch.equal(dz, dlogit), stride
    # (the loss sums are both sums of the same fp32 terms, in another grouping and the head's partly in fp32)
    assert abs(float(total) - float(head_total)) <= P.LOSS_RTOL * abs(float(head_total))


@pytest.mark.parametrize("B", P.SIZES)
@pytest.mark.parametrize("loss", P.LOSSES)
@pytest.mark.parametrize("pred", ("sigmoid", "linear"))
def test_against_fp64_torch(B, loss, pred):
    z, y = P.draws(B, pred, loss)
    p64, l64, g64 = P.reference64(B, pred, loss)
    for stride in (1, 3):
        out, dz, total, _ = point_loss(column(z, stride), y.to(DEV), pred, loss)
        perr = float((out.cpu().double() - p64).abs().max())
        lerr = abs(float(total) - float(l64))
        gerr = float((dz.cpu().double() - g64).abs().max())
        print(f"B={B} {loss} {pred} stride={stride}: pred {perr:.3e} loss rel {lerr / max(abs(float(l64)), 1e-300):.3e} dz {gerr:.3e}")
        assert perr <= P.PRED_RTOL * float(p64.abs().max())
        assert lerr <= P.LOSS_RTOL * abs(float(l64))
        assert gerr <= P.GRAD_RTOL * float(g64.abs().max()) + P.GRAD_ATOL


@pytest.mark.parametrize("loss", P.LOSSES)
def test_saturation(loss):
    """z = +-20, +-120 with both labels.  In fp32 the sigmoid is exactly 1 at z = 20 and 120 and exactly 0 at z = -120: there
    p(1-p) is 0, dz is exactly 0 and the cross-entropy is exactly 100 (the clamped log) against the other label, 0 with its own.
    At z = -20 the fp32 sigmoid is 2.06e-9, not 0: the cross-entropy with label 1 is -log(p) = 20, with label 0 exactly 0."""
    z = torch.tensor([20.0, 20.0, -20.0, -20.0, 120.0, 120.0, -120.0, -120.0])
    y = torch.tensor([0.0, 1.0] * 4)
    out, dz, total, _ = point_loss(column(z, 1), y.to(DEV), "sigmoid", loss)
    per = torch.stack([point_loss(column(z[i:i + 1], 1), y[i:i + 1].to(DEV), "sigmoid", loss)[2][0] for i in range(8)]).cpu()
    out, dz = out.cpu(), dz.cpu()
    for t in (out, dz, per, total.cpu()):
        assert bool(torch.isfinite(t).all())
    assert out.tolist()[:2] == [1.0, 1.0] and out.tolist()[4:] == [1.0, 1.0, 0.0, 0.0]
    flat = (out * (1.0 - out)) == 0
    assert flat.tolist() == [True, True, False, False, True, True, True, True]
    assert bool((dz[flat] == 0).all())
    if loss == "binary_crossentropy":
        assert per.tolist()[:2] == [100.0, 0.0] and per.tolist()[4:] == [100.0, 0.0, 0.0, 100.0]
        assert per[2] == 0.0 and abs(float(per[3]) + np.log(float(out[3].double()))) <= P.LOSS_RTOL * 20.0
    else:      # |p - t| and its square are exactly 0 or 1 at the saturated rows
        assert per.tolist()[:2] == [1.0, 0.0] and per.tolist()[4:] == [1.0, 0.0, 0.0, 1.0]
    assert float(total) == pytest.approx(float(per.sum()), rel=1e-15)


@pytest.mark.parametrize("B", (257, 8269))
def test_two_runs_same_bits_and_the_sum_accumulates(B):
    z, y = P.draws(B, "sigmoid", "binary_crossentropy")
    block, yd = column(z, 3), y.to(DEV)
    o1, d1, t1, _ = point_loss(block, yd, "sigmoid", "binary_crossentropy")
    o2, d2, t2, _ = point_loss(block, yd, "sigmoid", "binary_crossentropy")
    assert torch.equal(o1, o2) and torch.equal(d1, d2) and torch.equal(t1, t2)
    _, _, t3, _ = point_loss(block, yd, "sigmoid", "binary_crossentropy", loss_sum=t2)
    assert float(t3) == 2.0 * float(t1)                    # a + a is exact
    o1, _, t1, _ = point_loss(column(z[:200], 1), yd[:200].contiguous(), "sigmoid", "mse")      # one block adds its sum itself
    _, _, t4, _ = point_loss(column(z[:200], 1), yd[:200].contiguous(), "sigmoid", "mse", loss_sum=t1.clone())
    assert float(t4) == 2.0 * float(t1)


@pytest.mark.parametrize("B", (64, 1000))
def test_optional_outputs_stay_untouched(B):
    z, y = P.draws(B, "sigmoid", "binary_crossentropy")
    block, yd = column(z, 1), y.to(DEV)
    full = point_loss(block, yd, "sigmoid", "binary_crossentropy")
    out, dz, total, _ = point_loss(block, yd, "sigmoid", "binary_crossentropy", want_dz=False)      # evaluation: no dz
    assert torch.equal(out, full[0]) and torch.equal(total, full[2]) and bool((dz == -3.0).all())
    sentinel = torch.full((1,), 11.0, **F64)
    out, dz, total, part = point_loss(block, yd, "sigmoid", "binary_crossentropy", loss_sum=sentinel, with_y=False)      # no labels
    assert torch.equal(out, full[0]) and bool((dz == -3.0).all()) and float(total) == 11.0 and bool((part == -3.0).all())


@pytest.mark.parametrize("loss", P.LOSSES)
@pytest.mark.parametrize("task", ("binary", "regression"))
def test_point_loss_autograd(loss, task):
    B, pred = 257, {"binary": "sigmoid", "regression": "linear"}[task]
    z, y = P.draws(B, pred, loss)
    p64, l64, g64 = P.reference64(B, pred, loss)
    mod = PointLoss(loss, task)
    logit = z.to(DEV).view(B, 1).requires_grad_(True)
    total, out = mod(logit, y.to(DEV).view(B, 1))
    assert total.dtype == torch.float64 and total.dim() == 0 and out.shape == (B, 1) and not out.requires_grad
    total.backward()
    assert abs(float(total.detach()) - float(l64)) <= P.LOSS_RTOL * abs(float(l64))
    assert float((out.cpu().double().view(-1) - p64).abs().max()) <= P.PRED_RTOL * float(p64.abs().max())
    g = logit.grad.clone()
    assert float((g.cpu().double().view(-1) - g64).abs().max()) <= P.GRAD_RTOL * float(g64.abs().max()) + P.GRAD_ATOL
    logit.grad = None
    total2, _ = mod(logit, y.to(DEV))
    (total2 * 0.25).backward()                             # a non-unit upstream gradient scales dz (0.25: exactly)
    assert torch.equal(logit.grad, 0.25 * g)
    flat = z.to(DEV).requires_grad_(True)                  # [B] as well
    mod(flat, y.to(DEV))[0].backward()
    assert torch.equal(flat.grad, g.view(-1))
    with torch.no_grad():                                  # evaluation: the loss without a graph
        total3, out3 = mod(logit, y.to(DEV))
    assert torch.equal(total3, total.detach()) and torch.equal(out3, out) and not total3.requires_grad
    none, out4 = mod(logit)                                # prediction only
    assert none is None and torch.equal(out4, out)
