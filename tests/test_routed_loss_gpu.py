"""satrans_point_loss_routed on the GPU (csrc/point_loss.hip) and its autograd wrapper RoutedPointLoss: a [B, T] block of per-task
outputs, each row on the column of its own task.  The yardstick is PointLoss itself, bit for bit: with T = 1 the whole result, with
general T the rows of each task against PointLoss of that column.  The loss sum adds the same fp32 terms in another grouping (one
sum over all rows, not one per task), so it is held to the fp64 torch masked sum within tests/point_loss_cases.py's bound for the
sum.  Draws: tests/point_loss_cases.py's, one per column."""
import functools

import pytest
import torch

from satrans_amd import PointLoss, RoutedPointLoss
from tests import point_loss_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TASKS = (1, 2, 3, 7)
KIND = {"sigmoid": "binary", "linear": "regression"}
PREDS = ("sigmoid", "linear")


@functools.lru_cache(maxsize=None)
def block(B, T, pred, loss):
    """-> (z [B, T] fp32, task [B] int64 in [0, T), y [B]) on the CPU: column t holds P.draws' logits rolled by t rows and scaled by 1 - 0.05 t (with
    binary_crossentropy and the linear kind they are probabilities)."""
    z0, y = P.draws(B, pred, loss)
    z = torch.stack([torch.roll(z0, t) * (1.0 - 0.05 * t) for t in range(T)], dim=1).contiguous()
    g = torch.Generator().manual_seed(977 * B + T)
    task = torch.randint(0, T, (B,), generator=g)
    return z, task, y


@functools.lru_cache(maxsize=None)
def masked_sum64(B, T, pred, loss):
    """The reference's masked per-task sum (mtl_basemodel.py:268-269) in fp64 on the CPU."""
    z, task, y = block(B, T, pred, loss)
    total = torch.zeros((), dtype=torch.float64)
    for t in range(T):
        m = task == t
        if bool(m.any()):
            total = total + P.reference(z[m, t], y[m], pred, loss)[1]
    return float(total)


def routed(z, task, y, pred, loss):
    """-> (loss_sum, pred [B, 1], z.grad [B, T]) of RoutedPointLoss on the device."""
    zd = z.to(DEV).requires_grad_(True)
    total, out = RoutedPointLoss(loss, KIND[pred])(zd, task.to(DEV), y.to(DEV))
    total.backward()
    return total.detach(), out, zd.grad


def plain(zcol, y, pred, loss):
    zd = zcol.to(DEV).contiguous().requires_grad_(True)
    total, out = PointLoss(loss, KIND[pred])(zd, y.to(DEV))
    total.backward()
    return total.detach(), out, zd.grad


@pytest.mark.parametrize("B", P.SIZES)
@pytest.mark.parametrize("loss", P.LOSSES)
@pytest.mark.parametrize("pred", PREDS)
def test_one_task_is_point_loss(B, loss, pred):
    z, _, y = block(B, 1, pred, loss)
    total, out, dz = routed(z, torch.zeros(B, dtype=torch.int64), y, pred, loss)
    want_total, want_out, want_dz = plain(z[:, 0], y, pred, loss)
    assert total.dtype == torch.float64 and total.dim() == 0 and out.shape == (B, 1) and dz.shape == (B, 1)
    assert torch.equal(out, want_out) and torch.equal(dz.view(-1), want_dz.view(-1)) and torch.equal(total, want_total)


@pytest.mark.parametrize("B", P.SIZES)
@pytest.mark.parametrize("T", TASKS)
@pytest.mark.parametrize("loss", P.LOSSES)
@pytest.mark.parametrize("pred", PREDS)
def test_each_task_is_point_loss_of_its_column(B, T, loss, pred):
    z, task, y = block(B, T, pred, loss)
    total, out, dz = routed(z, task, y, pred, loss)
    want_dz = torch.zeros(B, T, device=DEV)
    for t in range(T):
        _, col_out, col_dz = plain(z[:, t], y, pred, loss)
        m = (task == t).to(DEV)
        assert torch.equal(out.view(-1)[m], col_out.view(-1)[m]), t
        want_dz[:, t] = torch.where(m, col_dz.view(-1), torch.zeros_like(col_dz.view(-1)))
    assert torch.equal(dz, want_dz)                        # the own column PointLoss's bits, every other entry exactly 0
    want = masked_sum64(B, T, pred, loss)
    err = abs(float(total) - want)
    print(f"B={B} T={T} {loss} {pred}: loss sum rel {err / max(abs(want), 1e-300):.3e}")
    assert err <= P.LOSS_RTOL * abs(want)


@pytest.mark.parametrize("B", (65, 1000))
@pytest.mark.parametrize("loss", P.LOSSES)
def test_rows_of_no_task(B, loss):
    """task = -1 and task = T: pred 0, a zero dz row, and the sum of the run without those rows."""
    T = 3
    z, task, y = block(B, T, "sigmoid", loss)
    total, out, dz = routed(z, task, y, "sigmoid", loss)
    extra = torch.tensor([-1, T, -1, T, 2 ** 31 - 1, -2 ** 31])
    n = B + len(extra)
    keep = torch.ones(n, dtype=torch.bool)
    keep[torch.tensor([0, 2, n // 2, n - 3, n - 2, n - 1])] = False      # where the rows of no task go
    z2, task2, y2 = torch.full((n, T), 0.3), torch.zeros(n, dtype=torch.int64), torch.ones(n)
    z2[keep], task2[keep], y2[keep] = z, task, y
    task2[~keep] = extra
    total2, out2, dz2 = routed(z2, task2, y2, "sigmoid", loss)
    keep = keep.to(DEV)
    assert bool((out2[~keep] == 0).all()) and bool((dz2[~keep] == 0).all())
    assert torch.equal(out2[keep], out) and torch.equal(dz2[keep], dz)
    # (the same fp32 terms and exact zeros, at other lanes: the grouping of the double sum moves)
    assert abs(float(total2) - float(total)) <= 1e-12 * abs(float(total))
    only = torch.full((B,), -1, dtype=torch.int64)                      # nobody has a task: nothing at all
    total3, out3, dz3 = routed(z, only, y, "sigmoid", loss)
    assert float(total3) == 0.0 and bool((out3 == 0).all()) and bool((dz3 == 0).all())


@pytest.mark.parametrize("B", (64, 257))
def test_a_task_without_rows_and_all_rows_in_one_task(B):
    T, loss = 3, "binary_crossentropy"
    z, task, y = block(B, T, "sigmoid", loss)
    task = torch.where(task == 1, torch.full_like(task, 2), task)       # task 1 has no rows
    total, out, dz = routed(z, task, y, "sigmoid", loss)
    assert bool((dz[:, 1] == 0).all())
    for t in (0, 2):
        _, col_out, col_dz = plain(z[:, t], y, "sigmoid", loss)
        m = (task == t).to(DEV)
        assert torch.equal(out.view(-1)[m], col_out.view(-1)[m]) and torch.equal(dz[m, t], col_dz.view(-1)[m])
    total, out, dz = routed(z, torch.full((B,), 2), y, "sigmoid", loss)      # all rows in the last task
    want_total, want_out, want_dz = plain(z[:, 2], y, "sigmoid", loss)
    assert torch.equal(total, want_total) and torch.equal(out, want_out) and torch.equal(dz[:, 2], want_dz.view(-1))
    assert bool((dz[:, :2] == 0).all())


@pytest.mark.parametrize("B", (257, 8269))
def test_two_runs_same_bits(B):
    z, task, y = block(B, 3, "sigmoid", "binary_crossentropy")
    a, b = routed(z, task, y, "sigmoid", "binary_crossentropy"), routed(z, task, y, "sigmoid", "binary_crossentropy")
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("B", (63, 1000))
def test_a_row_stride_and_a_dz_full_of_nan(B):
    from satrans_amd import native as N
    T = 3
    z, task, y = block(B, T, "sigmoid", "mse")
    total, out, dz = routed(z, task, y, "sigmoid", "mse")
    wide = torch.full((B, T + 2), float("nan"), device=DEV)
    wide[:, :T] = z.to(DEV)
    view = wide[:, :T]                                                  # row stride T + 2
    assert not view.is_contiguous()
    vd = view.detach().requires_grad_(True)
    total2, out2 = RoutedPointLoss("mse", "binary")(vd, task.to(DEV), y.to(DEV))
    total2.backward()
    assert torch.equal(total2.detach(), total) and torch.equal(out2, out) and torch.equal(vd.grad, dz)
    # the entry point itself, over outputs filled with NaN: every entry of pred and dz comes back written
    lib = N.lib()
    pred = torch.full((B,), float("nan"), device=DEV)
    raw = torch.full((B, T), float("nan"), device=DEV)
    acc = torch.zeros(1, dtype=torch.float64, device=DEV)
    part = torch.empty(max(int(lib.satrans_point_loss_partials(B)), 1), dtype=torch.float64, device=DEV)
    t32, yd = task.to(DEV).to(torch.int32), y.to(DEV)
    N.check(lib.satrans_point_loss_routed(view.data_ptr(), view.stride(0), t32.data_ptr(), yd.data_ptr(), B, T, 0, 1, pred.data_ptr(),
                                          raw.data_ptr(), acc.data_ptr(), part.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "satrans_point_loss_routed")
    assert not bool(torch.isnan(raw).any()) and not bool(torch.isnan(pred).any())
    assert torch.equal(raw, dz) and torch.equal(pred.view(B, 1), out) and torch.equal(acc[0], total)


@pytest.mark.parametrize("loss", P.LOSSES)
def test_autograd_scaling_no_grad_and_prediction_only(loss):
    B, T = 257, 3
    z, task, y = block(B, T, "sigmoid", loss)
    total, out, dz = routed(z, task, y, "sigmoid", loss)
    mod = RoutedPointLoss(loss, "binary")
    zd, td, yd = z.to(DEV).requires_grad_(True), task.to(DEV), y.to(DEV).view(B, 1)
    scaled, out2 = mod(zd, td, yd)
    assert not out2.requires_grad
    (scaled * 0.25).backward()                                          # 0.25: exactly
    assert torch.equal(zd.grad, 0.25 * dz)
    with torch.no_grad():
        total3, out3 = mod(zd, td, yd)
    assert torch.equal(total3, total) and torch.equal(out3, out) and not total3.requires_grad
    none, out4 = mod(zd, td)
    assert none is None and torch.equal(out4, out)
    with pytest.raises(ValueError):
        mod(zd, td.float(), yd)
    with pytest.raises(ValueError):
        mod(zd.view(-1), td, yd)
