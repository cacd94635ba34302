"""The draws and the fp64 references of the satrans_point_loss tests (test_point_loss_cpu.py, test_point_loss_gpu.py).

z = clamp(2 N(0,1), +-8), labels 0/1.  The linear prediction (task='regression') takes the logit itself as the prediction; with
binary_crossentropy torch refuses a prediction outside [0, 1], so for that pair the logit column is sigmoid(z), a probability.
The bounds are the sibling bounds of DESIGN.md §4."""
import functools

import torch
import torch.nn.functional as F

SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 8269)      # lane, wave and block edges; a ragged last block; more than 32 blocks
LOSSES = ("binary_crossentropy", "mse", "mae")
LOSS_KIND = {"binary_crossentropy": 0, "mse": 1, "mae": 2}
PRED_KIND = {"sigmoid": 0, "linear": 1}
PRED_RTOL, LOSS_RTOL, GRAD_RTOL, GRAD_ATOL = 2e-5, 2e-5, 1e-4, 5e-9
TORCH_LOSS = {"binary_crossentropy": F.binary_cross_entropy, "mse": F.mse_loss, "mae": F.l1_loss}


@functools.lru_cache(maxsize=None)
def draws(B, pred, loss):
    """-> (z [B] fp32, y [B] fp32), the same for every test that asks."""
    g = torch.Generator().manual_seed(20240 + B)
    z = (2.0 * torch.randn(B, generator=g)).clamp_(-8.0, 8.0)
    y = (torch.rand(B, generator=g) < 0.3).float()
    if pred == "linear" and loss == "binary_crossentropy":
        z = torch.sigmoid(z)
    return z, y


def reference(z, y, pred, loss, dtype=torch.float64):
    """torch's own composition at `dtype` on the CPU -> (pred, loss sum, d loss sum / dz)."""
    zz = z.to(dtype).clone().requires_grad_(True)
    p = torch.sigmoid(zz) if pred == "sigmoid" else zz * 1.0
    total = TORCH_LOSS[loss](p, y.to(dtype), reduction="sum")
    g, = torch.autograd.grad(total, zz)
    return p.detach(), total.detach(), g


@functools.lru_cache(maxsize=None)
def reference64(B, pred, loss):
    return reference(*draws(B, pred, loss), pred, loss)
