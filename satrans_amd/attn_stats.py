"""Scenario-specific attention maps: predict's `showattn` branch (reference models/meta_basemodel.py:421-426, 439-458, 506-514).

The reference sums every layer's `normalized_att_scores` [H, B, F, F] over the test set, split by scenario j (domain id j + bias,
bias = 1 when the smallest domain id of the WHOLE array is 1, else 0) and by label (pos: y == 1, neg: y == 0, all: every sample),
and divides each sum by its sample count.  Here the sums are taken on the device (csrc/attn_stats.hip) batch by batch, right behind
each layer's forward, from ONE reused attention buffer; the host side below turns domain ids and labels into one accumulator row per
sample (its key) and does the counting and the division.

One deliberate deviation: a (scenario, class) pair without samples crashes the reference (0.0 / 0, then .cpu() on a float); here
its mean is an all-NaN map.
"""
from __future__ import annotations

import numpy as np
import torch

from . import native as N

POS, NEG, OTHER = 0, 1, 2           # key = 3 j + class; the returned statistics use the class order (pos, neg, all)


def scenario_bias(domain_ids) -> int:
    """1 when the smallest domain id of the whole array is 1, else 0 (reference meta_basemodel.py:447-450)."""
    d = np.asarray(domain_ids)
    return 1 if d.size and d.min() == 1 else 0


def class_keys(domain_ids, y, S: int, bias: int) -> np.ndarray:
    """int32 [N]: 3 j + c for a sample of scenario j (domain id j + bias, j in [0, S)) and class c (0: y == 1, 1: y == 0,
    2: any other label), -1 for a sample whose domain id names no scenario (it counts nowhere, as in the reference)."""
    d = np.asarray(domain_ids).reshape(-1)
    lab = np.asarray(y).reshape(-1)
    if d.shape[0] != lab.shape[0]:
        raise ValueError(f"domain_ids has {d.shape[0]} entries, y has {lab.shape[0]}")
    j = d.astype(np.float64) - bias
    ok = (j >= 0) & (j < S) & (j == np.floor(j))
    c = np.where(lab == 1, POS, np.where(lab == 0, NEG, OTHER))
    return np.where(ok, 3 * np.where(ok, j, 0).astype(np.int64) + c, -1).astype(np.int32)


def class_counts(keys: np.ndarray, S: int) -> np.ndarray:
    """int64 [S, 3]: samples per scenario in the class order (pos, neg, all)."""
    k = np.asarray(keys).reshape(-1)
    raw = np.bincount(k[k >= 0], minlength=3 * S).astype(np.int64).reshape(S, 3)
    return np.stack([raw[:, POS], raw[:, NEG], raw.sum(1)], axis=1)


def finish(raw_sum: np.ndarray, keys: np.ndarray, S: int, bias: int) -> dict:
    """raw_sum: fp64 [L, 3 S, H, F, F] of the device accumulator (key rows) -> {"sum": [L, S, 3, H, F, F] (pos, neg, all),
    "count": int64 [S, 3], "mean": sum / count (NaN where the count is 0), "bias": int}."""
    L = raw_sum.shape[0]
    r = raw_sum.reshape(L, S, 3, *raw_sum.shape[2:])
    s = np.stack([r[:, :, POS], r[:, :, NEG], r[:, :, POS] + r[:, :, NEG] + r[:, :, OTHER]], axis=2)
    cnt = class_counts(keys, S)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s / cnt.reshape(1, S, 3, 1, 1, 1).astype(np.float64)
    mean[:, cnt == 0] = np.nan
    return {"sum": s, "count": cnt, "mean": mean, "bias": int(bias)}


class AttentionStatistics:
    """Device side of one pass: the fp64 accumulator [L, 3 S, H, F, F], the reused attention buffer [H, B, F, F] of the largest
    batch seen, the statistics kernel's workspace and the keys of the batch the next forward evaluates (`set_batch`).
    PathEngine.forward(..., stats=ctx) writes each layer's attention into the buffer and queues the accumulation behind it."""

    def __init__(self, engine, S: int):
        self.eng, self.S, self.K = engine, int(S), 3 * int(S)
        eng = engine
        self.acc = torch.zeros(eng.L, self.K, eng.H, eng.F, eng.F, dtype=torch.float64, device=eng.dev)
        self._att = None
        self._ws = None
        self._keys = None

    def set_batch(self, keys: torch.Tensor) -> None:
        """int32 [B] device keys (class_keys) of the samples of the next forward, in their order."""
        if keys.dtype != torch.int32 or not keys.is_cuda or not keys.is_contiguous():
            raise ValueError("keys must be a contiguous int32 device tensor")
        self._keys = keys

    def buffer(self, B: int) -> torch.Tensor:
        eng = self.eng
        need = eng.H * B * eng.F * eng.F
        if self._att is None or self._att.numel() < need:
            self._att = torch.empty(need, dtype=torch.float32, device=eng.dev)
        return self._att[:need].view(eng.H, B, eng.F, eng.F)

    def accumulate(self, l: int, att: torch.Tensor, B: int, stream) -> None:
        eng, lib = self.eng, self.eng.lib
        if self._keys is None or self._keys.shape[0] != B:
            raise ValueError(f"attention statistics: keys for {B} samples expected")
        need = int(lib.satrans_attn_stats_workspace_bytes(B, eng.H, eng.F, self.K))
        N.check(0 if need >= 0 else need, "satrans_attn_stats_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=eng.dev)
        N.check(lib.satrans_attn_stats_accumulate(att.data_ptr(), self._keys.data_ptr(), B, eng.H, eng.F, self.K,
                                                  self.acc[l].data_ptr(), self._ws.data_ptr(), self._ws.numel(), stream),
                "satrans_attn_stats_accumulate")

    def raw_sum(self) -> np.ndarray:
        """fp64 [L, 3 S, H, F, F] on the host (synchronises)."""
        return self.acc.cpu().numpy()

