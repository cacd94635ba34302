"""Host side of the scenario attention maps (satrans_amd/attn_stats.py): keys, bias, counts and the NaN rule against the numpy
transcription of the reference's `showattn` loop, and argument validation of the new C entry points without a device."""
import ctypes

import numpy as np
import pytest

from satrans_amd import attn_stats as AS
from satrans_amd import native
from tests.attn_stats_reference import reference_showattn


def _device_like_reduction(atts, keys, S):
    """What the device accumulator holds: per key row the fp64 sum of the samples' maps, [L, 3 S, H, F, F]."""
    L, H, _, F, _ = atts.shape
    raw = np.zeros((L, 3 * S, H, F, F))
    for k in range(3 * S):
        sel = keys == k
        raw[:, k] = atts[:, :, sel].astype(np.float64).sum(2)
    return raw


@pytest.mark.parametrize("bias_ids", [0, 1])
def test_keys_counts_and_means_match_the_reference_loop(bias_ids):
    rng = np.random.default_rng(7 + bias_ids)
    n, S, L, H, F = 700, 4, 2, 3, 5
    ids = rng.integers(bias_ids, S + bias_ids, n).astype(np.float32)
    ids[:13] = S + bias_ids + 1                      # out of range: count nowhere
    ids[13:17] = -1 if bias_ids == 0 else 2.5        # (a -1 would make the smallest id -1: bias 0)
    y = rng.integers(0, 2, n).astype(np.float64)
    y[20:30] = 0.5                                   # neither 0 nor 1: `all` only
    y[(ids == 2 + bias_ids)] = 0                     # one scenario without positives -> NaN there
    atts = rng.random((L, H, n, F, F)).astype(np.float32)
    bias = AS.scenario_bias(ids)
    assert bias == bias_ids
    keys = AS.class_keys(ids, y, S, bias)
    assert keys.dtype == np.int32 and keys.min() >= -1 and keys.max() < 3 * S
    assert (keys[:17] == -1).all()
    st = AS.finish(_device_like_reduction(atts, keys, S), keys, S, bias)
    assert st["bias"] == bias and st["count"].dtype == np.int64
    batches = [[atts[l][:, lo:lo + 128] for l in range(L)] for lo in range(0, n, 128)]
    pos, neg, al = reference_showattn(batches, y, ids, S, L)
    for l in range(L):
        for j in range(S):
            for c, ref in enumerate((pos, neg, al)):
                np.testing.assert_allclose(st["mean"][l, j, c], ref[l][j], rtol=1e-12, atol=0, equal_nan=True)
    assert np.isnan(st["mean"][:, 2, 0]).all() and st["count"][2, 0] == 0
    assert not np.isnan(st["mean"][:, :, 2]).any()
    want = np.array([[((ids == j + bias) & (y == 1)).sum(), ((ids == j + bias) & (y == 0)).sum(), (ids == j + bias).sum()]
                     for j in range(S)])
    assert np.array_equal(st["count"], want)


def test_keys_ignore_non_integer_ids_and_check_lengths():
    keys = AS.class_keys(np.array([0.0, 0.5, 1.0, 2.0]), np.array([1, 0, 0.25, 1]), 2, 0)
    assert keys.tolist() == [0, -1, 5, -1]
    with pytest.raises(ValueError):
        AS.class_keys(np.zeros(3), np.zeros(4), 2, 0)


def test_entry_points_validate_arguments_without_a_device():
    lib = native.lib()
    assert native.ABI_VERSION == 7 and lib.satrans_abi_version() == 7
    assert lib.satrans_attn_stats_workspace_bytes(0, 4, 19, 9) == -1
    assert lib.satrans_attn_stats_workspace_bytes(32768, 4, 19, -1) == -1
    assert lib.satrans_attn_stats_workspace_bytes(32768, 4, 19, 10) == -1      # K = 3 S
    assert lib.satrans_attn_stats_workspace_bytes(32768, 4, 19, 9) >= 32768 // 128 * 4 * 19 * 19 * 8
    assert lib.satrans_attn_stats_accumulate(None, None, 16, 2, 5, 3, None, None, 0, None) == -1
    assert b"null pointer" in lib.satrans_last_error()
    p = ctypes.c_void_p(16)                          # never dereferenced: the call returns before any launch
    assert lib.satrans_attn_stats_accumulate(p, p, 0, 2, 5, 3, p, p, 1 << 20, None) == -1
    assert b"bad sizes" in lib.satrans_last_error()
    assert lib.satrans_attn_stats_accumulate(p, p, 16, 2, 5, 4, p, p, 1 << 20, None) == -1
    assert lib.satrans_attn_stats_accumulate(p, p, 16, 2, 5, 3, p, p, 8, None) == -4
    assert b"workspace" in lib.satrans_last_error()
