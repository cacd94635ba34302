"""Numpy brute force of the instance-level attention search (satrans_amd/attn_inst.py, csrc/attn_inst.hip)  --  TEST
INFRASTRUCTURE, NOT PRODUCT CODE.

A rule is a list of clauses, a clause a list of atoms (q, k, thr); the rule holds on a map when every clause has an atom with
map[q, k] > float32(thr) (strict, fp32, false for a NaN).  The records come out ordered by sample, then head, then rule.
"""
import numpy as np

MATCH_DTYPE = np.dtype([("index", "<i8"), ("head", "<i4"), ("rule", "<i4")])


def rule_holds(att, rule):
    """att float32 [H, B, F, F] -> bool [H, B]."""
    att = np.asarray(att)
    assert att.dtype == np.float32
    ok = np.ones(att.shape[:2], dtype=bool)
    for clause in rule:
        some = np.zeros(att.shape[:2], dtype=bool)
        for q, k, thr in clause:
            with np.errstate(invalid="ignore"):
                some |= att[:, :, q, k] > np.float32(thr)
        ok &= some
    return ok


def brute_force(att, rules, eligible=None, first_index=0):
    """-> MATCH_DTYPE [total] records.  eligible: uint8 [B] rule bits (bit r: rule r may match the sample) or None."""
    H, B = att.shape[:2]
    hit = np.stack([rule_holds(att, r) for r in rules])                   # [R, H, B]
    if eligible is not None:
        e = np.asarray(eligible, dtype=np.uint8)
        allowed = np.stack([(e >> r) & 1 for r in range(len(rules))]).astype(bool)      # [R, B]
        hit &= allowed[:, None, :]
    b, h, r = np.nonzero(hit.transpose(2, 1, 0))                          # lexicographic: sample, head, rule
    rec = np.zeros(b.shape[0], dtype=MATCH_DTYPE)
    rec["index"], rec["head"], rec["rule"] = b + first_index, h, r
    return rec


def clauses_of(rule):
    """AttentionRule-like object or plain list -> plain [[(q, k, thr), ...], ...] with integer fields."""
    return [[(int(q), int(k), float(t)) for q, k, t in c] for c in getattr(rule, "clauses", rule)]
