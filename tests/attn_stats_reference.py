"""Test aid: the reference's `showattn` branch (models/meta_basemodel.py:421-426, 439-458, 506-514) transcribed in numpy fp64."""
import numpy as np


def reference_showattn(att_batches, y, domain_ids, S: int, L: int):
    """The reference's loop over per-batch attention [L][H, b, F, F] (batches in order),
    -> (attn_list_pos, attn_list_neg, attn_list_all) as [L][S] arrays, NaN for an empty pair instead of the reference's crash."""
    y = np.asarray(y).reshape(-1)
    domain_ids = np.asarray(domain_ids).reshape(-1)
    bias = 1 if domain_ids.min() == 1 else 0
    H, F = att_batches[0][0].shape[0], att_batches[0][0].shape[2]
    pos = [[np.zeros((H, F, F)) for _ in range(S)] for _ in range(L)]
    neg = [[np.zeros((H, F, F)) for _ in range(S)] for _ in range(L)]
    al = [[np.zeros((H, F, F)) for _ in range(S)] for _ in range(L)]
    offset = 0
    for atts in att_batches:
        n = atts[0].shape[1]
        yl, db = y[offset:offset + n], domain_ids[offset:offset + n]
        offset += n
        for i in range(L):
            a = np.asarray(atts[i], dtype=np.float64)
            for j in range(S):
                pos[i][j] += a[:, (yl == 1) & (db == j + bias)].sum(1)
                neg[i][j] += a[:, (yl == 0) & (db == j + bias)].sum(1)
                al[i][j] += a[:, db == j + bias].sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(L):
            for j in range(S):
                pos[i][j] = pos[i][j] / ((domain_ids == j + bias) & (y == 1)).sum()
                neg[i][j] = neg[i][j] / ((domain_ids == j + bias) & (y == 0)).sum()
                al[i][j] = al[i][j] / (domain_ids == j + bias).sum()
    return pos, neg, al
