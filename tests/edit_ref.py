"""The rule of the edit-distance scores (include/nmhip_edit.h) as a plain integer DP over whole batches."""
import numpy as np

END = 2


def ends(cols):
    """[N]: the first index of every column [T, N] that holds END, or T."""
    hit = cols == END
    return np.where(hit.any(0), hit.argmax(0), cols.shape[0])


def distances(refs, hyps):
    """(d, lr, lh), each [N]: the table D[i][j] of every pair of columns refs [T_ref, N], hyps [T_hyp, N] over the WHOLE
    columns, one anti-diagonal i + j = k at a time from the two before it (d1[i] = D[i][k - 1 - i], d2[i] =
    D[i][k - 2 - i]), and D[lr][lh] read off on the way: the distance of two prefixes does not depend on what follows."""
    (tr, n), th = refs.shape, hyps.shape[0]
    lr, lh = ends(refs), ends(hyps)
    out = np.where(lr + lh <= 1, lr + lh, -1)
    d2, d1 = np.zeros((tr + 1, n), np.int64), np.ones((tr + 1, n), np.int64)
    for k in range(2, tr + th + 1):
        new = np.full((tr + 1, n), k, np.int64)                 # D[0][k] = D[k][0] = k
        i = np.arange(max(1, k - th), min(tr, k - 1) + 1)
        new[i] = np.minimum(np.minimum(d1[i - 1], d1[i]) + 1, d2[i - 1] + (refs[i - 1] != hyps[k - i - 1]))
        hit = np.flatnonzero(lr + lh == k)
        out[hit] = new[lr[hit], hit]
        d2, d1 = d1, new
    return out.astype(np.int32), lr, lh


def score(kind, d, lr, lh):
    """float32 [N] from the integers, in double, rounded once."""
    if kind == "accuracy":
        longer = np.maximum(lr, lh)
        return np.where(longer == 0, 1.0, 1.0 - d / np.maximum(longer, 1)).astype(np.float32)
    return (-d.astype(np.int64) / np.maximum(lr, 1)).astype(np.float32)
