"""The numpy reference of the order and threshold queries (lc_ctx_score_quantiles, lc_ctx_score_counts,
lc_ctx_rows_beyond), written from the header's contract alone.  No GPU, no library.

The order is the IEEE total order restricted to non-NaN values: -inf < ... < -0.0 < +0.0 < ... < +inf.  key_map gives the
unsigned 64-bit integers that sort in that order; rank_rule is the header's formula for the rank of a probability."""
import numpy as np

QUANTILES_MAX = 16  # LC_QUANTILES_MAX (tests/test_score_select_host.py pins it to the header and to the binding)


def key_map(x):
    """uint64 keys, monotone in the total order: all bits flipped for a negative value (sign bit set), the sign bit
    flipped otherwise"""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    neg = (u >> np.uint64(63)).astype(bool)
    return np.where(neg, ~u, u ^ np.uint64(1 << 63))


def rank_rule(p, n):
    """r = min(n - 1, max(0, ceil(p * n) - 1)); -1 for n = 0"""
    if n == 0:
        return -1
    return int(min(n - 1, max(0, int(np.ceil(np.float64(p) * np.float64(n))) - 1)))


def _participants(col, labels, c):
    ok = ~np.isnan(col)
    if labels is not None:
        ok &= labels == c
    return ok


def quantiles(cols, probs, labels=None):
    """cols: (N, C) scores of the valid rows of all groups in order -> (count (C,), rank (C, P), value (C, P))"""
    N, Cn = cols.shape
    P = len(probs)
    count = np.zeros(Cn, dtype=np.int64)
    rank = np.full((Cn, P), -1, dtype=np.int64)
    value = np.full((Cn, P), np.nan)
    for c in range(Cn):
        s = cols[_participants(cols[:, c], labels, c), c]
        count[c] = s.size
        if s.size == 0:
            continue
        srt = s[np.argsort(key_map(s), kind="stable")]
        for i, p in enumerate(probs):
            rank[c, i] = rank_rule(p, s.size)
            value[c, i] = srt[rank[c, i]]
    return count, rank, value


def counts(cols, thr, labels=None):
    """-> (count (C,), atmost (C, T)): IEEE comparison, so -0.0 <= +0.0 both ways"""
    N, Cn = cols.shape
    count = np.zeros(Cn, dtype=np.int64)
    atmost = np.zeros((Cn, len(thr)), dtype=np.int64)
    for c in range(Cn):
        s = cols[_participants(cols[:, c], labels, c), c]
        count[c] = s.size
        for i, t in enumerate(thr):
            atmost[c, i] = np.sum(s <= t)
    return count, atmost


def beyond(col, sizes, thr, above, labels=None, c=0):
    """col: (N,) scores of one column -> (total, group, row, score) of every participating row beyond thr, in context
    order (np.flatnonzero order)"""
    ok = _participants(col, labels, c)
    with np.errstate(invalid="ignore"):
        ok &= (col >= thr) if above else (col <= thr)
    idx = np.flatnonzero(ok)
    grp = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    row = np.concatenate([np.arange(n) for n in sizes]).astype(np.int64) if len(col) else np.zeros(0, dtype=np.int64)
    return idx.size, grp[idx], row[idx], col[idx]
