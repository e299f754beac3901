"""What the launcher-level tests of the ranking and threshold kernels share (tests/test_gpu_rank_select_kernels.py; held to
the sources without a device by tests/test_sample_exact_refs_host.py): the constants the cases straddle, padded layouts with
row groups of any fill, column builders, and the numpy reference of the ranking (the references of the threshold queries
are tests/score_select_ref.py).  No GPU; only top_rows_ref touches the package, for the TopRows tuple of its binding."""
import numpy as np

import score_select_ref as ssr

RG = 16
# (lc_kernels.h, lc_kernels_rank.hip, lc_kernels_select.hip: compared with the sources' text by the host test)
TOP_CHUNK_ROWS, TOP_MAX_M = 8192, 64
SEL_MAX, SEL_GRID_BLOCKS, SEL_STATE_WORDS, SEL_HIST_WORDS = 16, 2048, 58, 16 * 256
TR_MERGE_WAVES, SCAN_THREADS = 16, 1024
MERGE_TRIP = TR_MERGE_WAVES * 64 * 4  # partial-list entries one trip of the merge kernel's loop takes
STATE_NACT_INT = (3 * 8 * SEL_MAX + 4 * SEL_MAX) // 4  # SelectState: pref, rem, rank (8 bytes each), slot (4), then nact


def top_rows_ref(cols, sizes, m, largest, labels=None):
    """cols: (N, C) scores of the rows of all groups in order; -> TopRows of numpy"""
    from libcluster_amd import capi

    N, Cn = cols.shape
    grp = np.repeat(np.arange(len(sizes)), sizes)
    row = np.concatenate([np.arange(n) for n in sizes]) if N else np.zeros(0, dtype=np.int64)
    count = np.zeros(Cn, dtype=np.int32)
    group, rows = np.full((Cn, m), -1, dtype=np.int32), np.full((Cn, m), -1, dtype=np.int64)
    score = np.full((Cn, m), np.nan)
    for c in range(Cn):
        s = cols[:, c]
        ok = ~np.isnan(s)
        if labels is not None:
            ok &= labels == c
        idx = np.flatnonzero(ok)
        key = -s[idx] if largest else s[idx]  # (-0.0 and +0.0 compare equal in the sort: the position decides)
        best = idx[np.lexsort((idx, key))[:m]]
        n = best.size
        count[c], group[c, :n], rows[c, :n], score[c, :n] = n, grp[best], row[best], s[best]
    return capi.TopRows(count, group, rows, score)


class Layout:
    """NP padded rows: `fill` = the valid rows of every row group of 16 (any of 0 ... 16, anywhere), or nrows alone (one
    group, the first nrows rows valid, no row-group words)"""

    def __init__(self, NP, nrows=None, fill=None):
        assert NP % RG == 0 and (nrows is None) != (fill is None)
        self.NP = NP
        if fill is None:
            self.rginfo, self.nrows = None, nrows
            self.valid = np.arange(NP) < nrows
        else:
            fill = np.asarray(fill, dtype=np.int32)
            assert fill.size == NP // RG and fill.min() >= 0 and fill.max() <= RG
            self.rginfo, self.nrows = (((np.arange(fill.size) % 5) << 5) | fill).astype(np.int32), 0  # (group ids: any)
            self.valid = (np.arange(NP) % RG) < np.repeat(fill, RG)
        self.pos = np.flatnonzero(self.valid)  # padded position of the i-th valid row

    def rows(self, lo, hi):
        """rows [lo, hi) as a layout of their own (valid and pos only)"""
        sub = Layout.__new__(Layout)
        sub.NP, sub.valid = hi - lo, self.valid[lo:hi]
        sub.pos = np.flatnonzero(sub.valid)
        return sub


def ragged_fill(NP, rng):
    """row groups of every fill, with empty and odd ones in the middle of the column"""
    fill = rng.integers(0, RG + 1, NP // RG)
    fill[: min(6, fill.size)] = [16, 0, 5, 16, 1, 15][: min(6, fill.size)]
    return fill


def top_ref_padded(col, lay, m, largest, label=None):
    """col [C x ld] padded columns -> (pos (C, m), score (C, m)) of numpy: top_rows_ref over the valid rows, positions padded"""
    C = col.shape[0]
    cols = col[:, : lay.NP][:, lay.valid].T
    want = top_rows_ref(cols, [cols.shape[0]], m, largest, None if label is None else label[: lay.NP][lay.valid])
    pos = np.where(want.row >= 0, lay.pos[np.maximum(want.row, 0)] if lay.pos.size else -1, -1)
    assert pos.shape == (C, m)
    return pos.astype(np.int64), want.score


def chunk_lists_ref(col, lay, m, largest, label=None):
    """the partial lists [nchunks x C x m]: each chunk's own best m as (key, position), best first; unused slots: position
    2^63 - 1 (their keys are not compared)"""
    C = col.shape[0]
    nch = (lay.NP + TOP_CHUNK_ROWS - 1) // TOP_CHUNK_ROWS
    key, pos = np.zeros((nch, C, m)), np.full((nch, C, m), np.iinfo(np.int64).max, dtype=np.int64)
    for ch in range(nch):
        lo, hi = ch * TOP_CHUNK_ROWS, min((ch + 1) * TOP_CHUNK_ROWS, lay.NP)
        p, s = top_ref_padded(col[:, lo:hi], lay.rows(lo, hi), m, largest, None if label is None else label[lo:hi])
        has = p >= 0
        pos[ch][has] = p[has] + lo
        key[ch][has] = s[has] if largest else -s[has]
    return key, pos


# ---- columns -----------------------------------------------------------------------------------------------------------------
def adversarial_columns(NP):
    """name -> column [NP] for the ranking: the orders that stress the insertion, and the values at the edges of the order"""
    r = np.arange(NP, dtype=np.float64)
    nan = np.where(np.arange(NP) % 3 == 0, np.nan, r)
    nan[-5:] = np.nan  # (the rows that would win `largest`)
    nan[:5] = np.nan
    return {
        "rising": r * 0.5 - 100.0, "falling": 100.0 - r * 0.5, "constant": np.full(NP, -2.5),
        "alternating": np.where(np.arange(NP) % 2 == 0, 1.0, -1.0) * (r + 1.0),
        "neg_inf": np.full(NP, -np.inf), "pos_inf": np.full(NP, np.inf),
        "zeros": np.where((np.arange(NP) * 7 // 3) % 2 == 0, 0.0, -0.0), "nan": nan,
    }


def from_keys(key):
    """the doubles whose monotone keys (score_select_ref.key_map) are `key`"""
    key = np.asarray(key, dtype=np.uint64)
    pos = (key >> np.uint64(63)).astype(bool)
    x = np.where(pos, key ^ np.uint64(1 << 63), ~key).view(np.float64)
    assert not np.isnan(x).any() and np.array_equal(ssr.key_map(x), key)
    return x


PASS_GROUP_BYTES = {0: [0x40 + g for g in range(8)] + [0xB8 + g for g in range(8)]}  # pass 0: both signs


def pass_family(p, n, rng):
    """n values (n a multiple of 16) in sixteen equal groups whose keys agree above byte p (0 = most significant), differ in
    byte p and are random below it, shuffled; with PASS_PROBS one requested rank lands in every group, so the radix select
    follows one prefix up to pass p and sixteen from then on"""
    assert n % 16 == 0 and 0 <= p <= 7
    gb = np.array(PASS_GROUP_BYTES.get(p, [3 + 16 * g for g in range(16)]), dtype=np.uint64)
    prefix = [0xBF, 0xE5, 0x17, 0x80, 0x00, 0xFF, 0x5A][:p]  # bytes 0 .. p - 1 (byte 0: a positive value of ordinary size)
    key = np.zeros(n, dtype=np.uint64)
    for b, v in enumerate(prefix):
        key |= np.uint64(v) << np.uint64(56 - 8 * b)
    key |= np.repeat(gb, n // 16) << np.uint64(56 - 8 * p)
    if p < 7:
        key |= rng.integers(0, 1 << (56 - 8 * p), n, dtype=np.uint64)
    return from_keys(rng.permutation(key))


PASS_PROBS = [(g + 0.5) / 16 for g in range(16)]


def interleaved_runs(NP, rng):
    """-> (column, label, fill): runs of 64 equal values in which NaN rows, pad rows and rows of another label are interleaved,
    so a wave instruction of the histogram kernel sees one bin and lanes that take no part"""
    col = (np.arange(NP) // 64 % 7 - 3.0).astype(np.float64)
    label = np.full(NP, 5, dtype=np.int32)
    col[rng.random(NP) < 0.2] = np.nan
    label[rng.random(NP) < 0.2] = 6
    label[rng.random(NP) < 0.05] = -1
    fill = np.where(rng.random(NP // RG) < 0.3, rng.integers(0, RG, NP // RG), RG)
    return col, label, fill


def quantiles_fast(cols, probs):
    """score_select_ref.quantiles for many NaN-free columns at once (cols (N, C)): one sort of the keys"""
    N, C = cols.shape
    order = np.sort(ssr.key_map(cols.T.copy()).reshape(C, N), axis=1)
    rank = np.array([ssr.rank_rule(p, N) for p in probs], dtype=np.int64)
    return np.full(C, N, dtype=np.int64), np.broadcast_to(rank, (C, len(probs))), from_keys(order[:, rank].copy())
