"""The map of the statistics pass's owner kernel (lck::fto_feature in csrc/lc_kernels.h), evaluated on the host
through lcx_test_suffstat_owner_deal (bound here): which feature lane w of accumulator t holds.  The kernel's epilogue stores
by this one map, and its loop multiplies x_w by the doubled row's entry w + t, which is column (w + t) mod 64.  No GPU."""
from __future__ import annotations

import ctypes as C
import functools
from collections import Counter

import numpy as np

import aux_hooks as ah

PRODUCT, LINEAR, COUNT, SPARE = 0, 1, 2, 3  # FtKind
D, ONE = 64, 64


def hook():
    fn = getattr(ah.hooks(), "lcx_test_suffstat_owner_deal")
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong]
    fn.restype = C.c_int
    return fn


@functools.lru_cache(maxsize=None)
def deal():
    """-> diagonals, accumulators, feat [accumulators][64 lanes][u, w, kind]"""
    info = np.full(3, -7, dtype=np.int64)
    feat = np.full(40 * 64 * 3, -7, dtype=np.int32)
    assert hook()(info.ctypes.data, feat.ctypes.data, feat.size) == 0
    nd, na = int(info[0]), int(info[1])
    assert (nd, na) == (33, 35) and info[2] in (0, 1)
    assert np.all(feat[na * 64 * 3:] == -7)
    feat = feat[:na * 64 * 3].reshape(na, 64, 3)
    feat.setflags(write=False)
    return nd, na, feat


def test_too_short_a_buffer_is_refused():
    info = np.full(3, -7, dtype=np.int64)
    feat = np.full(64, -7, dtype=np.int32)
    assert hook()(info.ctypes.data, feat.ctypes.data, feat.size) == -1
    assert np.all(info == -7) and np.all(feat == -7)


def test_every_feature_exactly_once():
    """the 2080 products (u <= w), the 64 linear features and the count: each stored from exactly one (accumulator, lane)"""
    nd, na, feat = deal()
    u, w, kind = (feat[..., i].ravel() for i in range(3))
    assert set(np.unique(kind)) == {PRODUCT, LINEAR, COUNT, SPARE}
    p = kind == PRODUCT
    assert np.all((u[p] >= 0) & (u[p] < D) & (w[p] >= 0) & (w[p] < D))
    pairs = Counter(zip(np.minimum(u[p], w[p]).tolist(), np.maximum(u[p], w[p]).tolist()))
    assert len(pairs) == D * (D + 1) // 2 == 2080
    assert pairs == Counter({(i, j): 1 for i in range(D) for j in range(i, D)})
    lin = kind == LINEAR
    assert sorted(u[lin].tolist()) == list(range(D)) and np.all(w[lin] == ONE)
    cnt = kind == COUNT
    assert cnt.sum() == 1 and u[cnt][0] == ONE and w[cnt][0] == ONE


def test_lane_w_owns_column_w_and_the_rotation_is_the_accumulator():
    """what the loop relies on: in accumulator t < 33 lane w multiplies its own column by column (w + t) mod 64 -- the entry
    w + t of the row stored twice; accumulator 33 is the lane's linear feature, 34 the count in lane 0"""
    nd, na, feat = deal()
    lanes = np.arange(64)
    for t in range(nd):
        assert np.array_equal(feat[t, :, 0], lanes) and np.array_equal(feat[t, :, 1], (lanes + t) % 64), t
    assert np.array_equal(feat[nd, :, 0], lanes) and np.all(feat[nd, :, 2] == LINEAR)
    assert feat[nd + 1, 0, 2] == COUNT and np.all(feat[nd + 1, 1:, 2] == SPARE)


def test_the_spare_products_are_the_upper_half_of_the_last_diagonal():
    """t = 32: lanes w and w + 32 hold the same pair; the upper lane is spare, and nothing else among the diagonals is"""
    nd, na, feat = deal()
    spare = feat[:nd, :, 2] == SPARE
    want = np.zeros((nd, 64), dtype=bool)
    want[32, 32:] = True
    assert np.array_equal(spare, want)
    for w in range(32):
        a, b = feat[32, w], feat[32, w + 32]
        assert {int(a[0]), int(a[1])} == {int(b[0]), int(b[1])} == {w, w + 32}
    # with the spares counted as products, those 32 pairs are the only ones that appear twice
    u, w_ = feat[:nd, :, 0].ravel(), feat[:nd, :, 1].ravel()
    pairs = Counter(zip(np.minimum(u, w_).tolist(), np.maximum(u, w_).tolist()))
    assert {p for p, n in pairs.items() if n > 1} == {(i, i + 32) for i in range(32)} and max(pairs.values()) == 2
