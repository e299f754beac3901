"""The tile map of the statistics pass's list kernel (lck::ftl_feature in csrc/lc_kernels.h), evaluated on the
host through lcx_test_suffstat_list_deal (bound here): which two staged columns lane (lo2, blk) of tile t of wave v
multiplies, and -- in the shared deal of DC = 64 -- which of the wave's two shared fragments a paired tile uses.  The kernel
builds its LDS addresses and its epilogue from this one map, so what holds here holds for both.  No GPU."""
from __future__ import annotations

import ctypes as C
import functools
from collections import Counter

import numpy as np
import pytest

import aux_hooks as ah

PRODUCT, LINEAR, COUNT, SPARE = 0, 1, 2, 3  # FtKind
WIDTHS = [(64, 64), (64, 56)]  # the list kernel's instances
CONVERTED = [(64, 64)]         # the widths of the shared deal (56 keeps the consecutive deal)


@functools.lru_cache(maxsize=None)
def deal(DP, DC):
    """-> info (shared, waves, tiles per wave, paired, split, ones-column), feat [waves][tiles][16][u, w, kind, shared]"""
    fn = getattr(ah.hooks(), "lcx_test_suffstat_list_deal")
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
    fn.restype = C.c_int
    info = np.full(6, -7, dtype=np.int64)
    feat = np.full(8 * 32 * 16 * 4, -7, dtype=np.int32)
    assert fn(DP, DC, info.ctypes.data, feat.ctypes.data, feat.size) == 0
    shared, waves, tiles, paired, split, one = (int(v) for v in info)
    assert waves == 8 and 0 < tiles <= 32
    used = waves * tiles * 16 * 4
    assert np.all(feat[used:] == -7)
    feat = feat[:used].reshape(waves, tiles, 16, 4)
    feat.setflags(write=False)
    return dict(shared=shared, waves=waves, tiles=tiles, paired=paired, split=split, one=one), feat


def test_the_hook_refuses_widths_without_an_instance():
    fn = getattr(ah.hooks(), "lcx_test_suffstat_list_deal")
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
    fn.restype = C.c_int
    info = np.full(6, -7, dtype=np.int64)
    feat = np.full(8 * 32 * 16 * 4, -7, dtype=np.int32)
    for DP, DC in ((32, 32), (96, 96), (128, 128), (64, 60)):
        assert fn(DP, DC, info.ctypes.data, feat.ctypes.data, feat.size) == -1
    assert fn(64, 64, info.ctypes.data, feat.ctypes.data, 16) == -1  # too short a buffer
    assert np.all(info == -7) and np.all(feat == -7)


@pytest.mark.parametrize("DP,DC", CONVERTED)
def test_converted_widths_run_the_shared_deal(DP, DC):
    info, _ = deal(DP, DC)
    assert info["shared"] == 1 and info["paired"] == DC // 4 - 1 and info["split"] == DC // 8
    assert info["tiles"] == info["paired"] + 2 and info["one"] == DP


@pytest.mark.parametrize("DP,DC", WIDTHS)
def test_every_feature_exactly_once(DP, DC):
    """Over waves 0-7 x tiles x 16 lanes: every product (u <= w) below the active width once, every linear feature once, the
    count once, everything else spare; no column at or beyond the active width is named but the ones-column."""
    info, feat = deal(DP, DC)
    one = info["one"]
    u, w, kind = (feat[..., i].ravel() for i in range(3))
    assert set(np.unique(kind)) <= {PRODUCT, LINEAR, COUNT, SPARE}
    assert np.all(((u < DC) & (u >= 0)) | (u == one)) and np.all(((w < DC) & (w >= 0)) | (w == one))
    p = kind == PRODUCT
    assert np.all(u[p] < DC) and np.all(w[p] < DC)
    pairs = Counter(zip(np.minimum(u[p], w[p]).tolist(), np.maximum(u[p], w[p]).tolist()))
    assert pairs == Counter({(i, j): 1 for i in range(DC) for j in range(i, DC)})
    lin = kind == LINEAR
    assert np.all(w[lin] == one) and sorted(u[lin].tolist()) == list(range(DC))
    cnt = kind == COUNT
    assert cnt.sum() == 1 and u[cnt][0] == one and w[cnt][0] == one
    sp = kind == SPARE
    assert np.all(u[sp] == one) and np.all(w[sp] == one)  # (an idle lane multiplies 1 * 1; it is not stored)
    assert p.sum() + lin.sum() + 1 + sp.sum() == kind.size


@pytest.mark.parametrize("DP,DC", WIDTHS)
def test_tiles_per_simd_are_those_of_the_consecutive_deal(DP, DC):
    """waves w and w + 4 share a matrix pipe: the tiles that hold a feature, per SIMD, are ft_deal_one's (D = 64: 34 34 34 33)"""
    info, feat = deal(DP, DC)
    nb = DC // 4
    features = 16 * (nb * (nb - 1) // 2) + 10 * nb + DC + 1
    tiles = -(-features // 16)
    live = (feat[..., 2] != SPARE).any(axis=2)  # [wave][tile]
    assert live.sum() == tiles
    per_simd = [int(live[s].sum() + live[s + 4].sum()) for s in range(4)]
    assert per_simd == [tiles // 4 + (1 if s < tiles % 4 else 0) for s in range(4)]
    assert info["tiles"] == (max(per_simd) + 1) // 2  # one batch body: nobody carries more than the fuller waves did
    if (DP, DC) == (64, 64):
        assert per_simd == [34, 34, 34, 33] and info["tiles"] == 17


@pytest.mark.parametrize("DP,DC", CONVERTED)
def test_paired_tiles_name_the_waves_shared_block(DP, DC):
    """In a paired tile all 16 lanes name the wave's shared block in the shared position (column 4 a + blk, w), tiles below the
    split the first block (a = wave), the others the second (a = wave + DC / 8); the tile's own block sits in the lo2
    position (u) and is one block for the whole tile.  The tiles behind the paired ones share nothing."""
    info, feat = deal(DP, DC)
    S, P = info["split"], info["paired"]
    lo2, blk = np.arange(16) & 3, np.arange(16) >> 2
    seen = set()
    for v in range(info["waves"]):
        for t in range(info["tiles"]):
            u, w, kind, sh = (feat[v, t, :, i] for i in range(4))
            if t >= P:
                assert np.all(sh == -1), (v, t)
                continue
            which = 0 if t < S else 1
            a = v + which * (DC // 8)
            assert np.all(sh == which) and np.all(kind == PRODUCT), (v, t)
            assert np.array_equal(w, 4 * a + blk), (v, t)
            o = int(u[0]) // 4
            assert np.array_equal(u, 4 * o + lo2) and o != a, (v, t)
            seen.add((min(a, o), max(a, o)))
    nb = DC // 4
    assert seen == {(i, j) for i in range(nb) for j in range(i + 1, nb)}  # every off-diagonal patch is a paired tile


@pytest.mark.parametrize("DP,DC", [w for w in WIDTHS if w not in CONVERTED])
def test_other_widths_share_nothing(DP, DC):
    info, feat = deal(DP, DC)
    assert info["shared"] == 0 and info["paired"] == 0 and info["split"] == 0 and np.all(feat[..., 3] == -1)
