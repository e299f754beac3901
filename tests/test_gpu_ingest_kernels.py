"""The kernels of lc_kernels_ingest.hip launcher by launcher, through the hooks of tests/ingest_hooks.py:
launch_pack_rows builds the padded image from strided device sources and leaves the minimum and the NaN count,
launch_unpack_qz copies rows of the column-major qZ into a strided destination.  Everything is compared with numpy bit for bit;
destinations are pre-filled (NaN / a sentinel) with guards on both sides, so a byte the kernel owes and a byte it must not
touch both show."""
from __future__ import annotations

import numpy as np
import pytest

import ingest_hooks as ih

pytestmark = pytest.mark.gpu

ROW_COUNTS = (1, 63, 64, 65, 129)
# one group of every row count, and four ragged groups with an empty one between two others (the second set has more rows
# than one block of either pack kernel takes, and blocks that straddle groups)
GROUP_SETS = tuple((n,) for n in ROW_COUNTS) + ((65, 0, 1, 129), (63, 300, 0, 64))
DIMS = (1, 4, 7, 16, 17, 23, 64, 65, 130)  # both sides of every step of the padded width and of a 64-wide tile
LAYOUTS = ("row", "rowpad", "col", "both")
POISON = -1e300  # what the source buffers hold outside the views: a kernel that reads there spoils the minimum


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def image_ref(views, D):
    """the padded image as Context::set_data builds it on the host: groups padded to 16 rows, rows to the padded width"""
    DP, blocks = ih.padded_dim(D), []
    for v in views:
        blk = np.zeros(((v.shape[0] + ih.RG - 1) // ih.RG * ih.RG, DP))
        blk[:v.shape[0], :D] = v
        blocks.append(blk)
    return np.vstack(blocks)


def lay_out(views, D, layout):
    """-> (flat source buffers, row stride, column stride) holding the views in the layout (one pair of strides for all
    groups, as lc_ctx_set_data_device takes them)"""
    nmax = max(max(v.shape[0] for v in views), 1)
    bufs = []
    if layout == "row":
        return [np.ascontiguousarray(v).reshape(-1) for v in views], D, 1
    if layout == "rowpad":  # a column slice of a wider array
        W = D + 5
        for v in views:
            b = np.full((v.shape[0], W), POISON)
            b[:, :D] = v
            bufs.append(b.reshape(-1))
        return bufs, W, 1
    if layout == "col":  # column-major with a common leading dimension
        ld = nmax + 3
        for v in views:
            b = np.full((D, ld), POISON)
            b[:, :v.shape[0]] = v.T
            bufs.append(b.reshape(-1) if v.shape[0] else np.zeros(0))
        return bufs, 1, ld
    for v in views:  # "both": every second row and every third column of a larger array
        b = np.full((2 * v.shape[0], 3 * D), POISON)
        b[::2, ::3] = v
        bufs.append(b.reshape(-1))
    return bufs, 6 * D, 3


def make_views(Nj, D, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, D)) for n in Nj]


def run_pack(views, D, layout):
    bufs, rs, cs = lay_out(views, D, layout)
    rc, img, guards, lo, nn, raw = ih.pack_rows(bufs, [v.shape[0] for v in views], D, rs, cs)
    assert rc == 0
    assert np.isnan(guards[0]).all() and np.isnan(guards[1]).all()  # nothing outside the image was written
    return img, lo, nn, raw


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("D", DIMS)
def test_pack_builds_the_padded_image_bit_for_bit(D, layout):
    for g, Nj in enumerate(GROUP_SETS):
        views = make_views(Nj, D, 100 * D + g)
        img, lo, nn, _ = run_pack(views, D, layout)
        ref = image_ref(views, D)
        assert img.shape == ref.shape
        # (bits: every pad row and pad column is +0.0, no NaN of the pre-filled destination is left)
        assert np.array_equal(bits(img), bits(ref)), (Nj, D, layout)
        allv = np.concatenate([v.reshape(-1) for v in views])
        assert lo == allv.min() and nn == 0, (Nj, D, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("D", (1, 7, 23, 64, 65))
def test_pack_minimum_and_nan_count(D, layout):
    Nj = (65, 0, 33, 129)
    # NaNs in the last valid column and in the last valid row (of the last group and of one in the middle)
    views = make_views(Nj, D, 7 + D)
    views[3][::5, D - 1] = np.nan
    views[3][-1, :] = np.nan
    views[0][-1, ::2] = np.nan
    img, lo, nn, raw = run_pack(views, D, layout)
    allv = np.concatenate([v.reshape(-1) for v in views])
    assert nn == int(np.isnan(allv).sum()) and nn > 0
    assert lo == np.nanmin(allv)
    assert np.array_equal(bits(img), bits(image_ref(views, D)))  # (the NaNs arrive as they are)
    # two runs: the same bits, image and range words
    img2, lo2, nn2, raw2 = run_pack(views, D, layout)
    assert np.array_equal(bits(img), bits(img2)) and np.array_equal(raw, raw2) and (lo2, nn2) == (lo, nn)
    # a single negative entry, in the last valid element
    views = [np.abs(v) + 0.5 for v in make_views(Nj, D, 11 + D)]
    _, lo, nn, _ = run_pack(views, D, layout)
    assert lo == min(v.min() for v in views if v.size) and lo > 0 and nn == 0
    views[3][-1, D - 1] = -2.5
    _, lo, nn, _ = run_pack(views, D, layout)
    assert lo == -2.5 and nn == 0


def test_pack_range_of_zeros_and_of_nothing():
    D = 5
    # -0.0 orders below +0.0 (the key is a total order: the result does not depend on which block came first)
    v = np.zeros((70, D))
    v[69, 4] = -0.0
    v[3, 1] = 1.0
    _, lo, nn, _ = run_pack([v], D, "row")
    assert lo == 0.0 and np.signbit(lo) and nn == 0
    # nothing but NaN, and nothing at all: +inf
    _, lo, nn, _ = run_pack([np.full((17, D), np.nan)], D, "col")
    assert lo == np.inf and nn == 17 * D
    rc, img, _, lo, nn, _ = ih.pack_rows([np.zeros(0), np.zeros(0)], [0, 0], D, D, 1)
    assert rc == 0 and img.size == 0 and lo == np.inf and nn == 0


def test_pack_hook_refuses_what_a_kernel_could_not_address():
    v = np.ones((8, 3))
    assert ih.pack_rows([v.reshape(-1)], [8], 3, 0, 1)[0] == -1      # a stride that is not positive
    assert ih.pack_rows([v.reshape(-1)], [9], 3, 3, 1)[0] == -1      # more rows than the buffer holds
    assert ih.pack_rows([v.reshape(-1)], [8], 3, 3, 2)[0] == -1      # a column stride that leaves the buffer


@pytest.mark.parametrize("dest", ("row", "col", "rowpad"))
@pytest.mark.parametrize("K", (1, 5, 33))
def test_unpack_copies_the_rows_and_nothing_else(K, dest):
    rng = np.random.default_rng(K)
    for n in ROW_COUNTS + (300,):
        off = 19  # (row0 > 0 inside a group that does not start the buffer)
        ldq = off + n + 13
        col = rng.standard_normal((K, ldq))
        rs, cs = {"row": (K, 1), "col": (1, n), "rowpad": (K + 3, 1)}[dest]
        q_elems = (n - 1) * rs + (K - 1) * cs + 1 + 4
        rc, q, guards = ih.unpack_qz(col, off, n, q_elems, rs, cs)
        assert rc == 0
        ref = np.full(q_elems, -7.0)
        r, k = np.meshgrid(np.arange(n), np.arange(K), indexing="ij")
        ref[r * rs + k * cs] = col[:, off:off + n].T
        assert np.array_equal(bits(q), bits(ref)), (K, dest, n)  # the values, and every other entry as it was
        assert (guards[0] == -7.0).all() and (guards[1] == -7.0).all()


def test_unpack_hook_refuses_what_a_kernel_could_not_address():
    col = np.ones((3, 40))
    assert ih.unpack_qz(col, 30, 11, 64, 3, 1)[0] == -1   # rows past the column's end
    assert ih.unpack_qz(col, 0, 10, 29, 3, 1)[0] == -1    # a destination that is too short
    assert ih.unpack_qz(col, 0, 10, 64, 3, 0)[0] == -1    # a stride that is not positive
    rc, q, _ = ih.unpack_qz(col, 0, 0, 8, 3, 1)           # no rows: nothing happens
    assert rc == 0 and (q == -7.0).all()
