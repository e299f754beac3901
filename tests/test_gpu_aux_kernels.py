"""The model-selection data passes and the device math of the normalisation sweeps, kernel by kernel.

Every launcher of libcluster_amd/csrc/lc_kernels_aux.hip (but the generator and the rank-order sum, which have tests of
their own) is handed host arrays through the lc_test_* entry points of libcluster_hip_testhooks.so (tests/aux_hooks.py) and
compared with plain numpy: bit for bit where the kernel only moves or compares values, against an 80-bit reference with a
bar written as a formula next to the assertion where it rounds.  Destination buffers are pre-filled with sentinels, so a
write outside the intended entries shows.  EPS is 2^-52; L is the longest chain of additions of the path taken."""
import math

import numpy as np
import pytest

import aux_hooks as ah
from aux_hooks import QHASH_NONE

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
TINY = float(np.finfo(np.float64).tiny)  # smallest normal double
DENORM = 2.0 ** -1074
SENT = -777.25  # what destination buffers hold before a launch (no kernel here produces it)


def test_the_reference_type_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2 ** -60


def ceil_div(a, b):
    return -(-a // b)


def wide(rng, shape):
    """Terms that span 24 orders of magnitude."""
    return rng.normal(size=shape) * 10.0 ** rng.integers(-12, 12, size=shape)


def cancel_pairs(rng, x, axis):
    """Every odd entry along `axis` becomes minus its even neighbour (up to 1e-13): sums over even-length runs nearly vanish."""
    v = np.moveaxis(x, axis, 0)
    h = v.shape[0] // 2
    v[1:2 * h:2] = -v[0:2 * h:2] * (1.0 + 1e-13 * rng.normal(size=v[0:2 * h:2].shape))
    return x


def steps(a, b):
    """Distance of two arrays of non-negative doubles in units of the last place of their bit patterns."""
    return np.abs(np.ascontiguousarray(a).view(np.int64) - np.ascontiguousarray(b).view(np.int64))


# =====================================================================================================================
# device math: exp_nonpos, rcp_pos
# =====================================================================================================================
def _exp_points():
    rng = np.random.default_rng(11)
    n64 = np.arange(-69100, 0, dtype=np.float64) + 0.5  # x * 64 / ln 2 within an ulp of a half-integer: the rint() edge
    half = n64 * (math.log(2.0) / 64.0)
    parts = [
        -rng.uniform(0.0, 40.0, 400_000), -rng.uniform(0.0, 708.0, 400_000), -rng.uniform(708.0, 750.0, 200_000),
        -np.exp(-rng.uniform(0.0, 740.0, 100_000)),  # towards zero from below
        half, np.nextafter(half, 0.0), np.nextafter(half, -np.inf),
        np.array([0.0, -0.0, -np.inf, -745.2, -750.0, -1e300, -708.3964185322641, -745.1332191019411, -745.1332191019412,
                  -5e-324, -2.0 ** -1022, -math.log(2.0), -math.log(2.0) / 64.0]),
    ]
    return np.concatenate(parts)


def test_exp_nonpos_is_within_one_step_of_the_rounded_exponential():
    """lc_device.hpp claims one unit in the last place for exp_nonpos.  Bar: the result, read as a bit pattern, is at most
    one step from exp() evaluated in 80-bit arithmetic and rounded to double -- normal and subnormal range alike."""
    x = _exp_points()
    assert x.size >= 1_000_000 and np.all(x <= 0)
    rc, got = ah.exp_nonpos(x)
    assert rc == 0
    with np.errstate(under="ignore"):
        ref_ld = np.exp(x.astype(LD))
        ref = ref_ld.astype(np.float64)
    assert np.all(got >= 0.0) and not np.any(np.isnan(got))
    st = steps(got, ref)
    ulp = np.spacing(ref)  # (2^-1074 in the subnormal range and at 0)
    err = np.abs(got.astype(LD) - ref_ld) / ulp.astype(LD)
    normal = ref >= TINY
    w, ws = int(np.argmax(np.where(normal, err, 0))), int(np.argmax(np.where(~normal, err, 0)))
    print(f"exp_nonpos: {x.size} points, worst |error| {float(err[w]):.4f} ulp of the true value at x = {x[w]!r} (normal range), "
          f"{float(err[ws]):.4f} units of 2^-1074 at x = {x[ws]!r} (subnormal range); {int((st == 1).sum())} results one step off, "
          f"{int((st > 1).sum())} further")
    bad = np.flatnonzero(st > 1)
    assert bad.size == 0, [(x[i], got[i], ref[i]) for i in bad[:5]]
    rc, edge = ah.exp_nonpos(np.array([0.0, -0.0, -np.inf, -1e300, -750.0]))
    assert rc == 0 and np.array_equal(edge, [1.0, 1.0, 0.0, 0.0, 0.0])


def test_rcp_pos_is_within_one_step_of_the_quotient():
    """lc_device.hpp: "< 1 ulp off the correctly rounded quotient".  Bar: at most one step from numpy's 1.0 / s."""
    rng = np.random.default_rng(12)
    pw = 2.0 ** np.arange(0, 1001)
    s = np.concatenate([rng.uniform(1.0, 72.0, 1_000_000), np.arange(1.0, 73.0), pw,
                        [1e300, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0), 3.0, 71.99999999999999]])
    rc, got = ah.rcp_pos(s)
    assert rc == 0
    ref = 1.0 / s
    st = steps(got, ref)
    err = np.abs(got.astype(LD) - 1 / s.astype(LD)) / np.spacing(ref).astype(LD)
    print(f"rcp_pos: {s.size} points, worst |error| {float(err.max()):.4f} ulp of the true quotient at s = {s[int(np.argmax(err))]!r}; "
          f"{int((st == 1).sum())} results one step off")
    bad = np.flatnonzero(st > 1)
    assert bad.size == 0, [(s[i], got[i], ref[i]) for i in bad[:5]]
    assert np.array_equal(ah.rcp_pos(pw)[1], 1.0 / pw)  # (a power of two has an exact reciprocal)


# =====================================================================================================================
# reductions
# =====================================================================================================================
def reduce_path(nparts, n, tmp):
    """(name, L) of the path launch_reduce_partials takes: L = additions of one accumulator + the folds behind it."""
    if tmp and nparts > 8192 and n <= ah.REDUCE_TMP_ELEMS:
        per = ceil_div(nparts, 64)
        return "two-stage", ceil_div(per, 256) + 8 + 6  # strided sum, 256-tree, then the wave sum of the 64 partials
    if nparts > 512 and n <= 4096:
        return "cols", ceil_div(nparts, 256) + 8
    return "tile", ceil_div(nparts, 64) + 3 + 2 + 4  # four accumulators (+ a tail of three), (s0 + s1) + (s2 + s3), 16-tree


REDUCE_SHAPES = [(1, 1, 0), (15, 17, 0), (16, 16, 0), (67, 100, 0), (512, 4096, 0), (513, 4096, 0), (513, 4097, 0), (8192, 512, 0),
                 (8192, 512, 1), (8193, 1, 0), (8193, 1, 1), (8193, 512, 0), (8193, 512, 1), (8193, 513, 0), (8193, 513, 1),
                 (100_000, 33, 0), (100_000, 33, 1)]
REDUCE_PATHS = {(1, 1, 0): "tile", (512, 4096, 0): "tile", (513, 4096, 0): "cols", (513, 4097, 0): "tile", (8192, 512, 1): "cols",
                (8193, 1, 1): "two-stage", (8193, 512, 1): "two-stage", (8193, 512, 0): "cols", (8193, 513, 1): "cols",
                (100_000, 33, 1): "two-stage", (100_000, 33, 0): "cols"}


@pytest.mark.parametrize("nparts,n,tmp", REDUCE_SHAPES)
@pytest.mark.parametrize("kind", ["wide", "cancelling"])
def test_reduce_partials_on_both_sides_of_every_dispatch_boundary(nparts, n, tmp, kind):
    rng = np.random.default_rng(nparts * 7 + n + tmp)
    x = wide(rng, (nparts, n))
    if kind == "cancelling":
        x = cancel_pairs(rng, x, 0)
    path, L = reduce_path(nparts, n, tmp)
    assert REDUCE_PATHS.get((nparts, n, tmp), path) == path
    rc, got = ah.reduce_partials(x, use_tmp=bool(tmp))
    assert rc == 0
    ref = x.astype(LD).sum(axis=0)
    mag = np.abs(x).astype(LD).sum(axis=0)
    err = np.abs(got.astype(LD) - ref)
    assert np.all(err <= L * EPS * mag), (path, L, float((err / np.maximum(mag, TINY)).max() / EPS))  # |err| <= L eps sum|x_i|
    rc, again = ah.reduce_partials(x, use_tmp=bool(tmp))
    assert rc == 0 and np.array_equal(got, again)  # fixed order: the same bits


@pytest.mark.parametrize("n", [1, 16, 17, 40])
@pytest.mark.parametrize("kind", ["wide", "cancelling"])
def test_reduce_records_sums_each_clusters_list(n, kind):
    lens = [17, 0, 1, 100, 16, 33, 0]
    rng = np.random.default_rng(n)
    nrec = 120
    x = wide(rng, (nrec, n))
    kptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    krec = rng.integers(0, nrec, kptr[-1]).astype(np.int32)  # (repeats allowed: a list names records, in its own order)
    if kind == "cancelling":  # the second half of every list names records that are minus the first half's
        x[60:] = -x[:60]
        for k, ln in enumerate(lens):
            b, h = kptr[k], ln // 2
            krec[b:b + h] = rng.integers(0, 60, h)
            krec[b + h:b + 2 * h] = krec[b:b + h] + 60
    rc, got = ah.reduce_records(x, kptr, krec)
    assert rc == 0
    for k, ln in enumerate(lens):
        rows = krec[kptr[k]:kptr[k + 1]]
        ref = x[rows].astype(LD).sum(axis=0)
        mag = np.abs(x[rows]).astype(LD).sum(axis=0)
        L = ceil_div(ln, 32) + 1 + 1 + 4  # two accumulators per part lane (+ a tail of one), s0 + s1, 16-tree
        assert np.all(np.abs(got[k].astype(LD) - ref) <= L * EPS * mag), (k, ln)
        if ln == 0:
            assert np.array_equal(got[k], np.zeros(n)) and not np.any(np.signbit(got[k]))
    assert np.array_equal(ah.reduce_records(x, kptr, krec)[1], got)
    assert ah.reduce_records(x, kptr, np.where(np.arange(krec.size) == 5, nrec, krec))[0] == -1  # a record outside the table


def colsum_path(J, K, use_tmp, rows, glen):
    if use_tmp and J * K * ah.GCS_SLICES <= ah.REDUCE_TMP_ELEMS * 64 and rows >= J * 65536:
        return "sliced", ceil_div(ceil_div(max(glen, 1), ah.GCS_SLICES), 256) + 8 + ah.GCS_SLICES
    if J > 1024:
        return "small", ceil_div(max(glen, 1), 64) + 6
    return "plain", ceil_div(max(glen, 1), 256) + 8


def _check_colsum(q, goff, use_tmp, rows, want_path):
    K, J = q.shape[0], goff.size - 1
    rc, got = ah.group_colsum(q, goff, use_tmp=use_tmp, rows=rows)
    assert rc == 0
    for j in range(J):
        b, e = int(goff[j]), int(goff[j + 1])
        path, L = colsum_path(J, K, use_tmp, rows, e - b)
        assert path == want_path
        if e == b:
            assert np.array_equal(got[j], np.zeros(K)), j  # an empty group sums to 0.0
            continue
        ref = q[:, b:e].astype(LD).sum(axis=1)
        mag = np.abs(q[:, b:e]).astype(LD).sum(axis=1)
        assert np.all(np.abs(got[j].astype(LD) - ref) <= L * EPS * mag), (path, j, L)  # |err| <= L eps sum|x_i|
    assert np.array_equal(ah.group_colsum(q, goff, use_tmp=use_tmp, rows=rows)[1], got)


@pytest.mark.parametrize("J,want", [(1, "plain"), (7, "plain"), (1024, "plain"), (1025, "small")])
@pytest.mark.parametrize("K", [1, 4, 5, 33])
@pytest.mark.parametrize("kind", ["wide", "cancelling"])
def test_group_colsum_plain_and_small_group_paths(J, want, K, kind):
    rng = np.random.default_rng(J * 100 + K)
    counts = rng.integers(0, 3, J) * rng.integers(1, 12, J) * 16  # a third of the groups are empty
    counts[0], counts[J // 2], counts[-1] = (0, 1600, 0) if J > 2 else (4000, 4000, 4000)
    goff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    NP = int(goff[-1])
    q = wide(rng, (K, NP))
    if kind == "cancelling":
        q = cancel_pairs(rng, q, 1)
    q = np.concatenate([q, np.full((K, 32), 1e30)], axis=1)  # ldq > NP: rows no group owns are never added
    for use_tmp in (False, True):  # (tmp alone does not open the sliced path: rows stays below 65536 J)
        _check_colsum(q, goff, use_tmp, NP, want)


@pytest.mark.parametrize("name,counts,K,use_tmp,want", [
    ("rows = 65536 J", [65536], 33, True, "sliced"),
    ("rows = 65536 J - 16", [65520], 33, True, "plain"),
    ("two groups, the first empty", [0, 131072], 4, True, "sliced"),
    ("two groups, the last empty", [131072, 0], 4, True, "sliced"),
    ("no scratch", [65536], 5, False, "plain"),
    ("J K = 512", [100_000, 0, 96_608, 65_536], 128, True, "sliced"),
    ("J K = 520", [100_000, 0, 96_608, 65_536], 130, True, "plain"),
])
def test_group_colsum_sliced_path_and_its_boundaries(name, counts, K, use_tmp, want):
    rng = np.random.default_rng(len(name))
    goff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    NP = int(goff[-1])
    q = rng.standard_normal((K, NP))
    q *= 10.0 ** rng.integers(-12, 12, size=(K, 1))
    q *= np.exp(6 * rng.standard_normal(NP))  # (24 orders of magnitude over the rows of a column, too)
    _check_colsum(q, goff, use_tmp, NP, want)
    q[:, 1::2] = -q[:, 0::2]  # ... and columns that cancel to nothing
    _check_colsum(q, goff, use_tmp, NP, want)


@pytest.mark.parametrize("form", ["nrows", "rginfo"])
@pytest.mark.parametrize("K", [1, 5, 72])
def test_fill_qz_writes_the_value_on_valid_rows_and_zero_on_pad_rows(form, K):
    counts = [40, 0, 1, 16, 17]
    valid = ah.valid_rows(counts)
    NP = valid.size
    if form == "nrows":
        valid = np.arange(NP) < 70
    q = np.full((K + 1, NP + 16), SENT)
    want = q.copy()
    want[:K, :NP] = np.where(valid, 0.3125, 0.0)
    rc = ah.fill_qz(q, K, NP // 16, 0.3125, rginfo=ah.rginfo_of(counts) if form == "rginfo" else None, nrows=70)
    assert rc == 0 and np.array_equal(q, want)
    assert ah.fill_qz(q, K + 2, NP // 16, 1.0) == -1 and ah.fill_qz(q, K, NP // 16 + 2, 1.0) == -1  # refused, not launched
    assert ah.fill_qz(q, K, NP // 16, 1.0, nrows=-1) == -1 and ah.fill_qz(q, K, NP // 16, 1.0, nrows=NP + 1) == -1
    assert np.array_equal(q, want)


# =====================================================================================================================
# select_count / select_compact / group_starts
# =====================================================================================================================
def _group_offsets(rng, NP, J):
    """J groups over NP rows, boundaries on multiples of 16, with empty groups whenever J is large against NP / 16."""
    cuts = np.sort(rng.integers(0, NP // 16 + 1, J - 1)) * 16 if J > 1 else np.zeros(0, np.int64)
    return np.concatenate([[0], cuts, [NP]]).astype(np.int64)


def _select_column(rng, NP, pattern, t):
    q = rng.uniform(0.0, t, NP)  # nothing selected
    if pattern == "all":
        q = rng.uniform(np.nextafter(t, 1.0), 1.0, NP)
    elif pattern == "row 0":
        q[0] = 0.75
    elif pattern == "last row":
        q[-1] = 0.75
    elif pattern == "alternating blocks":
        q[(np.arange(NP) // 1024) % 2 == 0] = 0.9
    elif pattern == "edges":
        q = rng.choice(np.array([t, np.nextafter(t, 1.0), np.nextafter(t, 0.0), np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 0.25]), NP)
    elif pattern == "random":
        q = rng.uniform(0.0, 1.0, NP)
    elif pattern == "ends on a block":
        n = min(NP, 1024)
        q[:] = 0.0
        q[rng.choice(n, n // 2, replace=False)] = 1.0
        q[n - 1] = 1.0
    return q


@pytest.mark.parametrize("NP", [16, 1008, 1024, 1040, 4112, 300_016])
@pytest.mark.parametrize("pattern", ["none", "all", "row 0", "last row", "alternating blocks", "edges", "random", "ends on a block"])
def test_select_rows_and_group_starts_equal_flatnonzero_and_searchsorted(NP, pattern):
    """select_count + host scan + select_compact + group_starts as Context::select_rows_col chains them: the selection is
    np.flatnonzero(q > t) -- strictly greater; NaN, t itself and -0.0 stay out, nextafter(t) and +inf are in --, starts are
    np.searchsorted(idx, goff, "left"), the per-block counts those of 1024-row blocks."""
    rng = np.random.default_rng(NP + len(pattern))
    t = 0.5
    q = _select_column(rng, NP, pattern, t)
    for J in (1, 31, 63, 64, 1500):
        goff = _group_offsets(rng, NP, J)
        qq = q.copy()
        if pattern in ("all", "random", "edges") and J > 1:  # groups WITH rows but without a selected one: first, middle, last
            for j in (0, J // 2, J - 1):
                qq[goff[j]:goff[j + 1]] = t
        with np.errstate(invalid="ignore"):
            idx_ref = np.flatnonzero(qq > t)
        rc, M, idx, starts, counts = ah.select_rows(qq, t, goff)
        assert rc == 0 and M == idx_ref.size, (J, M, idx_ref.size)
        assert np.array_equal(idx[:M], idx_ref)
        assert np.all(idx[M:] == -7)  # nothing written behind the selection
        assert np.array_equal(starts, np.searchsorted(idx_ref, goff, "left"))
        assert np.array_equal(counts, np.bincount(idx_ref // 1024, minlength=ceil_div(NP, 1024)))
        if pattern == "none":
            assert M == 0


def test_select_rows_threshold_zero_and_signed_zeros():
    q = np.tile(np.array([-0.0, 0.0, 5e-324, -5e-324, np.nan, 1.0]), 200)
    want = np.flatnonzero((q == 5e-324) | (q == 1.0))
    for t in (0.0, -0.0):
        rc, M, idx, starts, _ = ah.select_rows(q, t, np.array([0, q.size], dtype=np.int64))
        assert rc == 0 and np.array_equal(idx[:M], want) and list(starts) == [0, M]


# =====================================================================================================================
# gathers, scatter, aug_from_sub, transpose
# =====================================================================================================================
def _selection(rng, J, kind):
    """Source layout, a selection in it, and the gathered layout (every group re-padded to a multiple of 16 rows, as
    Context::build_layout does for a sub-problem).  Groups 0, J // 2 and J - 1 contribute nothing (J > 2)."""
    if kind == "sparse":
        counts = rng.integers(0, 3, J) * rng.integers(1, 50, J)
    else:
        counts = rng.integers(1, 200, J)
    valid = ah.valid_rows(counts)
    goff = ah.padded_offsets(counts)
    pick = valid & (rng.uniform(size=valid.size) < (0.5 if kind != "all" else 2.0))
    if J > 2:
        for j in (0, J // 2, J - 1):
            pick[goff[j]:goff[j + 1]] = False
    idx = np.flatnonzero(pick).astype(np.int64)
    starts = np.searchsorted(idx, goff, "left").astype(np.int64)
    goff_sub = ah.padded_offsets(np.diff(starts))
    dst_of = np.concatenate([goff_sub[j] + np.arange(starts[j + 1] - starts[j]) for j in range(J)] + [np.zeros(0, np.int64)]).astype(np.int64)
    assert idx.size > 0
    return valid.size, idx, starts, goff_sub, dst_of


SELECTIONS = [(1, "half"), (1, "all"), (5, "half"), (64, "sparse"), (1500, "sparse")]


@pytest.mark.parametrize("J,kind", SELECTIONS)
@pytest.mark.parametrize("DP", [16, 48, 128, 192])
def test_gather_rows_moves_whole_rows_into_the_repadded_layout(J, kind, DP):
    rng = np.random.default_rng(J + DP)
    NP, idx, starts, goff_sub, dst_of = _selection(rng, J, kind)
    X = rng.normal(size=(NP, DP))
    ndst = int(goff_sub[-1]) + 16
    got = np.full((ndst, DP), SENT)
    want = got.copy()
    want[dst_of] = X[idx]
    assert ah.gather_rows(X, idx, starts, goff_sub, got) == 0
    assert np.array_equal(got, want)
    plain = np.full((idx.size + 3, DP), SENT)
    want = plain.copy()
    order = rng.permutation(idx.size)  # (gather_rows_plain takes any row list: unordered, and with repeats)
    rows = np.concatenate([idx[order][: idx.size - idx.size // 4], idx[: idx.size // 4]])
    want[: rows.size] = X[rows]
    assert ah.gather_rows_plain(X, rows, plain) == 0
    assert np.array_equal(plain, want)
    assert ah.gather_rows(X, idx, starts, goff_sub, np.full((int(dst_of.max()), DP), SENT)) == -1  # destination one row short
    assert ah.gather_rows_plain(X, np.array([NP]), plain) == -1                                    # a source row outside X


@pytest.mark.parametrize("J,kind", SELECTIONS)
@pytest.mark.parametrize("K", [1, 33, 72])
def test_gather_cols_and_gather_rowmajor_fill_the_same_column_major_table(J, kind, K):
    rng = np.random.default_rng(J * 3 + K)
    NP, idx, starts, goff_sub, dst_of = _selection(rng, J, kind)
    lds, ldd = NP + 48, int(goff_sub[-1]) + 32
    src = rng.normal(size=(K, lds))
    want = np.full((K, ldd), SENT)
    want[:, dst_of] = src[:, idx]
    got = np.full((K, ldd), SENT)
    assert ah.gather_cols(src, NP, idx, starts, goff_sub, got) == 0
    assert np.array_equal(got, want)
    rm = np.full((NP, K + 5), 4e4)  # row-major source with a row stride larger than K
    rm[:, :K] = src[:, :NP].T
    got = np.full((K, ldd), SENT)
    assert ah.gather_rowmajor(rm, K, idx, starts, goff_sub, got) == 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("J,kind", SELECTIONS)
@pytest.mark.parametrize("cols", [[3], [7, 2], [5, 5, 0], [9, 1, 4, 1], [0, 1, 2, 3, 4], [9, 8, 7, 6, 5, 4], [2, 2, 2, 2, 2, 2, 2],
                                  [6, 0, 9, 3, 3, 1, 8, 0]])
def test_gather_rowmajor_cols_takes_unordered_and_repeated_columns(J, kind, cols):
    rng = np.random.default_rng(J + len(cols))
    NP, idx, starts, goff_sub, dst_of = _selection(rng, J, kind)
    src = rng.normal(size=(NP, 10))
    ldd = int(goff_sub[-1]) + 16
    got = np.full((len(cols), ldd), SENT)
    want = got.copy()
    want[:, dst_of] = src[idx][:, cols].T
    assert ah.gather_rowmajor_cols(src, cols, idx, starts, goff_sub, got) == 0
    assert np.array_equal(got, want)
    assert ah.gather_rowmajor_cols(src, cols[:-1] + [10], idx, starts, goff_sub, got) == -1  # a column outside the table


@pytest.mark.parametrize("ncol", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("M", [0, 1, 255, 256, 257, 5000])
def test_scatter_cols_writes_the_listed_rows_only(ncol, M):
    rng = np.random.default_rng(ncol * 10000 + M)
    ndst = 6000
    idx = rng.choice(ndst, M, replace=False).astype(np.int64)
    src = rng.normal(size=(ncol, M + 7))
    got = np.full((ncol, ndst), SENT)
    want = got.copy()
    want[:, idx] = src[:, :M]
    assert ah.scatter_cols(src, idx, got) == 0
    assert np.array_equal(got, want)


def test_scatter_cols_refuses_a_ninth_column():
    src, got = np.ones((9, 40)), np.full((9, 64), SENT)
    assert ah.scatter_cols(src, np.arange(40), got) == ah.HIP_ERROR_INVALID_VALUE
    assert np.all(got == SENT)


@pytest.mark.parametrize("J,kind", SELECTIONS)
@pytest.mark.parametrize("K,k", [(1, 0), (6, 0), (6, 5), (33, 17)])
@pytest.mark.parametrize("hashed", [False, True])
def test_aug_from_sub_moves_column_k_of_the_rows_above_one_half(J, kind, K, k, hashed):
    rng = np.random.default_rng(J + K + k)
    NP, idx, starts, goff_sub, dst_of = _selection(rng, J, kind)
    nsub = int(goff_sub[-1])
    qsub1 = np.full(nsub, 0.9)  # pad rows of the sub-problem hold something that WOULD move a row
    qsub1[dst_of] = rng.choice(np.array([0.5, np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0), 0.0, 1.0, 0.3, 0.9, np.nan]), idx.size)
    q = rng.uniform(size=(K + 1, NP + 16))
    q[K] = SENT  # (Context zeroes the new column first; here it shows which entries the kernel writes)
    with np.errstate(invalid="ignore"):
        moved = idx[qsub1[dst_of] > 0.5]
    assert not np.isin(idx[qsub1[dst_of] == 0.5], moved).any() and np.isin(idx[qsub1[dst_of] == np.nextafter(0.5, 1.0)], moved).all()
    want = q.copy()
    want[K, moved] = q[k, moved]
    want[k, moved] = 0.0
    qh = rng.integers(1, 1 << 62, NP).astype(np.int64) if hashed else None
    wanth = None
    if hashed:
        wanth = qh.copy()
        wanth[moved] = QHASH_NONE
    assert ah.aug_from_sub(q, NP, k, idx, starts, goff_sub, qsub1, qh) == 0
    assert np.array_equal(q, want)  # exactly 0.5 stays, just above moves; no other entry changes
    if hashed:
        assert np.array_equal(qh, wanth)  # exactly the moved rows lose their fingerprint


@pytest.mark.parametrize("K", [1, 63, 64, 65, 72, 130])
@pytest.mark.parametrize("NP", [16, 48, 64, 80, 100_016])
def test_transpose_qz_gives_the_row_major_table(K, NP):
    rng = np.random.default_rng(K + NP)
    q = rng.normal(size=(K, NP + 48))
    got = np.full(NP * K + 64, SENT)
    want = got.copy()
    want[: NP * K] = q[:, :NP].T.ravel()
    assert ah.transpose_qz(q, NP, got) == 0
    assert np.array_equal(got, want)


# =====================================================================================================================
# split_init
# =====================================================================================================================
def padded_dim(D):
    return (D + 15) // 16 * 16


SPLIT_DIMS = [1, 2, 15, 16, 23, 64, 100, 128]


def _split_layout(form):
    """-> counts, NP (NP mod 32 = 16), valid mask, group of every row, rginfo (None in the single-group form), nrows"""
    counts = [100, 0, 1, 333, 16, 50, 7] if form == "rginfo" else [520]  # padded: 560 and 528 rows
    valid, grp = ah.valid_rows(counts), ah.group_of_rows(counts)
    assert valid.size % 32 == 16
    return counts, valid.size, valid, grp, (ah.rginfo_of(counts) if form == "rginfo" else None), counts[0]


@pytest.mark.parametrize("D", SPLIT_DIMS)
@pytest.mark.parametrize("form", ["nrows", "rginfo"])
def test_split_init_mode0_on_exact_data_is_the_sign_of_the_projection(D, form):
    """Rows, mean and direction built from small integers: every product and partial sum is exact, so q0 = (s >= 0) can be
    asserted bit for bit, including the rows with s = 0 (x = m: products of -0.0 and +0.0).  Garbage in v[D .. DP) must not
    matter; pad rows are zero in both columns."""
    rng = np.random.default_rng(D)
    counts, NP, valid, grp, rginfo, nrows = _split_layout(form)
    DP = padded_dim(D)
    X = np.zeros((NP, DP))
    X[:, :D] = rng.integers(-8, 9, (NP, D))
    m, v = rng.integers(-4, 5, D).astype(float), rng.integers(-3, 4, D).astype(float)
    v[0] = v[0] or 1.0
    zero = np.flatnonzero(valid)[::5]  # rows with s == 0 exactly: x = m, and x = m shifted across the direction
    X[zero, :D] = m
    if D >= 2:
        X[zero[::2], 0] += v[1]
        X[zero[::2], 1] -= v[0]
    X[~valid] = 0.0
    s = (X[:, :D] - m) @ v
    assert np.all(s[zero] == 0) and (s[valid] > 0).any() and (s[valid] < 0).any()
    mv = np.zeros(2 * DP)
    mv[:D], mv[DP:DP + D] = m, v
    mv[DP + D:] = 1e300  # garbage behind the direction
    q = np.full((2, NP + 16), SENT)
    want = q.copy()
    want[0, :NP] = np.where(valid & (s >= 0), 1.0, 0.0)
    want[1, :NP] = np.where(valid & (s < 0), 1.0, 0.0)
    assert ah.split_init(X, D, mv, q, 0, rginfo=rginfo, nrows=nrows, ngroups=len(counts)) == 0
    assert np.array_equal(q, want)


@pytest.mark.parametrize("D", SPLIT_DIMS)
@pytest.mark.parametrize("form", ["nrows", "rginfo"])
def test_split_init_on_random_data_against_a_longdouble_projection(D, form):
    rng = np.random.default_rng(100 + D)
    counts, NP, valid, grp, rginfo, nrows = _split_layout(form)
    DP = padded_dim(D)
    X = np.zeros((NP, DP))
    X[:, :D] = rng.normal(size=(NP, D)) * 3 + 1
    X[~valid] = 0.0
    m, v = rng.normal(size=D) + 1, rng.normal(size=D)
    mv = np.zeros(2 * DP)
    mv[:D], mv[DP:DP + D] = m, v
    # mode 0: the sign of s, outside the band where rounding may decide it
    q = np.full((2, NP + 16), SENT)
    assert ah.split_init(X, D, mv, q, 0, rginfo=rginfo, nrows=nrows, ngroups=len(counts)) == 0
    terms = (X[:, :D].astype(LD) - m.astype(LD)) * v.astype(LD)
    s_ref = terms.sum(axis=1)
    band = 4 * D * EPS * np.abs(terms).sum(axis=1)
    sure = valid & (np.abs(s_ref) > band)
    assert (valid & ~sure).sum() <= 0.001 * valid.sum()  # the filter may leave out 0.1 % of a case's rows, no more
    assert np.array_equal(q[0, :NP][sure], (s_ref[sure] >= 0).astype(np.float64))
    assert np.array_equal(q[1, :NP][valid], 1.0 - q[0, :NP][valid]) and set(np.unique(q[0, :NP])) <= {0.0, 1.0}
    assert np.all(q[:, :NP][:, ~valid] == 0.0) and np.all(q[:, NP:] == SENT)
    # mode 1: the projection x . v itself; |err| <= D eps sum_d |x_d v_d|
    q = np.full((2, NP + 16), SENT)
    assert ah.split_init(X, D, mv, q, 1, rginfo=rginfo, nrows=nrows, ngroups=len(counts)) == 0
    t1 = X[:, :D].astype(LD) * v.astype(LD)
    err = np.abs(q[0, :NP].astype(LD) - t1.sum(axis=1))
    assert np.all(err[valid] <= D * EPS * np.abs(t1).sum(axis=1)[valid])
    assert np.all(q[0, :NP][~valid] == 0.0) and np.all(q[1, :NP] == 0.0) and np.all(q[:, NP:] == SENT)


@pytest.mark.parametrize("form", ["nrows", "rginfo"])
def test_split_init_mode2_compares_strictly_with_the_groups_threshold(form):
    rng = np.random.default_rng(5)
    counts, NP, valid, grp, rginfo, nrows = _split_layout(form)
    thr = rng.normal(size=len(counts))
    proj = rng.normal(size=NP)
    at = rng.uniform(size=NP)
    proj = np.where(at < 0.3, thr[grp], np.where(at < 0.5, np.nextafter(thr[grp], np.inf), np.where(at < 0.7, np.nextafter(thr[grp], -np.inf), proj)))
    q = np.full((2, NP + 16), SENT)
    q[0, :NP] = np.where(valid, proj, 1e9)  # pad rows: whatever they hold, they end as zero
    want = q.copy()
    want[0, :NP] = np.where(valid & (proj > thr[grp]), 1.0, 0.0)
    want[1, :NP] = np.where(valid & ~(proj > thr[grp]), 1.0, 0.0)
    X = np.zeros((NP, 16))
    assert ah.split_init(X, 3, np.zeros(32), q, 2, rginfo=rginfo, nrows=nrows, ngroups=len(counts), thr=thr) == 0
    assert np.array_equal(q, want)
    assert (valid & (proj == thr[grp])).sum() > 20


# =====================================================================================================================
# fingerprints: qhash_verify, qz_resync
# =====================================================================================================================
def _responsibilities(rng, K, NP, ld):
    q = np.zeros((K, ld))
    r = rng.dirichlet(np.full(K, 0.3), NP).T
    r[r < 1e-3] = 0.0  # zeros: entries the fingerprint chain skips
    q[:, :NP] = r
    return q


def test_python_qhash_skips_zero_entries_and_sees_the_column():
    row = np.array([0.25, 0.0, 0.75])
    assert ah.qhash(row) == ah.qhash(np.append(row, 0.0)) == ah.qhash(np.append(row, [0.0, 0.0]))
    assert ah.qhash(row) != ah.qhash(np.array([0.25, 0.75, 0.0])) and ah.qhash(row) != ah.qhash(np.array([0.75, 0.0, 0.25]))
    assert ah.qhash(np.zeros(5)) == ah.QHASH_SEED


@pytest.mark.parametrize("ncorrupt", [0, 1, 1000])
@pytest.mark.parametrize("K", [1, 9, 72])
def test_qhash_verify_counts_the_rows_whose_fingerprint_is_wrong(ncorrupt, K):
    rng = np.random.default_rng(K + ncorrupt)
    NP = 3000
    q = _responsibilities(rng, K, NP, NP + 16)
    h = ah.qhash_rows(q[:, :NP])
    h[rng.choice(NP, 100, replace=False)] = QHASH_NONE  # unknown fingerprints are not counted
    rc, bad = ah.qhash_verify(q, K, NP, h)
    assert (rc, bad) == (0, 0)  # the device chain is the Python chain
    known = np.flatnonzero(h != QHASH_NONE)
    rows = rng.choice(known, ncorrupt, replace=False)
    for i, r in enumerate(rows):
        if i % 2:
            h[r] ^= 1
        else:
            j = int(np.argmax(q[:, r]))
            q[j, r] = np.nextafter(q[j, r], 0.0)  # one bit of one entry
    rc, bad = ah.qhash_verify(q, K, NP, h)
    assert (rc, bad) == (0, ncorrupt)


@pytest.mark.parametrize("K,Kdst", [(1, 1), (8, 9), (33, 36), (71, 72)])
def test_qz_resync_copies_exactly_the_rows_whose_fingerprints_differ(K, Kdst):
    rng = np.random.default_rng(K)
    NP, ld = 2000, 2032
    src = rng.uniform(size=(K, ld))
    dst = rng.uniform(size=(Kdst, ld)) + 2.0  # differs from src everywhere: a copy shows
    shash = rng.integers(1, 1 << 62, NP).astype(np.int64)
    dhash = shash.copy()
    kind = rng.integers(0, 5, NP)  # 0: equal; 1: differ; 2: both unknown; 3: source unknown; 4: copy unknown
    dhash[kind == 1] += 1
    shash[(kind == 2) | (kind == 3)] = QHASH_NONE
    dhash[(kind == 2) | (kind == 4)] = QHASH_NONE
    copied = np.flatnonzero(kind != 0)
    want, wanth = dst.copy(), dhash.copy()
    want[:K, copied] = src[:K, copied]
    want[K:, copied] = 0.0
    wanth[copied] = shash[copied]
    assert ah.qz_resync(dst, src, K, NP, dhash, shash) == 0
    assert np.array_equal(dst, want)  # rows with equal fingerprints, and everything behind NP, untouched
    assert np.array_equal(dhash, wanth)


# =====================================================================================================================
# bound_select
# =====================================================================================================================
def _bound_reference(ref, sigma, bnorm, cnew, rmax, ramax, T, usable, dcj, K):
    """BoundSelectLaunch (lc_kernels.h), in float64 and in the kernel's order of operations."""
    ncol, NP = ref.shape
    j = ramax.astype(np.int64)
    inside = (j >= 0) & (j < K)
    jj = np.where(inside, j, 0)
    skip = inside & (usable[jj] != 0)
    with np.errstate(invalid="ignore"):
        low = (rmax + dcj[jj]) - T
        ub = np.empty_like(ref)
        for t in range(ncol):
            d2 = -2.0 * ref[t]
            s = np.maximum(sigma[t] * np.sqrt(np.maximum(d2, 0.0)) - bnorm[t], 0.0)  # (np.maximum keeps a NaN, as the header's
            ub[t] = (-0.5 * s) * s                                                   #  "NaN anywhere: recomputed" asks)
            skip = skip & (cnew[t] + ub[t] < low)  # NaN anywhere: False
    return skip, ub, low


@pytest.mark.parametrize("ncol", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("K", [1, 33, 72])
def test_bound_select_flags_and_bounds_equal_the_formula(ncol, K):
    """Inputs on a dyadic grid (distances m / 8, factors and offsets multiples of 1 / 16): every product of the formula is
    exact in double, so its float64 evaluation has ONE value whatever the compiler contracts -- the kernel's
    sigma * sqrt(d2) - bnorm is a fused multiply-add (docs/NOTEBOOK.md section 16) -- and need / dest can be compared bit
    for bit.  Ties cnew + ub == low occur by construction (strict <: such a row is recomputed)."""
    rng = np.random.default_rng(ncol * 100 + K)
    NP = 5000
    dist = rng.integers(0, 400, (ncol, NP)) / 8.0
    ref = -0.5 * dist * dist
    sigma, bnorm = rng.integers(4, 32, ncol) / 16.0, rng.integers(0, 64, ncol) / 16.0
    cnew = rng.integers(-64, 64, ncol) / 16.0
    ramax = rng.integers(0, K, NP).astype(np.int32)
    usable = (rng.uniform(size=K) < 0.8).astype(np.uint8)
    usable[0] = 1
    dcj = rng.integers(-32, 32, K) / 16.0
    T = 208.0
    # rmax chosen so that a third of the rows tie exactly in their tightest column, the others lie 1 / 16 or 50 to either side
    s = np.fmax(sigma[:, None] * dist - bnorm[:, None], 0.0)
    tight = (cnew[:, None] + (-0.5 * s) * s).max(axis=0)
    rmax = tight + T - dcj[ramax] + rng.choice(np.array([0.0, 0.0, 0.0625, -0.0625, 50.0, -50.0]), NP)
    edge = rng.uniform(size=NP)
    ramax[edge < 0.03] = -1
    ramax[(edge >= 0.03) & (edge < 0.06)] = K
    ramax[(edge >= 0.06) & (edge < 0.07)] = 1 << 30
    nanrows = np.flatnonzero(edge > 0.95)
    ref[rng.integers(0, ncol, nanrows.size), nanrows] = np.nan
    ref[0, (edge > 0.90) & (edge <= 0.95)] = 3.0  # a positive "-0.5 d^2": d2 < 0 is clamped to 0
    skip, ub, low = _bound_reference(ref, sigma, bnorm, cnew, rmax, ramax, T, usable, dcj, K)
    jj = np.clip(ramax, 0, K - 1)
    live = (ramax >= 0) & (ramax < K) & (usable[jj] != 0)
    with np.errstate(invalid="ignore"):
        ties = (cnew[:, None] + ub == low[None, :]).any(axis=0) & live
    assert ties.sum() > 100 and skip.sum() > 100 and not skip[ties].any()
    dest, need = np.full((ncol, NP), SENT), np.full(NP, SENT)
    assert ah.bound_select(K, ref, dest, sigma, bnorm, cnew, rmax, ramax, T, usable, dcj, need) == 0
    assert np.array_equal(need, np.where(skip, 0.0, 1.0))
    assert np.array_equal(dest, np.where(skip[None, :], ub, SENT))  # the bound on skipped rows, nothing where need = 1
    assert not skip[np.isnan(ref).any(axis=0)].any() and not skip[~live].any()


@pytest.mark.parametrize("ncol,K", [(9, 8), (2, 73)])
def test_bound_select_refuses_what_its_tables_cannot_hold(ncol, K):
    NP = 64
    dest, need = np.full((ncol, NP), SENT), np.full(NP, SENT)
    rc = ah.bound_select(K, np.zeros((ncol, NP)), dest, np.ones(ncol), np.zeros(ncol), np.zeros(ncol), np.zeros(NP),
                         np.zeros(NP, np.int32), 208.0, np.ones(K, np.uint8), np.zeros(K), need)
    assert rc == ah.HIP_ERROR_INVALID_VALUE
    assert np.all(dest == SENT) and np.all(need == SENT)


# =====================================================================================================================
# softmax_cached
# =====================================================================================================================
SOFTMAX_K = [1, 8, 9, 16, 17, 24, 25, 32, 33, 36, 37, 40, 41, 56, 57, 72]


def _softmax_case(K, form, cmkind, seed):
    """Inputs of one sweep.  Layout: one group with nrows < NP, or five groups (one empty, one of a single row)."""
    rng = np.random.default_rng(seed)
    if form == "nrows":
        NP, nrows, rginfo, J = 528, 500, None, 1
        valid, grp = np.arange(NP) < nrows, np.zeros(NP, np.int64)
    else:
        counts = [300, 0, 1, 77, 200]
        valid, grp, rginfo, J, nrows = ah.valid_rows(counts), ah.group_of_rows(counts), ah.rginfo_of(counts), 5, 0
        NP = valid.size
    ldc, ldf, nfresh = NP + 16, NP + 32, 3
    raw = -0.5 * rng.chisquare(4, (K, NP)) * rng.choice(np.array([1.0, 10.0, 60.0]), (1, NP))  # -0.5 d^2, near and far rows
    far = np.arange(NP) % 7 == 3  # rows whose other columns lie more than 745 below their best one: those q are exactly 0.0
    best = rng.integers(0, K, NP)
    raw[:, far] = -2000.0 - 100.0 * rng.uniform(size=(K, int(far.sum())))
    raw[best[far], np.flatnonzero(far)] = -3.0
    mid = np.arange(NP) % 7 == 5  # ... and rows with columns 250 .. 650 below: q between 1e-283 and 1e-109, kept in plain mode
    raw[:, mid] = -250.0 - 400.0 * rng.uniform(size=(K, int(mid.sum())))
    raw[best[mid], np.flatnonzero(mid)] = -1.0
    dcache, fresh, colmap = np.full((K if cmkind == "none" else K + 2, ldc), np.nan), None, None
    if cmkind == "none":
        dcache[:, :NP] = raw
    else:
        colmap = rng.permutation(K + 2)[:K].astype(np.int32)
        if cmkind == "mix":  # every third cluster comes from a fresh column (a fresh column may serve several clusters)
            fresh = np.full((nfresh, ldf), np.nan)
            for j in range(0, K, 3):
                colmap[j] = -(int(rng.integers(0, nfresh)) + 1)
            for f in range(nfresh):
                users = np.flatnonzero(colmap == -(f + 1))
                fresh[f, :NP] = raw[users[0]] if users.size else 0.0
                raw[users] = fresh[f, :NP]
        for j in range(K):
            if colmap[j] >= 0:
                dcache[colmap[j], :NP] = raw[j]
    ctab = rng.normal(size=(J, K)) * 3
    if K > 1:
        for j in range(J):  # -inf entries (sparse-inactive clusters), never a whole row
            ctab[j, rng.choice(K, min(K - 1, 1 + K // 8), replace=False)] = -np.inf
    return dict(K=K, NP=NP, nrows=nrows, rginfo=rginfo, valid=valid, grp=grp, dcache=dcache, fresh=fresh, colmap=colmap, ctab=ctab,
                raw=raw, J=J)


def _softmax_reference(c):
    """lq = fl(col + c) and d = fl(lq - max) in float64 -- the kernel's own operations, so that their rounding is not charged
    to it --, everything behind them in longdouble."""
    lq = c["raw"] + c["ctab"][c["grp"]].T  # [K x NP]
    mx = lq.max(axis=0)
    d = lq - mx
    with np.errstate(under="ignore"):
        e = np.exp(d.astype(LD))
    s = e.sum(axis=0)
    return lq, mx, d, e / s, np.log(s) + mx.astype(LD)


def _run_softmax(c, ll=False, moved=False, qZ=None, qhash_arr=None, qhash_in=0, bounds=False):
    K, NP = c["K"], c["NP"]
    nblk = ceil_div(NP, 256)
    out = dict(qZ=np.full((K + 1, NP + 16), SENT) if qZ is None else qZ, fz=np.full(nblk, SENT),
               ll=np.full((nblk, K), SENT) if ll else None)
    if moved:
        out.update(dq=np.full((NP, K + 3), SENT), amax=np.full(NP, SENT), colmask=np.zeros(2, np.uint64),
                   qhash=np.full(NP, QHASH_NONE, np.int64) if qhash_arr is None else qhash_arr)
    if bounds:
        out.update(rmax=np.full(NP, SENT), ramax=np.full(NP, -5, np.int32))
    rc = ah.softmax_cached(c["dcache"], c["ctab"], K, NP, out["qZ"], out["fz"], fresh=c["fresh"], colmap=c["colmap"], rginfo=c["rginfo"],
                           nrows=c["nrows"], ll_part=out["ll"], dq=out.get("dq"), amax=out.get("amax"), qhash_arr=out.get("qhash"),
                           qhash_in=qhash_in, rmax=out.get("rmax"), ramax=out.get("ramax"), colmask=out.get("colmask"))
    return rc, out


def _check_q(c, q, with_ll):
    """q [K x NP] against the longdouble reference; returns the worst error of a normal q in units of eps * q."""
    K, valid = c["K"], c["valid"]
    lq, mx, d, q_ref, logZ = _softmax_reference(c)
    assert np.all(q[:, ~valid] == 0.0)  # pad rows are exactly zero
    qv, rv = q[:, valid], q_ref[:, valid]
    finite = np.where(np.isfinite(lq[:, valid]), np.abs(lq[:, valid]), 0.0)
    absz = np.abs(logZ[valid]).astype(np.float64)
    if with_ll:  # q = exp(lq - logZ): the second exponential sees the rounding of logZ and of the difference
        bar = (4 + K + absz[None, :] + finite) * EPS
    else:        # q = e / sum e: 1.3 exponential + 1 reciprocal + 0.5 product + K / 2 sum, margin of about two
        bar = np.full(qv.shape, (4 + K) * EPS)
    normal = rv >= TINY
    err = np.abs(qv.astype(LD) - rv)
    assert np.all(err[normal] <= bar[normal] * rv[normal]), float((err[normal] / rv[normal]).max() / EPS)
    # below the normal range the exponential's and the product's roundings are absolute: 1.1 + 0.5 units of 2^-1074
    assert np.all(err[~normal] <= bar[~normal] * rv[~normal] + 2 * DENORM)
    assert np.all(qv[d[:, valid] < -746.0] == 0.0)  # columns more than 745 below the row's maximum: exactly 0.0
    assert np.all(qv[np.isneginf(lq[:, valid])] == 0.0)
    # rows sum to 1 to K eps; behind the second exponential the rounding of logZ and lq - logZ is common to a row's entries
    sumbar = (K + absz + finite.max(axis=0)) * EPS if with_ll else K * EPS
    assert np.all(np.abs(qv.astype(LD).sum(axis=0) - 1) <= sumbar)
    return float((err[normal] / rv[normal]).max() / EPS) if normal.any() else 0.0


def _check_fz(c, fz, logZ):
    """F_z partial of a 256-row block = -sum logZ of its valid rows.  Per row: log s carries the K eps of s and an ulp of
    its own, logZ = log s + max one rounding; then L = 6 (wave) + 3 (four waves) additions."""
    K, valid = c["K"], c["valid"]
    blk = np.arange(c["NP"]) // 256
    for b in range(fz.size):
        lz = logZ[valid & (blk == b)]
        bar = ((K + 2) * EPS * lz.size + EPS * np.abs(lz).sum()) + 9 * EPS * np.abs(lz).sum()
        assert abs(LD(fz[b]) + lz.sum()) <= bar, (b, float(fz[b]), float(-lz.sum()))


@pytest.mark.parametrize("K", SOFTMAX_K)
@pytest.mark.parametrize("form,cmkind", [("nrows", "none"), ("rginfo", "perm"), ("rginfo", "mix"), ("nrows", "mix")])
def test_softmax_cached_plain_mode_every_instance(K, form, cmkind):
    c = _softmax_case(K, form, cmkind, 1000 + K)
    NP, valid = c["NP"], c["valid"]
    lq, mx, d, q_ref, logZ = _softmax_reference(c)
    # --- one exponential per entry (no ll_part), with rmax / ramax
    rc, o = _run_softmax(c, bounds=True)
    assert rc == 0
    assert np.all(o["qZ"][K:] == SENT) and np.all(o["qZ"][:, NP:] == SENT)  # nothing outside the K x NP block
    worst = _check_q(c, o["qZ"][:K, :NP], with_ll=False)
    assert np.array_equal(o["rmax"], mx)  # the row's maximum, bit for bit, pad rows included
    assert np.all((o["ramax"] >= 0) & (o["ramax"] < K)) and np.array_equal(lq[o["ramax"], np.arange(NP)], mx)
    _check_fz(c, o["fz"], logZ)
    # --- with ll_part: the second exponential behind logZ
    rc, o2 = _run_softmax(c, ll=True)
    assert rc == 0
    assert np.all(o2["qZ"][K:] == SENT) and np.all(o2["qZ"][:, NP:] == SENT)
    worst2 = _check_q(c, o2["qZ"][:K, :NP], with_ll=True)
    _check_fz(c, o2["fz"], logZ)
    with np.errstate(invalid="ignore"):
        diff = np.where(np.isfinite(lq), lq - c["ctab"][c["grp"]].T, 0.0)  # fl(lq - c), as the kernel forms it
    term = q_ref * diff.astype(LD)
    finite = np.where(np.isfinite(lq), np.abs(lq), 0.0)
    # per entry q's bar, one rounding of the product, then L = 6 + 3 additions; a subnormal q is 2 units of 2^-1074 off at most
    rel = (4 + K + np.abs(logZ).astype(np.float64)[None, :] + finite + 1 + 9) * EPS
    blk = np.arange(NP) // 256
    for b in range(o2["fz"].size):
        rows = valid & (blk == b)
        ref = term[:, rows].sum(axis=1)
        bar = (rel[:, rows] * np.abs(term[:, rows]) + 2 * DENORM * np.abs(diff[:, rows])).sum(axis=1) + 9 * DENORM
        assert np.all(np.abs(o2["ll"][b].astype(LD) - ref) <= bar), b
    print(f"softmax_cached K = {K} ({form}, colmap {cmkind}): worst |q - q_ref| / q = {worst:.2f} eps (bar {4 + K}), "
          f"with ll_part {worst2:.2f} eps")


def test_softmax_cached_refuses_73_columns():
    c = _softmax_case(73, "nrows", "none", 73)
    rc, o = _run_softmax(c, bounds=True)
    assert rc == ah.HIP_ERROR_INVALID_VALUE
    assert np.all(o["qZ"] == SENT) and np.all(o["fz"] == SENT) and np.all(o["rmax"] == SENT)


def test_softmax_cached_argmax_is_the_maximum_itself_not_a_near_one():
    """A later column one ulp below the row's maximum: ramax must name a column whose value EQUALS rmax."""
    K, NP = 9, 512
    rng = np.random.default_rng(3)
    raw = np.full((K, NP), -50.0)
    top = rng.integers(0, K - 1, NP)
    raw[top, np.arange(NP)] = -1.0
    raw[K - 1] = np.nextafter(-1.0, -np.inf)
    c = dict(K=K, NP=NP, nrows=NP, rginfo=None, valid=np.ones(NP, bool), grp=np.zeros(NP, np.int64), dcache=raw.copy(), fresh=None,
             colmap=None, ctab=np.zeros((1, K)), raw=raw, J=1)
    rc, o = _run_softmax(c, bounds=True)
    assert rc == 0 and np.array_equal(o["rmax"], np.full(NP, -1.0)) and np.array_equal(o["ramax"], top)


@pytest.mark.parametrize("K", [9, 33, 72])
@pytest.mark.parametrize("form,cmkind", [("nrows", "none"), ("rginfo", "mix")])
def test_softmax_cached_moved_row_mode(K, form, cmkind):
    c = _softmax_case(K, form, cmkind, 2000 + K)
    NP = c["NP"]
    rc, plain = _run_softmax(c)
    assert rc == 0
    qp = plain["qZ"][:K, :NP]
    assert ((qp > 0) & (qp < 2.0 ** -300)).sum() > 50  # plain mode keeps the specks ...
    want = np.where(qp < 2.0 ** -300, 0.0, qp)          # ... moved-row mode stores them as zero, and nothing else differs
    # --- first sweep: from sentinel old values, fingerprints unknown
    old = 0.123
    q = np.full((K + 1, NP + 16), SENT)
    q[:K, :NP] = old
    rc, o = _run_softmax(c, moved=True, qZ=q)
    assert rc == 0
    assert np.array_equal(q[:K, :NP], want) and np.all(q[K:] == SENT) and np.all(q[:, NP:] == SENT)
    assert np.array_equal(o["dq"][:, :K], (want - old).T) and np.all(o["dq"][:, K:] == SENT)  # dq = fl(q_new - q_old)
    assert np.array_equal(o["amax"], np.abs(want - old).max(axis=0))                          # amax = max_j |dq|
    full = [(1 << min(K, 64)) - 1, (1 << max(K - 64, 0)) - 1]
    assert [int(v) for v in o["colmask"]] == full  # every column moved somewhere
    hashes = ah.qhash_rows(want)
    assert np.array_equal(o["qhash"], hashes)  # the stored fingerprints are those of the stored rows
    assert ah.qhash_verify(q, K, NP, o["qhash"]) == (0, 0)
    q1 = np.vstack([want, np.zeros((1, NP))])
    assert ah.qhash_verify(q1, K + 1, NP, o["qhash"]) == (0, 0)  # a zero column appended: the same fingerprint
    assert np.array_equal(o["fz"], plain["fz"])
    # --- (a) again on its own output, fingerprints in: no row is read or written.  The stored q is REPLACED by garbage
    # here: a sweep that read it would find a difference and write.
    garbage = np.full((K + 1, NP + 16), SENT)
    rc, a = _run_softmax(c, moved=True, qZ=garbage, qhash_arr=o["qhash"].copy(), qhash_in=1)
    assert rc == 0
    assert np.all(garbage == SENT) and np.all(a["dq"] == SENT)
    assert np.all(a["amax"] == 0.0) and [int(v) for v in a["colmask"]] == [0, 0]
    assert np.array_equal(a["qhash"], hashes)
    # --- (b) known rows, perturbed in known columns (their fingerprints unknown or stale): exactly those entries come back
    rng = np.random.default_rng(K)
    rows = rng.choice(NP, 40, replace=False)
    cols = sorted({0, K - 1, K // 2} | ({64, 66, 71} if K > 64 else set()))
    q = np.full((K + 1, NP + 16), SENT)
    q[:K, :NP] = want
    for r in rows:
        for j in cols:
            q[j, r] = want[j, r] + 0.25
    qh = hashes.copy()
    qh[rows] = QHASH_NONE
    qh[rows[:5]] = hashes[rows[:5]] ^ 0x55
    before = q.copy()
    rc, b = _run_softmax(c, moved=True, qZ=q, qhash_arr=qh, qhash_in=1)
    assert rc == 0
    assert np.array_equal(q[:K, :NP], want) and np.all(q[K:] == SENT) and np.all(q[:, NP:] == SENT)
    mask = [sum(1 << j for j in cols if j < 64), sum(1 << (j - 64) for j in cols if j >= 64)]
    assert [int(v) for v in b["colmask"]] == mask  # exactly those bits, in both words
    dq_want = np.full((NP, K + 3), SENT)
    dq_want[rows, :K] = (want[:, rows] - before[:K, rows]).T
    assert np.array_equal(b["dq"], dq_want)  # written for the rows that were compared, all K entries; no other row
    amax_want = np.zeros(NP)
    amax_want[rows] = np.abs(want[:, rows] - before[:K, rows]).max(axis=0)
    assert np.array_equal(b["amax"], amax_want)
    assert np.array_equal(b["qhash"], hashes) and ah.qhash_verify(q, K, NP, b["qhash"]) == (0, 0)
