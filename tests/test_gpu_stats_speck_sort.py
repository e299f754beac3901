"""Sorted batches in the speck-skipping statistics pass (SuffstatLaunch::speck_skip == 2): a staged batch whose
rows all keep at most one cluster quad is sorted by that quad (stable; the rows that keep nothing last), and the 4-row steps
are formed from the rows as placed; a batch with a row that keeps two quads stays in order.  Everything goes through
lcx_test_suffstat_speck with the mode given (0 dense, 1 skipping, 2 skipping with sorted batches), on the shapes and row
counts of tests/test_gpu_stats_speck_skip.py, whose helpers are used here.

The constructions (pure_step_q, mixed_q) and the numpy restatement of the slot rule (slots) are checked on the CPU in
tests/test_stats_speck_sort_refs_host.py."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import aux_hooks as ah
import hot_refs as hr
import test_gpu_stats_speck_skip as sk

pytestmark = pytest.mark.gpu

TAU = sk.TAU
SPECK = 2.0 ** -350
BATCH_ROWS = (24, 32, 48)  # rows of a staged batch, by width (ft_batch_rows); row chunks are multiples of 32 rows


def exact_rows(DP, DC, K, NP):
    """X of test_threshold_edges_and_nan without its invalid rows: signed powers of two, every product and sum exact"""
    rng = np.random.default_rng(DP + DC + K)
    X = np.zeros((NP, DP))
    X[:, :DC - 1] = rng.choice([-1.0, 1.0], size=(NP, DC - 1)) * 2.0 ** rng.integers(-3, 4, size=(NP, DC - 1))
    return X


def group_quads(K, NP):
    """per group of eight rows the two owning quads (a, b), different, among the quads with four clusters"""
    nfull = K // 4
    g = np.arange(NP // 8)
    a = g % nfull
    b = (a + 1 + (g // nfull) % (nfull - 1)) % nfull
    assert np.all(a != b)
    return a, b


def pure_step_q(K, NP):
    """Rows in groups of eight with owners a, b, a, b, a, b, a, b (q = 1.0 on cluster 4 a of the a-rows, 4 b + 1 of the
    b-rows); every a-row carries 2^-350 on cluster 4 b + 2, every b-row on 4 a + 3.  -> q, the clusters that hold only specks"""
    assert NP % 8 == 0
    a, b = group_quads(K, NP)
    q = np.zeros((K, NP))
    r = np.arange(NP)
    ga, gb = a[r // 8], b[r // 8]
    ar = r % 2 == 0
    q[(4 * ga)[ar], r[ar]] = 1.0
    q[(4 * gb + 2)[ar], r[ar]] = SPECK
    q[(4 * gb + 1)[~ar], r[~ar]] = 1.0
    q[(4 * ga + 3)[~ar], r[~ar]] = SPECK
    specks = np.arange(K) % 4 >= 2
    specks[4 * (K // 4):] = False
    return q, specks


def mixed_q(K, NP):
    """pure_step_q with the first row of every group of eight keeping two quads: 0.5 on cluster 4 a and 0.5 on 4 b + 1"""
    q, specks = pure_step_q(K, NP)
    a, b = group_quads(K, NP)
    r = np.arange(0, NP, 8)
    q[4 * a, r] = 0.5
    q[4 * b + 1, r] = 0.5
    return q, specks


def row_masks(q):
    """per row the bit mask of its kept quads (a value is kept when it is not below 2^-300: a NaN is kept)"""
    K, NP = q.shape
    with np.errstate(invalid="ignore"):
        kept = ~(q < TAU)
    m = np.zeros(NP, dtype=np.int64)
    for c in range(-(-K // 4)):
        m |= kept[4 * c:4 * c + 4].any(axis=0).astype(np.int64) << c
    return m


def slots(masks, NQ):
    """the slot rule of one staged batch: the rows as they come when any row keeps more than one quad, else a stable sort by
    the owning quad with the rows that keep nothing last -> slot of every row"""
    masks = np.asarray(masks, dtype=np.int64)
    pop = np.array([bin(int(v)).count("1") for v in masks])
    if (pop > 1).any():
        return np.arange(masks.size)
    key = np.array([NQ if v == 0 else (int(v) & -int(v)).bit_length() - 1 for v in masks])
    order = np.argsort(key, kind="stable")
    s = np.empty(masks.size, dtype=np.int64)
    s[order] = np.arange(masks.size)
    return s


def placed_step_masks(q, BR):
    """the masks of the steps of every batch of BR rows as the kernel forms them (OR over the four rows placed in a step;
    rows past the end keep nothing) -> list over batches of [BR / 4] masks"""
    K, NP = q.shape
    NQ = -(-K // 4)
    m = row_masks(q)
    out = []
    for b0 in range(0, NP, BR):
        mb = np.zeros(BR, dtype=np.int64)
        mb[: min(BR, NP - b0)] = m[b0:b0 + BR]
        placed = np.zeros(BR, dtype=np.int64)
        placed[slots(mb, NQ)] = mb
        out.append(np.bitwise_or.reduce(placed.reshape(BR // 4, 4), axis=1))
    return out


def flushed(q):
    with np.errstate(invalid="ignore"):
        return np.where(q < TAU, 0.0, q)


@pytest.mark.parametrize("NP", sk.NPS)
@pytest.mark.parametrize("DP,DC,K", sk.FEAT)
def test_premise_sorted_skipping_and_dense_give_the_same_bits(DP, DC, K, NP):
    """The premise of sorting by default: on continuous X and hard rows (sk.same_bits_problem: every cluster outside the
    empty quad owns a row) modes 2, 1 and 0 give bit-identical folded records -- the fp64 MFMA adds a step's four rows to the
    accumulator as a chain in row order, so a cluster's own rows meet its accumulator in the same order wherever the sort
    puts them, and the specks and zeros in between change nothing."""
    sk.feat_shape(DP, DC, K, NP)
    X, q = sk.same_bits_problem(DP, DC, K, NP)
    m = sk.low(DP, DC)
    two, one, off = (sk.folded(X, DC, q, K, s)[:, m] for s in (2, 1, 0))
    d21 = int((two.view(np.uint64) != one.view(np.uint64)).sum())
    d10 = int((one.view(np.uint64) != off.view(np.uint64)).sum())
    print(f"DP={DP} DC={DC} K={K} NP={NP}: entries that differ, mode 2 / mode 1: {d21}, mode 1 / dense: {d10} of {two.size}")
    assert sk.same_bits(two, one) and sk.same_bits(one, off)


@pytest.mark.parametrize("DP,DC,K", sk.FEAT)
def test_sorted_steps_drop_the_specks_the_unsorted_rule_keeps(DP, DC, K):
    """pure_step_q on exact X: unsorted, every step holds rows of two owners and both quads are kept, so every speck is
    multiplied (those clusters' N_k are count x 2^-350 exactly); sorted, every step is pure and every speck is dropped
    (exact zeros).  The owners' records equal the exact sums in both modes."""
    NP = 272
    sk.feat_shape(DP, DC, K, NP)
    X = exact_rows(DP, DC, K, NP)
    q, specks = pure_step_q(K, NP)
    m = sk.low(DP, DC)
    ref = hr.stats_ref(X, q)
    one, two = sk.folded(X, DC, q, K, 1), sk.folded(X, DC, q, K, 2)
    count = (q == SPECK).sum(axis=1)
    assert count[specks].sum() == NP and not count[~specks].any()
    assert sk.exact_equal(one[:, m], ref[:, m]) and np.array_equal(one[specks, 0], count[specks] * SPECK)
    assert sk.exact_equal(two[~specks][:, m], ref[~specks][:, m]), "an owner's record changed"
    assert sk.exact_equal(two[specks][:, m], np.zeros((int(specks.sum()), int(m.sum())))), "a speck survived: the batch was not sorted"


@pytest.mark.parametrize("DP,DC,K", sk.FEAT)
def test_a_batch_with_a_row_of_two_quads_stays_in_order(DP, DC, K):
    """mixed_q: every eighth row keeps two quads, so every batch holds such a row and keeps its order -- mode 2 equals mode 1
    bit for bit, the specks of the kept pairs included (all of them, as in the exact sums)."""
    NP = 272
    sk.feat_shape(DP, DC, K, NP)
    X = exact_rows(DP, DC, K, NP)
    q, specks = mixed_q(K, NP)
    m = sk.low(DP, DC)
    one, two = sk.folded(X, DC, q, K, 1), sk.folded(X, DC, q, K, 2)
    assert sk.same_bits(two[:, m], one[:, m])
    count = (q == SPECK).sum(axis=1)
    assert sk.exact_equal(two[:, m], hr.stats_ref(X, q)[:, m]) and np.array_equal(two[specks, 0], count[specks] * SPECK)
    assert count[specks].sum() == NP


@functools.lru_cache(maxsize=None)
def flushed_refs(DP, DC, K, NP):
    """long-double sums and sums of absolute values of sk.hard_problem's q with everything below 2^-300 zeroed"""
    X, q, _, _, _, _ = sk.hard_problem(DP, DC, K, NP)
    qz = flushed(q)
    ref = np.zeros((K, hr.stat_stride(DP)), dtype=hr.LD)
    absrec = np.zeros((K, hr.stat_stride(DP)))
    for k in range(K):
        rows = np.nonzero(qz[k])[0]
        if rows.size:
            ref[k] = hr.stats_ref(X[rows], qz[k:k + 1, rows], dtype=hr.LD)[0]
            absrec[k] = hr.stats_abs(X[rows], qz[k:k + 1, rows])[0]
    ref.setflags(write=False)
    absrec.setflags(write=False)
    return ref, absrec


@pytest.mark.parametrize("NP", sk.NPS)
@pytest.mark.parametrize("DP,DC,K", sk.FEAT)
def test_hard_rows_sorted_sum_to_the_owned_rows(DP, DC, K, NP):
    """sk.hard_problem (one owner per row, a quad without owners), mode 2: within hr.stats_bar of the long-double sums of q
    with everything below 2^-300 zeroed (a speck that shares a kept pair is at most 2^-301 of an owner's term: far inside the
    bar); the empty quad's clusters are exact zeros; S_k exactly symmetric; no guard word written (sk.folded).  Two launches
    agree bit for bit."""
    sk.feat_shape(DP, DC, K, NP)
    X, q, _, _, _, _ = sk.hard_problem(DP, DC, K, NP)
    ref, absrec = flushed_refs(DP, DC, K, NP)
    got = sk.folded(X, DC, q, K, 2)
    m = sk.low(DP, DC)
    bar = hr.stats_bar(absrec, NP)
    err = np.abs((got.astype(hr.LD) - ref).astype(np.float64))
    print(f"DP={DP} DC={DC} K={K} NP={NP}: max err / bar {np.max(err[:, m] / np.maximum(bar[:, m], hr.TINY)):.3f}")
    assert not np.isnan(got[:, m]).any() and np.all(err[:, m] <= bar[:, m])
    assert q[sk.EMPTY].any(axis=1).all()
    assert sk.exact_equal(got[sk.EMPTY][:, m], np.zeros((4, int(m.sum())))), "the clusters of the quad without an owner are not exact zeros"
    S = got[:, 1 + DP:].reshape(K, DP, DP)[:, :DC, :DC]
    assert sk.same_bits(S, S.transpose(0, 2, 1)), "S_k is not exactly symmetric"
    assert sk.same_bits(sk.folded(X, DC, q, K, 2), got), "two launches differ"


@pytest.mark.parametrize("DP,DC,K", sk.FEAT)
def test_threshold_and_nan_rows_are_placed_with_their_quads(DP, DC, K):
    """Exact X, every row with one owner (never cluster 1 or 10, never a cluster of quad 1), so every batch is sorted.  One
    row's only kept value is exactly 2^-300 on cluster 1: it is placed with quad 0 and its products come out exactly.  One
    row's only kept value is a NaN on cluster 10: it is kept and poisons cluster 10's record alone.  Both rows carry 2^-350 on
    cluster 5, whose quad is never kept: exact zeros."""
    NP = 272
    sk.feat_shape(DP, DC, K, NP)
    X = exact_rows(DP, DC, K, NP)
    rng = np.random.default_rng(5 * DP + DC + K)
    owners = np.array([k for k in range(K) if k not in (1, 4, 5, 6, 7, 10)])
    q = np.zeros((K, NP))
    q[rng.choice(owners, size=NP), np.arange(NP)] = 1.0
    for r, k, v in ((4 * 3 + 1, 1, TAU), (4 * 41 + 2, 10, np.nan)):
        q[:, r] = 0.0
        q[k, r] = v
        q[5, r] = SPECK
    assert np.all(np.array([bin(int(v)).count("1") for v in row_masks(q)]) == 1)
    got = sk.folded(X, DC, q, K, 2)
    m = sk.low(DP, DC)
    ok = np.arange(K) != 10
    ref = hr.stats_ref(X, np.where(np.isnan(q), 0.0, flushed(q)))
    assert sk.exact_equal(got[ok][:, m], ref[ok][:, m])
    assert got[1][0] == TAU and ref[1][0] == TAU and not ref[5].any()
    assert np.isnan(got[10][m]).all()


@pytest.mark.parametrize("DP,DC,K,mode", [(32, 32, 13, "dense"), (64, 64, 8, "dense"), (64, 64, 32, "zero_skip"), (16, 16, 20, "dense")])
def test_mode_two_is_refused_where_mode_one_is(DP, DC, K, mode):
    """the routes without a skipping instance: hipErrorInvalidValue, nothing written"""
    NP = 272
    assert ah.suffstat_plan(DP, DC, NP, K, mode)["route"] != "feat"
    rng = np.random.default_rng(DP + K)
    X = hr.exact_X(rng, NP, DC - 1, DP)
    q = hr.exact_q(rng, K, NP)
    rc, plan, fo, part = sk.run(X, DC, q, K, 2, mode)
    assert rc == ah.HIP_ERROR_INVALID_VALUE and np.all(fo == sk.SENT) and np.all(part == sk.SENT), rc


def test_mode_three_is_no_mode():
    """the hook refuses a flag value past 2 before anything runs"""
    DP, DC, K, NP = 64, 64, 32, 272
    rng = np.random.default_rng(3)
    X = hr.exact_X(rng, NP, DC - 1, DP)
    q = hr.exact_q(rng, K, NP)
    rc, plan, fo, part = sk.run(X, DC, q, K, 3)
    assert rc == -1 and np.all(fo == sk.SENT) and np.all(part == sk.SENT), rc
