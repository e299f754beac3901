"""The list kernel's step schedule (suffstat_list_kernel, DESIGN 4.2b: the next step's fragment reads go out behind this
step's MFMAs) on the list lengths at which such a schedule can go wrong.  A staged batch is 48 list rows = 12 steps, a
trip of the kernel's loop two batches (buffer 0, buffer 1).  One quad's list gets, in consecutive row chunks, the lengths
47, 48, 52 (one step short of a batch, exactly one, one step into the second buffer), 95, 96, 100 (the same around a
whole trip), 144 (three batches: the loop leaves after buffer 0), 192 and 193; the last quad takes every other valid row
of every chunk; the last three rows are invalid.  Everything goes through lcx_test_suffstat_lists and the helpers of
tests/test_gpu_stats_lists.py."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import aux_hooks as ah
import hot_refs as hr
import test_gpu_stats_lists as tl
import test_gpu_stats_speck_skip as sk

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 32), (64, 56, 30)]
LENGTHS = [47, 48, 52, 95, 96, 100, 144, 192, 193]
QUAD = 2  # the quad whose lists have LENGTHS (clusters 8 ... 11)


@functools.lru_cache(maxsize=None)
def rows_for(DC, K):
    """the smallest row count (a multiple of 16) whose plan has a chunk per length, each long enough for its list"""
    NP = 16 * (sum(LENGTHS) // 16)
    while True:
        plan = ah.suffstat_plan(64, DC, NP, K, "dense")
        R = plan["chunk_rows"]
        if plan["nchunks"] >= len(LENGTHS) and all(i * R + 1 + n <= NP - 3 for i, n in enumerate(LENGTHS)):
            return NP
        NP += 16
        assert NP < 16384


def owners(DC, K):
    """-> NP, plan, [(rows, cluster)]: chunk i's LENGTHS[i] consecutive rows from its second row on, their owners walking
    through QUAD's four clusters; every other valid row for the last cluster"""
    NP = rows_for(DC, K)
    plan = ah.suffstat_plan(64, DC, NP, K, "dense")
    R = plan["chunk_rows"]
    assert plan["route"] == "feat" and 200 <= R <= 1024, plan  # (a few hundred rows per chunk)
    rows = np.concatenate([i * R + 1 + np.arange(n) for i, n in enumerate(LENGTHS)])
    return NP, plan, rows, 4 * QUAD + rows % 4


def check_lengths(DC, K, q, plan, lens, ent):
    tl.check_lists(q, plan, lens, ent)
    nq, R, NP = (K + 3) // 4, plan["chunk_rows"], q.shape[1]
    assert lens[:len(LENGTHS), QUAD].tolist() == LENGTHS and not lens[len(LENGTHS):, QUAD].any()
    for i in range(plan["nchunks"]):
        r = np.arange(i * R, min((i + 1) * R, NP - 3))
        assert lens[i, nq - 1] == (r % 2 == 1).sum()
    assert lens[0, nq - 1] > 96  # (more than one trip)
    others = np.setdiff1d(np.arange(nq), [QUAD, nq - 1])
    assert not lens[:, others].any()


@functools.lru_cache(maxsize=None)
def exact_case(DP, DC, K):
    NP, plan, rows, own = owners(DC, K)
    rng = np.random.default_rng(31 * DC + K)
    valid = np.arange(NP) < NP - 3
    X = hr.exact_X(rng, NP, DC - 1, DP, valid)
    q = np.zeros((K, NP))
    q[own, rows] = 2.0 ** -(rows % 3).astype(np.float64)
    q[K - 1, 1::2] = 1.0
    q[:, ~valid] = 0.0
    return X, q


@functools.lru_cache(maxsize=None)
def split_case(DP, DC, K):
    """continuous X; a listed row's responsibility r in (0.5, 1) is no power of two and 1 - r goes to another cluster of the
    same quad, so all four q of a step's quad are in use and nothing is exact"""
    NP, plan, rows, own = owners(DC, K)
    rng = np.random.default_rng(57 * DC + K)
    X = np.zeros((NP, DP))
    X[:, :DC] = rng.normal(size=(NP, DC))
    q = np.zeros((K, NP))
    r = rng.uniform(0.5, 1.0, size=rows.size)
    q[own, rows] = r
    q[4 * QUAD + (own + 1 + rng.integers(0, 3, size=rows.size)) % 4, rows] = 1.0 - r
    odd = np.arange(1, NP, 2)
    r = rng.uniform(0.5, 1.0, size=odd.size)
    q[K - 1, odd] = r
    q[K - 2, odd] = 1.0 - r
    q[:, NP - 3:] = 0.0
    assert not ((q > 0.0) & (q < sk.TAU)).any()
    return X, q


@functools.lru_cache(maxsize=None)
def launched(kind, DP, DC, K):
    X, q = (exact_case if kind == "exact" else split_case)(DP, DC, K)
    out = tl.run(X, DC, q, K)  # (tl.run asserts the guards behind both buffers)
    assert out[0] == 0, out[0]
    return out


@pytest.mark.parametrize("DP,DC,K", SHAPES)
def test_exact_data_gives_the_exact_sums_at_every_length(DP, DC, K):
    """X and q powers of two: every product and every sum is exact, and the folded records equal hr.stats_ref on the low
    triangle -- a step whose fragments were read from the wrong buffer, too early or not at all shows here."""
    X, q = exact_case(DP, DC, K)
    rc, plan, got, lens, ent, _, _ = launched("exact", DP, DC, K)
    check_lengths(DC, K, q, plan, lens, ent)
    m = sk.low(DP, DC)
    assert sk.exact_equal(got[:, m], hr.stats_ref(X, q)[:, m])


@pytest.mark.parametrize("DP,DC,K", SHAPES)
def test_split_rows_same_bits_as_the_dense_pass_at_every_length(DP, DC, K):
    """Continuous data, responsibilities split inside a quad: the same bits as the dense pass (lcx_test_suffstat_speck,
    mode 0), S exactly symmetric, no NaN."""
    X, q = split_case(DP, DC, K)
    rc, plan, got, lens, ent, _, _ = launched("split", DP, DC, K)
    check_lengths(DC, K, q, plan, lens, ent)
    m = sk.low(DP, DC)
    ref = sk.folded(X, DC, q, K, 0)
    assert sk.same_bits(got[:, m], ref[:, m])
    S = got[:, 1 + DP:].reshape(K, DP, DP)[:, :DC, :DC]
    assert sk.same_bits(S, np.ascontiguousarray(S.transpose(0, 2, 1)))
    assert not np.isnan(got[:, m]).any()
    assert np.all(got[4 * QUAD:4 * QUAD + 4, 0] > 0.0) and np.all(got[K - 2:, 0] > 0.0)


@pytest.mark.parametrize("DP,DC,K", SHAPES)
def test_two_launches_give_the_same_bits_at_every_length(DP, DC, K):
    X, q = split_case(DP, DC, K)
    a = launched("split", DP, DC, K)
    b = tl.run(X, DC, q, K)
    assert b[0] == 0
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and sk.same_bits(a[5], b[5]) and sk.same_bits(a[2], b[2])
