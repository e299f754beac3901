"""The list route of a skipping statistics pass (launch_suffstat_list_build + suffstat_list_kernel): per (row
chunk, cluster quad) the ascending list of the rows that keep a value of the quad, one block per list.  Everything goes through
lcx_test_suffstat_lists (bound here) and is compared with tests/stats_lists_ref.py, with lcx_test_suffstat_speck's modes 0, 1
and 2 (tests/test_gpu_stats_speck_skip.py's helpers) and with tests/hot_refs.py; the last tests drive a context."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import aux_hooks as ah
import hot_refs as hr
import stats_lists_ref as sl
import test_gpu_stats_speck_skip as sk

pytestmark = pytest.mark.gpu

TAU = sl.TAU
WIDTHS = [(64, 64), (64, 56)]
KS = [32, 20, 30, 40]  # whole quads; five quads; a last quad of two clusters; ten quads in one launch


@functools.lru_cache(maxsize=None)
def np3(DC, K):
    """the smallest row count (a multiple of 16) at which the plan gives at least three chunks"""
    NP = 288
    while ah.suffstat_plan(64, DC, NP, K, "dense")["nchunks"] < 3:
        NP += 16
    return NP


def rows_of(DC, K):
    return (272, np3(DC, K))


CASES = [(DP, DC, K, big) for DP, DC in WIDTHS for K in KS for big in (False, True)]


def case_rows(DC, K, big):
    return rows_of(DC, K)[1] if big else 272


def lists_hook():
    fn = getattr(ah.hooks(), "lcx_test_suffstat_lists")
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_longlong,
                   C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
    fn.restype = C.c_int
    return fn


def run(X, DC, q, K, sums=True):
    """-> status, plan, folded [K x SS] or None, lens [nchunks x quads], segments [nchunks x quads x chunk_rows] (-7 where
    nothing was written), the partial records' buffer, the folded buffer"""
    X, q = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
    NP, DP = X.shape
    SS = hr.stat_stride(DP)
    plan = ah.suffstat_plan(DP, DC, NP, K, "dense")
    nq = (K + 3) // 4
    part = np.full(plan["nchunks"] * plan["KR"] * SS + 64, sk.SENT)
    fo = np.full(K * SS + 64, sk.SENT)
    lens = np.full(plan["nchunks"] * nq, -7, dtype=np.int32)
    ent = np.full(plan["nchunks"] * nq * plan["chunk_rows"], -7, dtype=np.int32)
    out = np.full(7, -7, dtype=np.int64)
    rc = lists_hook()(X.ctypes.data, DP, DC, NP, q.ctypes.data, K, q.shape[1], int(sums), part.ctypes.data, part.size, int(sums),
                      fo.ctypes.data, fo.size, out.ctypes.data, lens.ctypes.data, lens.size, ent.ctypes.data, ent.size)
    got = None
    if rc == 0 and sums:
        assert np.all(fo[K * SS:] == sk.SENT) and np.all(part[plan["nchunks"] * plan["KR"] * SS:] == sk.SENT), "a guard was written"
        got = fo[:K * SS].reshape(K, SS)
    return rc, plan, got, lens.reshape(plan["nchunks"], nq), ent.reshape(plan["nchunks"], nq, plan["chunk_rows"]), part, fo


def folded(X, DC, q, K):
    rc, plan, got, lens, ent, _, _ = run(X, DC, q, K)
    assert rc == 0 and plan["route"] == "feat", (rc, plan)
    return got


def check_lists(q, plan, lens, ent):
    rlens, rlists = sl.list_rule(q, plan["nchunks"], plan["chunk_rows"])
    assert np.array_equal(lens, rlens), (lens, rlens)
    for i in range(plan["nchunks"]):
        for c in range(lens.shape[1]):
            n = rlens[i, c]
            assert np.array_equal(ent[i, c, :n], rlists[i][c]), (i, c)
            assert np.all(ent[i, c, n:] == -7)


def mixed_q(rng, K, NP):
    """hard rows (sk.hard_q, the clusters of sk.EMPTY exact zeros); every eighth row keeps a second quad; rows 64 ... 95 soft
    in every quad; the last three rows invalid"""
    q = sk.hard_q(rng, K, NP)
    q[sk.EMPTY] = 0.0
    nq = (K + 3) // 4
    for n in range(0, NP - 3, 8):
        own = int(np.argmax(q[:, n])) // 4
        c = (own + 2) % nq
        c = c + 1 if c == 1 else c  # (never the quad without owners)
        q[min(4 * (c % nq), K - 1), n] = 0.25
    soft = rng.dirichlet(np.full(K - 4, 0.5), 32).T
    q[np.setdiff1d(np.arange(K), sk.EMPTY), 64:96] = soft
    q[:, NP - 3:] = 0.0
    return q


@pytest.mark.parametrize("DP,DC,K,big", CASES)
def test_lists_are_those_of_the_rule(DP, DC, K, big):
    """The builder alone, on hard rows, mixed rows and soft rows (every row in every list but for the pad rows): lengths and
    entries equal the numpy rule, nothing is written behind a list's end.  A value of exactly 2^-300 puts its row on the list,
    the next value below does not, a NaN does; the three pad rows are in no list."""
    NP = case_rows(DC, K, big)
    rng = np.random.default_rng(100 * DC + K + NP)
    X = np.zeros((NP, DP))
    hard = sk.hard_q(rng, K, NP)
    hard[sk.EMPTY] = 0.0
    hard[4, 10] = TAU
    hard[5, 21] = np.nextafter(TAU, 0.0)
    hard[6, 33] = np.nan
    soft = rng.dirichlet(np.full(K, 0.3), NP).T.copy()
    soft[:, NP - 3:] = 0.0
    for name, q in (("hard", hard), ("mixed", mixed_q(rng, K, NP)), ("soft", soft)):
        rc, plan, _, lens, ent, part, _ = run(X, DC, q, K, sums=False)
        assert rc == 0 and plan["route"] == "feat" and (not big or plan["nchunks"] >= 3), (name, rc, plan)
        assert np.all(part == sk.SENT)
        check_lists(q, plan, lens, ent)
        listed = {int(i * plan["chunk_rows"] + r) for i in range(plan["nchunks"]) for c in range(lens.shape[1]) for r in ent[i, c, :lens[i, c]]}
        assert not listed & {NP - 3, NP - 2, NP - 1}
        if name == "hard":
            assert 10 in ent[0, 1, :lens[0, 1]] and 33 in ent[0, 1, :lens[0, 1]] and 21 not in ent[0, 1, :lens[0, 1]]
        if name == "soft":
            assert lens.sum() == (NP - 3) * lens.shape[1]


@pytest.mark.parametrize("DP,DC,K,big", CASES)
def test_hard_rows_same_bits_as_the_other_modes(DP, DC, K, big):
    """Hard rows (sk.same_bits_problem): the folded records of the list route equal those of modes 0, 1 and 2 bit for bit, and
    the clusters of the quad without owners -- an empty list in every chunk -- come out as exact zeros."""
    NP = case_rows(DC, K, big)
    sk.feat_shape(DP, DC, K, NP)
    X, q = sk.same_bits_problem(DP, DC, K, NP)
    m = sk.low(DP, DC)
    rc, plan, got, lens, ent, _, _ = run(X, DC, q, K)
    assert rc == 0 and not lens[:, 1].any()
    check_lists(q, plan, lens, ent)
    for mode in (0, 1, 2):
        assert sk.same_bits(got[:, m], sk.folded(X, DC, q, K, mode)[:, m]), mode
    assert sk.exact_equal(got[sk.EMPTY][:, m], np.zeros((4, int(m.sum()))))
    # with the specks of the quad without owners left in place, its lists stay empty and its records exact zeros
    Xh, qh, _, _, _, _ = sk.hard_problem(DP, DC, K, NP)
    assert sk.exact_equal(folded(Xh, DC, qh, K)[sk.EMPTY][:, m], np.zeros((4, int(m.sum()))))


@pytest.mark.parametrize("DP,DC,K,big", CASES)
def test_exact_data_gives_the_exact_sums(DP, DC, K, big):
    """X and the owners' responsibilities powers of two: every product and every sum is exact, and the records equal
    hr.stats_ref of the kept (row, quad) pairs."""
    NP = case_rows(DC, K, big)
    rng = np.random.default_rng(7 * DC + K + NP)
    X = np.zeros((NP, DP))
    X[:, :DC - 1] = rng.choice([-1.0, 1.0], size=(NP, DC - 1)) * 2.0 ** rng.integers(-3, 4, size=(NP, DC - 1))
    X[NP - 3:] = 0.0
    q = np.zeros((K, NP))
    own = rng.integers(0, K, size=NP)
    q[own, np.arange(NP)] = 2.0 ** rng.integers(-4, 1, size=NP)
    q[(own + 8) % K, np.arange(NP)] = 2.0 ** -400  # a speck in another quad: on no list, so never summed
    q[:, NP - 3:] = 0.0
    kept = np.repeat(sl.kept_rows(q), 4, axis=0)[:K]
    m = sk.low(DP, DC)
    assert sk.exact_equal(folded(X, DC, q, K)[:, m], hr.stats_ref(X, np.where(kept, q, 0.0))[:, m])


@pytest.mark.parametrize("DP,DC,K,big", CASES)
def test_mixed_rows_same_bits_as_the_dense_pass(DP, DC, K, big):
    """Every eighth row keeps two quads and a block of rows is soft in all of them (such rows are in several lists): bit-identical
    to mode 0, and within hr.stats_bar of the long-double sums."""
    NP = case_rows(DC, K, big)
    X, _, _, _, _, _ = sk.hard_problem(DP, DC, K, NP)
    q = mixed_q(np.random.default_rng(K + NP), K, NP)
    assert (sl.kept_rows(q).sum(axis=0) > 1).sum() >= NP // 8
    m = sk.low(DP, DC)
    got = folded(X, DC, q, K)
    assert sk.same_bits(got[:, m], sk.folded(X, DC, q, K, 0)[:, m])
    ref = hr.stats_ref(X, q, dtype=hr.LD)
    bar = hr.stats_bar(hr.stats_abs(X, q), NP)
    err = np.abs((got.astype(hr.LD) - ref).astype(np.float64))
    print(f"DC={DC} K={K} NP={NP}: max err / bar {np.max(err[:, m] / np.maximum(bar[:, m], hr.TINY)):.3f}")
    assert np.all(err[:, m] <= bar[:, m])


@pytest.mark.parametrize("DP,DC,K", [(64, 64, 32), (64, 56, 30)])
def test_list_lengths(DP, DC, K):
    """Three chunks or more.  Quad 0: one row in the first chunk, none in the second (an empty list in the middle), 49 in the
    third (one past a staged batch); quad 2: 5, 51 and 97 rows (no multiple of 4 or of the batch); the last quad: every
    other valid row.  The last three rows invalid.  Exact data: the exact sums."""
    NP = np3(DC, K)
    plan = ah.suffstat_plan(DP, DC, NP, K, "dense")
    R, nq = plan["chunk_rows"], (K + 3) // 4
    assert plan["nchunks"] >= 3 and R >= 97 + 51
    rng = np.random.default_rng(K)
    valid = np.arange(NP) < NP - 3
    X = hr.exact_X(rng, NP, DC - 1, DP, valid)
    q = np.zeros((K, NP))
    q[1, 7] = 0.5
    q[2, 2 * R + 3:2 * R + 3 + 49] = 0.25
    q[9, 11:16] = 1.0
    q[8, R + 1:R + 1 + 51] = 0.5
    q[10, 2 * R:2 * R + 97] = 2.0
    q[K - 1, 1::2] = 1.0
    q[:, ~valid] = 0.0
    rc, plan, got, lens, ent, _, _ = run(X, DC, q, K)
    assert rc == 0
    check_lists(q, plan, lens, ent)
    assert lens[:3, 0].tolist() == [1, 0, 49] and lens[:3, 2].tolist() == [5, 51, 97] and lens[0, nq - 1] == R // 2
    m = sk.low(DP, DC)
    assert sk.exact_equal(got[:, m], hr.stats_ref(X, q)[:, m])


@pytest.mark.parametrize("DP,DC,K", [(64, 64, 32), (64, 56, 20)])
def test_nan_poisons_what_it_poisons_in_mode_1(DP, DC, K):
    NP = 272
    X, q = sk.same_bits_problem(DP, DC, K, NP)
    q = q.copy()
    q[9, 40] = np.nan
    m = sk.low(DP, DC)
    got, ref = folded(X, DC, q, K), sk.folded(X, DC, q, K, 1)
    assert np.array_equal(np.isnan(got[:, m]), np.isnan(ref[:, m])) and np.isnan(got[9][m]).all()
    assert not np.isnan(np.delete(got, 9, axis=0)[:, m]).any()
    assert sk.same_bits(np.delete(got, 9, axis=0)[:, m], np.delete(ref, 9, axis=0)[:, m])


def test_two_launches_give_the_same_bits():
    DP, DC, K = 64, 64, 32
    NP = np3(DC, K)
    X, _, _, _, _, _ = sk.hard_problem(DP, DC, K, NP)
    q = mixed_q(np.random.default_rng(3), K, NP)
    a, b = run(X, DC, q, K), run(X, DC, q, K)
    assert a[0] == 0 and b[0] == 0
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and sk.same_bits(a[5], b[5]) and sk.same_bits(a[2], b[2])


@pytest.mark.parametrize("DP,DC,K", [(32, 32, 20), (96, 96, 29), (64, 64, 8), (128, 128, 64)])
def test_widths_without_an_instance_are_refused(DP, DC, K):
    """the feature GEMM's other widths and a shape on another route: hipErrorInvalidValue from both launchers, nothing written"""
    NP = 272
    rng = np.random.default_rng(DP + K)
    X = hr.exact_X(rng, NP, DC - 1, DP)
    q = hr.exact_q(rng, K, NP)
    for sums in (False, True):
        rc, plan, _, lens, ent, part, fo = run(X, DC, q, K, sums=sums)
        assert rc == ah.HIP_ERROR_INVALID_VALUE, (rc, plan)
        assert np.all(part == sk.SENT) and np.all(fo == sk.SENT) and np.all(lens == -7) and np.all(ent == -7)


def test_context_takes_the_list_route_on_hard_rows_only():
    """N = 8192, D = 64: hard rows take the list route (K = 32 and K = 20); the quarter / soft / less constructions of
    test_probe_sends_soft_passes_to_the_dense_kernel do not, and count as they did; with the setter off nothing does.  The
    statistics equal those of the pass with the setter off, bit for bit, in every case."""
    from libcluster_amd import capi

    N, D = 8192, 64
    rng = np.random.default_rng(99)

    def constructions(K):
        X = rng.normal(size=(N, D)) + rng.integers(0, K, (N, 1))
        soft = rng.dirichlet(np.full(K, 0.3), N)
        hard = 2.0 ** -rng.uniform(301.0, 1000.0, size=(N, K))
        hard[np.arange(N), np.arange(N) % K] = 1.0
        quarter = soft.copy()
        quarter[:, :8] = 0.0
        less = quarter.copy()
        less[0, 0] = 0.5
        return X, {"soft": soft, "hard": hard, "quarter": quarter, "less": less}

    expect = {"soft": ((0, 1), 0), "hard": ((1, 0), 1), "quarter": ((1, 0), 0), "less": ((0, 1), 0)}
    for K, names in ((32, ("soft", "hard", "quarter", "less")), (20, ("hard",))):
        assert ah.suffstat_plan(64, 64, N, K, "dense")["route"] == "feat"
        X, qs = constructions(K)
        for name in names:
            out = []
            for on in (True, False):
                with capi.Context(0) as ctx:
                    ctx.set_speck_skip(on)
                    ctx.set_data(X)
                    ctx.set_qz(qs[name])
                    out.append(ctx.suffstat()[:3])
                    want = expect[name] if on else ((0, 0), 0)
                    assert (ctx.speck_passes(), ctx.speck_list_passes()) == want, (K, name, on, ctx.speck_passes(), ctx.speck_list_passes())
            for u, v in zip(*out):
                assert sk.same_bits(u, v), (K, name)
