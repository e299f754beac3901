"""The owner kernel of the statistics pass's list route (suffstat_owner_kernel): at DC = 64 a list is summed by
one wave per cluster of the quad, a listed row going into a cluster only where that cluster's own q is kept (not below
2^-300), the products on the VALU in fto_feature's diagonals (tests/test_stats_owner_deal.py has the map).  Everything goes
through lcx_test_suffstat_lists as tests/test_gpu_stats_lists.py binds it; the references are hr.stats_ref on exact data and
the dense MFMA pass (sk.folded, mode 0) for the bits; the last test drives a context."""
from __future__ import annotations

import sys

import numpy as np
import pytest

import aux_hooks as ah
import hot_refs as hr
import test_gpu_stats_lists as tl
import test_gpu_stats_speck_skip as sk

pytestmark = pytest.mark.gpu

TAU = sk.TAU
DP = DC = 64
KS = [32, 30, 20]  # whole quads; a last quad of two clusters; five quads
DEPTH = 4          # LC_FTO_DEPTH: the rows of a group the kernel keeps in flight
NP = 1040          # five chunks of 224 rows (asserted: three or more, no multiple of 64), the last three rows invalid


def plan_of(K):
    p = ah.suffstat_plan(DP, DC, NP, K, "dense")
    assert p["route"] == "feat" and p["nchunks"] >= 3 and p["chunk_rows"] % 64 != 0 and p["chunk_rows"] >= 130, p
    return p


def exact_rows(rng):
    """+-2^e in EVERY column (a wrong column in the wrap of the doubled row changes a sum), the last three rows zero"""
    X = rng.choice([-1.0, 1.0], size=(NP, DP)) * 2.0 ** rng.integers(-3, 4, size=(NP, DP))
    X[NP - 3:] = 0.0
    return X


def kept_q(q):
    """the rule: a (row, cluster) pair is summed unless q < 2^-300 (a NaN is summed)"""
    with np.errstate(invalid="ignore"):
        return np.where(q < TAU, 0.0, q)


def check_exact(X, q, K):
    rc, plan, got, lens, ent, _, _ = tl.run(X, DC, q, K)
    assert rc == 0 and plan["route"] == "feat", (rc, plan)
    tl.check_lists(q, plan, lens, ent)
    assert sk.exact_equal(got, hr.stats_ref(X, kept_q(q)))
    S = got[:, 1 + DP:].reshape(K, DP, DP)
    assert sk.same_bits(S, S.transpose(0, 2, 1)), "S_k is not exactly symmetric"
    return plan, got, lens


@pytest.mark.parametrize("K", KS)
def test_exact_data_gives_the_exact_sums_of_the_kept_pairs(K):
    """X = +-2^e in all 64 columns, q powers of two: one owner per row, every fifth row a second kept cluster (any quad), a
    speck of 2^-400 in a third cluster of the OWNER'S quad (its row is listed, the speck is not summed).  exact_equal to
    hr.stats_ref of the kept (row, cluster) pairs."""
    plan_of(K)
    rng = np.random.default_rng(11 + K)
    X = exact_rows(rng)
    n = np.arange(NP)
    q = np.zeros((K, NP))
    own = rng.integers(0, K, size=NP)
    q[own, n] = 2.0 ** rng.integers(-4, 1, size=NP)
    second = (own + rng.integers(1, K, size=NP)) % K
    q[second[::5], n[::5]] = 2.0 ** rng.integers(-4, 1, size=n[::5].size)
    speck = 4 * (own // 4) + (own + 1) % 4
    ok = (speck < K) & (q[np.minimum(speck, K - 1), n] == 0.0)
    q[speck[ok], n[ok]] = 2.0 ** -400
    q[:, NP - 3:] = 0.0
    check_exact(X, q, K)


@pytest.mark.parametrize("K", KS)
def test_list_lengths_and_waves_that_find_nothing(K):
    """One launch, three chunks or more of 224 rows.  Lists of 0, 1, 63, 64, 65, 127 and 129 rows (a window is 64 places); a
    quad whose listed rows all belong to one cluster (three waves find nothing and store exact zeros); clusters 1, 5, ...
    without a kept row in the middle chunk while their quads are listed there."""
    plan = plan_of(K)
    R, nq = plan["chunk_rows"], (K + 3) // 4
    rng = np.random.default_rng(23 + K)
    X = exact_rows(rng)
    q = np.zeros((K, NP))
    want = np.zeros((plan["nchunks"], nq), dtype=np.int64)
    lengths = [0, 1, 63, 64, 65, 127, 129, 63, 64, 130, 7, 66, 5, 128, 33]
    for j, n in enumerate(lengths[:3 * nq]):
        i, c = j % 3, j // 3
        want[i, c] = n
        rows = i * R + np.sort(rng.permutation(R)[:n])
        width = min(4, K - 4 * c)
        if j == 7:  # (chunk 1, quad 2): every listed row is cluster 8's
            cl = np.zeros(n, dtype=np.int64)
        elif i == 1:  # the middle chunk: never the quad's second cluster
            cl = rng.choice([w for w in range(width) if w != 1], size=n)
        else:
            cl = rng.integers(0, width, size=n)
        q[4 * c + cl, rows] = 2.0 ** rng.integers(-4, 1, size=n)
    assert q[8, R:2 * R].any() and not q[9:12, R:2 * R].any() and not q[1, R:2 * R].any() and q[1].any()
    _, got, lens = check_exact(X, q, K)
    assert np.array_equal(lens[:3], want[:3]) and not lens[3:].any()


@pytest.mark.parametrize("K", KS)
def test_own_row_counts_around_the_depth_in_flight(K):
    """Within one window a wave takes its rows in groups of DEPTH: clusters with 0, 1, DEPTH - 1, DEPTH, DEPTH + 1 and
    2 DEPTH + 1 rows of their own in a list of fewer than 64 rows, and the same counts once more spread over two windows."""
    plan = plan_of(K)
    R = plan["chunk_rows"]
    counts = [0, 1, DEPTH - 1, DEPTH, DEPTH + 1, 2 * DEPTH + 1, 2 * DEPTH, 3 * DEPTH + 2]
    rng = np.random.default_rng(37 + K)
    X = exact_rows(rng)
    q = np.zeros((K, NP))
    for i, (c0, filler) in enumerate(((0, 0), (2, 70))):  # chunk i: quads c0 and c0 + 1 carry the counts
        for c in (c0, c0 + 1):
            mine = counts[4 * (c - c0):4 * (c - c0) + 4]
            cl = np.repeat(np.arange(4), mine)
            if filler:  # rows that belong to the quad's first cluster push the others' rows into the second window
                cl = np.concatenate([np.zeros(filler, dtype=np.int64), cl])
            rng.shuffle(cl)
            rows = i * R + np.sort(rng.permutation(R)[:cl.size])
            q[4 * c + cl, rows] = 2.0 ** rng.integers(-4, 1, size=cl.size)
    assert (q[:16] > 0).sum(axis=1).tolist()[:8] == counts
    _, _, lens = check_exact(X, q, K)
    assert lens[0, 0] == sum(counts[:4]) < 64 and lens[1, 3] == sum(counts[4:]) + 70 > 64


@pytest.mark.parametrize("K", KS)
def test_rows_kept_by_several_clusters_of_one_quad(K):
    """rows kept by two, three and four clusters of quad 0 (and, at K = 30, by both clusters of the ragged last quad) next to
    rows with one owner: every wave that keeps the row sums it, with its own q"""
    plan_of(K)
    rng = np.random.default_rng(41 + K)
    X = exact_rows(rng)
    n = np.arange(NP - 3)
    q = np.zeros((K, NP))
    q[rng.integers(0, K, size=n.size), n] = 2.0 ** rng.integers(-4, 1, size=n.size)
    for m, first in ((2, 3), (3, 5), (4, 7)):
        rows = n[first::11]
        for c in rng.permutation(4)[:m]:
            q[c, rows] = 2.0 ** rng.integers(-4, 1, size=rows.size)
    last = 4 * ((K - 1) // 4)
    q[last:K, n[9::13]] = 0.5
    several = (kept_q(q)[:4] != 0).sum(axis=0)
    assert {2, 3, 4} <= set(several.tolist())
    check_exact(X, q, K)


@pytest.mark.parametrize("K", KS)
def test_boundary_values_and_nans(K):
    """q = 2^-300 is summed, the value just below and -0.0 are not, although their rows are on the quad's list (a neighbour
    cluster keeps them).  A NaN q poisons its own cluster's record and nothing else; a NaN in X poisons, in exactly the
    clusters that keep its row, the features of its column and nothing else."""
    plan = plan_of(K)
    R = plan["chunk_rows"]
    rng = np.random.default_rng(53 + K)
    X = exact_rows(rng)
    q = np.zeros((K, NP))
    n = np.arange(NP - 3)
    own = 12 + rng.integers(0, K - 12, size=n.size)  # clusters 0 ... 11 hold only what is placed below
    q[own, n] = 2.0 ** rng.integers(-4, 1, size=n.size)
    q[:12] = 0.0
    under = np.nextafter(TAU, 0.0)
    q[0, 10], q[1, 10] = TAU, 1.0          # cluster 0: the one term 2^-300 x x^T, exact
    q[2, 75], q[1, 75] = under, 0.5        # cluster 2: nothing
    q[3, R + 5], q[1, R + 5] = -0.0, 0.25  # cluster 3: nothing
    q[5, 2 * R + 9], q[4, 2 * R + 9] = np.nan, 1.0
    q[4, 33] = 0.5
    xrow, xcol = R + 77, 41                # kept by clusters 8 and 10, listed for quad 2; cluster 9 holds a speck there
    q[:, xrow] = 0.0
    q[8, xrow], q[9, xrow], q[10, xrow] = 0.5, 2.0 ** -301, 1.0
    q[9, 50] = 1.0
    Xn = X.copy()
    Xn[xrow, xcol] = np.nan
    rc, plan, got, lens, ent, _, _ = tl.run(Xn, DC, q, K)
    assert rc == 0
    tl.check_lists(q, plan, lens, ent)
    qk = kept_q(q)
    qk[5] = 0.0
    qx = qk.copy()
    qx[:, xrow] = 0.0
    ref, ref_row = hr.stats_ref(X, qx), hr.stats_ref(X, qk)
    hit = np.zeros(hr.stat_stride(DP), dtype=bool)  # the features of column xcol
    hit[1 + xcol] = True
    Sm = np.zeros((DP, DP), dtype=bool)
    Sm[xcol, :] = Sm[:, xcol] = True
    hit[1 + DP:] = Sm.reshape(-1)
    for k in range(K):
        if k == 5:
            assert np.isnan(got[k]).all()
        elif k in (8, 10):
            assert np.isnan(got[k][hit]).all() and sk.exact_equal(got[k][~hit], ref_row[k][~hit]), k
        else:
            assert sk.exact_equal(got[k], ref[k]), k
    assert got[0, 0] == TAU and not got[2].any() and not got[3].any() and got[9, 0] == 1.0


@pytest.mark.parametrize("K", KS)
def test_hard_and_mixed_rows_same_bits_as_the_dense_pass(K):
    """The hard construction of tests/test_gpu_stats_speck_skip.py (one owner per row, specks of 2^-301 ... 2^-1000 in the other
    clusters, listed rows' specks among them) and the mixed one of tests/test_gpu_stats_lists.py (soft, non-power-of-two q;
    rows on several lists) on continuous X: bit-identical to the dense MFMA pass, and two launches give the same bits."""
    NPB = tl.np3(DC, K)
    X, q = sk.same_bits_problem(DP, DC, K, NPB)
    got = tl.folded(X, DC, q, K)
    assert sk.same_bits(got, sk.folded(X, DC, q, K, 0))
    assert sk.exact_equal(got[sk.EMPTY], np.zeros((4, hr.stat_stride(DP))))
    qm = tl.mixed_q(np.random.default_rng(K + NPB), K, NPB)
    a, b = tl.run(X, DC, qm, K), tl.run(X, DC, qm, K)
    assert a[0] == 0 and b[0] == 0 and a[1]["nchunks"] >= 3
    assert sk.same_bits(a[2], sk.folded(X, DC, qm, K, 0))
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and sk.same_bits(a[5], b[5]) and sk.same_bits(a[2], b[2])


def test_context_three_iterations_from_hard_rows_same_bits():
    """N = 8192, D = 64, K = 32, bench.py's separated mixture from hard labels, three fixed VBEM iterations with the kept-quad
    masks on: F, the trace and the three statistics arrays equal those of a context with set_speck_skip(False) bit for bit; the
    passes that skip are list passes, all but at most the first built from masks, and none is with the setter off."""
    sys.path.insert(0, str(ah.ROOT))
    import bench
    from libcluster_amd import capi

    N, D, K = 8192, 64, 32
    assert ah.suffstat_plan(64, 64, N, K, "dense")["route"] == "feat"
    mu, L = bench.mixture(D, K, 1004)
    res = []
    for on in (True, False):
        with capi.Context(0) as ctx:
            ctx.set_speck_skip(on)
            ctx.set_estep_masks(True)
            ctx.synth(N, D, K, mu, L, 1004, 0, 1.0)
            F, tr, mdl = ctx.vbem(capi.W_DIRICHLET, fixed_iters=3)
            mdl.close()
            stats = ctx.suffstat()[:3]
            lists, masks = ctx.speck_list_passes(), ctx.speck_mask_passes()
            print(f"skip {'on' if on else 'off'}: speck passes {ctx.speck_passes()}, list passes {lists}, built from masks {masks}")
            if on:
                assert lists >= 3 and lists - 1 <= masks <= lists, (lists, masks)
            else:
                assert (lists, masks) == (0, 0)
            res.append([np.array([F]), np.asarray(tr)] + [np.asarray(s, dtype=np.float64) for s in stats])
    for u, v in zip(*res):
        assert u.shape == v.shape and sk.same_bits(u, v)


def test_chunks_of_more_than_65536_rows_have_32_bit_entries():
    """lcx_test_suffstat_lists_chunked (bound here) with 65568 rows per chunk, three chunks, K = 20: the segments hold 32-bit
    offsets (the other instance of the kernel).  A few hundred listed rows, most of them beyond offset 65535 of their chunk;
    exact data: lists by the rule, the exact sums of the kept pairs."""
    import ctypes as C

    import stats_lists_ref as sl

    K, R, nch = 20, 65568, 3
    NPW, nq, SS = nch * R, 5, hr.stat_stride(DP)
    fn = getattr(ah.hooks(), "lcx_test_suffstat_lists_chunked")
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.c_longlong,
                   C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
    fn.restype = C.c_int
    rng = np.random.default_rng(65568)
    X = rng.choice([-1.0, 1.0], size=(NPW, DP)) * 2.0 ** rng.integers(-3, 4, size=(NPW, DP))
    X[NPW - 3:] = 0.0
    q = np.zeros((K, NPW))
    rows = np.concatenate([i * R + np.concatenate([rng.permutation(300)[:40], 65536 + rng.permutation(R - 65536 - 3)[:25],
                                                   65000 + rng.permutation(536)[:150]]) for i in range(nch)])
    own = rng.integers(0, K, size=rows.size)
    q[own, rows] = 2.0 ** rng.integers(-4, 1, size=rows.size)
    q[(own[::3] + 1) % K, rows[::3]] = 2.0 ** rng.integers(-4, 1, size=rows[::3].size)
    q[(own[::4] + 2) % K, rows[::4]] = 2.0 ** -400
    part = np.full(nch * K * SS + 64, sk.SENT)
    fo = np.full(K * SS + 64, sk.SENT)
    lens = np.full(nch * nq, -7, dtype=np.int32)
    ent = np.full(nch * nq * R, -7, dtype=np.int32)
    out = np.full(7, -7, dtype=np.int64)
    rc = fn(X.ctypes.data, DP, DC, NPW, q.ctypes.data, K, NPW, R, part.ctypes.data, part.size, fo.ctypes.data, fo.size,
            out.ctypes.data, lens.ctypes.data, lens.size, ent.ctypes.data, ent.size)
    assert rc == 0 and out[1] == nch and out[2] == R, (rc, out)
    assert np.all(fo[K * SS:] == sk.SENT) and np.all(part[nch * K * SS:] == sk.SENT), "a guard was written"
    lens, ent = lens.reshape(nch, nq), ent.reshape(nch, nq, R)
    rlens, rlists = sl.list_rule(q, nch, R)
    assert np.array_equal(lens, rlens) and ent.max() > 65535
    for i in range(nch):
        for c in range(nq):
            assert np.array_equal(ent[i, c, :rlens[i, c]], rlists[i][c]), (i, c)
    listed = np.unique(rows)
    ref = hr.stats_ref(X[listed], kept_q(q)[:, listed])
    assert sk.exact_equal(fo[:K * SS].reshape(K, SS), ref)
