"""Speck skipping in the feature-GEMM statistics pass (suffstat_feat_kernel<..., SPECK>): a (4-row step,
cluster quad) pair issues no MFMA when all sixteen of its responsibilities are below 2^-300.  Everything goes through the
test hooks (tests/aux_hooks.py; the entry point that takes the flag explicitly, lcx_test_suffstat_speck, is bound here) and
tests/hot_refs.py.

The rule, restated in numpy (speck_rule): quads are the clusters 4 c ... 4 c + 3, steps the rows 4 s ... 4 s + 3 (row chunks
and cluster ranges start at multiples of 32, so both are aligned globally); a pair is KEPT when not every value satisfies
q < TAU -- a NaN is kept."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import aux_hooks as ah
import hot_refs as hr

pytestmark = pytest.mark.gpu

TAU = 2.0 ** -300
SENT = -7.25e300  # (no sum of the cases comes near it)
#          DP   DC   K    the path the shape reaches (the plan's route is asserted in feat_shape)
SHAPES = [(64, 64, 32),     # grouped path, 8 waves, uneven deal
          (64, 56, 20),     # active width, 5 quads
          (32, 32, 13),     # the few-cluster (quad) kernel owns this shape: no skipping instance, the flag is refused
          (32, 32, 20),     # ungrouped path, 4 waves
          (96, 96, 29),     # grouped path at 96
          (128, 128, 64)]   # 16 quads, one set of q quads
FEAT = [s for s in SHAPES if s != (32, 32, 13)]
NPS = (272, 1040)  # several staged batches with a ragged last one; at least two row chunks (asserted)


def speck_hook():
    fn = getattr(ah.hooks(), "lcx_test_suffstat_speck")
    fn.argtypes = ah.PROTOTYPES["lc_test_suffstat"] + [C.c_int]
    fn.restype = C.c_int
    return fn


def run(X, DC, q, K, speck, mode="dense"):
    """one dense pass with the flag given -> status, route, folded [K x SS] (guards checked), partial records"""
    X, q = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(q, dtype=np.float64)
    NP, DP = X.shape
    SS = hr.stat_stride(DP)
    plan = ah.suffstat_plan(DP, DC, NP, K, mode)
    nrec = plan["nchunks"] * plan["KR"]
    part = np.full(nrec * SS + 64, SENT)
    fo = np.full(K * SS + 64, SENT)
    out = np.full(7, -7, dtype=np.int64)
    rc = speck_hook()(X.ctypes.data, DP, DC, NP, q.ctypes.data, K, q.shape[1], ah.SS_MODES.index(mode), None, None, 0, 0, None, None,
                      None, None, None, None, 0, 0, 0, part.ctypes.data, part.size, 1, fo.ctypes.data, fo.size, out.ctypes.data,
                      int(speck))
    return rc, plan, fo, part


def folded(X, DC, q, K, speck):
    rc, plan, fo, part = run(X, DC, q, K, speck)
    assert rc == 0 and plan["route"] == "feat", (rc, plan)
    SS = hr.stat_stride(X.shape[1])
    assert np.all(fo[K * SS:] == SENT) and np.all(part[plan["nchunks"] * plan["KR"] * SS:] == SENT), "a guard was written"
    return fo[:K * SS].reshape(K, SS)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def exact_equal(got, ref):
    got, ref = np.asarray(got), np.asarray(ref, dtype=np.float64)
    return got.shape == ref.shape and not np.isnan(got).any() and np.array_equal(got, ref)


def low(DP, DC):
    """what the host reads and the mirror image above the diagonal: everything but the idle columns (never written)"""
    s_idle, S_idle, _ = hr.region_masks(DP, DC)
    return ~(s_idle | S_idle)


def speck_rule(q):
    """q' = q with the skipped pairs zeroed"""
    K, NP = q.shape
    K4 = -(-K // 4) * 4
    qq = np.zeros((K4, NP))
    qq[:K] = q
    with np.errstate(invalid="ignore"):
        below = (qq < TAU).reshape(K4 // 4, 4, NP // 4, 4)
    kept = ~below.all(axis=(1, 3))  # [quad][step]
    return np.where(np.repeat(np.repeat(kept, 4, axis=0), 4, axis=1)[:K], q, 0.0), kept


EMPTY = np.arange(4, 8)  # the clusters of quad 1 own no row in the hard problems


def hard_q(rng, K, NP):
    """one owner per valid row (q = 1.0; random, never a cluster of EMPTY, every other cluster at least once); the others
    log-uniform in 2^-1000 ... 2^-301, one in eight exactly 0.0; the last three rows invalid"""
    q = 2.0 ** -rng.uniform(301.0, 1000.0, size=(K, NP))
    q[rng.random((K, NP)) < 0.125] = 0.0
    own = rng.integers(0, K - 4, size=NP)
    own[rng.permutation(NP - 3)[:K - 4]] = np.arange(K - 4)
    own[own >= 4] += 4
    q[own, np.arange(NP)] = 1.0
    q[:, NP - 3:] = 0.0
    return q


@functools.lru_cache(maxsize=None)
def hard_problem(DP, DC, K, NP):
    """X (continuous: hr.rounding_problem), q (hard rows), q', the long-double sums of q' and the sums of absolute values
    (the scale of hr.stats_bar) -- computed once per shape"""
    rng = np.random.default_rng(7000 + DP * 100 + DC + K + NP)
    valid = np.arange(NP) < NP - 3
    X, _, _, _ = hr.rounding_problem(rng, K, DC - 1, NP, DP, valid)
    q = hard_q(rng, K, NP)
    qs, kept = speck_rule(q)
    ref = np.zeros((K, hr.stat_stride(DP)), dtype=hr.LD)
    absrec = np.zeros((K, hr.stat_stride(DP)))
    for k in range(K):  # (over the rows that q' leaves a cluster)
        rows = np.nonzero(qs[k])[0]
        if rows.size:
            ref[k] = hr.stats_ref(X[rows], qs[k:k + 1, rows], dtype=hr.LD)[0]
            absrec[k] = hr.stats_abs(X[rows], qs[k:k + 1, rows])[0]
    for a in (X, q, qs, ref, absrec):
        a.setflags(write=False)
    return X, q, qs, kept, ref, absrec


def same_bits_problem(DP, DC, K, NP):
    """X and q of hard_problem with the columns of the clusters that own no row set to exact zeros"""
    X, q, _, _, _, _ = hard_problem(DP, DC, K, NP)
    q = q.copy()
    q[EMPTY] = 0.0
    return X, q


def feat_shape(DP, DC, K, NP):
    p = ah.suffstat_plan(DP, DC, NP, K, "dense")
    assert p["route"] == "feat" and p["name"] == "suffstat_feat_kernel", p
    assert NP < 1000 or p["nchunks"] >= 2, p
    return p


@pytest.mark.parametrize("NP", NPS)
@pytest.mark.parametrize("DP,DC,K", FEAT)
def test_hard_rows_sum_to_the_kept_pairs(DP, DC, K, NP):
    """Hard rows, flag on: the folded result lies within hr.stats_bar of the long-double sums of q' (q with the skipped pairs
    zeroed by the rule, in numpy); the clusters of the quad that owns no row anywhere (EMPTY: nothing but specks in any of its
    pairs -- a cluster without rows whose quad has owners keeps the specks of the kept pairs, as the rule says) come out as
    exact zeros.  A step has one to four kept quads (owners are random), and most pairs are skipped."""
    feat_shape(DP, DC, K, NP)
    X, q, qs, kept, ref, absrec = hard_problem(DP, DC, K, NP)
    nq = kept.sum(axis=0)[: (NP - 3) // 4]
    assert nq.min() >= 1 and nq.max() <= 4 and kept.mean() < 0.75
    got = folded(X, DC, q, K, 1)
    m = low(DP, DC)
    bar = hr.stats_bar(absrec, NP)
    err = np.abs((got.astype(hr.LD) - ref).astype(np.float64))
    print(f"DP={DP} DC={DC} K={K} NP={NP}: kept {kept.mean():.3f} of the pairs, max err / bar {np.max(err[:, m] / np.maximum(bar[:, m], hr.TINY)):.3f}")
    assert not np.isnan(got[:, m]).any() and np.all(err[:, m] <= bar[:, m])
    assert not qs[EMPTY].any() and q[EMPTY].any(axis=1).all() and not kept[1].any()
    assert exact_equal(got[EMPTY][:, m], np.zeros((4, int(m.sum())))), "the clusters of the quad without an owner are not exact zeros"
    S = got[:, 1 + DP:].reshape(K, DP, DP)[:, :DC, :DC]
    assert same_bits(S, S.transpose(0, 2, 1)), "S_k is not exactly symmetric"


@pytest.mark.parametrize("NP", NPS)
@pytest.mark.parametrize("DP,DC,K", FEAT)
def test_hard_rows_same_bits_with_and_without_skipping(DP, DC, K, NP):
    """The same X and q: flag on and flag off give bit-identical folded records -- a speck of 1e-91 added to an accumulator
    of order one changes nothing.  The clusters for which that cannot hold are those that own no row (their dense records are
    the sums of their specks, 1e-91, their skipped ones zero: the deviation DESIGN 4.2b bounds); here their columns are exact zeros.  The
    float64 reference has the same property at every shape and row count with these seeds: hr.stats_ref of q and of q' agree bit
    for bit (tests/test_stats_speck_refs_host.py checks that on the CPU; every other cluster owns a row by construction)."""
    feat_shape(DP, DC, K, NP)
    X, q = same_bits_problem(DP, DC, K, NP)
    m = low(DP, DC)
    on, off = folded(X, DC, q, K, 1), folded(X, DC, q, K, 0)
    assert same_bits(on[:, m], off[:, m])


@pytest.mark.parametrize("DP,DC,K", FEAT)
def test_threshold_edges_and_nan(DP, DC, K):
    """Exact X (powers of two: every product is exact, every cluster has one term).  A pair whose largest value is exactly
    2^-300 is kept -- that product and the speck next to it come out exactly; the same pair with nextafter(2^-300, 0) yields
    exact zeros; a pair of specks next to one NaN is kept and the NaN stays in its own cluster's record."""
    NP = 272
    feat_shape(DP, DC, K, NP)
    rng = np.random.default_rng(DP + DC + K)
    X = np.zeros((NP, DP))
    X[:, :DC - 1] = rng.choice([-1.0, 1.0], size=(NP, DC - 1)) * 2.0 ** rng.integers(-3, 4, size=(NP, DC - 1))
    X[NP - 3:] = 0.0
    q = np.zeros((K, NP))
    under = np.nextafter(TAU, 0.0)
    # (step, quad): three batches apart, the last one in the ragged batch; quads 0, 1, 2
    q[0, 4 * 3 + 1] = TAU
    q[1, 4 * 3 + 2] = 2.0 ** -350
    q[4, 4 * 20 + 0] = under
    q[5, 4 * 20 + 3] = 2.0 ** -350
    q[10, 4 * 66 + 2] = np.nan
    q[8, 4 * 66 + 1] = 2.0 ** -350
    q[9, 4 * 66 + 2] = 2.0 ** -301
    qs, kept = speck_rule(q)
    assert kept.sum() == 2 and kept[0, 3] and kept[2, 66] and not kept[1, 20]
    got = folded(X, DC, q, K, 1)
    m = low(DP, DC)
    ok = np.arange(K) != 10
    ref = hr.stats_ref(X, np.where(np.isnan(qs), 0.0, qs))
    assert exact_equal(got[ok][:, m], ref[ok][:, m])
    assert ref[0][0] == TAU and ref[1][0] == 2.0 ** -350 and not ref[4].any() and not ref[5].any() and ref[9][0] == 2.0 ** -301
    assert np.isnan(got[10][m]).all() and not np.isnan(got[ok][:, m]).any()
    # flag off: the pair under the threshold is multiplied
    off = folded(X, DC, q, K, 0)
    assert off[4][0] == under and off[5][0] == 2.0 ** -350


@pytest.mark.parametrize("DP,DC,K", FEAT)
def test_nothing_to_skip_is_bit_identical(DP, DC, K):
    """Soft responsibilities (Dirichlet(0.3): nothing near 2^-300) on continuous X, and hr.exact_q with and without whole
    all-zero steps on exact X: flag on equals flag off bit for bit at both row counts, and the exact cases equal the exact sums
    -- pairs of exact zeros are skipped exactly."""
    rng = np.random.default_rng(31 * DP + DC + K)
    m = low(DP, DC)
    for NP in NPS:
        feat_shape(DP, DC, K, NP)
        valid = np.arange(NP) < NP - 3
        X, _, _, _ = hr.rounding_problem(rng, K, DC - 1, NP, DP, valid)
        q = rng.dirichlet(np.full(K, 0.3), NP).T.copy()
        q[:, ~valid] = 0.0
        assert speck_rule(q)[1][:, : (NP - 3) // 4].all()
        assert same_bits(folded(X, DC, q, K, 1)[:, m], folded(X, DC, q, K, 0)[:, m])
        Xe = hr.exact_X(rng, NP, DC - 1, DP, valid)
        for zs in (False, True):
            q = hr.exact_q(rng, K, NP, zero_steps=zs)
            q[:, ~valid] = 0.0
            if zs:
                q[: 4 * (K // 8), 40:120] = 0.0  # whole pairs of exact zeros in the first quads
                assert not speck_rule(q)[1][:, : (NP - 3) // 4].all()
            on = folded(Xe, DC, q, K, 1)
            assert same_bits(on[:, m], folded(Xe, DC, q, K, 0)[:, m]) and exact_equal(on[:, m], hr.stats_ref(Xe, q)[:, m])


def test_context_setter_leaves_three_iterations_bit_identical():
    """N = 4096, D = 64, K = 32, bench.py's separated mixture, three fixed VBEM iterations with lc_ctx_set_speck_skip on and
    off: the F trace, every cluster posterior, the weights and qZ are equal bit for bit.  The context's pass counters show that
    the skipping kernel really ran with the setter on -- once: the first pass sees smoothed labels and the second the
    responsibilities of the first E-step, none of them below 2^-300 (DESIGN 4.2b's census), so the probe sends both to the
    dense kernel; the third sees hard rows -- and never with it off."""
    import sys

    sys.path.insert(0, str(ah.ROOT))
    import bench
    from libcluster_amd import capi

    N, D, K = 4096, 64, 32
    assert ah.suffstat_plan(64, 64, N, K, "dense")["route"] == "feat"
    mu, L = bench.mixture(D, K, 1004)
    res = []
    for on in (True, False):
        with capi.Context(0) as ctx:
            ctx.set_speck_skip(on)
            ctx.synth(N, D, K, mu, L, 1004, 0, 0.9)
            F, tr, mdl = ctx.vbem(capi.W_DIRICHLET, fixed_iters=3)
            cl = [mdl.cluster(k) for k in range(K)]
            skipping, dense = ctx.speck_passes()
            assert (skipping, dense) == ((1, 2) if on else (0, 0)), (on, skipping, dense)
            res.append((np.array([F]), tr, np.concatenate(mdl.weights(0)), ctx.get_qz([N])[0], cl))
            mdl.close()
    a, b = res
    for u, v in zip(a[:4], b[:4]):
        assert u.shape == v.shape and same_bits(u, v)
    assert (a[3].max(axis=1) == 1.0).mean() > 0.9, "the rows have not hardened: nothing was skipped"
    for ca, cb in zip(a[4], b[4]):
        for key in ca:
            assert same_bits(np.asarray(ca[key], dtype=np.float64), np.asarray(cb[key], dtype=np.float64)), key


def test_probe_sends_soft_passes_to_the_dense_kernel():
    """The selector in front of a context's pass (launch_speck_probe): N = 8192, D = 64, K = 32 -- every 4-row step is sampled,
    2048 x 8 pairs.  Soft responsibilities: dense.  Hard rows: skipping.  Exactly a quarter of the pairs skippable (the
    clusters of quads 0 and 1 exact zeros everywhere): skipping; one pair fewer: dense.  The statistics are those of the pass
    with the setter off, bit for bit, in all four."""
    from libcluster_amd import capi

    N, D, K = 8192, 64, 32
    assert ah.suffstat_plan(64, 64, N, K, "dense")["route"] == "feat"
    rng = np.random.default_rng(99)
    X = rng.normal(size=(N, D)) + rng.integers(0, K, (N, 1))
    soft = rng.dirichlet(np.full(K, 0.3), N)
    hard = 2.0 ** -rng.uniform(301.0, 1000.0, size=(N, K))
    hard[np.arange(N), np.arange(N) % K] = 1.0
    quarter = soft.copy()
    quarter[:, :8] = 0.0
    less = quarter.copy()
    less[0, 0] = 0.5
    expect = {"soft": (0, 1), "hard": (1, 0), "quarter": (1, 0), "less": (0, 1)}
    for name, q in (("soft", soft), ("hard", hard), ("quarter", quarter), ("less", less)):
        out = []
        for on in (True, False):
            with capi.Context(0) as ctx:
                ctx.set_speck_skip(on)
                ctx.set_data(X)
                ctx.set_qz(q)
                out.append(ctx.suffstat()[:3])
                assert ctx.speck_passes() == (expect[name] if on else (0, 0)), (name, on, ctx.speck_passes())
        for u, v in zip(*out):
            assert same_bits(u, v), name


@pytest.mark.parametrize("DP,DC,K,mode", [(32, 32, 13, "dense"), (64, 64, 8, "dense"), (64, 64, 32, "zero_skip"), (16, 16, 20, "dense")])
def test_flag_is_refused_where_no_skipping_instance_exists(DP, DC, K, mode):
    """the few-cluster kernel, the per-cluster kernel (few clusters, zero-skip mode, D = 16): hipErrorInvalidValue, nothing
    written; flag off, the same launch runs"""
    NP = 272
    assert ah.suffstat_plan(DP, DC, NP, K, mode)["route"] != "feat"
    rng = np.random.default_rng(DP + K)
    X = hr.exact_X(rng, NP, DC - 1, DP)
    q = hr.exact_q(rng, K, NP)
    rc, plan, fo, part = run(X, DC, q, K, 1, mode)
    assert rc == ah.HIP_ERROR_INVALID_VALUE and np.all(fo == SENT) and np.all(part == SENT), rc
    rc, plan, fo, part = run(X, DC, q, K, 0, mode)
    SS = hr.stat_stride(DP)
    m = hr.lower_mask(DP, DC)
    assert rc == 0 and exact_equal(fo[:K * SS].reshape(K, SS)[:, m], hr.stats_ref(X, q)[:, m])
