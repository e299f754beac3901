"""The prediction and document-inference kernels, launcher by launcher.

launch_predict_rows, launch_predict_diag, launch_predict_cond (libcluster_amd/csrc/lc_kernels_predict.hip), launch_topic_infer
(lc_kernels_topic.hip) and the device function log1p_nonneg (lc_device.hpp) are handed host arrays through the lc_test_* entry
points of libcluster_hip_testhooks.so (tests/aux_hooks.py), at the widths, cluster counts and row counts on both sides of every
batch, chunk, panel and dispatch boundary, and compared with np.longdouble restatements of the formulas in the launch structs'
comments: bit for bit where the kernel only moves or compares values, otherwise against a bar written as a formula in
EPS = 2^-52 next to the assertion -- first-order in EPS, every rounded operation of the path counted once, relative to the sum
of absolute values the REFERENCE computes.  Destination buffers hold SENT before a launch; every launch runs twice and must
leave the same bits."""
import math

import numpy as np
import pytest

import aux_hooks as ah

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
SENT = -777.25  # what destination buffers hold before a launch (no kernel here produces it)
ISENT = -7777
INVALID = ah.HIP_ERROR_INVALID_VALUE
GAP = 1e-9  # labels are compared where the reference's two largest terms are further apart than this


def test_the_reference_type_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2 ** -60


def steps(a, b):
    """Distance of two arrays of non-negative doubles in units of the last place of their bit patterns."""
    return np.abs(np.ascontiguousarray(a).view(np.int64) - np.ascontiguousarray(b).view(np.int64))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def lse(v, axis):
    """log sum exp in 80-bit arithmetic (-inf terms add nothing) -> value, max, log of the scaled sum"""
    m = np.max(v, axis=axis, keepdims=True)
    with np.errstate(invalid="ignore"):
        s = np.sum(np.where(np.isneginf(v), LD(0), np.exp(v - m)), axis=axis, keepdims=True)
    ls = np.log(s)
    return np.squeeze(m + ls, axis), np.squeeze(m, axis), np.squeeze(ls, axis)


def lse_bar(n, m, ls):
    """Bar of the online log-sum-exp of n terms (lse_push, then m + log(s)), the terms themselves taken as exact.  Per push:
    the subtraction v - m (EPS/2 |d|, which reaches s with the weight e^-|d| |d| <= 1/e), exp_nonpos (1 ulp = EPS) and the
    addition or fma into s (EPS/2): < 2 EPS of s.  log(s): 1 ulp, EPS |log s|; the final addition: EPS/2 |m + log s|."""
    return EPS * (2 * n + 2) * (1 + np.abs(m) + np.abs(ls)).astype(np.float64)


def words_of(groups):
    """rginfo words of [(group, nvalid), ...] blocks: full row groups, then one partial (nvalid = 0: one row group of padding)"""
    out = []
    for j, n in groups:
        full, rest = divmod(n, 16)
        out += [(j << 5) | 16] * full + ([(j << 5) | rest] if rest or n == 0 else [])
    return np.array(out, dtype=np.int32)


def rows_of(words=None, nrows=None):
    """-> NP, valid mask [NP], group of every row [NP]"""
    if words is None:
        NP = -(-max(nrows, 1) // 16) * 16
        return NP, np.arange(NP) < nrows, np.zeros(NP, dtype=np.int64)
    NP = 16 * words.size
    valid = (np.arange(NP) % 16) < np.repeat(words & 31, 16)
    return NP, valid, np.repeat(words >> 5, 16).astype(np.int64)


def twice(run):
    """run() -> (status, tuple of output arrays): launched twice on fresh copies, the same bits both times"""
    rc1, out1 = run()
    rc2, out2 = run()
    assert rc1 == rc2
    for a, b in zip(out1, out2):
        assert same_bits(a, b), "two launches on the same input differ"
    return rc1, out1


# =====================================================================================================================
# device math: log1p_nonneg
# =====================================================================================================================
def _log1p_points():
    rng = np.random.default_rng(21)
    s = np.array([0, 1, 2, 3, 7, 20, 51, 52, 53, 60, 200, 1000])
    u = ((1.0 + np.arange(1, 128) / 128.0)[None, :] * 2.0 ** s[:, None]).ravel()  # the 127 table edges in the binade 2^s
    lo, hi = np.nextafter(u, 0.0), np.nextafter(u, np.inf)
    edges = np.concatenate([u - 1.0, lo - 1.0, hi - 1.0])  # (exact differences for u >= 1: 1 + z lands on the neighbours of u)
    edges = np.concatenate([edges, np.nextafter(edges, 0.0), np.nextafter(edges, np.inf)])
    p2 = 2.0 ** np.arange(-1074, 1024)
    parts = [rng.uniform(0.0, 1.0, 500_000), rng.uniform(0.0, 2.0 ** -7, 300_000),
             np.exp(rng.uniform(math.log(5e-324), math.log(1e308), 600_000)), edges, p2, np.nextafter(p2, 0.0), np.nextafter(p2, np.inf),
             np.array([0.0, 5e-324, 2.0 ** -1022, 2.0 ** -53, 2.0 ** -52, 1.0, 1e300, np.finfo(np.float64).max, np.inf])]
    x = np.concatenate(parts)
    return x[x >= 0]


def test_log1p_nonneg_is_within_two_steps_of_the_rounded_log1p():
    """lc_device.hpp claims "within about 2 ulp" for log1p_nonneg.  Bar: the result, read as a bit pattern, is at most two
    steps from log1p() evaluated in 80-bit arithmetic and rounded to double, from the subnormals to DBL_MAX; 0 -> 0 and
    inf -> inf exactly, never a NaN or a negative value."""
    x = _log1p_points()
    assert 1_400_000 <= x.size <= 1_500_000
    rc, got = ah.log1p_nonneg(x)
    assert rc == 0
    assert same_bits(ah.log1p_nonneg(x)[1], got)
    ref_ld = np.log1p(x.astype(LD))
    ref = ref_ld.astype(np.float64)
    assert not np.any(np.isnan(got)) and np.all(got >= 0.0) and not np.any(np.signbit(got))
    fin = np.isfinite(x)
    assert np.all(np.isposinf(got[~fin])) and np.all(np.isfinite(got[fin]))
    st = steps(got[fin], ref[fin])
    err = np.abs(got[fin].astype(LD) - ref_ld[fin]) / np.spacing(ref[fin]).astype(LD)
    w = int(np.argmax(err))
    print(f"log1p_nonneg: {x.size} points, worst |error| {float(err[w]):.4f} ulp of the true value at z = {x[fin][w]!r}; "
          f"{int((st == 1).sum())} results one step off, {int((st == 2).sum())} two, {int((st > 2).sum())} further; "
          f"worst steps / bar = {int(st.max())} / 2")
    bad = np.flatnonzero(st > 2)
    assert bad.size == 0, [(x[fin][i], got[fin][i], ref[fin][i]) for i in bad[:5]]
    rc, edge = ah.log1p_nonneg(np.array([0.0, np.inf]))
    assert rc == 0 and same_bits(edge, np.array([0.0, np.inf]))


# =====================================================================================================================
# predict_rows_kernel
# =====================================================================================================================
ROW_LAYOUTS = [("n1", None, 1), ("n16", None, 16), ("n17", None, 17), ("n255", None, 255), ("n256", None, 256), ("n257", None, 257),
               # three groups over two blocks: 277 rows, a row group of padding only, an empty group, a group of one row
               ("ragged", [(0, 277), (0, 0), (2, 1)], None)]
NINF_PATTERNS = ["none", "first", "all_but_one", "scattered"]


def _ninf_mask(pattern, J, K, rng):
    m = np.zeros((J, K), dtype=bool)
    if pattern == "first":  # (from nine clusters on: the whole first batch of PR_COLS columns and one of the second)
        m[:, :min(K - 1, ah.PR_COLS + 1)] = True
    elif pattern == "all_but_one":
        m[:] = True
        m[np.arange(J), rng.integers(0, K, J)] = False
    elif pattern == "scattered":
        for j in range(J):
            m[j, rng.permutation(K)[:K // 2]] = True
    return m


def _predict_rows_ref(col, ctab, ptab, pscale, pexp, grp, K, Kp):
    """80-bit restatement of PredictRowsLaunch's comment on every row (valid or not) -> dict"""
    NPr = grp.size
    r = {}
    v = ctab.astype(LD)[grp].T + col[:K, :NPr].astype(LD)  # [K x NP]
    r["v"] = v
    r["logZ"], m, ls = lse(v, 0)
    r["barZ"] = (EPS / 2 * np.max(np.where(np.isfinite(v), np.abs(v), 0), axis=0).astype(np.float64)  # the rounding of c + col
                 + lse_bar(K, m, ls))
    r["label"] = np.argmax(v, axis=0)
    top = np.sort(v, axis=0)[::-1]
    with np.errstate(invalid="ignore"):
        r["gap"] = (top[0] - top[1]).astype(np.float64) if K > 1 else np.full(NPr, np.inf)
    r["gap"] = np.where(np.isnan(r["gap"]), np.inf, r["gap"])
    with np.errstate(invalid="ignore"):
        r["q"] = np.where(np.isneginf(v), LD(0), np.exp(v - r["logZ"][None, :]))
    if Kp:
        L = np.log1p(pscale.astype(LD)[:, None] * (-2 * col[:Kp, :NPr].astype(LD)))
        eL = pexp.astype(LD)[:, None] * L
        t = ptab.astype(LD)[grp].T - eL
        r["logp"], m, ls = lse(t, 0)
        # a term: s * (-2 col) EPS/2, log1p_nonneg 2 ulp, e * L EPS/2 -- 3 EPS e L -- and the subtraction EPS/2 |t|
        A = (np.abs(ptab.astype(LD)[grp].T) + np.abs(eL)).astype(np.float64)
        r["barP"] = 3.5 * EPS * np.max(A, axis=0) + lse_bar(Kp, m, ls)
    return r


@pytest.mark.parametrize("K,pattern", [(K, p) for K in (1, 7, 8, 9, 16, 17, 72) for p in NINF_PATTERNS if K > 1 or p == "none"])
def test_predict_rows_at_every_column_batch_and_row_edge(K, pattern):
    """label / logZ / logp / q of predict_rows_kernel for Kp in {0, K, K + 1} (K = 8, Kp = 9: the prior component alone in a
    batch of PR_COLS), every row layout and -inf constants where `pattern` puts them (the online log-sum-exp then starts
    from m = -inf).
      logZ, logp: |got - ref| <= bar of _predict_rows_ref (terms + lse_bar)
      q_k:        |got - ref| <= ref (EPS (1 + |v - logZ| / 2) + EPS/2 |v| + barZ) + 2^-1000   (exp_nonpos 1 ulp, the subtraction,
                  the rounding of v, the error of logZ; exp_nonpos gives 0 below e^-745), row sums within the sum of these bars
    keep_q = 0 leaves col as it was; keep_q = 1 rewrites the K columns of the valid rows and nothing else."""
    worst = 0.0
    for kpi, Kp in enumerate((0, K, K + 1)):
        for li, (name, groups, nrows) in enumerate(ROW_LAYOUTS):
            rng = np.random.default_rng(1000 * K + 100 * kpi + 10 * li + NINF_PATTERNS.index(pattern))
            words = None if groups is None else words_of(groups)
            NP, valid, grp = rows_of(words, nrows)
            J = 1 if groups is None else 3
            ncols, ldq = max(K, Kp) + 1, NP + 16
            col0 = np.full((ncols, ldq), SENT)
            col0[:, :NP] = -rng.uniform(0.0, 8.0, (ncols, NP))  # (pad rows hold ordinary values: they are scored nowhere)
            ctab = -rng.uniform(0.0, 3.0, (J, K))
            ctab[_ninf_mask(pattern, J, K, rng)] = -np.inf
            ptab = -rng.uniform(0.0, 5.0, (J, Kp)) if Kp else None
            pscale, pexp = (rng.uniform(0.01, 2.0, Kp), rng.uniform(1.0, 20.0, Kp)) if Kp else (None, None)
            ref = _predict_rows_ref(col0, ctab, ptab, pscale, pexp, grp, K, Kp)
            assert np.all(ref["gap"][valid] > GAP)
            for keep_q in (0, 1):
                def run():
                    col, label = col0.copy(), np.full(NP, ISENT, dtype=np.int32)
                    logZ, logp = np.full(NP, SENT), np.full(NP, SENT)
                    rc = ah.predict_rows(col, K, Kp, NP // 16, ctab, ptab, pscale, pexp, keep_q, label, logZ, logp, rginfo=words,
                                         nrows=nrows or 0)
                    return rc, (col, label, logZ, logp)
                rc, (col, label, logZ, logp) = twice(run)
                tag = (K, Kp, name, pattern, keep_q)
                assert rc == 0, tag
                assert np.all(label[~valid] == ISENT) and np.all(logZ[~valid] == SENT) and np.all(logp[~valid] == SENT), tag
                assert np.array_equal(label[valid], ref["label"][valid]), tag
                eZ = np.abs(logZ.astype(LD) - ref["logZ"]).astype(np.float64)[valid]
                assert np.all(eZ <= ref["barZ"][valid]), (tag, float(np.max(eZ / ref["barZ"][valid])))
                worst = max(worst, float(np.max(eZ / ref["barZ"][valid])))
                if Kp:
                    eP = np.abs(logp.astype(LD) - ref["logp"]).astype(np.float64)[valid]
                    assert np.all(eP <= ref["barP"][valid]), (tag, float(np.max(eP / ref["barP"][valid])))
                    worst = max(worst, float(np.max(eP / ref["barP"][valid])))
                else:
                    assert np.all(logp == SENT), tag
                if not keep_q:
                    assert same_bits(col, col0), tag
                    continue
                keep = np.ones_like(col0, dtype=bool)
                keep[:K, :NP] = ~valid[None, :]
                assert same_bits(col[keep], col0[keep]), tag  # pad rows, rows beyond NP, column K and the spare column
                q, qr, v = col[:K, :NP][:, valid], ref["q"][:, valid], ref["v"][:, valid]
                with np.errstate(invalid="ignore"):
                    dv = np.where(np.isneginf(v), LD(0), np.abs(v - ref["logZ"][valid][None, :])).astype(np.float64)
                    av = np.where(np.isneginf(v), LD(0), np.abs(v)).astype(np.float64)
                barq = qr.astype(np.float64) * (EPS * (1 + dv / 2) + EPS / 2 * av + ref["barZ"][valid][None, :]) + 2.0 ** -1000
                eq = np.abs(q.astype(LD) - qr).astype(np.float64)
                assert np.all(eq <= barq), (tag, float(np.max(eq / barq)))
                assert np.all(q[np.isneginf(v)] == 0.0), tag
                worst = max(worst, float(np.max(eq / barq)))
                assert np.all(np.abs(q.astype(LD).sum(0) - 1).astype(np.float64) <= barq.sum(0) + K * EPS), tag
    print(f"predict_rows K = {K}, -inf constants {pattern}: worst error / bar = {worst:.3f}")


@pytest.mark.parametrize("K", [2, 7, 9, 17])
def test_predict_rows_labels_the_lowest_cluster_of_an_exact_tie(K):
    """c + col built from multiples of 1/8: every sum is exact, and on every second row two (or all) clusters share the maximum
    exactly.  The label is the lowest of them."""
    rng = np.random.default_rng(40 + K)
    NP, nrows = 272, 261
    col0 = -rng.integers(8, 64, (K, NP)) / 8.0
    ctab = -rng.integers(0, 24, (1, K)) / 8.0
    expect = np.argmax(ctab.T + col0, axis=0)
    for n in range(0, NP, 2):
        ks = np.arange(K) if n % 8 == 0 else np.sort(rng.permutation(K)[:2])
        col0[ks, n] = 1.0 - ctab[0, ks]  # c + col = 1 there, below 0 elsewhere
        expect[n] = ks[0]
    v = ctab.T + col0
    assert np.all(np.sort(v, axis=0)[-1, ::2] == np.sort(v, axis=0)[-2, ::2]) and np.array_equal(np.argmax(v, axis=0), expect)

    def run():
        col, label, logZ, logp = col0.copy(), np.full(NP, ISENT, dtype=np.int32), np.full(NP, SENT), np.full(NP, SENT)
        return ah.predict_rows(col, K, 0, NP // 16, ctab, None, None, None, 0, label, logZ, logp, nrows=nrows), (col, label, logZ)
    rc, (col, label, logZ) = twice(run)
    assert rc == 0 and same_bits(col, col0)
    assert np.array_equal(label[:nrows], expect[:nrows]) and np.all(label[nrows:] == ISENT)
    print(f"predict_rows ties K = {K}: {nrows} labels equal, error / bar = 0")


def test_predict_rows_hook_refuses_what_would_be_an_address():
    col, lab, z = np.zeros((3, 32)), np.zeros(32, dtype=np.int32), np.zeros(32)
    ct = np.zeros((1, 3))
    assert ah.predict_rows(col, 3, 0, 3, ct, None, None, None, 0, np.zeros(48, dtype=np.int32), np.zeros(48), np.zeros(48)) == -1
    assert ah.predict_rows(col, 3, 0, 2, ct, None, None, None, 0, lab, z, z.copy(), nrows=33) == -1  # more rows than row groups
    assert ah.predict_rows(col, 3, 0, 2, ct, None, None, None, 0, lab, z, z.copy(), rginfo=[(1 << 5) | 16, 16]) == -1  # group 1 of 1


# =====================================================================================================================
# predict_diag_kernel
# =====================================================================================================================
DIAG_D = {16: 16, 32: 29, 48: 48, 64: 61, 80: 77, 192: 190}  # real columns of every padded width
DIAG_LAYOUTS = [("n300", None, 300), ("grouped", [(0, 37), (1, 5), (2, 0), (2, 16), (1, 277)], None)]


def _diag_data(rng, mode, DP, Kp, NP, J, big):
    D = DIAG_D[DP]
    X, a, w = np.zeros((NP, DP)), np.zeros((Kp, DP)), np.zeros((Kp, DP))
    if not big:
        X[:, :D] = rng.uniform(0.0, 4.0, (NP, D)) if mode else rng.normal(size=(NP, D)) * 2
        a[:, :D] = rng.normal(size=(Kp, D))
        w[:, :D] = rng.uniform(0.05, 2.0, (Kp, D))
    elif mode:  # w x in [2^100, 2^250)
        X[:, :D] = 2.0 ** rng.uniform(50, 125, (NP, D))
        w[:, :D] = 2.0 ** rng.uniform(50, 125, (Kp, D))
    else:  # w (x - a)^2 in [2^100, 2^250): |x| in [2^26.5, 2^60), |a| < 2^23, w in [2^49, 2^130)
        X[:, :D] = 2.0 ** rng.uniform(26.5, 60, (NP, D)) * rng.choice([-1.0, 1.0], (NP, D))
        a[:, :D] = rng.normal(size=(Kp, D)) * 2.0 ** 20
        w[:, :D] = 2.0 ** rng.uniform(49, 130, (Kp, D))
    ptab = -rng.uniform(0.0, 5.0, (J, Kp))
    pexp = rng.uniform(0.5, 6.0, Kp)
    return X, a, w, ptab, pexp


def _diag_ref(mode, X, a, w, ptab, pexp, grp):
    """80-bit restatement of PredictDiagLaunch's comment -> logp [NP], bar [NP]"""
    NP, DP = X.shape
    Kp = pexp.size
    t = np.empty((Kp, NP), dtype=LD)
    bar_t = np.empty((Kp, NP))
    for k in range(Kp):
        Xl = X.astype(LD)
        f = 1 + w[k].astype(LD) * (Xl if mode else (Xl - a[k].astype(LD)) ** 2)
        L = np.log(f).sum(axis=1)
        eL = LD(pexp[k]) * L
        t[k] = ptab.astype(LD)[grp, k] - eL
        # a factor: x - a EPS/2 (twice in the square), w t EPS/2, the fma EPS/2 -- 2 EPS; DP multiplications EPS/2 each; frexp and
        # the exponent sums exact; log 1 ulp of |log p| < 1.4; the fma and the addition of the two parts of ex ln 2 EPS |L|: within
        # EPS (2.5 DP + 2 + 1.5 L) on L; then e L EPS/2 and the subtraction EPS/2 |t|
        bar_t[k] = EPS * (pexp[k] * (2.5 * DP + 2 + 1.5 * L.astype(np.float64)) + 0.5 * np.abs(t[k]).astype(np.float64))
    logp, m, ls = lse(t, 0)
    return logp, np.max(bar_t, axis=0) + lse_bar(Kp, m, ls), t


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("DP", [16, 32, 48, 64, 80, 192])
def test_predict_diag_instances_and_the_renormalised_product(DP, mode):
    """The four register-resident instances and the generic one, Kp in {1, 5, 33}, 300 rows (not a multiple of 256) and a
    grouped layout, on moderate data and on factors in [2^100, 2^250) whose plain product overflows after five columns (the
    summed binary exponent reaches DP * 175).  |logp - ref| <= bar of _diag_ref.  The flag stays as it was: no valid negative
    value in mode 1 (the pad rows hold one), mode 0 never sets it."""
    worst, maxex = 0.0, 0.0
    for Kp in (1, 5, 33):
        for li, (name, groups, nrows) in enumerate(DIAG_LAYOUTS):
            for big in (False, True):
                rng = np.random.default_rng(DP * 100 + Kp * 4 + li * 2 + big + 1000 * mode)
                words = None if groups is None else words_of(groups)
                NP, valid, grp = rows_of(words, nrows)
                J = 1 if groups is None else 3
                X, a, w, ptab, pexp = _diag_data(rng, mode, DP, Kp, NP, J, big)
                X[~valid] = -rng.uniform(1.0, 2.0, (int((~valid).sum()), DP))  # negative values in pad rows: not observations
                ref, bar, t = _diag_ref(mode, np.where(valid[:, None], X, 1.0), a, w, ptab, pexp, grp)
                if big:
                    Lk = ((ptab.astype(LD)[grp].T - t) / pexp.astype(LD)[:, None]).astype(np.float64)[:, valid]
                    assert Lk.min() / math.log(2) > 100 * DIAG_D[DP] and DIAG_D[DP] * 100 > 1024  # the plain product overflows
                    maxex = max(maxex, Lk.max() / math.log(2))

                def run():
                    logp, flag = np.full(NP, SENT), np.array([ISENT], dtype=np.int32)
                    return ah.predict_diag(mode, X, a, w, ptab, pexp, logp, flag, rginfo=words, nrows=nrows or 0), (logp, flag)
                rc, (logp, flag) = twice(run)
                tag = (DP, mode, Kp, name, big)
                assert rc == 0 and flag[0] == ISENT, (tag, rc, flag)
                assert np.all(logp[~valid] == SENT), tag
                e = np.abs(logp.astype(LD) - ref).astype(np.float64)[valid]
                assert np.all(e <= bar[valid]), (tag, float(np.max(e / bar[valid])))
                worst = max(worst, float(np.max(e / bar[valid])))
    assert DP < 80 or maxex > 10000
    print(f"predict_diag DP = {DP}, mode {mode}: worst error / bar = {worst:.3f}; largest summed exponent {maxex:.0f}")


@pytest.mark.parametrize("DP", [16, 48, 80])
def test_predict_diag_flag_means_a_valid_negative_observation(DP):
    """Mode 1: the flag is set iff a valid row holds a value below zero: -0.0 does not count, nor does a negative value in a pad
    row.  Mode 0 never sets it."""
    rng = np.random.default_rng(DP)
    words = words_of([(0, 37), (1, 5), (1, 0), (0, 262)])
    NP, valid, grp = rows_of(words)
    assert NP > 256
    X, a, w, ptab, pexp = _diag_data(rng, 1, DP, 5, NP, 2, False)
    vr, pr = np.flatnonzero(valid), np.flatnonzero(~valid)

    def flag_of(mode, Xc):
        def run():
            logp, flag = np.full(NP, SENT), np.array([ISENT], dtype=np.int32)
            return ah.predict_diag(mode, Xc, a, w, ptab, pexp, logp, flag, rginfo=words), (logp, flag)
        rc, (logp, flag) = twice(run)
        assert rc == 0
        return int(flag[0])
    assert flag_of(1, X) == ISENT
    Xz = X.copy()
    Xz[vr[::3], ::2] = -0.0
    assert flag_of(1, Xz) == ISENT
    Xp = X.copy()
    Xp[pr] = -1.0
    assert flag_of(1, Xp) == ISENT
    for r, c in ((vr[0], 0), (vr[-1], DIAG_D[DP] - 1), (vr[40], 7), (vr[-1], DP - 1), (int(vr[vr >= 256][0]), 3)):
        Xn = X.copy()
        Xn[r, c] = -1e-3
        assert flag_of(1, Xn) == 1, (r, c)
        assert flag_of(0, Xn) == ISENT, (r, c)
    Xn = X.copy()
    Xn[vr[5], 2] = -5e-324  # the smallest negative value there is
    assert flag_of(1, Xn) == 1
    print(f"predict_diag flag DP = {DP}: exact, error / bar = 0")


@pytest.mark.parametrize("DP", [18, 30, 63])
def test_predict_diag_refuses_a_width_that_is_no_multiple_of_the_renormalisation_group(DP):
    assert DP % ah.PRED_RENORM != 0
    NP, Kp = 32, 2
    X, a, w = np.ones((NP, DP)), np.zeros((Kp, DP)), np.ones((Kp, DP))
    for mode in (0, 1):
        logp, flag = np.full(NP, SENT), np.array([ISENT], dtype=np.int32)
        assert ah.predict_diag(mode, X, a, w, np.zeros((1, Kp)), np.ones(Kp), logp, flag, nrows=20) == INVALID
        assert np.all(logp == SENT) and flag[0] == ISENT


# =====================================================================================================================
# predict_cond_kernel
# =====================================================================================================================
COND_DA = [1, 3, 4, 31, 32, 33, 63]
COND_DB = [1, 4, 5, 31, 32, 33, 65]
COND_PAIRS = [(COND_DA[i], COND_DB[(i + s) % 7]) for s in (0, 3) for i in range(7)]  # every Da with two Db, every Db with two Da
COND_KP = [1, 8, 9, 35]
COND_LAYOUTS = [("n1", None, 1), ("n16", None, 16), ("n48", None, 48), ("n64", None, 64), ("n80", None, 80), ("n1040", None, 1040),
                ("grouped", [(0, 37), (1, 5), (2, 16), (3, 0)], None)]


def _cond_case(pi, li):
    """Kp and DP of the case (pair pi, layout li): every Kp meets every layout and every pair; DP is the padded layout width of
    Da (for Da = 32 that is below Dae = 36), and 64 -- beyond Dae -- for the pair with Da = 4"""
    Da, Db = COND_PAIRS[pi]
    DP = 64 if pi == 2 else -(-Da // 16) * 16
    Kp = COND_KP[(pi + li) % 4]
    if COND_LAYOUTS[li][2] == 1040 and Kp * (Da + 1) * Db > 20000:
        Kp = 8  # (the 80-bit reference of 1040 rows stays below a second; the wave and block edges do not depend on Kp)
    return Da, Db, Kp, DP


def test_predict_cond_cases_cover_what_the_edges_need():
    assert all(sum(1 for a, b in COND_PAIRS if a == da) == 2 for da in COND_DA) and len(set(COND_PAIRS)) == 14
    assert all(sum(1 for a, b in COND_PAIRS if b == db) == 2 for db in COND_DB)
    assert ah.PC_CHUNK == 32 and ah.PC_PANEL == 32 and ah.PC_WAVE_ROWS == 64 and ah.PC_THREADS == 256  # what the lists straddle
    seen = {(_cond_case(pi, li)[2], li) for pi in range(14) for li in range(7)}
    assert all((kp, li) in seen for kp in COND_KP for li in range(7))
    assert (33, 33) in COND_PAIRS or (63, 33) in COND_PAIRS or (33, 65) in COND_PAIRS  # partial last quad and partial last panel


def _cond_ref(X, Da, Dae, Db, col0, ttab, pscale, pexp, mext, T, grp):
    """80-bit restatement of PredictCondLaunch's comment on every row -> t [Kp x NP], logp, mean [NP x Db] and their bars"""
    Kp, NP = pscale.size, grp.size
    L = np.log1p(pscale.astype(LD)[:, None] * (-2 * col0[:Kp, :NP].astype(LD)))
    eL = pexp.astype(LD)[:, None] * L
    tt = ttab.astype(LD)[grp].T
    t = tt - eL
    bar_t = 3.5 * EPS * (np.abs(tt) + np.abs(eL)).astype(np.float64)  # as the logp terms of predict_rows_kernel
    logp, m, ls = lse(t, 0)
    bar_p = np.max(bar_t, axis=0) + lse_bar(Kp, m, ls)
    r = np.exp(t - logp[None, :])
    # r_k: the subtraction EPS/2 |t - logp|, exp_nonpos EPS, and what t and logp are off by
    rel_r = (EPS * (1 + 0.5 * np.abs(t - logp[None, :]).astype(np.float64)) + bar_t + bar_p[None, :]).max(axis=0)
    xe = np.zeros((NP, Dae), dtype=LD)
    xe[:, :Da] = X[:, :Da]
    xe[:, Da] = 1
    mean = np.zeros((NP, Db), dtype=LD)
    S = np.zeros((NP, Db), dtype=LD)
    for k in range(Kp):
        A = r[k][:, None] * (xe - mext[k].astype(LD)[None, :])
        mean += A @ T[k].astype(LD)[:, :Db]
        S += np.abs(A) @ np.abs(T[k].astype(LD)[:, :Db])
    # an operand r_k (x - m): rel_r, the subtraction EPS/2, the product EPS/2; Kp (Da + 1) products accumulated one rounding each
    bar_m = S.astype(np.float64) * (rel_r[:, None] + EPS * (1 + 0.5 * Kp * (Da + 1)))
    return t, bar_t, logp, bar_p, mean, bar_m, r


@pytest.mark.parametrize("pi", range(14), ids=[f"Da{a}-Db{b}" for a, b in COND_PAIRS])
def test_predict_cond_at_every_chunk_panel_and_wave_edge(pi):
    """logp, the rewritten columns t_k and the conditional mean for one (Da, Db) pair on every row layout (1040 rows: five
    blocks of 256, the last wave 16 rows; grouped: per-group ttab, an empty group), Kp cycling through {1, 8, 9, 35}.
    Bars: _cond_ref.  Pad rows of col, mean and logp keep what they held."""
    worst = 0.0
    for li, (name, groups, nrows) in enumerate(COND_LAYOUTS):
        Da, Db, Kp, DP = _cond_case(pi, li)
        Dae, Dbp = (Da + 1 + 3) // 4 * 4, (Db + 3) // 4 * 4
        rng = np.random.default_rng(977 * pi + li)
        words = None if groups is None else words_of(groups)
        NP, valid, grp = rows_of(words, nrows)
        J = 1 if groups is None else 4
        ldq = NP + 16
        X = np.zeros((NP, DP))
        X[:, :Da] = rng.normal(size=(NP, Da)) * 2
        col0 = np.full((Kp, ldq), SENT)
        col0[:Kp, :NP] = -rng.uniform(0.0, 3.0, (Kp, NP))
        col0[:Kp, :NP][:, ~valid] = SENT
        ttab = -rng.uniform(0.0, 1.0, (J, Kp))
        pscale, pexp = rng.uniform(0.2, 1.0, Kp), rng.uniform(1.0, 4.0, Kp)
        B, ma, mb = rng.normal(size=(Kp, Db, Da)), rng.normal(size=(Kp, Da)), rng.normal(size=(Kp, Db)) * 3
        mext, T = np.zeros((Kp, Dae)), np.zeros((Kp, Dae, Dbp))
        mext[:, :Da] = ma
        T[:, :Da, :Db] = B.transpose(0, 2, 1)
        T[:, Da, :Db] = mb
        t, bar_t, logp_r, bar_p, mean_r, bar_m, r = _cond_ref(X, Da, Dae, Db, col0, ttab, pscale, pexp, mext, T, grp)
        if Kp >= 8:
            assert np.mean(r[:, valid].max(axis=0) < 0.99) >= 0.2  # responsibilities genuinely mixed

        def run():
            col, mean, logp = col0.copy(), np.full((NP, Db), SENT), np.full(NP, SENT)
            rc = ah.predict_cond(X, Da, Dae, Db, Dbp, col, ttab, pscale, pexp, mext, T, mean, logp, rginfo=words, nrows=nrows or 0)
            return rc, (col, mean, logp)
        rc, (col, mean, logp) = twice(run)
        tag = (Da, Db, Kp, DP, name)
        assert rc == 0, tag
        keep = np.ones_like(col0, dtype=bool)
        keep[:Kp, :NP] = ~valid[None, :]
        assert same_bits(col[keep], col0[keep]), tag
        assert np.all(mean[~valid] == SENT) and np.all(logp[~valid] == SENT), tag
        for got, ref, bar, what in ((logp[valid], logp_r[valid], bar_p[valid], "logp"), (col[:Kp, :NP][:, valid], t[:, valid], bar_t[:, valid], "t"),
                                    (mean[valid], mean_r[valid], bar_m[valid], "mean")):
            e = np.abs(got.astype(LD) - ref).astype(np.float64)
            assert np.all(e <= bar), (tag, what, float(np.max(e / bar)))
            worst = max(worst, float(np.max(e / bar)))
    print(f"predict_cond Da = {COND_PAIRS[pi][0]}, Db = {COND_PAIRS[pi][1]}: worst error / bar = {worst:.3f}")


def test_predict_cond_refuses_every_combination_its_launcher_names():
    NP, Kp = 32, 2
    good = dict(DP=16, Da=3, Dae=4, Db=5, Dbp=8, Kp=2)
    bad = [dict(Kp=0), dict(Da=0), dict(Db=0), dict(DP=2), dict(Dae=3), dict(Da=4, Dae=4), dict(Dae=6), dict(Dbp=4), dict(Dbp=6),
           dict(Db=-1), dict(Da=-3)]
    for change in bad:
        c = {**good, **change}
        X = np.zeros((NP, c["DP"]))
        col, mean, logp = np.full((Kp, NP), -1.0), np.full((NP, max(c["Db"], 1)), SENT), np.full(NP, SENT)
        rc = ah.predict_cond(X, c["Da"], c["Dae"], c["Db"], c["Dbp"], col, np.zeros((1, Kp)), np.ones(Kp), np.ones(Kp),
                             np.zeros((Kp, 8)), np.zeros((Kp, 8, 8)), mean, logp, nrows=20, check_shapes=False, Kp=c["Kp"])
        assert rc == INVALID, (change, rc)
        assert np.all(col == -1.0) and np.all(mean == SENT) and np.all(logp == SENT)


# =====================================================================================================================
# topic_infer_kernel
# =====================================================================================================================
def _topic_ref(L, a, E, max_sweeps, tol):
    """The fixed point TopicInferLaunch documents, for one document, in 80-bit arithmetic on L [N x K], a [T], E [T x K]:
    qY^0 = softmax(a); per sweep c = qY E, q = softmax_k(c + L), N_k = sum_n q_nk, like = E N, qY = softmax(a + like); stop when
    max |qY - qY_old| <= tol (tol >= 0) or after max_sweeps; then one more c, q for label / logZ per row.
    Next to every value, its first-order error bound in the kernel's double arithmetic: what a sweep adds by its own rounded
    operations (formulas below), and what it inherits -- the bound on qY times the infinity norm of the sweep's Jacobian
    dqY_new / dqY = (diag(qY_new) - qY_new qY_new^T) E (diag(N) - Q^T Q) E^T, computed here: the reference's own sensitivity."""
    N, K = L.shape
    T = a.size
    L, a, E = L.astype(LD), a.astype(LD), E.astype(LD)
    aE = np.abs(E)
    nsum = EPS / 2 * (N / 64 + 10)  # a sum over the document's rows: per thread <= N / nth additions, six butterfly steps, <= 4 waves

    def softmax(x):
        lz, m, ls = lse(x, 0)
        return np.exp(x - lz), lz

    def vbez(qy, dqy):
        c = qy @ E
        dc = dqy * aE.sum(0) + T * EPS / 2 * (np.abs(qy)[:, None] * aE).sum(0)  # T fmas
        v = c[None, :] + L
        dv = (dc[None, :] + EPS / 2 * np.abs(v)).max(axis=1)  # per row
        lz, m, ls = lse(v, 1)
        q = np.exp(v - lz[:, None])
        rho = 2 * dv + (K + 4) * EPS  # relative error of a row of q: softmax of perturbed v; K exponentials summed, rcp_pos, product
        return v, lz, q, rho

    qy, lz0 = softmax(a)
    dqy = float((qy * (T + 4 + np.abs(a - lz0) + abs(lz0)) * EPS).max())
    deltas, margins, R, Fyz, dFyz = [], [], 0, LD(0), 0.0
    for r in range(1, max_sweeps + 1):
        v, lz, q, rho = vbez(qy, 0.0)
        nk = q.sum(0)
        dnk = (q * rho[:, None]).sum(0) + nsum * nk
        like = E @ nk
        dlike = aE @ dnk + K * EPS / 2 * (aE @ nk)
        x = a + like
        darg = float((dlike + EPS / 2 * np.abs(x)).max())
        qyn, lzy = softmax(x)
        # softmax of arguments off by <= darg: dq_t = q_t |sum_{j != t} q_j (dx_t - dx_j)| <= q_t (1 - q_t) 2 darg; its own roundings
        # (T exponentials summed, log 1 ulp and the addition m + log s -- EPS |lz|, common to every class --, the subtraction x - lz, exp)
        fresh = float((qyn * (2 * darg * (1 - qyn) + (T + 4 + np.abs(x - lzy) + abs(lzy)) * EPS)).max())
        H = E @ (np.diag(nk) - q.T @ q) @ E.T
        Jn = float(np.abs((np.diag(qyn) - np.outer(qyn, qyn)) @ H).sum(axis=1).max())
        dqy_new = Jn * dqy + fresh
        dx = float(np.abs(H).sum(axis=1).max()) * dqy + darg  # a + like as the kernel has it
        Fyz = qyn @ like - lzy
        dFyz = float(np.abs(like).max() * T * dqy_new + dx + (dx + (T + 4) * EPS * (1 + abs(lzy))) + (T + 1) * EPS / 2 * (np.abs(qyn * like).sum() + abs(lzy)))
        deltas.append(float(np.abs(qyn - qy).max()))
        margins.append(dqy + dqy_new)  # what the kernel's delta may be off by
        qy, dqy, R = qyn, dqy_new, r
        if tol >= 0 and deltas[-1] <= tol:
            break
    v, lz, q, rho = vbez(qy, dqy)
    dlz = (rho + EPS * (1 + np.abs(lz))).astype(np.float64)  # log(sum) with the sum's relative error, log 1 ulp, the addition
    top = np.sort(v, axis=1)
    tq = np.sort(qy)
    return dict(qY=qy, dqY=dqy, R=R, deltas=deltas, margins=margins, F=np.array([Fyz, -lz.sum()]),
                dF=np.array([dFyz, float(dlz.sum() + nsum * np.abs(lz).sum())]), label=np.argmax(v, axis=1), logZ=lz, dlogZ=dlz, q=q,
                dq=(q * rho[:, None]).astype(np.float64) + 2.0 ** -1000, gap=(top[:, -1] - top[:, -2]).astype(np.float64) if K > 1 else np.full(N, np.inf),
                label_t=int(np.argmax(qy)), gap_t=float(tq[-1] - tq[-2]) if T > 1 else np.inf)


def _topic_launch(rng, K, T, sizes, scale=1.0):
    """Documents of the given sizes in a padded layout -> goff, NP, col0 [K x ldq], a [docs x T], E [T x K]"""
    goff = ah.padded_offsets(sizes)
    NP = int(goff[-1])
    ldq = NP + 16
    col0 = np.full((K, ldq), SENT)
    col0[:, :NP] = -rng.uniform(0.0, 6.0, (K, NP)) * scale
    a = -rng.uniform(0.0, 2.0, (len(sizes), T))
    E = np.log(rng.dirichlet(np.ones(K) * 2.0, T)) if K > 1 else np.zeros((T, 1))
    return goff[:-1].copy(), NP, col0, a, E


def _topic_check(K, T, sizes, goff, NP, col0, a, E, max_sweeps, tol, keep_q, threads, tag):
    """One launch (twice) against _topic_ref document by document -> worst error / bar"""
    docs = len(sizes)
    sizes = np.asarray(sizes, dtype=np.int64)

    def run():
        col, label, logZ = col0.copy(), np.full(NP, ISENT, dtype=np.int32), np.full(NP, SENT)
        qY, F, dint = np.full((docs, T), SENT), np.full((docs, 2), SENT), np.full((docs, 2), ISENT, dtype=np.int32)
        rc = ah.topic_infer(col, NP, K, T, goff, sizes, a, E, max_sweeps, tol, keep_q, threads, label, logZ, qY, F, dint)
        return rc, (col, label, logZ, qY, F, dint)
    rc, (col, label, logZ, qY, F, dint) = twice(run)
    assert rc == 0, tag
    valid = np.zeros(NP, dtype=bool)
    worst = 0.0

    def within(got, ref, bar, what, i):
        nonlocal worst
        e = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
        bar = np.broadcast_to(np.asarray(bar, dtype=np.float64), e.shape)
        if e.size:
            ratio = float(np.max(e / np.maximum(bar, 2.0 ** -1000)))
            assert np.all(e <= bar), (tag, what, i, ratio)
            worst = max(worst, ratio)
    for i in range(docs):
        n, g = int(sizes[i]), int(goff[i])
        valid[g:g + n] = True
        ref = _topic_ref(col0[:K, g:g + n].T, a[i], E, max_sweeps, tol)
        if tol >= 0:  # the stopping sweep is the reference's: no delta near tol, and the error bound far below the distance
            assert all(abs(d / tol - 1) > 1e-6 and abs(d - tol) > 2 * mg for d, mg in zip(ref["deltas"], ref["margins"])), (tag, i, ref["deltas"])
        else:
            assert ref["R"] == max_sweeps
        assert dint[i, 1] == ref["R"], (tag, i, dint[i], ref["R"])
        within(qY[i], ref["qY"], ref["dqY"], "qY", i)
        within(F[i], ref["F"], ref["dF"], "F", i)
        assert ref["gap_t"] > GAP and ref["gap_t"] > 4 * ref["dqY"] and dint[i, 0] == ref["label_t"], (tag, i)
        if n:
            within(logZ[g:g + n], ref["logZ"], ref["dlogZ"], "logZ", i)
            assert np.all(ref["gap"] > GAP) and np.all(ref["gap"] > 4 * ref["dlogZ"]), (tag, i)
            assert np.array_equal(label[g:g + n], ref["label"]), (tag, i)
            if keep_q:
                within(col[:K, g:g + n].T, ref["q"], ref["dq"], "q", i)
    assert np.all(label[~valid] == ISENT) and np.all(logZ[~valid] == SENT), tag
    keep = np.ones_like(col0, dtype=bool)
    if keep_q:
        keep[:K, :NP] = ~valid[None, :]
    assert same_bits(col[keep], col0[keep]), tag  # without keep_q all of col, with it the pad rows
    return worst


TOPIC_KT = [(1, 1), (4, 3), (16, 8), (16, 9), (17, 3), (40, 5)]
TOPIC_SIZES = [0, 1, 63, 64, 65, 128, 129, 256, 257, 1000]


@pytest.mark.parametrize("K,T", TOPIC_KT)
def test_topic_infer_paths_workgroup_sizes_and_stopping_modes(K, T):
    """Documents of 0 ... 1000 rows in one launch, with the workgroup size forced to 64, 128 and 256 and chosen by the hook as
    the API chooses it; a fixed number of sweeps (tol < 0: 1, 3, 8) and tol = 1e-6 (the reference's sweep count).  (16, 8) and
    (16, 9) sit on either side of T K = TOPIC_E_LDS, (16, *) and (17, 3) on either side of TI_KR.  Bars: _topic_ref."""
    rng = np.random.default_rng(300 + 10 * K + T)
    goff, NP, col0, a, E = _topic_launch(rng, K, T, TOPIC_SIZES)
    lds, cap, el = ah.topic_plan(K, T, 256, TOPIC_SIZES)
    assert lds > 0 and el == (1 if T * K <= ah.TOPIC_E_LDS else 0) and el == {(16, 8): 1, (16, 9): 0}.get((K, T), el)
    worst = 0.0
    for threads, max_sweeps, tol, keep_q in ((64, 1, -1.0, 0), (128, 3, -1.0, 1), (256, 8, -1.0, 0), (0, 50, 1e-6, 1), (64, 50, 1e-6, 0)):
        worst = max(worst, _topic_check(K, T, TOPIC_SIZES, goff, NP, col0, a, E, max_sweeps, tol, keep_q, threads,
                                        (K, T, threads, max_sweeps, tol, keep_q)))
    print(f"topic_infer K = {K}, T = {T}: worst error / bar = {worst:.3f}")


@pytest.mark.parametrize("keep_q", [0, 1])
@pytest.mark.parametrize("K,T", [(4, 3), (16, 8), (17, 3), (40, 5)])
def test_topic_infer_tiled_and_untiled_documents_in_one_launch(K, T, keep_q):
    """From the plan's own numbers: one document whose tile fills the LDS allowance exactly and one with a row more, which is
    then re-read from global memory every sweep -- and, with keep_q, overwritten in place by the last pass."""
    threads = 256
    lds1, cap1, el = ah.topic_plan(K, T, threads, [1])
    assert cap1 == K
    room = (ah.TOPIC_LDS_BYTES - (lds1 - 8 * K)) // 8  # doubles left for a tile
    nfit = room // K
    sizes = [nfit, nfit + 1, 33]
    lds, cap, el2 = ah.topic_plan(K, T, threads, sizes)
    assert cap == nfit * K and (nfit + 1) * K > room >= cap and lds <= ah.TOPIC_LDS_BYTES and el2 == el
    assert sizes[0] * K <= cap < sizes[1] * K  # the kernel's own condition: tiled, untiled (and a small tiled one)
    rng = np.random.default_rng(500 + K + keep_q)
    goff, NP, col0, a, E = _topic_launch(rng, K, T, sizes)
    a *= 0.01  # (documents of thousands of rows: keep the classes apart by the rows, not by a)
    worst = _topic_check(K, T, sizes, goff, NP, col0, a, E, 2, -1.0, keep_q, threads, (K, T, "cap", keep_q))
    print(f"topic_infer K = {K}, T = {T}, keep_q = {keep_q}: documents of {nfit} (tiled) and {nfit + 1} rows (untiled), "
          f"worst error / bar = {worst:.3f}")


@pytest.mark.parametrize("K", [2, 16, 17])
def test_topic_infer_labels_the_lowest_segment_of_an_exact_tie(K):
    """Identical L columns and identical E columns: every row's K terms are the same number.  Label 0, q = 1 / K, and the
    document's class is the first of two classes with identical a and E rows."""
    T, sizes = 2, [70, 5]
    rng = np.random.default_rng(K)
    goff, NP, col0, a, E = _topic_launch(rng, K, T, sizes)
    col0[:K, :NP] = col0[0:1, :NP]
    E[:] = -rng.uniform(0.5, 2.0)  # every entry the same: identical columns, identical rows
    a[:] = a[:, :1]
    col, label, logZ = col0.copy(), np.full(NP, ISENT, dtype=np.int32), np.full(NP, SENT)
    qY, F, dint = np.full((2, T), SENT), np.full((2, 2), SENT), np.full((2, 2), ISENT, dtype=np.int32)
    assert ah.topic_infer(col, NP, K, T, goff, sizes, a, E, 4, -1.0, 1, 0, label, logZ, qY, F, dint) == 0
    for i, n in enumerate(sizes):
        g = int(goff[i])
        assert np.all(label[g:g + n] == 0) and dint[i, 0] == 0 and qY[i, 0] == qY[i, 1]
        assert np.all(np.abs(col[:K, g:g + n] - 1.0 / K) <= 4 * EPS / K)  # exp(0) = 1 exactly; the sum, rcp_pos, the product
    print(f"topic_infer ties K = {K}: labels equal, error / bar = 0")


def test_topic_infer_refusals_and_the_empty_launch():
    K, T, sizes = 4, 3, [20, 7]
    rng = np.random.default_rng(9)
    goff, NP, col0, a, E = _topic_launch(rng, K, T, sizes)

    def call(K=K, T=T, goff=goff, sizes=sizes, max_sweeps=2, threads=64, lds_request=0, check=True):
        docs = len(sizes)
        col, label, logZ = col0.copy(), np.full(NP, ISENT, dtype=np.int32), np.full(NP, SENT)
        qY, F, dint = np.full((docs, 3), SENT), np.full((docs, 2), SENT), np.full((docs, 2), ISENT, dtype=np.int32)
        rc = ah.topic_infer(col, NP, K, T, goff, sizes, a[:docs], E, max_sweeps, -1.0, 1, threads, label, logZ, qY, F, dint,
                            lds_request=lds_request, check_shapes=check)
        untouched = (same_bits(col, col0) and np.all(label == ISENT) and np.all(logZ == SENT) and np.all(qY == SENT) and np.all(F == SENT)
                     and np.all(dint == ISENT))
        return rc, untouched
    rc, untouched = call()
    assert rc == 0 and not untouched
    assert call(threads=96) == (INVALID, True)
    assert call(max_sweeps=0) == (INVALID, True)
    assert call(K=0, check=False) == (INVALID, True)
    assert call(lds_request=ah.TOPIC_LDS_BYTES + 8) == (INVALID, True)
    assert call(goff=np.zeros(0, dtype=np.int64), sizes=np.zeros(0, dtype=np.int64)) == (0, True)  # docs = 0
    assert call(goff=np.array([0, 16]), sizes=[20, 7])[0] == -1  # overlapping documents: refused by the hook
    assert ah.topic_plan(4000, 4000, 256, [1])[0] == 0  # the E-free fixed part alone exceeds the budget


def _wave_sum(v):
    """wave_sum (lc_device.hpp) in double: the butterfly over the lane distances 1, 2, 4, 8, 16, 32 -> what lane 0 holds"""
    v = np.asarray(v, dtype=np.float64).copy()
    for x in (1, 2, 4, 8, 16, 32):
        v = v + v[np.arange(64) ^ x]
    return float(v[0])


def _nk_register_order(q):
    """N_k as vbez_pass documents it for K <= TI_KR, one wave: a lane's rows in ascending order, then the butterfly once"""
    acc = np.zeros(64)
    for n0 in range(0, q.size, 64):
        b = q[n0:n0 + 64]
        acc[:b.size] = acc[:b.size] + b
    return _wave_sum(acc)


def _nk_batch_order(q):
    """... and for larger K: the butterfly per batch of 64 rows, the batches added in ascending order"""
    part = 0.0
    for n0 in range(0, q.size, 64):
        b = np.zeros(64)
        b[:min(64, q.size - n0)] = q[n0:n0 + 64]
        part = part + _wave_sum(b)
    return part


@pytest.mark.parametrize("K", [4, 16, 17, 40])
def test_topic_infer_sums_the_segment_counts_in_the_order_its_path_documents(K):
    """Which instance ran, seen from outside.  lc_kernels_topic.hip fixes the order of the N_k sums per path: registers per
    lane first for K <= TI_KR, one butterfly per batch of rows above.  One document of 65 rows on 64 threads: rows 0 ... 63 give
    q_n0 = 1 exactly (the other columns lie 800 below: exp_nonpos returns 0), row 64 gives q_0 = t = 1.45 * 2^-46.  In lane
    order 1 + t rounds to 1 + 93 ulp and the butterfly's ties carry that up to 64 + 2^-45; batch order adds t to 64 in one
    step: 64 + 2^-46.  With E = [[1, 0, ...], [0, ...]] and a = [-64, 0] the class arguments are [N_0 - 64, 0] exactly, so
    qY_0 - qY_1 = (N_0 - 64) / 2 up to the roundings of softmax_serial: exp_nonpos twice (1 ulp of 0.5 each: 2^-53), the
    subtraction of lz (2^-54 each), everything else common to both classes -- bar 2^-50, an eighth of what separates the orders."""
    t = 1.45 * 2.0 ** -46
    q0 = np.concatenate([np.ones(64), [t]])
    for scale in (1 - 1e-3, 1.0, 1 + 1e-3):  # (the device's t is within a few ulp of this one: the outcome does not hang on that)
        qs = np.concatenate([np.ones(64), [t * scale]])
        assert _nk_register_order(qs) == 64 + 2.0 ** -45 and _nk_batch_order(qs) == 64 + 2.0 ** -46
    expect = _nk_register_order(q0) if K <= ah.TI_KR else _nk_batch_order(q0)
    T, N, NP = 2, 65, 80
    col0 = np.full((K, NP), SENT)
    col0[:, :N] = -800.0
    col0[0, :64] = 0.0
    col0[1, 64], col0[0, 64] = 0.0, math.log(t)
    E = np.zeros((T, K))
    E[0, 0] = 1.0
    a = np.array([[-64.0, 0.0]])

    def run():
        col, label, logZ = col0.copy(), np.full(NP, ISENT, dtype=np.int32), np.full(NP, SENT)
        qY, F, dint = np.full((1, T), SENT), np.full((1, 2), SENT), np.full((1, 2), ISENT, dtype=np.int32)
        rc = ah.topic_infer(col, NP, K, T, [0], [N], a, E, 1, -1.0, 0, 64, label, logZ, qY, F, dint)
        return rc, (qY, dint, label)
    rc, (qY, dint, label) = twice(run)
    assert rc == 0 and dint[0, 1] == 1
    got = float(qY[0, 0] - qY[0, 1])
    err = abs(got - (expect - 64) / 2)
    print(f"topic_infer N_k order K = {K}: qY_0 - qY_1 = {got / 2.0 ** -47:.4f} * 2^-47, expected {(expect - 64) / 2 / 2.0 ** -47:.0f}; "
          f"error / bar = {err / 2.0 ** -50:.3f}")
    assert err <= 2.0 ** -50, (K, got, expect)
    assert np.all(label[:64] == 0) and label[64] == 1
