"""Order and threshold queries on the device (lc_ctx_score_quantiles, lc_ctx_score_counts, lc_ctx_rows_beyond, DESIGN
4.13.1): quantiles by radix select, counts at thresholds, the rows beyond a threshold in context order.

The kernels are driven through the C ABI alone: lc_ctx_set_data + lc_ctx_set_qz put any column content on the device
(lc_ctx_set_qz copies the bytes: non-finite values, signed zeros and denormals arrive unchanged).  The reference is numpy
(tests/score_select_ref.py).  Every comparison is exact: ranks, counts, groups and rows equal, values and scores bitwise
equal; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import libcluster_amd as lc
import score_select_ref as ref
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

TOP_CHUNK_ROWS = 8192  # lck::TOP_CHUNK_ROWS: the chunk of the compaction and of the histogram blocks
BIG_N = 3 * TOP_CHUNK_ROWS + 17
SIZES = [1, 15, 16, 17, 63, 64, 65, 257, BIG_N]
NAMES = ["normal", "equal", "duplicates", "low8", "signs", "zeros", "inf", "denormal", "nan40", "allnan"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _contents(rng, N):
    """one column per content of NAMES, (N, 10)"""
    low8 = (np.float64(1.5).view(np.uint64) + rng.integers(0, 256, N).astype(np.uint64)).view(np.float64)  # the last pass decides
    signs = rng.integers(-4, 5, N) * 0.5 + np.where(rng.random(N) < 0.5, 1e-3, -1e-3)
    zeros = np.where(rng.random(N) < 0.5, 0.0, -0.0)
    inf = rng.standard_normal(N)
    inf[rng.random(N) < 0.3] = np.inf
    inf[rng.random(N) < 0.3] = -np.inf
    den = rng.integers(-1000, 1001, N) * 5e-324
    nan = rng.standard_normal(N)
    nan[rng.random(N) < 0.4] = np.nan
    cols = [rng.standard_normal(N), np.full(N, 0.5), rng.integers(0, 3, N) / 4.0, low8, signs, zeros, inf, den, nan,
            np.full(N, np.nan)]
    assert len(cols) == len(NAMES)
    return np.stack(cols, axis=1)


def _probs(N):
    sixteen = [0.9, 0.1, 0.5, 0.5, 1.0, 0.0, 0.33, 0.1, 0.999, 0.001, 0.75, 0.25, 0.5, 2.0 / 3.0, 0.9, 0.05]  # repeats, unsorted
    exact = [0.25, 0.5, 0.75, 1.0 / N, 0.125]  # p n is an exact integer for the N that are multiples of 8 (and 1 / N * N = 1)
    return [[0.0, 1.0], [0.5], sixteen, exact, [1e-12]]  # 1e-12: the rank is 0


def _same_quantiles(got, want):
    count, rank, value = want
    assert got.count.dtype == np.int64 and got.rank.dtype == np.int64 and got.value.dtype == np.float64
    assert got.rank.shape == rank.shape and got.value.shape == value.shape
    assert np.array_equal(got.count, count), (got.count, count)
    assert np.array_equal(got.rank, rank), (got.rank, rank)
    ok = rank >= 0
    assert np.array_equal(_bits(got.value)[ok], _bits(value)[ok]), (got.value, value)  # bitwise, the sign of zero included
    assert np.all(np.isnan(got.value[~ok]))


def _thresholds(col):
    """up to 16: present values, values between them, +-inf, -0.0"""
    s = np.unique(col[np.isfinite(col)])
    t = [-np.inf, np.inf, -0.0]
    if s.size:
        pick = s[np.linspace(0, s.size - 1, min(s.size, 6)).astype(int)]
        t += list(pick) + list((pick[:-1] + pick[1:]) / 2) + [s[0] - 1.0, s[-1] + 1.0]
    return np.array(t[:capi.QUANTILES_MAX])


def _same_rows(got, want, capacity):
    total, group, row, score = want
    n = min(total, capacity)
    assert got.total == total  # (exact also when the output is truncated)
    assert got.group.dtype == np.int32 and got.row.dtype == np.int64
    assert got.group.shape == got.row.shape == got.score.shape == (n,)
    assert np.array_equal(got.group, group[:n]) and np.array_equal(got.row, row[:n])
    assert np.array_equal(_bits(got.score), _bits(score[:n]))


def _check_rows_beyond(ctx, q, sizes, c, thr, above, labels=None, by_label=False):
    want = ref.beyond(q[:, c], sizes, thr, above, labels, c)
    total = want[0]
    for cap in sorted({0, max(total - 1, 0), total, total + 5}):
        _same_rows(ctx.rows_beyond(thr, by="qz", col=c, above=above, limit=cap, by_label=by_label), want, cap)
    return total


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


@pytest.mark.parametrize("N", SIZES)
def test_one_group_every_content(ctx, N):
    rng = np.random.default_rng(2000 + N)
    ctx.set_data(rng.standard_normal((N, 2)))
    q = _contents(rng, N)
    ctx.set_qz(q)
    for probs in _probs(N):
        got = ctx.score_quantiles(probs, by="qz")
        _same_quantiles(got, ref.quantiles(q, probs))
        again = ctx.score_quantiles(probs, by="qz")  # the same query twice: the same bits
        for x, y in zip(got, again):
            assert x.tobytes() == y.tobytes()
        # consistency: at least rank + 1 scores are at most the value of that rank
        for c in range(q.shape[1]):
            if got.count[c] == 0:
                continue
            v = got.value[c][:capi.QUANTILES_MAX]
            cnt = ctx.score_counts(v, by="qz")
            assert np.all(cnt.atmost[c] >= got.rank[c] + 1)
    assert ctx.score_quantiles([0.5], by="qz").count[NAMES.index("allnan")] == 0
    _same_quantiles(ctx.score_quantiles([0.3, 0.6], by="qz", ncols=3), ref.quantiles(q[:, :3], [0.3, 0.6]))  # fewer columns
    for c in range(q.shape[1]):
        thr = _thresholds(q[:, c])
        got = ctx.score_counts(thr, by="qz")
        count, atmost = ref.counts(q, thr)
        assert got.count.dtype == np.int64 and got.atmost.dtype == np.int64
        assert np.array_equal(got.count, count) and np.array_equal(got.atmost, atmost), (NAMES[c], got.atmost, atmost)
    got = ctx.score_counts([0.5], by="qz", ncols=2)
    assert got.atmost.shape == (2, 1) and np.array_equal(got.atmost, ref.counts(q[:, :2], [0.5])[1])
    for c in range(q.shape[1]):
        s = q[:, c]
        fin = s[np.isfinite(s)]
        mid = np.median(fin) if fin.size else 0.0
        totals = set()
        for above in (False, True):
            for thr in (-np.inf, np.inf, mid, -0.0):  # none / some / all rows, depending on the column and the direction
                totals.add(_check_rows_beyond(ctx, q, [N], c, thr, above))
        if NAMES[c] == "normal" and N > 2:
            assert 0 in totals or N in totals
            assert any(0 < t < N for t in totals)
    assert ctx.rows_beyond(-np.inf, by="qz", col=0, above=True).total == N  # every row
    assert ctx.rows_beyond(-1e300, by="qz", col=0).total == 0  # none


@pytest.mark.parametrize("sizes", [(5, 0, TOP_CHUNK_ROWS + 3), (16, 1, 48)])
def test_groups_and_pad_rows(ctx, sizes):
    """ragged groups with an empty one: the pad rows of EVERY group hold 0.0 in the qZ, below every score here -- each
    would be counted, selected as the minimum and flagged"""
    rng = np.random.default_rng(sum(sizes))
    ctx.set_data([rng.standard_normal((n, 2)) for n in sizes])
    N = sum(sizes)
    q = np.stack([rng.uniform(0.5, 2.0, N), np.arange(N) + 1.0, N - np.arange(N) + 0.0, np.full(N, 3.0),
                  np.where(rng.random(N) < 0.4, np.nan, rng.uniform(1.0, 2.0, N))], axis=1)  # strictly positive or NaN
    ctx.set_qz(np.split(q, np.cumsum(sizes)[:-1]))
    for probs in _probs(N):
        got = ctx.score_quantiles(probs, by="qz")
        _same_quantiles(got, ref.quantiles(q, probs))
        assert np.all(got.value > 0.0)
    assert np.array_equal(ctx.score_quantiles([0.0], by="qz").count[:4], [N] * 4)
    thr = np.array([0.0, 0.25, 1.0, 1.5, 3.0, N / 2.0, np.inf, -np.inf])
    got = ctx.score_counts(thr, by="qz")
    count, atmost = ref.counts(q, thr)
    assert np.array_equal(got.count, count) and np.array_equal(got.atmost, atmost)
    assert np.all(got.atmost[:, :2] == 0)  # no pad row
    for c in range(q.shape[1]):
        for above in (False, True):
            for t in (0.25, 1.5, N / 2.0, np.inf, -np.inf):
                _check_rows_beyond(ctx, q, sizes, c, t, above)
    flagged = ctx.rows_beyond(np.inf, by="qz", col=0)
    assert flagged.total == N
    if 0 in sizes:
        assert not np.any(flagged.group == sizes.index(0))
    assert np.array_equal(np.bincount(flagged.group, minlength=len(sizes)), sizes)


# ---- models -----------------------------------------------------------------------------------------------------------
def _mixture(rng, N, D, K, spread=6.0):
    mu = rng.normal(0, spread, (K, D))
    return mu[rng.integers(0, K, N)] + rng.normal(size=(N, D))


@pytest.fixture(scope="module")
def fitted():
    """fixed-K VBEM on the device: (model, training rows)"""
    rng = np.random.default_rng(21)
    K = 4
    X = _mixture(rng, 900, 5, K)
    with capi.Context(0) as c:
        c.set_data(X)
        c.set_qz(rng.dirichlet(np.ones(K), X.shape[0]))
        _, _, m = c.vbem(capi.W_DIRICHLET, fixed_iters=6, ckind=capi.C_GAUSSWISH)
        yield m, X
        m.close()


def test_a_context_whose_blocks_are_all_empty(fitted):
    model, X = fitted
    K = model.dims()[1]
    with capi.Context(0) as c:
        c.set_data([np.zeros((0, X.shape[1])), np.zeros((0, X.shape[1]))])
        model.predict_context(c, groups=[0, 0])
        for by, cols in (("logp", 1), ("logz", 1), ("qz", K)):
            got = c.score_quantiles([0.0, 0.5], by=by)
            assert got.value.shape == (cols, 2)
            assert np.all(got.count == 0) and np.all(got.rank == -1) and np.all(np.isnan(got.value))
            cnt = c.score_counts([0.0, np.inf], by=by)
            assert cnt.atmost.shape == (cols, 2) and np.all(cnt.count == 0) and np.all(cnt.atmost == 0)
            fl = c.rows_beyond(np.inf, by=by)
            assert fl.total == 0 and fl.row.size == 0 and fl.group.size == 0 and fl.score.size == 0


def test_label_filter_with_a_label_no_row_carries(fitted):
    model, X = fitted
    K = model.dims()[1]
    rng = np.random.default_rng(22)
    with capi.Context(0) as c:
        c.set_data(X)
        model.predict_context(c)
        label, logZ, logp = c.get_predictions(0, 0, X.shape[0])
        N = X.shape[0]
        for by, col in (("logz", logZ), ("logp", logp)):
            col2 = col.reshape(-1, 1)
            probs = [0.0, 0.001, 0.1, 0.5, 1.0]
            got = c.score_quantiles(probs, by=by)
            _same_quantiles(got, ref.quantiles(col2, probs))
            thr = np.concatenate([got.value[0], [np.inf, -np.inf]])
            cnt = c.score_counts(thr, by=by)
            rc, ra = ref.counts(col2, thr)
            assert np.array_equal(cnt.count, rc) and np.array_equal(cnt.atmost, ra)
            for above in (False, True):
                want = ref.beyond(col, [N], got.value[0, 2], above)
                _same_rows(c.rows_beyond(got.value[0, 2], by=by, above=above), want, 1 << 20)
        # values of the test's own in the columns (the labels stay those of the prediction), ties included
        q = np.round(rng.standard_normal((N, K)), 1)
        c.set_qz(q)
        probs = [0.0, 0.5, 0.9, 1.0]
        _same_quantiles(c.score_quantiles(probs, by="qz", by_label=True), ref.quantiles(q, probs, labels=label))
        _same_quantiles(c.score_quantiles(probs, by="qz", ncols=2, by_label=True), ref.quantiles(q[:, :2], probs, labels=label))
        thr = [-0.5, 0.0, 0.5, np.inf]
        cnt = c.score_counts(thr, by="qz", by_label=True)
        rc, ra = ref.counts(q, thr, labels=label)
        assert np.array_equal(cnt.count, rc) and np.array_equal(cnt.atmost, ra)
        assert np.array_equal(cnt.count, np.bincount(label, minlength=K))
        for k in range(K):
            for above in (False, True):
                _check_rows_beyond(c, q, [N], k, 0.1, above, labels=label, by_label=True)
    # only the rows of ONE label: every other column has no participating row
    k0 = int(np.argmax(np.bincount(label, minlength=K)))
    rows = X[label == k0]
    with capi.Context(0) as c:
        c.set_data(rows)
        model.predict_context(c)
        lab = c.get_predictions(0, 0, rows.shape[0], logp=False)[0]
        assert np.all(lab == k0)
        q = rng.standard_normal((rows.shape[0], K))
        c.set_qz(q)
        got = c.score_quantiles([0.0, 0.5, 1.0], by="qz", by_label=True)
        _same_quantiles(got, ref.quantiles(q, [0.0, 0.5, 1.0], labels=lab))
        empty = np.arange(K) != k0
        assert np.all(got.count[empty] == 0) and np.all(got.rank[empty] == -1) and np.all(np.isnan(got.value[empty]))
        assert got.count[k0] == rows.shape[0]
        cnt = c.score_counts([np.inf], by="qz", by_label=True)
        assert np.all(cnt.count[empty] == 0) and np.all(cnt.atmost[empty] == 0) and cnt.atmost[k0, 0] == rows.shape[0]
        other = int(np.flatnonzero(empty)[0])
        assert c.rows_beyond(np.inf, by="qz", col=other, by_label=True).total == 0
        assert c.rows_beyond(np.inf, by="qz", col=k0, by_label=True).total == rows.shape[0]


@pytest.mark.parametrize("algo", ["bgmm", "dgmm"])
def test_end_to_end_and_nothing_disturbed(algo):
    rng = np.random.default_rng(31)
    X = _mixture(rng, 3000, 5, 3)
    _, model, _ = capi.learn(capi.ALGO_BGMM if algo == "bgmm" else capi.ALGO_DGMM, X)
    try:
        p = model.predict(X)
        probs = [0.001, 0.01, 0.5, 0.999]
        got = model.logp_quantiles(X, probs)
        assert isinstance(got, lc.ScoreQuantiles)
        _same_quantiles(got, ref.quantiles(p.logp.reshape(-1, 1), probs))
        assert np.array_equal(got.value[0], np.quantile(p.logp, probs, method="inverted_cdf"))
        thr = got.value[0, 1]
        fl = model.flag(X, thr)
        assert isinstance(fl, lc.FlaggedRows)
        idx = np.flatnonzero(p.logp <= thr)
        assert fl.total == idx.size == got.rank[0, 1] + 1
        assert np.all(fl.group == 0) and np.array_equal(fl.row, idx) and np.array_equal(_bits(fl.score), _bits(p.logp[idx]))
        cut = model.flag(X, thr, limit=7)
        assert cut.total == idx.size and np.array_equal(cut.row, idx[:7])
        with capi.Context(0) as c:
            c.set_data(X)
            model.predict_context(c, keep_qz=True)
            K = c.dims()[3]

            def snapshot():
                tops = [c.top_rows(5, by=by, largest=False) for by in ("qz", "logz", "logp")]
                return [a.tobytes() for t in tops for a in t] + [a.tobytes() for a in c.get_predictions(0, 0, X.shape[0])] \
                    + [c.get_qz([X.shape[0]])[0].tobytes()]

            before = snapshot()
            c.score_quantiles(probs, by="logp")
            c.score_quantiles(probs, by="qz", by_label=True)
            c.score_counts([thr, 0.0], by="logz")
            c.score_counts([0.5], by="qz", ncols=K)
            c.rows_beyond(thr, by="logp")
            c.rows_beyond(0.5, by="qz", col=K - 1, above=True, by_label=True)
            assert snapshot() == before
    finally:
        model.close()


def _raw_error(fn, *args):
    rc = fn(*args)
    return rc, capi.lib().lc_last_error().decode()


def test_errors(fitted):
    model, X = fitted
    K = model.dims()[1]
    L = capi.lib()
    one = (C.c_double * 1)(0.5)
    i64 = (C.c_int64 * 64)()
    dbl = (C.c_double * 64)()
    with capi.Context(0) as c:
        for call in (lambda: c.score_quantiles([0.5], by="qz", ncols=1), lambda: c.score_counts([0.5], by="qz", ncols=1),
                     lambda: c.rows_beyond(0.5, by="qz", ncols=1)):
            with pytest.raises(ValueError, match="no observations"):  # a context without data
                call()
        c.set_data(X[:50])
        c.set_qz(np.ones((50, K)))
        # an unknown source (the binding never passes one)
        rc, msg = _raw_error(L.lc_ctx_score_quantiles, c._h, 7, 1, 0, one, 1, i64, i64, dbl)
        assert rc == capi.LC_EINVAL and "unknown ranking source" in msg
        rc, msg = _raw_error(L.lc_ctx_score_counts, c._h, -1, 1, 0, one, 1, i64, i64)
        assert rc == capi.LC_EINVAL and "unknown ranking source" in msg
        rc, msg = _raw_error(L.lc_ctx_rows_beyond, c._h, 3, 1, 0, 0, 0.5, 0, 0, i64, None, None, None)
        assert rc == capi.LC_EINVAL and "unknown ranking source" in msg
        for ncols in (0, K + 1):
            with pytest.raises(ValueError, match="ncols must be in 1 ... K"):
                c.score_quantiles([0.5], by="qz", ncols=ncols)
            with pytest.raises(ValueError, match="ncols must be in 1 ... K"):
                c.score_counts([0.5], by="qz", ncols=ncols)
            with pytest.raises(ValueError, match="ncols must be in 1 ... K"):
                c.rows_beyond(0.5, by="qz", ncols=ncols)
        for call in (lambda **k: c.score_quantiles([0.5], **k), lambda **k: c.score_counts([0.5], **k),
                     lambda **k: c.rows_beyond(0.5, **k)):
            with pytest.raises(ValueError, match="no prediction.*no labels to rank by"):
                call(by="qz", by_label=True)
            for by in ("logz", "logp"):
                with pytest.raises(ValueError, match="no prediction"):
                    call(by=by)
            with pytest.raises(ValueError, match="by must be"):
                call(by="logq")
        model.predict_context(c)
        for call in (lambda **k: c.score_quantiles([0.5], **k), lambda **k: c.score_counts([0.5], **k),
                     lambda **k: c.rows_beyond(0.5, **k)):
            for by in ("logz", "logp"):
                with pytest.raises(ValueError, match="by_label ranks the columns of qZ"):
                    call(by=by, by_label=True)
        # the arguments of the new calls
        for probs in ([], [0.5] * 17):
            with pytest.raises(ValueError, match="nprobs must be in 1 ... 16"):
                c.score_quantiles(probs)
        for bad in (-0.1, 1.0000001, np.nan):
            with pytest.raises(ValueError, match=r"prob must be in \[0, 1\]"):
                c.score_quantiles([0.5, bad])
        for thr in ([], [0.5] * 17):
            with pytest.raises(ValueError, match="nthr must be in 1 ... 16"):
                c.score_counts(thr)
        with pytest.raises(ValueError, match="threshold is NaN"):
            c.score_counts([0.5, np.nan])
        with pytest.raises(ValueError, match="threshold is NaN"):
            c.rows_beyond(np.nan)
        for col in (-1, K):
            with pytest.raises(ValueError, match="col must be in"):
                c.rows_beyond(0.5, by="qz", col=col)
        with pytest.raises(ValueError, match="col must be in"):
            c.rows_beyond(0.5, by="logp", col=1)
        with pytest.raises(ValueError, match="capacity must not be negative"):
            c.rows_beyond(0.5, limit=-1)
        # NULL outputs with room asked for: the count only
        total = C.c_int64(-1)
        assert L.lc_ctx_rows_beyond(c._h, capi.RANK_LOGP, 1, 0, 0, float("inf"), 0, 10, C.byref(total), None, None, None) == capi.LC_OK
        assert total.value == 50
        assert c.score_quantiles([0.5]).count[0] == 50
        c.set_data(X[:5])  # new observations: the prediction is gone
        with pytest.raises(ValueError, match="no prediction"):
            c.score_quantiles([0.5])


def test_logp_of_a_prediction_without_log_density():
    """a two-level model's prediction leaves logZ and labels, no logp"""
    import lc_oracle as o
    import topic_infer_ref as tir

    rng = np.random.default_rng(3)
    X, _, _ = tir.synthetic_documents(rng, 2, 6, 40, 2, 3, 2)
    m = lc.learnSCM(X, trunc=3, qY0=[o.random_qY(6, 3, rng) for _ in range(2)], return_model=True)[-1]
    with capi.Context(0) as c:
        c.set_data(X[1])
        m.predict_context(c, max_sweeps=4, tol=-1.0, keep_qz=True)
        assert c.score_quantiles([0.5], by="logz").count[0] == sum(d.shape[0] for d in X[1])
        for call in (lambda: c.score_quantiles([0.5], by="logp"), lambda: c.score_counts([0.5], by="logp"),
                     lambda: c.rows_beyond(0.5, by="logp")):
            with pytest.raises(ValueError, match="no log density"):
                call()
