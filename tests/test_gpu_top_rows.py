"""Ranking on the device (lc_ctx_top_rows, lc_model_exemplars): the m best rows of each column.

The kernel is driven through the C ABI alone: lc_ctx_set_data + lc_ctx_set_qz put any column content on the device
(lc_ctx_set_qz copies the bytes: non-finite values and signed zeros arrive unchanged), lc_ctx_top_rows ranks it.  The
reference is numpy, np.lexsort((position, -+score))[:m] over the valid rows: the order is total, so indices must be equal and
scores bitwise equal.  Exemplars are checked against the oracle's Eloglike with the model's posteriors set into oracle
objects, never against the library."""
import numpy as np
import pytest

import lc_oracle as o
from libcluster_amd import capi
from rank_select_cases import top_rows_ref as _ref

pytestmark = pytest.mark.gpu

TOP_CHUNK_ROWS = 8192  # lck::TOP_CHUNK_ROWS (tests/test_top_rows_host.py pins it to the source)
BIG_N = 3 * TOP_CHUNK_ROWS + 17


# ---- the reference --------------------------------------------------------------------------------------------------
# (the reference itself lives in tests/rank_select_cases.py: the launcher-level tests rank with it too)


def _same(got, want):
    assert got.count.dtype == np.int32 and got.group.dtype == np.int32 and got.row.dtype == np.int64
    assert got.count.shape == want.count.shape and got.score.shape == want.score.shape
    assert np.array_equal(got.count, want.count), (got.count, want.count)
    assert np.array_equal(got.group, want.group)
    assert np.array_equal(got.row, want.row)
    ok = ~np.isnan(want.score)
    assert np.array_equal(got.score.view(np.int64)[ok], want.score.view(np.int64)[ok])  # bitwise
    assert np.all(np.isnan(got.score[~ok]))


def _columns(rng, N):
    """five columns: random, strictly ascending (every row would insert), strictly descending, all equal, duplicates"""
    asc = np.arange(N, dtype=np.float64) * 0.25 - 3.0
    return np.stack([rng.standard_normal(N), asc, -asc, np.full(N, 0.5), rng.integers(0, max(2, N // 7), N) / 4.0], axis=1)


def _special(rng, N):
    """four columns: +0.0 / -0.0 mixed, +-inf among finite values, some NaN, all NaN"""
    z = np.where(rng.random(N) < 0.5, 0.0, -0.0)
    inf = rng.standard_normal(N)
    inf[rng.random(N) < 0.3] = np.inf
    inf[rng.random(N) < 0.3] = -np.inf
    nan = rng.standard_normal(N)
    nan[rng.random(N) < 0.4] = np.nan
    return np.stack([z, inf, nan, np.full(N, np.nan)], axis=1)


@pytest.fixture(scope="module")
def ctx():
    with capi.Context(0) as c:
        yield c


@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 257, BIG_N])
def test_one_group_every_content(ctx, N):
    rng = np.random.default_rng(1000 + N)
    ctx.set_data(rng.standard_normal((N, 2)))
    for make in (_columns, _special):
        q = make(rng, N)
        ctx.set_qz(q)
        for m in (1, 2, 63, 64):
            for largest in (True, False):
                _same(ctx.top_rows(m, largest=largest), _ref(q, [N], m, largest))
    q = _columns(rng, N)
    ctx.set_qz(q)
    for ncols in (1, 3):  # fewer columns than the qZ holds
        _same(ctx.top_rows(2, ncols=ncols, largest=False), _ref(q[:, :ncols], [N], 2, False))
    a, b = ctx.top_rows(64), ctx.top_rows(64)  # the same query twice: the same bits
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_rows_that_meet_only_in_the_merge(ctx):
    """the best rows spread one per wave share and chunk, and a column whose every row beats the ones before it in the
    scan of its wave (the insertion's worst case)"""
    N = BIG_N
    rng = np.random.default_rng(5)
    ctx.set_data(np.zeros((N, 2)))
    spread = rng.standard_normal(N)
    spread[np.arange(0, N, 2048 - 1)] += 100.0
    # the scan of a wave takes the steps of 512 rows in order and, within a step, the fourth 128 rows first, odd rows before
    # even ones, the highest lane (pair of rows) first: values that rise in that order
    r = np.arange(N)
    e = 2 * (r % 512 // 128) + r % 2
    saw = (r // 512) * 512.0 + (7 - e) * 64 + (63 - r % 128 // 2)
    q = np.stack([spread, saw, -saw], axis=1)
    ctx.set_qz(q)
    for m in (1, 13, 64):
        for largest in (True, False):
            _same(ctx.top_rows(m, largest=largest), _ref(q, [N], m, largest))


@pytest.mark.parametrize("sizes", [(5, 0, 37), (16, 1, 48)])
def test_groups_pad_rows_and_fillers(ctx, sizes):
    rng = np.random.default_rng(sum(sizes))
    ctx.set_data([rng.standard_normal((n, 2)) for n in sizes])
    N = sum(sizes)
    q = np.stack([rng.uniform(0.5, 2.0, N), np.arange(N) + 1.0, N - np.arange(N) + 0.0, np.full(N, 3.0)], axis=1)  # strictly positive
    ctx.set_qz(np.split(q, np.cumsum(sizes)[:-1]))
    for m in (1, 2, 63, 64):  # 63, 64: more than there are rows
        for largest in (True, False):
            got = ctx.top_rows(m, largest=largest)
            _same(got, _ref(q, sizes, m, largest))
            assert np.all(got.count == min(m, N))
            # no pad row (q = 0 there: each would win a smallest-m query) and nothing from the empty group
            assert np.all(got.score[:, :min(m, N)] > 0.0)
            if 0 in sizes:
                assert not np.any(got.group == sizes.index(0))
    got = ctx.top_rows(64, largest=False)
    assert np.all(got.group[:, N:] == -1) and np.all(got.row[:, N:] == -1) and np.all(np.isnan(got.score[:, N:]))


# ---- models -----------------------------------------------------------------------------------------------------------
WCLS = {capi.W_DIRICHLET: lambda: o.Dirichlet(), capi.W_STICKBREAK: lambda: o.StickBreak(),
        capi.W_GDIRICHLET: lambda: o.GDirichlet()}
CCLS = {capi.C_GAUSSWISH: o.GaussWish, capi.C_NORMGAMMA: o.NormGamma, capi.C_EXPGAMMA: o.ExpGamma}


def _mixture(rng, N, D, K, family=capi.C_GAUSSWISH, spread=4.0, use=None):
    mu = rng.normal(0, spread, (K, D))
    z = rng.integers(0, K, N) if use is None else rng.choice(use, N)
    if family == capi.C_EXPGAMMA:
        rate = rng.uniform(0.3, 3.0, (K, D))
        return rng.exponential(1.0 / rate[z])
    if family == capi.C_NORMGAMMA:
        return mu[z] + rng.normal(size=(N, D)) * rng.uniform(0.5, 2.0, (K, D))[z]
    return mu[z] + rng.normal(size=(N, D))


def _start(Xs, K, seed):
    rng = np.random.default_rng(seed)
    return [rng.dirichlet(np.ones(K), x.shape[0]) for x in Xs]


def _fit(Xs, wkind, ckind, K, iters=6, seed=0):
    """fixed-K VBEM on the device -> (model, training context)"""
    ctx = capi.Context(0)
    ctx.set_data(Xs)
    ctx.set_qz(_start(Xs, K, seed))
    _, _, m = ctx.vbem(wkind, fixed_iters=iters, ckind=ckind)
    return m, ctx


def _oracle(m):
    """the model's posteriors in oracle objects: (weights per group, clusters)"""
    J, K, D = m.dims()
    wk, ck = m.kinds()
    ws = []
    for j in range(J):
        w = WCLS[wk]()
        w.update(m.weights(j)[1])
        ws.append(w)
    cls = []
    for k in range(K):
        p = m.cluster(k)
        c = CCLS[ck](1.0, D)
        if ck == capi.C_GAUSSWISH:
            c.nu, c.beta, c.m, c.iW, c.logdW = p["nu"], p["beta"], p["mean"], p["iW"], p["logdW"]
        elif ck == capi.C_NORMGAMMA:
            c.nu, c.beta, c.m, c.L, c.logL = p["nu"], p["beta"], p["mean"], p["L"], p["logL"]
        else:
            c.a, c.ib, c.logb = p["a"], p["ib"], p["logb"]
        c.N = p["N"]
        cls.append(c)
    return ws, cls


# (name, weights, family, D, K, training rows per group, blocks to rank, learned group of every block, m, seed)
CASES = {
    "gausswish": (capi.W_DIRICHLET, capi.C_GAUSSWISH, 5, 4, (600,), (300,), None, 10, 11),
    "normgamma": (capi.W_DIRICHLET, capi.C_NORMGAMMA, 5, 4, (600,), (301,), None, 10, 12),
    "expgamma": (capi.W_STICKBREAK, capi.C_EXPGAMMA, 5, 3, (600,), (299,), None, 10, 13),
    "grouped": (capi.W_GDIRICHLET, capi.C_GAUSSWISH, 5, 4, (500, 400), (150, 0, 117, 33), (0, 1, 1, 0), 8, 14),
}
MARGIN = 1e-6


def _case(name):
    wk, ck, D, K, ntrain, nblocks, groups, m, seed = CASES[name]
    rng = np.random.default_rng(seed)
    X = _mixture(rng, sum(ntrain) + sum(nblocks), D, K, ck)
    cut = np.cumsum(ntrain + nblocks)[:-1]
    parts = np.split(X, cut)
    return parts[:len(ntrain)], parts[len(ntrain):], groups, m


def _expected(ws, cls, blocks, groups, m):
    """the oracle's exemplars: per cluster k the m rows with the largest Eloglike_k among the rows whose oracle label is
    k.  Exact indices need a margin: asserted here on the oracle's numbers."""
    K = len(cls)
    sizes = [b.shape[0] for b in blocks]
    X = np.vstack(blocks)
    E = np.stack([c.Eloglike(X).reshape(-1) for c in cls], axis=1)  # Eloglike_k(x_n) = c_k + L_nk without the weights
    g = np.repeat([0] * len(blocks) if groups is None else list(groups), sizes)
    Elw = np.stack([w.Elogweight() for w in ws])
    v = E + Elw[g]
    label = np.argmax(v, axis=1)
    top2 = np.sort(v, axis=1)[:, -2:]
    assert np.min(top2[:, 1] - top2[:, 0]) > MARGIN  # every row's label is clear
    for k in range(K):
        s = np.sort(E[label == k, k])[::-1][:m + 1]
        assert s.size < 2 or np.min(-np.diff(s)) > MARGIN, (k, s)  # ... and so is the order around the cut
    return _ref(E, sizes, m, True, labels=label), label


def _check_exemplars(got, want):
    assert np.array_equal(got.count, want.count), (got.count, want.count)
    assert np.array_equal(got.group, want.group) and np.array_equal(got.row, want.row)
    ok = ~np.isnan(want.score)
    np.testing.assert_allclose(got.score[ok], want.score[ok], rtol=1e-9, atol=0)
    assert np.all(np.isnan(got.score[~ok]))


@pytest.fixture(scope="module")
def fitted():
    """every case's model, fitted once"""
    out = {}
    for name, (wk, ck, D, K, *_rest) in CASES.items():
        train, blocks, groups, m = _case(name)
        model, tctx = _fit(train, wk, ck, K, seed=CASES[name][-1])
        out[name] = (model, tctx, blocks, groups, m)
    yield out
    for model, tctx, *_ in out.values():
        model.close()
        tctx.close()


@pytest.mark.parametrize("name", list(CASES))
def test_exemplars_against_the_oracle(fitted, name):
    model, _, blocks, groups, m = fitted[name]
    ws, cls = _oracle(model)
    want, label = _expected(ws, cls, blocks, groups, m)
    with capi.Context(0) as c:
        c.set_data(blocks)
        got = model.exemplars_context(c, m, groups)
        _check_exemplars(got, want)
        # the side effect is that of predict_context(ctx, groups): its labels are readable, and are the oracle's
        lab = np.concatenate([c.get_predictions(j, 0, b.shape[0], logp=False)[0] for j, b in enumerate(blocks)])
        assert np.array_equal(lab, label)
    assert np.all(got.count <= m) and got.score.shape == (model.dims()[1], m)


def test_exemplars_and_outliers_of_host_rows(fitted):
    model, _, blocks, groups, m = fitted["grouped"]
    ws, cls = _oracle(model)
    want, _ = _expected(ws, cls, blocks, groups, m)
    _check_exemplars(model.exemplars(blocks, m, groups), want)  # a list of blocks
    one, _ = _expected(ws, cls, blocks[:1], None, m)
    _check_exemplars(model.exemplars(blocks[0], m), one)  # one array
    for X, g in ((blocks, groups), (blocks[2], None)):
        preds = model.predict(X, groups=g)
        preds = preds if isinstance(preds, list) else [preds]
        logp = np.concatenate([p.logp for p in preds])
        sizes = [p.logp.size for p in preds]
        for mm in (1, 7, 64):
            got = model.outliers(X, mm, groups=g)
            order = np.argsort(logp, kind="stable")[:mm]
            grp = np.repeat(np.arange(len(sizes)), sizes)[order]
            row = np.concatenate([np.arange(n) for n in sizes])[order]
            assert got.count.shape == (1,) and got.count[0] == order.size
            assert np.array_equal(got.group[0, :order.size], grp) and np.array_equal(got.row[0, :order.size], row)
            assert np.array_equal(got.score[0, :order.size], logp[order])


def test_label_filter_and_prediction_buffers(fitted):
    """rows drawn from two of the four clusters: the other columns get few or no labelled rows"""
    model, _, _, _, _ = fitted["gausswish"]
    K = model.dims()[1]
    wk, ck, D, _, ntrain, nblocks, _, _, seed = CASES["gausswish"]
    rng = np.random.default_rng(seed)  # the stream of _case: the same cluster centres
    X = _mixture(rng, 333, D, K, ck, use=[1, 3])
    with capi.Context(0) as c:
        c.set_data(X)
        model.predict_context(c)
        label, logZ, logp = c.get_predictions(0, 0, 333)
        assert np.min(np.bincount(label, minlength=K)) < 64  # (a column with fewer labelled rows than the longest list)
        for by, col in (("logz", logZ), ("logp", logp)):
            for m in (1, 7, 64):
                for largest in (True, False):
                    _same(c.top_rows(m, by=by, largest=largest), _ref(col.reshape(-1, 1), [333], m, largest))
        # values of the test's own in the columns (the labels stay those of the prediction), ties included
        q = np.round(rng.standard_normal((333, K)), 1)
        c.set_qz(q)
        for m in (1, 5, 64):
            for largest in (True, False):
                got = c.top_rows(m, largest=largest, by_label=True)
                _same(got, _ref(q, [333], m, largest, labels=label))
                _same(c.top_rows(m, ncols=2, largest=largest, by_label=True), _ref(q[:, :2], [333], m, largest, labels=label))
        assert np.array_equal(got.count, np.minimum(64, np.bincount(label, minlength=K)))


def test_errors(fitted):
    model, _, blocks, _, _ = fitted["gausswish"]
    K = model.dims()[1]
    with capi.Context(0) as c:
        with pytest.raises(ValueError, match="no observations"):  # a context without data
            c.top_rows(3, ncols=1)
        with pytest.raises(ValueError, match="no observations"):
            model.exemplars_context(c, 3)
        c.set_data(blocks[0])
        c.set_qz(np.ones((blocks[0].shape[0], K)))
        for m in (0, 65):
            with pytest.raises(ValueError, match="m must be"):
                c.top_rows(m)
            with pytest.raises(ValueError, match="m must be"):
                model.exemplars_context(c, m)
        for ncols in (0, K + 1):
            with pytest.raises(ValueError, match="ncols"):
                c.top_rows(3, ncols=ncols)
        with pytest.raises(ValueError, match="no prediction"):
            c.top_rows(3, by_label=True)
        for by in ("logz", "logp"):
            with pytest.raises(ValueError, match="no prediction"):
                c.top_rows(3, by=by)
        model.predict_context(c)
        for by in ("logz", "logp"):
            with pytest.raises(ValueError, match="by_label"):
                c.top_rows(3, by=by, by_label=True)
        assert c.top_rows(3, by="logp").count[0] == 3
        c.set_data(blocks[0][:5])  # new observations: the prediction is gone
        with pytest.raises(ValueError, match="no prediction"):
            c.top_rows(3, by="logp")
