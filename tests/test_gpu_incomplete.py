"""Rows whose unknown columns differ from row to row (lc_model_predict_incomplete): a NaN marks an unknown
value; the call fills it with E[x_unknown | x_known] and leaves log p(x_known) per row.

The reference is numpy / scipy per row on the model's posteriors (m.cluster(k)) and the expected weights of the oracle's
weight objects (tests/incomplete_ref.py, direct()): the Student-t marginal of the row's observed columns and the linear
expert m_b + iW_ba iW_aa^-1 (x_a - m_a) per cluster, mixed by the responsibilities.  Never the device, never the emulation
of its route.  Models and recipe are those of tests/test_gpu_conditional.py: six fixed-K VBEM iterations on the device from
a Dirichlet(1) start, 300 held-out rows.

Bars (those of tests/test_gpu_conditional.py): logp to rtol 1e-10, filled values to |d| <= 1e-9 S_n with
S_n = max_{k,b} |M_k(x_n)_b| from the reference.  One exception, logp of the model that sits 1e3 away from the origin
(cond(iW) about 2e5): max(1e-10, 4 E) with E the largest relative logp error of the numpy emulation of the route against
the reference on the same rows, computed here -- the normal-equations form pays for the conditioning, and the factor 4
covers the device's own summation order in d_full^2.  Every case prints its largest ratios."""
import functools

import numpy as np
import pytest

import incomplete_ref as ref
import lc_oracle as o
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

WCLS = {capi.W_DIRICHLET: o.Dirichlet, capi.W_STICKBREAK: o.StickBreak, capi.W_GDIRICHLET: o.GDirichlet}
NEW_ROWS = 300
HMAX = capi.HOLES_MAX


def _mixture(rng, N, D, K, spread=4.0):
    mu = rng.normal(0, spread, (K, D))
    return mu[rng.integers(0, K, N)] + rng.normal(size=(N, D))


def _fit(Xs, wkind, K, iters=6, seed=0, clusterprior=1.0, ckind=capi.C_GAUSSWISH):
    """fixed-K VBEM on the device -> (model, training context)"""
    rng = np.random.default_rng(seed)
    ctx = capi.Context(0)
    ctx.set_data(Xs)
    ctx.set_qz([rng.dirichlet(np.ones(K), x.shape[0]) for x in Xs])
    _, _, m = ctx.vbem(wkind, fixed_iters=iters, ckind=ckind, clusterprior=clusterprior)
    return m, ctx


def _expected_weights(w):
    """E[pi_k], E[pi_rest] from the oracle's alpha / alpha1 / alpha2 / sort order"""
    if isinstance(w, o.Dirichlet):
        return w.alpha / w.alpha.sum(), 0.0
    Epi, rest = np.zeros(w.alpha1.size), 1.0
    for i, k in enumerate(w.order):
        if isinstance(w, o.GDirichlet) and i == len(w.order) - 1:
            Epi[k], rest = rest, 0.0
            break
        Epi[k] = w.alpha1[k] / (w.alpha1[k] + w.alpha2[k]) * rest
        rest *= w.alpha2[k] / (w.alpha1[k] + w.alpha2[k])
    return Epi, rest


def _posteriors(m, clusterprior=1.0):
    """[(nu, beta, m, iW)] of the K clusters, the same of the cluster prior, (E[pi], E[pi_rest]) per learned group, N_k"""
    J, K, D = m.dims()
    cls, Nk = [], []
    for k in range(K):
        p = m.cluster(k)
        cls.append((p["nu"], p["beta"], p["mean"], p["iW"]))
        Nk.append(p["N"])
    pr = o.GaussWish(clusterprior, D)  # clearobs state
    ws = []
    for j in range(J):
        w = WCLS[m.kinds()[0]]()
        w.update(m.weights(j)[1])
        ws.append(_expected_weights(w))
    return cls, (pr.nu, pr.beta, pr.m, pr.iW), ws, Nk


MODELS = {  # name: (D, K, weights, cluster prior, offset, spread)
    "d2": (2, 3, capi.W_STICKBREAK, 1.0, 0.0, 4.0),
    "d5": (5, 4, capi.W_DIRICHLET, 1.0, 0.0, 4.0),
    "d23": (23, 5, capi.W_STICKBREAK, 2.5, 0.0, 4.0),
    "d23_offset": (23, 5, capi.W_STICKBREAK, 2.5, 1e3, 4.0),
    "d64": (64, 35, capi.W_DIRICHLET, 1.0, 0.0, 4.0),
    "d200": (200, 3, capi.W_GDIRICHLET, 1.0, 0.0, 4.0),
}


@functools.lru_cache(maxsize=None)
def _model(name):
    """-> (model, held-out rows, posteriors): fitted once, shared by the tests and never changed"""
    D, K, wk, cp, offset, spread = MODELS[name]
    rng = np.random.default_rng(1000 + D)  # (the offset model sees the same rows, moved)
    ntrain = 1200 if D < 100 else 700
    X = _mixture(rng, ntrain + NEW_ROWS, D, K, spread) + offset
    m, _ = _fit([X[:ntrain]], wk, K, clusterprior=cp)
    return m, X[ntrain:], _posteriors(m, cp)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (rows with holes, reference): computed once, shared and never changed"""
    m, Xnew, (cls, prior, ws, _) = _model(name)
    Xh = ref.make_holes(np.random.default_rng(4150 + Xnew.shape[1]), Xnew)
    Xh.setflags(write=False)
    return Xh, ref.direct(Xh, cls, prior, *ws[0])


def _records(Xh):
    """count and cols as the call has to report them"""
    holes = np.isnan(Xh)
    count = holes.sum(axis=1).astype(np.int32)
    cols = np.full((Xh.shape[0], HMAX), -1, dtype=np.int32)
    for n in range(Xh.shape[0]):
        cols[n, : count[n]] = np.flatnonzero(holes[n])
    return count, cols


def _compare(got, Xh, reference, what, logp_rtol=1e-10):
    rows, logp, _, S = reference
    holes = np.isnan(Xh)
    assert got.rows.shape == Xh.shape and got.logp.shape == logp.shape
    ratio = float(np.max(np.abs(got.rows - rows)[holes] / np.broadcast_to(S[:, None], Xh.shape)[holes], initial=0.0))
    rel = float(np.max(np.abs(got.logp - logp) / np.abs(logp), initial=0.0))
    print(f"{what}: max |filled - ref| / S_n = {ratio:.3e}, max rel. logp error = {rel:.3e} (bar {logp_rtol:.3e})")
    count, cols = _records(Xh)
    assert got.count.dtype == np.int32 and got.cols.dtype == np.int32
    assert np.array_equal(got.count, count) and np.array_equal(got.cols, cols)
    assert np.array_equal(got.rows[~holes].view(np.int64), np.asarray(Xh)[~holes].view(np.int64))  # every observed value keeps its bits
    assert np.all(np.isfinite(got.rows))
    np.testing.assert_allclose(got.logp, logp, rtol=logp_rtol, atol=0)
    assert np.all(np.abs(got.rows - rows) <= 1e-9 * S[:, None]), ratio


@pytest.mark.parametrize("name", ["d2", "d5", "d23", "d64", "d200", "d23_offset"])
def test_against_numpy_scipy(name):
    m, Xnew, (cls, prior, ws, Nk) = _model(name)
    D = m.dims()[2]
    Xh, reference = _case(name)
    count = np.isnan(Xh).sum(axis=1)
    top = min(HMAX, D - 1)
    assert count.max() == top and count[0] == top and np.isnan(Xh[1, 0]) and np.isnan(Xh[2, D - 1])
    assert 0.2 <= np.mean(count == 0) <= 0.45  # about a third of the rows are complete
    # not vacuous: by the reference alone, the mixing matters for at least a fifth of the rows with holes
    share = float(np.mean(reference[2][count > 0] < 0.99))
    print(f"{name}: share of rows with holes whose max_k r_k < 0.99 = {share:.2f}")
    assert share >= 0.2, share
    bar = 1e-10
    if name == "d23_offset":  # the one bar that is not the project's own: see the module docstring
        _, elogp = ref.emulate(Xh, cls, prior, *ws[0], ref.fill_value(cls, Nk))
        E = float(np.max(np.abs(elogp - reference[1]) / np.abs(reference[1])))
        bar = max(1e-10, 4 * E)
        print(f"{name}: largest rel. logp error of the emulated route E = {E:.3e}")
    keep = np.array(Xh)
    got = m.predict_incomplete(keep)
    assert np.array_equal(np.isnan(keep), np.isnan(Xh))  # the caller's array keeps its NaNs: a copy was filled
    _compare(got, Xh, reference, name, bar)


def test_complete_rows_only():
    m, Xnew, (cls, prior, ws, _) = _model("d23")
    got = m.predict_incomplete(Xnew)
    _compare(got, Xnew, ref.direct(Xnew, cls, prior, *ws[0]), "no holes")
    assert not got.count.any() and np.all(got.cols == -1) and np.array_equal(got.rows, Xnew)
    np.testing.assert_allclose(got.logp, m.predict(Xnew).logp, rtol=1e-12, atol=0)  # (a cross-check: the same predictive)


def test_same_pattern_in_every_row():
    m, Xnew, (cls, prior, ws, _) = _model("d23")
    Xh = Xnew.copy()
    Xh[:, [3, 17]] = np.nan
    reference = ref.direct(Xh, cls, prior, *ws[0])
    got = m.predict_incomplete(Xh)
    _compare(got, Xh, reference, "holes [3, 17] in every row")
    filled = m.impute(Xh, [3, 17])
    ratio = float(np.max(np.abs(got.rows - filled) / reference[3][:, None]))
    print(f"against impute: max |filled - impute| / S_n = {ratio:.3e}")
    assert ratio <= 1e-9


@functools.lru_cache(maxsize=None)
def _grouped_model():
    rng = np.random.default_rng(77)
    D, K = 5, 4
    mu = rng.normal(0, 4.0, (K, D))
    mix = [[0.7, 0.1, 0.1, 0.1], [0.1, 0.6, 0.2, 0.1], [0.05, 0.05, 0.3, 0.6]]
    Xs = [mu[rng.choice(K, 460, p=p)] + rng.normal(size=(460, D)) for p in mix]
    m, _ = _fit([x[:400] for x in Xs], capi.W_GDIRICHLET, K)
    return m, [x[400:] for x in Xs], _posteriors(m)


def test_blocks_groups_and_pad_rows():
    """blocks of 37, 5, 16 and 1 rows (pad rows, the row-group word), each mixed with another learned group's weights"""
    m, held, (cls, prior, ws, _) = _grouped_model()
    rng = np.random.default_rng(41)
    whole = [held[0][:37], held[1][:5], held[2][:16]]
    blocks = [ref.make_holes(rng, x) for x in whole]
    for b, x in zip(blocks, whole):  # the last valid row of every block: in front of a pad row (37, 5) or of the next block (16)
        b[-1] = x[-1]
        b[-1, [1, 4]] = np.nan
    blocks.append(blocks[0][:1].copy())
    groups = [2, 0, 1, 2]
    got = m.predict_incomplete(blocks, groups=groups)
    assert len(got) == 4
    for b, (Xh, g) in enumerate(zip(blocks, groups)):
        _compare(got[b], Xh, ref.direct(Xh, cls, prior, *ws[g]), f"block {b} as group {g}")
    # the groups' weights differ: the same rows as another group give another answer
    other = m.predict_incomplete(blocks[0], groups=[0])
    assert np.max(np.abs(other.rows - got[0].rows)) > 1e-6 and np.max(np.abs(other.logp - got[0].logp)) > 1e-6
    # a one-row block equals that row inside a larger block, bit for bit
    assert got[3].count[0] == 4
    for a_, b_ in zip(got[3], got[0]):
        assert np.array_equal(a_, b_[:1])


def test_repeatability_and_side_effects():
    m, Xnew, _ = _model("d23")
    Xh, _ = _case("d23")
    a, b = m.predict_incomplete(np.array(Xh)), m.predict_incomplete(np.array(Xh))
    for x, y in zip(a, b):  # no float atomics: the same bits
        assert np.array_equal(x, y)
    with capi.Context(0) as ctx:
        ctx.set_data(np.array(Xh))
        with pytest.raises(ValueError, match="no completed rows"):
            ctx.get_completed(0, 0, 4)
        m.predict_incomplete_context(ctx)
        first = ctx.get_completed(0, 0, NEW_ROWS)
        for x, y in zip(first, a):
            assert np.array_equal(x, y)
        assert np.array_equal(ctx.get_rows(0, 0, NEW_ROWS), first.rows)
        with pytest.raises(ValueError, match="no prediction"):
            ctx.get_predictions(0, 0, 4)
        with pytest.raises(ValueError, match="no conditional prediction"):
            ctx.get_conditional(0, 0, 4, 3)
        part = ctx.get_completed(0, 5, 7)
        for x, y in zip(part, first):
            assert np.array_equal(x, y[5:12])
        with pytest.raises(ValueError, match="out of bounds"):
            ctx.get_completed(0, NEW_ROWS - 2, 3)
        with pytest.raises(ValueError, match="out of bounds"):
            ctx.get_completed(1, 0, 1)
        L = capi.lib()
        assert L.lc_ctx_get_completed(ctx._h, 0, 0, 4, None, 0, None, None, None) == capi.LC_OK  # any output may be NULL
        buf = np.zeros((4, 23))
        assert L.lc_ctx_get_completed(ctx._h, 0, 0, 4, capi.dptr(buf), 22, None, None, None) == capi.LC_EINVAL
        assert b"row_stride" in L.lc_last_error()
        # a second call finds no NaN: it scores the completed rows as observed
        m.predict_incomplete_context(ctx)
        second = ctx.get_completed(0, 0, NEW_ROWS)
        assert not second.count.any() and np.all(second.cols == -1) and np.array_equal(second.rows, first.rows)
        assert np.array_equal(second.logp, m.predict_incomplete(first.rows).logp)
        # lc_model_predict on the same context works afterwards, and takes the completed rows' records away
        m.predict_context(ctx)
        assert np.array_equal(ctx.get_predictions(0, 0, NEW_ROWS)[2], m.predict(first.rows).logp)
        with pytest.raises(ValueError, match="no completed rows"):
            ctx.get_completed(0, 0, 4)


def test_far_row_is_finite():
    m, Xnew, _ = _model("d23")
    Xh = Xnew[:20].copy()
    Xh[7] = Xnew.mean(axis=0) + 1e3 * Xnew.std(axis=0)  # 1e3 standard deviations from every cluster
    Xh[7, [0, 11, 22]] = np.nan
    Xh[3, 5] = np.nan
    got = m.predict_incomplete(Xh)
    assert np.all(np.isfinite(got.rows)) and np.all(np.isfinite(got.logp))
    assert got.logp[7] < got.logp[np.arange(20) != 7].min()
    assert list(got.count[[3, 7]]) == [1, 3] and list(got.cols[7, :4]) == [0, 11, 22, -1]


def test_errors():
    m, Xnew, _ = _model("d23")
    good = Xnew[:10].copy()
    good[2, 4] = np.nan
    bad = Xnew[10:30].copy()
    bad[4, 3:12] = np.nan    # 9 holes
    bad[9, 0:20] = np.nan    # (a later offender: the first one is named)
    bad[1, 7] = np.nan
    with capi.Context(0) as ctx:
        ctx.set_data([good])
        m.predict_incomplete_context(ctx)  # a prediction to lose
        assert ctx.get_completed(0, 0, 10).count[2] == 1
        ctx.set_data([good, bad])
        with pytest.raises(ValueError, match=r"row 4 of block 1 has 9 unknown.*lc_model_predict_conditional"):
            m.predict_incomplete_context(ctx)
        for j, x in enumerate((good, bad)):  # nothing was written: the rows still hold their NaNs
            assert np.array_equal(ctx.get_rows(j, 0, x.shape[0]), x, equal_nan=True)
        with pytest.raises(ValueError, match="no completed rows"):
            ctx.get_completed(0, 0, 4)
        with pytest.raises(ValueError, match="group index"):
            m.predict_incomplete_context(ctx, groups=[0, 1])
        with pytest.raises(ValueError, match="group index"):
            m.predict_incomplete_context(ctx, groups=[-1, 0])
        ctx.set_data(Xnew[:10, :22])
        with pytest.raises(ValueError, match="Mismatched dims"):
            m.predict_incomplete_context(ctx)
    # no known column
    m2, X2, _ = _model("d2")
    none = X2[:6].copy()
    none[5, 0] = np.nan
    none[3] = np.nan
    with pytest.raises(ValueError, match="row 3 of block 0 has 2 unknown"):
        m2.predict_incomplete(none)
    # an empty block list, a block without rows
    assert m.predict_incomplete([]) == []
    empty = m.predict_incomplete(np.zeros((0, 23)))
    assert empty.rows.shape == (0, 23) and empty.logp.shape == (0,) and empty.count.shape == (0,) and empty.cols.shape == (0, HMAX)
    mixed = m.predict_incomplete([good, np.zeros((0, 23))])
    assert mixed[1].rows.shape == (0, 23) and mixed[0].count[2] == 1
    # clusters that are not Gauss-Wishart
    rng = np.random.default_rng(5)
    Xd = _mixture(rng, 500, 3, 2)
    ng, _ = _fit([Xd], capi.W_DIRICHLET, 2, ckind=capi.C_NORMGAMMA)
    with pytest.raises(ValueError, match="Gauss-Wishart"):
        ng.predict_incomplete(Xd[:10])
    ng.close()
    # a freed model
    f, _ = _fit([Xd], capi.W_DIRICHLET, 2)
    handle = f._h.value
    f.close()
    with capi.Context(0) as ctx:
        ctx.set_data(Xd[:10])
        import ctypes as C

        assert capi.lib().lc_model_predict_incomplete(C.c_void_p(handle), ctx._h, None) == capi.LC_EINVAL
        assert b"freed" in capi.lib().lc_last_error()
