"""Predictive variance of the values filled into rows with holes (lc_model_predict_incomplete_var).

The reference is numpy / scipy per row on the model's posteriors (tests/incomplete_var_ref.py, direct_var()): the Schur
complement on iW, g, 1 + s d^2 and the mixture sum centred on the mean.  Never the device, never the emulation of its
route.  Models and rows are built as tests/test_gpu_incomplete.py builds them (its helpers are used as they are): six
fixed-K VBEM iterations on the device from a Dirichlet(1) start, 300 held-out rows, a third of them complete.

The bar is the project's own: |var - ref| <= 1e-9 V_n with V_n = max_{k,i} [Cov_k,ii + (M_k,i - mean_i)^2]
from the reference.  Every case prints its largest ratio and its largest error relative to var itself."""
import functools

import numpy as np
import pytest

import incomplete_ref as ref
import incomplete_var_ref as vref
import test_gpu_incomplete as base
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

NEW_ROWS = base.NEW_ROWS
HMAX = capi.HOLES_MAX

MODELS = {  # name: (D, K, weights, cluster prior, offset, spread, seed)
    "d2": (2, 3, capi.W_DIRICHLET, 1.0, 0.0, 4.0, 1002),  # (a StickBreak model fails the domain check at D = 2)
    "d5": (5, 4, capi.W_DIRICHLET, 1.0, 0.0, 4.0, 1005),
    "d23": (23, 5, capi.W_STICKBREAK, 2.5, 0.0, 4.0, 1023),
    "d23_offset": (23, 5, capi.W_STICKBREAK, 2.5, 1e3, 4.0, 1023),  # (the same rows, moved)
    "d64": (64, 35, capi.W_DIRICHLET, 1.0, 0.0, 4.0, 1064),
    "d200": (200, 3, capi.W_GDIRICHLET, 1.0, 0.0, 4.0, 1200),
    "k70": (5, 70, capi.W_DIRICHLET, 1.0, 0.0, 4.0, 1070),  # Kp = 70: two chunks of clusters
    "k1": (23, 1, capi.W_DIRICHLET, 1.0, 0.0, 4.0, 1001),
    "vdp5": (5, 4, capi.W_STICKBREAK, 1.0, 0.0, 4.0, 1005),  # the prior component has nu = 5
}


@functools.lru_cache(maxsize=None)
def _model(name):
    """-> (model, held-out rows, posteriors): fitted once, shared by the tests and never changed"""
    D, K, wk, cp, offset, spread, seed = MODELS[name]
    rng = np.random.default_rng(seed)
    ntrain = 1200 if D < 100 else 700
    X = base._mixture(rng, ntrain + NEW_ROWS, D, K, spread) + offset
    m, _ = base._fit([X[:ntrain]], wk, K, clusterprior=cp)
    X.setflags(write=False)
    return m, X[ntrain:], base._posteriors(m, cp)


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (rows with holes, direct_var's reference): computed once, shared and never changed"""
    m, Xnew, (cls, prior, ws, _) = _model(name)
    Xh = ref.make_holes(np.random.default_rng(4151 + Xnew.shape[1]), Xnew)
    Xh.setflags(write=False)
    return Xh, vref.direct_var(Xh, cls, prior, *ws[0])


def _compare_var(got, Xh, reference, what):
    """the bar, with the figures printed first; the zero slots exactly"""
    var, Vn, _, _ = reference
    count = np.isnan(Xh).sum(axis=1)
    assert got.var.shape == (Xh.shape[0], HMAX) and got.var.dtype == np.float64
    used = np.arange(HMAX)[None, :] < count[:, None]
    err = np.abs(got.var - var)
    ratio = float(np.max(err / Vn[:, None], initial=0.0))
    rel = float(np.max(err[used] / var[used], initial=0.0))
    print(f"{what}: max |var - ref| / V_n = {ratio:.3e}, max |var - ref| / var = {rel:.3e}")
    assert np.array_equal(got.count, count)
    assert not got.var[~used].any()  # exactly 0.0 beyond count and in rows without holes
    assert np.all(np.isfinite(got.var)) and np.all(got.var[used] > 0)
    assert np.all(err <= 1e-9 * Vn[:, None]), ratio


@pytest.mark.parametrize("name", ["d2", "d5", "d23", "d64", "d200", "d23_offset", "k70"])
def test_against_numpy_scipy(name):
    m, Xnew, (cls, prior, ws, Nk) = _model(name)
    D = m.dims()[2]
    Xh, reference = _case(name)
    count = np.isnan(Xh).sum(axis=1)
    top = min(HMAX, D - 1)
    assert count.max() == top and count[0] == top and np.isnan(Xh[1, 0]) and np.isnan(Xh[2, D - 1])
    assert 0.2 <= np.mean(count == 0) <= 0.45  # about a third of the rows are complete
    # not vacuous: by the reference alone, the between-expert term is at least 1 % of var in some hole of at least a
    # quarter of the rows with holes (the offset case shares d23's rows: there V_n is the prior component's own variance)
    between = float(np.mean(reference[2][count > 0] >= 0.01))
    print(f"{name}: share of rows with holes whose between term reaches 1 % of var = {between:.2f}")
    if name != "d23_offset":
        assert between >= 0.25, between
    got = m.predict_incomplete(np.array(Xh), variance=True)
    assert isinstance(got, capi.CompletionVar)
    _compare_var(got, Xh, reference, name)
    if name == "k70":  # no other case has Kp > 64: the completed rows and logp at the bars of tests/test_gpu_incomplete.py
        assert len(cls) + (ws[0][1] > 0) > 64
        base._compare(got, Xh, ref.direct(Xh, cls, prior, *ws[0]), name)


def test_same_pattern_against_impute():
    """the route of DESIGN 4.14.1 (one Schur complement per cluster on the host, a separate variance kernel)"""
    m, Xnew, (cls, prior, ws, _) = _model("d23")
    Xh = np.array(Xnew)
    Xh[:, [3, 17]] = np.nan
    reference = vref.direct_var(Xh, cls, prior, *ws[0])
    got = m.predict_incomplete(Xh, variance=True)
    _compare_var(got, Xh, reference, "holes [3, 17] in every row")
    _, var = m.impute(Xh, [3, 17], return_var=True)
    ratio = float(np.max(np.abs(got.var[:, :2] - var) / reference[1][:, None]))
    print(f"against impute: max |var - impute's var| / V_n = {ratio:.3e}")
    assert ratio <= 1e-9


def test_one_cluster_is_the_conditional_student_t():
    """K = 1, no rest: the variance of one conditional Student-t with nu' + Da degrees of freedom, in its textbook form
    df / (df - 2) * scale, scale = (nu' + delta_a) / (nu' + Da) * c * Schur, c = (1 + beta) / (beta nu')"""
    m, Xnew, (cls, prior, ws, _) = _model("k1")
    assert len(cls) == 1 and ws[0][1] == 0
    nu, beta, mm, iW = cls[0]
    D = mm.size
    Xh = ref.make_holes(np.random.default_rng(9), Xnew[:60])
    got = m.predict_incomplete(Xh, variance=True)
    worst = 0.0
    for n in range(Xh.shape[0]):
        b = np.flatnonzero(np.isnan(Xh[n]))
        if not b.size:
            assert not got.var[n].any()
            continue
        a = np.setdiff1d(np.arange(D), b)
        nup, Da, c = nu + 1 - D, a.size, (1 + beta) / (beta * (nu + 1 - D))
        Saa, Sab = iW[np.ix_(a, a)], iW[np.ix_(a, b)]
        ya = Xh[n, a] - mm[a]
        delta = ya @ np.linalg.solve(c * Saa, ya)
        schur = iW[np.ix_(b, b)] - Sab.T @ np.linalg.solve(Saa, Sab)
        df = nup + Da
        want = df / (df - 2) * (nup + delta) / df * c * np.diag(schur)
        worst = max(worst, float(np.max(np.abs(got.var[n, : b.size] - want) / want.max())))
    print(f"K = 1: max |var - Student-t variance| / V_n = {worst:.3e}")
    assert worst <= 1e-9


def test_bits():
    m, Xnew, _ = _model("d23")
    Xh, _ = _case("d23")
    plain = m.predict_incomplete(np.array(Xh))
    a, b = m.predict_incomplete(np.array(Xh), variance=True), m.predict_incomplete(np.array(Xh), variance=True)
    assert plain.var is None and len(plain) == 4
    for x, y in zip(plain, a):  # completed rows, logp, count, cols: the same bits with and without variance
        assert np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
    for x, y in zip(a, b):  # no float atomics, fixed trees: the same bits on every call
        assert np.array_equal(x, y)
    # a row gives the same bits wherever it sits in its block: another lane, another wave, another thread block
    count = np.isnan(Xh).sum(axis=1)
    src = int(np.flatnonzero(count == count.max())[0])
    for dst in (src + 1, 77, 299):
        moved = np.array(Xh)
        moved[[src, dst]] = moved[[dst, src]]
        c = m.predict_incomplete(moved, variance=True)
        for x, y in zip(a, c):
            assert np.array_equal(x[src], y[dst]) and np.array_equal(x[dst], y[src])


def test_blocks_groups_pad_rows_and_reuse():
    """blocks of 37, 5 and 16 rows (pad rows, the row-group word), each mixed with another learned group's weights"""
    m, held, (cls, prior, ws, _) = base._grouped_model()
    rng = np.random.default_rng(43)
    blocks = [ref.make_holes(rng, x) for x in (held[0][:37], held[1][:5], held[2][:16])]
    groups = [2, 0, 1]
    got = m.predict_incomplete(blocks, groups=groups, variance=True)
    for b, (Xh, g) in enumerate(zip(blocks, groups)):
        _compare_var(got[b], Xh, vref.direct_var(Xh, cls, prior, *ws[g]), f"block {b} as group {g}")
    with capi.Context(0) as ctx:
        ctx.set_data([np.array(x) for x in blocks])
        m.predict_incomplete_context(ctx, groups, variance=True)
        first = [ctx.get_completed(j, 0, x.shape[0], variance=True) for j, x in enumerate(blocks)]
        for f, g in zip(first, got):
            for x, y in zip(f, g):
                assert np.array_equal(x, y)
        part = ctx.get_completed(0, 5, 7, variance=True)
        assert np.array_equal(part.var, first[0].var[5:12])
        # a second call finds no NaN: every count 0, and the re-used buffer shows no stale value
        m.predict_incomplete_context(ctx, groups, variance=True)
        for j, x in enumerate(blocks):
            second = ctx.get_completed(j, 0, x.shape[0], variance=True)
            assert not second.count.any() and not second.var.any() and second.var.shape == (x.shape[0], HMAX)
        # a plain call takes the variance away
        m.predict_incomplete_context(ctx, groups)
        assert ctx.get_completed(0, 0, 4).var is None
        with pytest.raises(ValueError, match="no variance"):
            ctx.get_completed(0, 0, 4, variance=True)


def test_far_row_is_finite():
    m, Xnew, _ = _model("d23")
    Xh = np.array(Xnew[:20])
    Xh[7] = Xnew.mean(axis=0) + 1e6 * Xnew.std(axis=0)  # 1e6 standard deviations from every cluster
    Xh[7, [0, 11, 22]] = np.nan
    Xh[3, 5] = np.nan
    Xh[12, [2, 9]] = np.nan
    got = m.predict_incomplete(Xh, variance=True)
    assert np.all(np.isfinite(got.var)) and np.all(np.isfinite(got.rows)) and np.all(np.isfinite(got.logp))
    assert list(got.count[[3, 7, 12]]) == [1, 3, 2] and not got.var[7, 3:].any()
    assert got.var[7, :3].min() > got.var[np.arange(20) != 7].max() > 0


def test_domain():
    """a VDP model at D = 5: the prior component has nu = 5, so a row with four holes has no variance"""
    m, Xnew, _ = _model("vdp5")
    assert m.kinds()[0] == capi.W_STICKBREAK
    Xh = np.array(Xnew[:30])
    Xh[4, [0, 2]] = np.nan
    Xh[9, [1, 2, 4]] = np.nan
    ok = Xh.copy()
    Xh[17, [0, 1, 3, 4]] = np.nan
    with capi.Context(0) as ctx:
        ctx.set_data(Xh)
        with pytest.raises(capi.DomainError, match=r"prior component.*4 unknown"):
            m.predict_incomplete_context(ctx, variance=True)
        assert np.array_equal(ctx.get_rows(0, 0, 30), Xh, equal_nan=True)  # nothing was written: the NaNs stay
        with pytest.raises(ValueError, match="no completed rows"):
            ctx.get_completed(0, 0, 4)
        with pytest.raises(ValueError, match="no completed rows"):
            ctx.get_completed(0, 0, 4, variance=True)
        m.predict_incomplete_context(ctx)  # the completed rows and logp do exist
        plain = ctx.get_completed(0, 0, 30)
        assert plain.count[17] == 4 and np.all(np.isfinite(plain.rows))
        ctx.set_data(ok)
        m.predict_incomplete_context(ctx, variance=True)  # at most three holes: nu - 1 - 3 = 1
        got = ctx.get_completed(0, 0, 30, variance=True)
        assert list(got.count[[4, 9, 17]]) == [2, 3, 0] and np.all(got.var[9, :3] > 0) and np.all(np.isfinite(got.var))
        # a context without holes never fails the check
        ctx.set_data(np.array(Xnew[:30]))
        m.predict_incomplete_context(ctx, variance=True)
        assert not ctx.get_completed(0, 0, 30, variance=True).var.any()


def test_getter_errors():
    m, Xnew, _ = _model("d23")
    Xh, _ = _case("d23")
    L = capi.lib()
    buf = np.zeros((4, HMAX))
    with capi.Context(0) as ctx:
        ctx.set_data(np.array(Xh))
        assert L.lc_ctx_get_completed_var(ctx._h, 0, 0, 4, capi.dptr(buf), HMAX) == capi.LC_EINVAL  # no prediction on ctx
        assert b"no completed rows" in L.lc_last_error()
        m.predict_incomplete_context(ctx, variance=True)
        assert L.lc_ctx_get_completed_var(ctx._h, 0, 0, 4, capi.dptr(buf), HMAX) == capi.LC_OK
        assert L.lc_ctx_get_completed_var(ctx._h, 0, 0, 4, None, HMAX) == capi.LC_OK  # var may be NULL: the checks only
        assert L.lc_ctx_get_completed_var(ctx._h, 0, 0, 4, capi.dptr(buf), HMAX - 1) == capi.LC_EINVAL
        assert b"row_stride" in L.lc_last_error()
        assert L.lc_ctx_get_completed_var(ctx._h, 0, 0, 4, None, HMAX - 1) == capi.LC_EINVAL
        assert L.lc_ctx_get_completed_var(ctx._h, 0, NEW_ROWS - 2, 3, capi.dptr(buf), HMAX) == capi.LC_EINVAL
        assert b"out of bounds" in L.lc_last_error()
        assert L.lc_ctx_get_completed_var(ctx._h, 1, 0, 1, capi.dptr(buf), HMAX) == capi.LC_EINVAL
        wide = np.full((4, HMAX + 3), -1.0)  # a wider stride leaves the columns beyond HOLES_MAX alone
        assert L.lc_ctx_get_completed_var(ctx._h, 0, 0, 4, capi.dptr(wide), HMAX + 3) == capi.LC_OK
        assert np.array_equal(wide[:, :HMAX], ctx.get_completed(0, 0, 4, variance=True).var) and np.all(wide[:, HMAX:] == -1.0)
