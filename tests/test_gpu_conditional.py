"""Conditional prediction (lc_model_predict_conditional): E[x_target | x_given] and log p(x_given) of new rows.

The reference is numpy / scipy on the model's posteriors (m.cluster(k)) and the expected weights of the oracle's weight
objects: per cluster the Student-t marginal of the given columns and the linear expert m_b + iW_ba iW_aa^-1 (x_a - m_a),
mixed by the responsibilities.  Models come from six fixed-K VBEM iterations on the device from a Dirichlet(1) start (the
recipe of tests/test_gpu_predict.py), which leaves clusters that overlap: the mixing matters in every case, and each case
asserts so.

Bars: logp to rtol 1e-10 (what test_gpu_predict.py holds logp to), mean to |d| <= 1e-9 S_n with S_n = max_{k,b}
|M_k(x_n)_b| (the project's 1e-9 on responsibilities carried through the sum).  Every case prints its largest ratio."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy import stats
from scipy.special import logsumexp

import lc_oracle as o
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

WCLS = {capi.W_DIRICHLET: o.Dirichlet, capi.W_STICKBREAK: o.StickBreak, capi.W_GDIRICHLET: o.GDirichlet}
NEW_ROWS = 300


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
    """[(nu, beta, m, iW)] of the K clusters, the same of the cluster prior, and (E[pi], E[pi_rest]) per learned group"""
    J, K, D = m.dims()
    cls = []
    for k in range(K):
        p = m.cluster(k)
        cls.append((p["nu"], p["beta"], p["mean"], p["iW"]))
    pr = o.GaussWish(clusterprior, D)  # clearobs state
    ws = []
    for j in range(J):
        w = WCLS[m.kinds()[0]]()
        w.update(m.weights(j)[1])
        ws.append(_expected_weights(w))
    return cls, (pr.nu, pr.beta, pr.m, pr.iW), ws


def _reference(Xa, given, target, D, cls, prior, Epi, rest):
    """-> mean (N, Db), logp (N,), responsibilities (N, Kp), S_n (N,)"""
    comps = [(np.log(Epi[k]), c) for k, c in enumerate(cls)]
    if rest > 0:
        comps.append((np.log(rest), prior))
    T, M = [], []
    for lw, (nu, beta, mm, iW) in comps:
        nup = nu + 1 - D
        Saa, Sab = iW[np.ix_(given, given)], iW[np.ix_(given, target)]
        lp = stats.multivariate_t(loc=mm[given], shape=(1 + beta) / (beta * nup) * Saa, df=nup).logpdf(Xa)
        T.append(lw + np.asarray(lp).reshape(-1))
        M.append(mm[target] + (Xa - mm[given]) @ np.linalg.solve(Saa, Sab))
    T, M = np.stack(T, axis=1), np.stack(M, axis=1)  # (N, Kp), (N, Kp, Db)
    logp = logsumexp(T, axis=1)
    r = np.exp(T - logp[:, None])
    return np.einsum("nk,nkb->nb", r, M), logp, r, np.abs(M).max(axis=(1, 2))


def _targets(D, given, target):
    return list(target) if target is not None else [c for c in range(D) if c not in set(given)]


def _compare(got, ref, what):
    mean, logp, _, S = ref
    assert got.mean.shape == mean.shape and got.logp.shape == logp.shape
    ratio = float(np.max(np.abs(got.mean - mean) / S[:, None], initial=0.0))
    rel = float(np.max(np.abs(got.logp - logp) / np.abs(logp), initial=0.0))
    print(f"{what}: max |mean - ref| / S_n = {ratio:.3e}, max rel. logp error = {rel:.3e}")
    np.testing.assert_allclose(got.logp, logp, rtol=1e-10, atol=0)
    assert np.all(np.abs(got.mean - mean) <= 1e-9 * S[:, None]), ratio


_perm64 = np.random.default_rng(64).permutation(64)
_perm200 = np.random.default_rng(200).permutation(200)
MODELS = {  # name: (D, K, weights, cluster prior, offset, spread)
    "d2": (2, 3, capi.W_STICKBREAK, 1.0, 0.0, 4.0),
    "d5": (5, 4, capi.W_DIRICHLET, 1.0, 0.0, 4.0),
    "d23": (23, 5, capi.W_STICKBREAK, 2.5, 0.0, 4.0),
    "d23_offset": (23, 5, capi.W_STICKBREAK, 2.5, 1e3, 4.0),
    "d64": (64, 35, capi.W_DIRICHLET, 1.0, 0.0, 4.0),
    "d200": (200, 3, capi.W_GDIRICHLET, 1.0, 0.0, 4.0),
}
CASES = {  # name: (model, given, target)
    "d2_prior_component": ("d2", [0], [1]),                       # Kp = 4, one given column
    "d5_permuted_given": ("d5", [3, 0], None),                    # Db = 3
    "d23_da8": ("d23", list(range(0, 23, 3)), [1, 7, 22]),
    "d23_da8_offset_1e3": ("d23_offset", list(range(0, 23, 3)), [1, 7, 22]),
    "d64_k35": ("d64", sorted(int(c) for c in _perm64[:40]), [int(c) for c in _perm64[40:]]),  # DPa = 48, Kp = 35
    "d64_db17": ("d64", sorted(int(c) for c in _perm64[:40]), [int(c) for c in _perm64[40:57]]),  # one past a 16-wide tile
    # the wide E-step, more than one target panel, tables that cannot sit in LDS whole
    "d200_wide": ("d200", sorted(int(c) for c in _perm200[:130]), sorted(int(c) for c in _perm200[130:])),
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


@pytest.mark.parametrize("case", list(CASES))
def test_against_numpy_scipy(case):
    name, given, target = CASES[case]
    m, Xnew, (cls, prior, ws) = _model(name)
    D = m.dims()[2]
    tg = _targets(D, given, target)
    ref = _reference(Xnew[:, given], given, tg, D, cls, prior, *ws[0])
    # not vacuous: by the reference alone, the mixing matters for at least a fifth of the rows
    share = float(np.mean(ref[2].max(axis=1) < 0.99))
    print(f"{case}: share of rows with max_k r_k < 0.99 = {share:.2f}")
    assert share >= 0.2, share
    got = m.predict_conditional(Xnew[:, given], given, target)
    _compare(got, ref, case)


def test_one_cluster_is_one_linear_expert():
    rng = np.random.default_rng(9)
    D = 6
    X = rng.normal(size=(900, D)) @ rng.normal(size=(D, D)) + 3.0
    m, _ = _fit([X[:600]], capi.W_DIRICHLET, 1)
    cls, prior, ws = _posteriors(m)
    given, target = [4, 1, 2], [0, 5, 3]
    got = m.predict_conditional(X[600:, given], given, target)
    nu, beta, mm, iW = cls[0]
    expert = mm[target] + (X[600:, given] - mm[given]) @ np.linalg.solve(iW[np.ix_(given, given)], iW[np.ix_(given, target)])
    S = np.abs(expert).max(axis=1)
    assert np.all(np.abs(got.mean - expert) <= 1e-9 * S[:, None])
    _compare(got, _reference(X[600:, given], given, target, D, cls, prior, *ws[0]), "K = 1")


@functools.lru_cache(maxsize=None)
def _grouped_model():
    rng = np.random.default_rng(77)
    D, K = 5, 4
    mu = rng.normal(0, 4.0, (K, D))
    mix = [[0.7, 0.1, 0.1, 0.1], [0.1, 0.6, 0.2, 0.1], [0.05, 0.05, 0.3, 0.6]]
    Xs = [mu[rng.choice(K, 460, p=p)] + rng.normal(size=(460, D)) for p in mix]
    m, _ = _fit([x[:400] for x in Xs], capi.W_GDIRICHLET, K)
    return m, [x[400:] for x in Xs], _posteriors(m)


def test_groups_pad_rows_and_one_row_block():
    """blocks of 37, 5 and 16 rows (pad rows, the row-group word), each mixed with another learned group's weights"""
    m, held, (cls, prior, ws) = _grouped_model()
    D = m.dims()[2]
    given, target = [2, 4, 0], [3, 1]
    blocks = [held[0][:37, given], held[1][:5, given], held[2][:16, given]]
    groups = [2, 0, 1]
    got = m.predict_conditional(blocks, given, target, groups=groups)
    assert len(got) == 3
    for b, (Xa, g) in enumerate(zip(blocks, groups)):
        _compare(got[b], _reference(Xa, given, target, D, cls, prior, *ws[g]), f"block {b} as group {g}")
    # the groups' weights differ: the same rows as another group give another answer
    other = m.predict_conditional(blocks[0], given, target, groups=[0])
    assert np.max(np.abs(other.mean - got[0].mean)) > 1e-6
    one = m.predict_conditional([blocks[0][:1]], given, target, groups=[2])[0]
    assert one.mean.shape == (1, 2) and one.logp.shape == (1,)
    assert np.array_equal(one.mean, got[0].mean[:1]) and np.array_equal(one.logp, got[0].logp[:1])


def test_far_row_is_finite():
    m, Xnew, _ = _model("d23")
    given = list(range(0, 23, 3))
    Xa = Xnew[:20, given].copy()
    Xa[7] = Xnew[:, given].mean(axis=0) + 1e3 * Xnew[:, given].std(axis=0)  # 1e3 standard deviations from every cluster
    got = m.predict_conditional(Xa, given, [1, 7, 22])
    assert np.all(np.isfinite(got.mean)) and np.all(np.isfinite(got.logp))
    assert got.logp[7] < got.logp[np.arange(20) != 7].min()


def test_invariances():
    m, Xnew, (cls, prior, ws) = _model("d23")
    D = m.dims()[2]
    given, target = list(range(0, 23, 3)), [1, 7, 22]
    a = m.predict_conditional(Xnew[:, given], given, target)
    b = m.predict_conditional(Xnew[:, given], given, target)
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.logp, b.logp)  # no atomics: the same bits
    perm = np.random.default_rng(3).permutation(len(given))
    gp = [given[i] for i in perm]
    c = m.predict_conditional(Xnew[:, gp], gp, target)
    S = _reference(Xnew[:, given], given, target, D, cls, prior, *ws[0])[3]
    ratio = float(np.max(np.abs(c.mean - a.mean) / S[:, None]))
    print(f"permuted given: max |mean - mean'| / S_n = {ratio:.3e}")
    assert ratio <= 1e-12
    # impute: the same numbers, the missing columns not looked at
    Xfull = Xnew.copy()
    Xfull[:, target] = np.nan
    rest = [c_ for c_ in range(D) if c_ not in target]
    filled = m.impute(Xfull, target)
    direct = m.predict_conditional(Xnew[:, rest], rest, target)
    assert np.array_equal(filled[:, target], direct.mean) and np.array_equal(filled[:, rest], Xnew[:, rest])
    assert np.isnan(Xfull[:, target]).all()  # (a copy was filled)


def test_errors_and_side_effects():
    m, Xnew, _ = _model("d5")
    D = 5
    with capi.Context(0) as ctx:
        ctx.set_data(Xnew[:, [3, 0]])
        cases = [
            (dict(given=[], target=[1]), "at least one"),
            (dict(given=[3, 0], target=[]), "at least one"),
            (dict(given=[3, 5], target=[1]), "outside"),
            (dict(given=[3, 0], target=[-1]), "outside"),
            (dict(given=[3, 3], target=[1]), "twice"),
            (dict(given=[3, 0], target=[1, 1]), "twice"),
            (dict(given=[3, 0], target=[1, 0]), "both given and target"),
            (dict(given=[3, 0, 2], target=[1]), "columns"),           # ctx width != ngiven
            (dict(given=[3, 0], target=[1], groups=[1]), "group index"),
            (dict(given=[3, 0], target=[1], groups=[-1]), "group index"),
        ]
        for kw, word in cases:
            m.predict_conditional_context(ctx, [3, 0])  # a prediction to lose
            assert ctx.get_conditional(0, 0, 4, 3).mean.shape == (4, 3)
            with pytest.raises(ValueError, match=word):
                m.predict_conditional_context(ctx, **kw)
            with pytest.raises(ValueError, match="no conditional prediction"):  # a failed call leaves none behind
                ctx.get_conditional(0, 0, 4, 3)
        # a plain prediction is replaced, and none is reported afterwards
        nt = m.predict_conditional_context(ctx, [3, 0])
        assert nt == 3
        with pytest.raises(ValueError, match="no prediction"):
            ctx.get_predictions(0, 0, 4)
        with pytest.raises(ValueError, match="out of bounds"):
            ctx.get_conditional(0, NEW_ROWS - 2, 3, 3)
        with pytest.raises(ValueError, match="out of bounds"):
            ctx.get_conditional(1, 0, 1, 3)
        part = ctx.get_conditional(0, 5, 7, 3)
        whole = ctx.get_conditional(0, 0, NEW_ROWS, 3)
        assert np.array_equal(part.mean, whole.mean[5:12]) and np.array_equal(part.logp, whole.logp[5:12])
        rc = capi.lib().lc_ctx_get_conditional(ctx._h, 0, 0, 4, None, 0, None)  # either output may be NULL
        assert rc == capi.LC_OK
        # lc_model_predict on the same context still works afterwards (and takes the conditional prediction away)
        ctx.set_data(Xnew)
        m.predict_context(ctx)
        label, logZ, logp = ctx.get_predictions(0, 0, NEW_ROWS)
        ref = m.predict(Xnew)
        assert np.array_equal(label, ref.label) and np.array_equal(logp, ref.logp)
        with pytest.raises(ValueError, match="no conditional prediction"):
            ctx.get_conditional(0, 0, 4, 3)
    # clusters that are not Gauss-Wishart
    rng = np.random.default_rng(5)
    Xd = _mixture(rng, 500, 3, 2)
    ng, _ = _fit([Xd], capi.W_DIRICHLET, 2, ckind=capi.C_NORMGAMMA)
    with pytest.raises(ValueError, match="Gauss-Wishart"):
        ng.predict_conditional(Xd[:10, [0]], [0])
    ng.close()
    # a freed model
    f, _ = _fit([Xd], capi.W_DIRICHLET, 2)
    handle = f._h.value
    f.close()
    with capi.Context(0) as ctx:
        ctx.set_data(Xd[:10, [0]])
        gv = (C.c_int * 1)(0)
        assert capi.lib().lc_model_predict_conditional(C.c_void_p(handle), ctx._h, None, gv, 1, None, 0) == capi.LC_EINVAL
        assert b"freed" in capi.lib().lc_last_error()
