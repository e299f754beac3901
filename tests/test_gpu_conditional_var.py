"""Predictive variance of the conditional prediction (lc_model_predict_conditional_var).

The reference is tests/cond_var_ref.py: numpy / scipy on the model's posteriors, the mixture's variance centred on its
mean.  Models and recipe are those of tests/test_gpu_conditional.py (its MODELS table, seeds, six fixed-K VBEM iterations on
the device from a Dirichlet(1) start); 300 held-out rows are four full waves of the kernel and one of 44 rows.

Bars: |var - ref| <= 1e-9 V_n with V_n = max_{k,b} [Cov_k,bb(x_n) + (M_k,b - mean_b)^2] -- the project's 1e-9 on
responsibilities carried through the sum, as the mean's bar is.  The offset case (data 1e3 from the origin) is held to
max(1e-9, 4 E) V_n, E the largest |ref_float64 - ref_mpmath| / V_n on its rows, measured here (the rule of
tests/test_gpu_incomplete.py).  Every case prints its largest ratio."""
import functools

import numpy as np
import pytest

import cond_var_ref as cref
import lc_oracle as o
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

WCLS = {capi.W_DIRICHLET: o.Dirichlet, capi.W_STICKBREAK: o.StickBreak, capi.W_GDIRICHLET: o.GDirichlet}
NEW_ROWS = 300


def _mixture(rng, N, D, K, spread=4.0):
    mu = rng.normal(0, spread, (K, D))
    return mu[rng.integers(0, K, N)] + rng.normal(size=(N, D))


def _fit(Xs, wkind, K, iters=6, seed=0, clusterprior=1.0):
    """fixed-K VBEM on the device -> model"""
    rng = np.random.default_rng(seed)
    ctx = capi.Context(0)
    ctx.set_data(Xs)
    ctx.set_qz([rng.dirichlet(np.ones(K), x.shape[0]) for x in Xs])
    _, _, m = ctx.vbem(wkind, fixed_iters=iters, clusterprior=clusterprior)
    return m


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


def _targets(D, given, target):
    return list(target) if target is not None else [c for c in range(D) if c not in set(given)]


_perm64 = np.random.default_rng(64).permutation(64)
_perm200 = np.random.default_rng(200).permutation(200)
MODELS = {  # name: (D, K, weights, cluster prior, offset, spread) -- as in test_gpu_conditional.py
    "d2": (2, 3, capi.W_STICKBREAK, 1.0, 0.0, 4.0),
    "d5": (5, 4, capi.W_DIRICHLET, 1.0, 0.0, 4.0),
    "d23": (23, 5, capi.W_STICKBREAK, 2.5, 0.0, 4.0),
    "d23_offset": (23, 5, capi.W_STICKBREAK, 2.5, 1e3, 4.0),
    "d64": (64, 35, capi.W_DIRICHLET, 1.0, 0.0, 4.0),
    "d200": (200, 3, capi.W_GDIRICHLET, 1.0, 0.0, 4.0),
}
CASES = {  # name: (model, given, target)
    "d5_permuted_given": ("d5", [3, 0], None),                    # Db = 3, a padded quad of targets
    "d23_da8": ("d23", list(range(0, 23, 3)), [1, 7, 22]),        # Kp = 6 with the prior component
    "d23_da8_offset_1e3": ("d23_offset", list(range(0, 23, 3)), [1, 7, 22]),  # cancellation
    # two chunks of given columns, Kp = 35, empty clusters
    "d64_k35": ("d64", sorted(int(c) for c in _perm64[:40]), [int(c) for c in _perm64[40:]]),
    # Dae = 32: exactly one full chunk, x resident; Db = 33: a last panel of one column
    "d64_da31": ("d64", sorted(int(c) for c in _perm64[:31]), [int(c) for c in _perm64[31:]]),
    # five chunks, several panels, the wide E-step
    "d200_wide": ("d200", sorted(int(c) for c in _perm200[:130]), sorted(int(c) for c in _perm200[130:])),
}


@functools.lru_cache(maxsize=None)
def _model(name):
    """-> (model, held-out rows, posteriors): fitted once, shared by the tests and never changed"""
    D, K, wk, cp, offset, spread = MODELS[name]
    rng = np.random.default_rng(1000 + D)  # (the offset model sees the same rows, moved)
    ntrain = 1200 if D < 100 else 700
    X = _mixture(rng, ntrain + NEW_ROWS, D, K, spread) + offset
    m = _fit([X[:ntrain]], wk, K, clusterprior=cp)
    return m, X[ntrain:], _posteriors(m, cp)


def _compare(got, ref, what, bar=1e-9):
    mean, var, logp, _, _, _, V = ref
    assert got.var.shape == var.shape and got.mean.shape == mean.shape
    ratio = float(np.max(np.abs(got.var - var) / V[:, None], initial=0.0))
    print(f"{what}: max |var - ref| / V_n = {ratio:.3e} (bar {bar:.3e})")
    np.testing.assert_allclose(got.logp, logp, rtol=1e-10, atol=0)
    assert np.all(np.isfinite(got.var)) and np.all(got.var > 0)
    assert np.all(np.abs(got.var - var) <= bar * V[:, None]), ratio


@pytest.mark.parametrize("case", list(CASES))
def test_against_numpy_scipy(case):
    name, given, target = CASES[case]
    m, Xnew, (cls, prior, ws) = _model(name)
    D = m.dims()[2]
    tg = _targets(D, given, target)
    Xa = Xnew[:, given]
    ref = cref.reference(Xa, given, tg, D, cls, prior, *ws[0])
    var, between = ref[1], ref[5]
    # not vacuous: by the reference alone, the experts disagree -- in at least a fifth of the rows the between-expert term is
    # 1 % of the variance or more in some target
    share = float(np.mean((between / var).max(axis=1) >= 0.01))
    print(f"{case}: share of rows whose between-expert term is >= 1 % of var in some target = {share:.2f}")
    assert share >= 0.2, share
    bar = 1e-9
    if MODELS[name][4] != 0.0:  # the offset case: how far float64 itself is from 50 digits, measured
        E = float(np.max(np.abs(var - cref.reference_mp(Xa, given, tg, D, cls, prior, *ws[0])) / ref[6][:, None]))
        bar = max(1e-9, 4 * E)
        print(f"{case}: float64 reference against mpmath, E = {E:.3e}")
    got = m.predict_conditional(Xa, given, target, variance=True)
    _compare(got, ref, case, bar)


def test_one_cluster_is_its_conditional_student_t():
    rng = np.random.default_rng(9)
    D = 6
    X = rng.normal(size=(900, D)) @ rng.normal(size=(D, D)) + 3.0
    m = _fit([X[:600]], capi.W_DIRICHLET, 1)
    cls, prior, ws = _posteriors(m)
    given, target = [4, 1, 2], [0, 5, 3]
    Xa = X[600:, given]
    got = m.predict_conditional(Xa, given, target, variance=True)
    nu, beta, mm, iW = cls[0]
    _, schur, g, s = cref.cluster_tables(nu, beta, mm, iW, given, target, D)
    ya = Xa - mm[given]
    d2 = nu * np.einsum("na,na->n", ya, np.linalg.solve(iW[np.ix_(given, given)], ya.T).T)
    want = g * (1 + s * d2)[:, None] * schur[None, :]
    assert np.all(np.abs(got.var - want) <= 1e-9 * want.max(axis=1)[:, None])
    assert np.ptp(got.var[:, 0]) > 1e-3 * got.var[:, 0].mean()  # (1 + s d^2: the bar differs from row to row)
    _compare(got, cref.reference(Xa, given, target, D, cls, prior, *ws[0]), "K = 1")


def test_mean_and_logp_unchanged_same_bits_permuted_given():
    m, Xnew, (cls, prior, ws) = _model("d23")
    D = m.dims()[2]
    given, target = list(range(0, 23, 3)), [1, 7, 22]
    plain = m.predict_conditional(Xnew[:, given], given, target)
    a = m.predict_conditional(Xnew[:, given], given, target, variance=True)
    b = m.predict_conditional(Xnew[:, given], given, target, variance=True)
    assert plain.var is None and isinstance(plain, capi.Conditional)
    assert np.array_equal(a.mean, plain.mean) and np.array_equal(a.logp, plain.logp)  # the mean-only path is untouched
    assert np.array_equal(a.var, b.var)  # no atomics: the same bits
    perm = np.random.default_rng(3).permutation(len(given))
    gp = [given[i] for i in perm]
    c = m.predict_conditional(Xnew[:, gp], gp, target, variance=True)
    V = cref.reference(Xnew[:, given], given, target, D, cls, prior, *ws[0])[6]
    ratio = float(np.max(np.abs(c.var - a.var) / V[:, None]))
    print(f"permuted given: max |var - var'| / V_n = {ratio:.3e}")
    assert ratio <= 1e-12


@functools.lru_cache(maxsize=None)
def _grouped_model():
    rng = np.random.default_rng(77)
    D, K = 5, 4
    mu = rng.normal(0, 4.0, (K, D))
    mix = [[0.7, 0.1, 0.1, 0.1], [0.1, 0.6, 0.2, 0.1], [0.05, 0.05, 0.3, 0.6]]
    Xs = [mu[rng.choice(K, 460, p=p)] + rng.normal(size=(460, D)) for p in mix]
    m = _fit([x[:400] for x in Xs], capi.W_GDIRICHLET, K)
    return m, [x[400:] for x in Xs], _posteriors(m)


def test_groups_pad_rows_and_one_row_block():
    """blocks of 37, 5 and 16 rows (pad rows, the row-group word), each mixed with another learned group's weights"""
    m, held, (cls, prior, ws) = _grouped_model()
    D = m.dims()[2]
    given, target = [2, 4, 0], [3, 1]
    blocks = [held[0][:37, given], held[1][:5, given], held[2][:16, given]]
    groups = [2, 0, 1]
    got = m.predict_conditional(blocks, given, target, groups=groups, variance=True)
    assert len(got) == 3
    for b, (Xa, g) in enumerate(zip(blocks, groups)):
        _compare(got[b], cref.reference(Xa, given, target, D, cls, prior, *ws[g]), f"block {b} as group {g}")
    one = m.predict_conditional([blocks[0][:1]], given, target, groups=[2], variance=True)[0]
    assert one.var.shape == (1, 2)
    assert np.array_equal(one.var, got[0].var[:1]) and np.array_equal(one.mean, got[0].mean[:1])


def test_far_row_is_finite_and_widest():
    m, Xnew, _ = _model("d23")
    given = list(range(0, 23, 3))
    Xa = Xnew[:20, given].copy()
    Xa[7] = Xnew[:, given].mean(axis=0) + 1e3 * Xnew[:, given].std(axis=0)  # 1e3 standard deviations from every cluster
    got = m.predict_conditional(Xa, given, [1, 7, 22], variance=True)
    assert np.all(np.isfinite(got.var)) and np.all(np.isfinite(got.mean))
    assert np.all(got.var[7] > got.var[np.arange(20) != 7].max(axis=0))


def test_impute_returns_the_same_variance():
    m, Xnew, _ = _model("d23")
    D = m.dims()[2]
    target = [1, 7, 22]
    rest = [c for c in range(D) if c not in target]
    Xfull = Xnew.copy()
    Xfull[:, target] = np.nan
    filled, var = m.impute(Xfull, target, return_var=True)
    direct = m.predict_conditional(Xnew[:, rest], rest, target, variance=True)
    assert np.array_equal(var, direct.var) and var.shape == (NEW_ROWS, 3)
    assert np.array_equal(filled, m.impute(Xfull, target))  # the filled copy is today's
    fl, vl = m.impute([Xfull[:40], Xfull[40:90]], target, return_var=True)
    assert len(fl) == 2 and len(vl) == 2 and np.array_equal(vl[1], var[40:90]) and np.array_equal(fl[0], filled[:40])


def test_domain_error_where_the_variance_does_not_exist():
    m, Xnew, _ = _model("d2")  # StickBreak: the prior component has nu' = 1, and one given column makes 2
    with capi.Context(0) as ctx:
        ctx.set_data(Xnew[:, [0]])
        m.predict_conditional_context(ctx, [0], [1])  # a prediction to lose
        assert ctx.get_conditional(0, 0, 4, 1).mean.shape == (4, 1)
        with pytest.raises(capi.DomainError, match="prior component"):
            m.predict_conditional_context(ctx, [0], [1], variance=True)
        with pytest.raises(ValueError, match="no conditional prediction"):
            ctx.get_conditional(0, 0, 4, 1)
        with pytest.raises(ValueError, match="no conditional prediction"):
            ctx.get_conditional(0, 0, 4, 1, variance=True)
        assert m.predict_conditional_context(ctx, [0], [1]) == 1  # the same call without the variance keeps working
        assert np.all(np.isfinite(ctx.get_conditional(0, 0, NEW_ROWS, 1).mean))


def test_getter_errors_and_side_effects():
    m, Xnew, _ = _model("d5")
    with capi.Context(0) as ctx:
        ctx.set_data(Xnew[:, [3, 0]])
        assert m.predict_conditional_context(ctx, [3, 0]) == 3
        with pytest.raises(ValueError, match="no variance"):  # a mean-only prediction
            ctx.get_conditional(0, 0, 4, 3, variance=True)
        assert m.predict_conditional_context(ctx, [3, 0], variance=True) == 3
        whole = ctx.get_conditional(0, 0, NEW_ROWS, 3, variance=True)
        part = ctx.get_conditional(0, 5, 7, 3, variance=True)
        assert np.array_equal(part.var, whole.var[5:12]) and np.array_equal(part.mean, whole.mean[5:12])
        with pytest.raises(ValueError, match="out of bounds"):
            ctx.get_conditional(0, NEW_ROWS - 2, 3, 3, variance=True)
        with pytest.raises(ValueError, match="out of bounds"):
            ctx.get_conditional(1, 0, 1, 3, variance=True)
        buf = np.zeros((4, 3))
        assert capi.lib().lc_ctx_get_conditional_var(ctx._h, 0, 0, 4, capi.dptr(buf), 2) == capi.LC_EINVAL  # row_stride < ntarget
        assert b"row_stride" in capi.lib().lc_last_error()
        assert capi.lib().lc_ctx_get_conditional_var(ctx._h, 0, 0, 4, None, 0) == capi.LC_OK  # var may be NULL
        wide = np.full((4, 5), -1.0)
        assert capi.lib().lc_ctx_get_conditional_var(ctx._h, 0, 0, 4, capi.dptr(wide), 5) == capi.LC_OK
        assert np.array_equal(wide[:, :3], whole.var[:4]) and np.all(wide[:, 3:] == -1.0)
        # a later mean-only call, and a later plain prediction, take the variance away
        m.predict_conditional_context(ctx, [3, 0])
        with pytest.raises(ValueError, match="no variance"):
            ctx.get_conditional(0, 0, 4, 3, variance=True)
        m.predict_conditional_context(ctx, [3, 0], variance=True)
        ctx.set_data(Xnew)
        m.predict_context(ctx)
        with pytest.raises(ValueError, match="no conditional prediction"):
            ctx.get_conditional(0, 0, 4, 3, variance=True)
