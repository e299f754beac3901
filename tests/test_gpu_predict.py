"""Prediction with a learned mixture (lc_model_predict) on held-out rows.

The VB outputs (q, logZ, label) are checked against the oracle's vbexpectation (cluster.cpp:91-138) with the model's
posteriors set into oracle objects; the predictive log density against scipy's Student-t / Lomax densities mixed with
the expected weights; and both against what the library already computes (lc_estep_posterior, the free energy of
lc_vbem).  Every model comes from a few fixed-K VBEM iterations on the device (lc_vbem), so the whole file stays small."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from scipy import stats
from scipy.special import logsumexp

import lc_oracle as o
import libcluster_amd as lc
from libcluster_amd import capi

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

WCLS = {capi.W_DIRICHLET: lambda: o.Dirichlet(), capi.W_STICKBREAK: lambda: o.StickBreak(),
        capi.W_GDIRICHLET: lambda: o.GDirichlet()}
CCLS = {capi.C_GAUSSWISH: o.GaussWish, capi.C_NORMGAMMA: o.NormGamma, capi.C_EXPGAMMA: o.ExpGamma}


def _mixture(rng, N, D, K, family=capi.C_GAUSSWISH, spread=4.0):
    mu = rng.normal(0, spread, (K, D))
    z = rng.integers(0, K, N)
    if family == capi.C_EXPGAMMA:
        rate = rng.uniform(0.3, 3.0, (K, D))
        return rng.exponential(1.0 / rate[z])
    if family == capi.C_NORMGAMMA:
        return mu[z] + rng.normal(size=(N, D)) * rng.uniform(0.5, 2.0, (K, D))[z]
    return mu[z] + rng.normal(size=(N, D))


def _fit(Xs, wkind, ckind, K, iters=6, sparse=False, seed=0, clusterprior=1.0):
    """fixed-K VBEM on the device -> (model, training context)"""
    rng = np.random.default_rng(seed)
    ctx = capi.Context(0)
    ctx.set_data(Xs)
    ctx.set_qz([rng.dirichlet(np.ones(K), x.shape[0]) for x in Xs])
    _, _, m = ctx.vbem(wkind, fixed_iters=iters, sparse=sparse, ckind=ckind, clusterprior=clusterprior)
    return m, ctx


def _oracle(m, clusterprior=1.0):
    """the model's posteriors in oracle objects: (weights per group, clusters, prior cluster of `clusterprior`)"""
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
        c = CCLS[ck](clusterprior, D)
        if ck == capi.C_GAUSSWISH:
            c.nu, c.beta, c.m, c.iW, c.logdW = p["nu"], p["beta"], p["mean"], p["iW"], p["logdW"]
        elif ck == capi.C_NORMGAMMA:
            c.nu, c.beta, c.m, c.L, c.logL = p["nu"], p["beta"], p["mean"], p["L"], p["logL"]
        else:
            c.a, c.ib, c.logb = p["a"], p["ib"], p["logb"]
        c.N = p["N"]
        cls.append(c)
    return ws, cls, CCLS[ck](clusterprior, D)


def _oracle_vb(X, w, cls, sparse):
    K = len(cls)
    q, _ = o.vbexpectation(X, w, cls, sparse)
    Kful, _ = o._kful(K, sparse, w.getNk())
    logq = np.stack([w.Elogweight()[k] + cls[k].Eloglike(X) for k in Kful], axis=1)
    return q, o.logsumexp(logq).reshape(-1), logq, np.asarray(Kful)


def _expected_weights(w):
    """E[pi_k], E[pi_rest] from the oracle's alpha1 / alpha2 / sort order (the contract of lc_weights_predictive)"""
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


def _scipy_logpdf(c, X):
    if isinstance(c, o.GaussWish):
        D = c.D
        nup = c.nu + 1 - D
        shape = (1 + c.beta) / (nup * c.beta) * c.iW
        return stats.multivariate_t(loc=c.m, shape=shape, df=nup).logpdf(X).reshape(-1)
    if isinstance(c, o.NormGamma):
        scale = np.sqrt(c.L * (1 + c.beta) / (c.nu * c.beta))
        return stats.t.logpdf(X, df=2 * c.nu, loc=c.m, scale=scale).sum(axis=1)
    return stats.lomax.logpdf(X, c.a, scale=1.0 / c.ib).sum(axis=1)


def _scipy_logp(X, w, cls, prior):
    Epi, rest = _expected_weights(w)
    terms = [np.log(Epi[k]) + _scipy_logpdf(c, X) for k, c in enumerate(cls)]
    if rest > 0:
        terms.append(np.log(rest) + _scipy_logpdf(prior, X))
    return logsumexp(np.stack(terms, axis=1), axis=1)


def _check(pred, X, w, cls, prior, sparse, rtol_logp=1e-10):
    q, logZ, logq, Kful = _oracle_vb(X, w, cls, sparse)
    assert pred.label.dtype == np.int32 and pred.label.shape == (X.shape[0],)
    if pred.qZ is not None:
        assert np.max(np.abs(pred.qZ - q), initial=0.0) <= 1e-9
    np.testing.assert_allclose(pred.logZ, logZ, rtol=1e-10, atol=0)
    top = np.sort(q, axis=1)
    clear = (top[:, -1] - top[:, -2] > 1e-9) if q.shape[1] > 1 else np.ones(q.shape[0], bool)
    want = Kful[np.argmax(logq, axis=1)]
    assert np.array_equal(pred.label[clear], want[clear])
    ref = _scipy_logp(X, w, cls, prior)
    np.testing.assert_allclose(pred.logp, ref, rtol=rtol_logp, atol=0)
    # Jensen: exp E[log .] <= E[.] factor by factor
    assert np.all(pred.logZ <= pred.logp + 1e-12 * np.maximum(1.0, np.abs(pred.logp)))


FLAT = [  # (D, K, weights, family, cluster prior)
    (2, 3, capi.W_STICKBREAK, capi.C_GAUSSWISH, 1.0),   # xcat
    (5, 4, capi.W_DIRICHLET, capi.C_GAUSSWISH, 1.0),
    (23, 5, capi.W_STICKBREAK, capi.C_GAUSSWISH, 2.5),  # the prior component with a cluster prior other than 1
    (64, 6, capi.W_DIRICHLET, capi.C_GAUSSWISH, 1.0),
    (200, 3, capi.W_GDIRICHLET, capi.C_GAUSSWISH, 1.0),  # estep_wide_kernel
    # predict_diag_kernel: x in registers at DP = 32, 48, 64 (D = 23, 40, 64), re-read from the cache beyond (D = 100)
    (23, 4, capi.W_DIRICHLET, capi.C_NORMGAMMA, 1.0),
    (23, 4, capi.W_STICKBREAK, capi.C_EXPGAMMA, 1.0),
    (40, 4, capi.W_STICKBREAK, capi.C_NORMGAMMA, 0.5),
    (40, 3, capi.W_DIRICHLET, capi.C_EXPGAMMA, 1.0),
    (64, 3, capi.W_DIRICHLET, capi.C_NORMGAMMA, 1.0),
    (64, 3, capi.W_GDIRICHLET, capi.C_EXPGAMMA, 1.0),
    (100, 3, capi.W_DIRICHLET, capi.C_NORMGAMMA, 1.0),
    (100, 3, capi.W_STICKBREAK, capi.C_EXPGAMMA, 3.0),
]


@pytest.mark.parametrize("D,K,wk,ck,cp", FLAT)
def test_flat_models_vs_oracle_and_scipy(xcat, D, K, wk, ck, cp):
    rng = np.random.default_rng(100 + D + ck)
    if D == 2:
        Xall = xcat["Xcat"][rng.permutation(xcat["Xcat"].shape[0])]
        Xtr, Xte = Xall[: Xall.shape[0] // 2], Xall[Xall.shape[0] // 2:]
    else:
        Xall = _mixture(rng, (1200 if D < 100 else 700) + 1003, D, K, ck)
        Xtr, Xte = Xall[:-1003], Xall[-1003:]  # 1003 held-out rows: not a multiple of 16
    m, _ = _fit([Xtr], wk, ck, K, clusterprior=cp)
    w, cls, prior = _oracle(m, cp)
    p = m.predict(Xte, qz=True)
    _check(p, Xte, w[0], cls, prior, False)
    p1 = m.predict(Xte[:1])  # one row
    assert p1.qZ is None
    assert p1.label[0] == p.label[0] and abs(p1.logp[0] - p.logp[0]) <= 1e-12 * abs(p.logp[0])


def test_model_from_cluster():
    """a model of lc_cluster (model selection on device-resident rows) predicts like its posteriors say"""
    rng = np.random.default_rng(31)
    X = _mixture(rng, 2500, 6, 4)
    with capi.Context(0) as ctx:
        ctx.set_data(X[:1500])
        _, m = ctx.cluster(capi.W_STICKBREAK, maxclusters=6)
        w, cls, prior = _oracle(m)
        _check(m.predict(X[1500:], qz=True), X[1500:], w[0], cls, prior, False)
        m.close()


def test_sharded_models_predict_like_unsharded(xcat):
    """models of the in-process sharded learners (LIBCLUSTER_FORCE_SHARDED: one shard takes that path on one GPU; row
    blocks for learnVDP, whole groups for learnGMC, whose group weights are gathered from the shards) keep their
    parameters on the host: prediction gives what the unsharded model gives"""
    code = (
        "import json, sys\n"
        f"sys.path.insert(0, {str(ROOT)!r}); sys.path.insert(0, {str(ROOT / 'tests')!r})\n"
        "import numpy as np\n"
        "import libcluster_amd as lc\n"
        f"d = json.load(open({str(ROOT / 'tests' / 'golden' / 'xcat.json')!r}))\n"
        "X = [np.array(g) for g in d['X']]; Xn = np.vstack([x[:40] for x in X])\n"
        "out = {}\n"
        "for name, arg in (('learnVDP', np.vstack(X)), ('learnGMC', X)):\n"
        "    m = getattr(lc, name)(arg, return_model=True)[-1]\n"
        "    m.release_data()\n"
        "    p = m.predict([Xn, Xn], groups=[0, m.dims()[0] - 1])\n"
        "    out[name] = [[q.label.tolist(), q.logZ.tolist(), q.logp.tolist()] for q in p]\n"
        "    m.close()\n"
        "print('RESULT ' + json.dumps(out))\n")
    outs = []
    for env in ({}, {"LIBCLUSTER_GPUS": "1", "LIBCLUSTER_FORCE_SHARDED": "1"}):
        e = dict(os.environ)
        for k in ("LIBCLUSTER_GPUS", "LIBCLUSTER_GPUS_SAME_DEVICE", "LIBCLUSTER_FORCE_SHARDED", "LIBCLUSTER_COMM"):
            e.pop(k, None)
        e.update(env)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=e, cwd=str(ROOT))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(json.loads([x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1][7:]))
    a, b = outs
    for name in a:
        for pa, pb in zip(a[name], b[name]):
            assert pa[0] == pb[0]
            np.testing.assert_allclose(pb[1], pa[1], rtol=1e-10, atol=0)
            np.testing.assert_allclose(pb[2], pa[2], rtol=1e-10, atol=0)


@pytest.mark.parametrize("wk,sparse", [(capi.W_DIRICHLET, False), (capi.W_STICKBREAK, False),
                                       (capi.W_GDIRICHLET, False), (capi.W_GDIRICHLET, True)])
def test_grouped_models_and_empty_group(wk, sparse):
    rng = np.random.default_rng(7 + wk + 10 * sparse)
    D, K = 5, 5
    mu = rng.normal(0, 4.0, (K, D))
    # group 0 uses clusters 0-2, group 1 clusters 2-4: sparse mode leaves clusters out of each group's Kful
    X0 = mu[rng.integers(0, 3, 900)] + rng.normal(size=(900, D))
    X1 = mu[rng.integers(2, 5, 700)] + rng.normal(size=(700, D))
    m, _ = _fit([X0[:600], X1[:400]], wk, capi.C_GAUSSWISH, K, iters=8, sparse=sparse)
    w, cls, prior = _oracle(m)
    blocks = [X0[600:], np.zeros((0, D)), X1[400:], X1[400:417]]
    groups = [0, 1, 1, 0]
    preds = m.predict(blocks, groups=groups, qz=True)
    assert len(preds) == 4 and preds[1].label.shape == (0,) and preds[1].qZ.shape == (0, K)
    for X, g, p in zip(blocks, groups, preds):
        if X.shape[0]:
            _check(p, X, w[g], cls, prior, sparse)
    if sparse:
        assert any(np.all(p.qZ == 0.0, axis=0).any() for p in preds if p.qZ.shape[0])


def test_qz_equals_estep_posterior_and_vbem_free_energy():
    rng = np.random.default_rng(21)
    D, K = 7, 4
    X = _mixture(rng, 2000, D, K)
    with capi.Context(0) as ctx:
        ctx.set_data(X[:1500])
        ctx.set_qz(rng.dirichlet(np.ones(K), 1500))
        F, _, m = ctx.vbem(capi.W_DIRICHLET, fixed_iters=5)
        qtrain = ctx.get_qz([1500])[0]
        Fw, Fc = m.fenergy()
        own = m.predict(X[:1500], qz=True)  # the model's own training rows
        assert np.max(np.abs(own.qZ - qtrain)) <= 1e-12
        Fpred = Fw.sum() + Fc.sum() - own.logZ.sum()
        assert abs(Fpred - F) <= 1e-10 * abs(F), (Fpred, F)
        held = m.predict(X[1500:], qz=True)
        cl = [m.cluster(k) for k in range(K)]
        with capi.Context(0) as c2:
            c2.set_data(X[1500:])
            c2.estep_posterior([c["nu"] for c in cl], [c["beta"] for c in cl], np.array([c["mean"] for c in cl]),
                               np.array([c["iW"] for c in cl]), [c["logdW"] for c in cl], m.weights(0)[0])
            q = c2.get_qz([500])[0]
        assert np.max(np.abs(held.qZ - q)) <= 1e-13
        m.close()


def test_far_from_the_origin():
    """offset / sigma = 1e4: the predictive density to 1e-7 relative.  What limits it is the E-step's distance, formed
    as y = A x - b (tests/test_gpu_offset.py): |y| carries an error of about eps * |A x| ~ eps * 1e4 * sqrt(nu D)
    per row, d^2 = |y|^2 one of 2 |y| times that, and logp moves by (nu + 1) / (2 nu) of the change of d^2 -- about
    1e-9 absolute here, next to |logp| ~ 10 (the bar holds with two orders of magnitude to spare)."""
    rng = np.random.default_rng(5)
    D, K = 5, 3
    X = _mixture(rng, 2500, D, K, spread=3.0) + 1e4 * rng.uniform(0.5, 1.5, D)
    m, _ = _fit([X[:1500]], capi.W_STICKBREAK, capi.C_GAUSSWISH, K)
    w, cls, prior = _oracle(m)
    p = m.predict(X[1500:])
    np.testing.assert_allclose(p.logp, _scipy_logp(X[1500:], w[0], cls, prior), rtol=1e-7, atol=0)
    assert np.all(p.logZ <= p.logp + 1e-12 * np.maximum(1.0, np.abs(p.logp)))


@pytest.mark.parametrize("wk,ck", [(capi.W_STICKBREAK, capi.C_GAUSSWISH), (capi.W_DIRICHLET, capi.C_GAUSSWISH),
                                   (capi.W_DIRICHLET, capi.C_EXPGAMMA), (capi.W_STICKBREAK, capi.C_NORMGAMMA)])
def test_density_integrates_to_one_in_one_dimension(wk, ck):
    rng = np.random.default_rng(11 + ck)
    X = _mixture(rng, 800, 1, 3, ck, spread=3.0)
    m, _ = _fit([X], wk, ck, 3)
    # x = s tan(u) puts the heavy tails (Student-t with 1 degree of freedom for the prior component) into a bounded
    # integrand; midpoint rule in u
    n, s = 400_000, 2.0
    lo = 0.0 if ck == capi.C_EXPGAMMA else -np.pi / 2
    h = (np.pi / 2 - lo) / n
    u = lo + (np.arange(n) + 0.5) * h
    x = s * np.tan(u)
    p = m.predict(x.reshape(-1, 1))
    total = np.sum(np.exp(p.logp) * s / np.cos(u) ** 2) * h
    assert abs(total - 1.0) <= 1e-6, total


def test_device_resident_scale():
    """N = 2M, D = 64, K = 32 generated on the device, predicted without qZ; 20 000 rows checked against the oracle."""
    D, K, N = 64, 32, 2_000_000
    rng = np.random.default_rng(2)
    mu = rng.normal(0, 1.5, (K, D))
    L = np.tile(np.eye(D), (K, 1, 1)) * rng.uniform(0.5, 1.5, (K, 1, 1))
    with capi.Context(0) as tr, capi.Context(0) as ctx:
        tr.synth(200_000, D, K, mu, L, seed=9, row_offset=N, hard=0.6)
        _, _, m = tr.vbem(capi.W_DIRICHLET, fixed_iters=3)
        ctx.synth(N, D, K, mu, L, seed=9, row_offset=0)
        m.predict_context(ctx)
        w, cls, prior = _oracle(m)
        for r0 in rng.integers(0, N - 5000, 4):
            X = ctx.get_rows(0, int(r0), 5000)
            label, logZ, logp = ctx.get_predictions(0, int(r0), 5000)
            q, lz, logq, Kful = _oracle_vb(X, w[0], cls, False)
            np.testing.assert_allclose(logZ, lz, rtol=1e-10, atol=0)
            top = np.sort(q, axis=1)
            clear = top[:, -1] - top[:, -2] > 1e-9
            assert np.array_equal(label[clear], np.argmax(logq, axis=1)[clear])
            assert np.all(logZ <= logp + 1e-12 * np.maximum(1.0, np.abs(logp)))
        m.close()


def test_errors_and_release():
    rng = np.random.default_rng(3)
    X = np.abs(_mixture(rng, 900, 4, 3))
    m, tctx = _fit([X[:400], X[400:800]], capi.W_GDIRICHLET, capi.C_EXPGAMMA, 3)
    with capi.Context(0) as ctx:
        ctx.set_data(np.zeros((10, 5)))
        with pytest.raises(ValueError, match="Mismatched dims"):
            m.predict_context(ctx)
        ctx.set_data([X[800:850], X[850:]])
        for g in ([0, 2], [-1, 0]):
            with pytest.raises(ValueError, match="group index"):
                m.predict_context(ctx, groups=g)
        m.predict_context(ctx, groups=[1, 0])
        Xn = X[800:].copy()
        Xn[17, 2] = -1e-3
        ctx.set_data(Xn)
        with pytest.raises(ValueError, match=r"X has to be in the range \[0, inf\)!"):
            m.predict_context(ctx)
        with pytest.raises(ValueError):
            ctx.get_predictions(0, 0, 5)  # (new observations: no prediction yet)
    before = m.predict(X[800:])
    m.release_data()
    with pytest.raises(ValueError):
        m.qz_all([400, 400])
    after = m.predict(X[800:])
    assert np.array_equal(before.label, after.label) and np.array_equal(before.logp, after.logp)
    handle = m._h.value
    m.close()
    with capi.Context(0) as ctx:
        ctx.set_data(X[800:])
        assert capi.lib().lc_model_predict(C.c_void_p(handle), ctx._h, None, 0) == capi.LC_EINVAL
        assert b"freed" in capi.lib().lc_last_error()


@pytest.mark.parametrize("name", ["learnVDP", "learnBGMM", "learnDGMM", "learnBEMM", "learnGMC", "learnSGMC",
                                  "learnDGMC", "learnEGMC"])
def test_return_model_on_every_learner(xcat, name):
    grouped = name in ("learnGMC", "learnSGMC", "learnDGMC", "learnEGMC")
    Xs = [np.abs(x) if name.endswith("EMM") or name == "learnEGMC" else x for x in xcat["X"]]
    X = Xs if grouped else np.vstack(Xs)
    out = getattr(lc, name)(X, maxclusters=4, return_model=True)
    assert len(out) == 6
    m = out[-1]
    plain = getattr(lc, name)(X, maxclusters=4)
    assert len(plain) == 5 and plain[0] == out[0]
    K = m.dims()[1]
    Xn = np.vstack(Xs)[:37]
    p = m.predict(Xn, qz=True)
    assert isinstance(p, capi.Prediction)
    assert p.label.dtype == np.int32 and p.label.shape == (37,)
    assert p.logZ.dtype == np.float64 and p.logZ.shape == (37,) and p.logp.shape == (37,)
    assert p.qZ.shape == (37, K) and np.allclose(p.qZ.sum(axis=1), 1.0)
    assert np.all((p.label >= 0) & (p.label < K))
    m.close()
