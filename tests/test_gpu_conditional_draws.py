"""Draws of the conditional prediction (lc_model_predict_conditional_draws).

The reference is tests/sample_ref.py: numpy / scipy on the model's posteriors -- the responsibilities r_k(x_a) of the
marginal Student-t mixture and, per component, the conditional Student-t with eta = nu' + Da degrees of freedom, location
M_k(x_a) and scale c_k (1 + s_k d_k^2) S_k.  Whitened with the component its label names, a draw has t(eta) coordinates and
radius^2 / Db ~ F(Db, eta) whatever x_a is, so the draws of different rows pool.  Models are fitted on few rows (fixed-K VBEM
on the device from the true labels), so that eta is small.  Bars: KS p >= 1e-4 (on >= 50 000 draws per tested component in
the distribution test), frequencies within 5 binomial standard errors.  Seeds are fixed; none had to be changed."""
import functools

import numpy as np
import pytest

import lc_oracle as o
import sample_ref as sr
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

MODELS = {  # name: (weights, D, rows per training cluster, cluster prior)
    "d2_stick": (capi.W_STICKBREAK, 2, [5, 8, 11], 1.0),   # Da = Db = 1; the prior component has nu' = 1
    "d5_dir": (capi.W_DIRICHLET, 5, [5, 9, 7], 1.0),       # nu' = 6, 10, 8
    "d23_stick": (capi.W_STICKBREAK, 23, [5, 8, 12], 2.5),
    "d5_k1": (capi.W_DIRICHLET, 5, [9], 1.0),              # Kp = 1
    "d64_k34_stick": (capi.W_STICKBREAK, 64, [6] * 34, 1.0),  # Kp = 35 with the prior component
    "d140_stick": (capi.W_STICKBREAK, 140, [5, 8, 12], 1.0),  # wide enough to cross the draws kernel's own 64-wide panels
}
_perm64 = np.random.default_rng(64).permutation(64)
_perm140 = np.random.default_rng(140).permutation(140)
SPLITS = {  # name: (model, given, target)
    "d2_1|1": ("d2_stick", [1], [0]),
    "d5_2|3": ("d5_dir", [3, 0], None),                                                    # Db = 3: a padded quad
    "d23_8|3": ("d23_stick", list(range(0, 23, 3)), [1, 7, 22]),
    "d5_k1": ("d5_k1", [4, 1], [0, 3]),
    "d64_31|33": ("d64_k34_stick", sorted(int(c) for c in _perm64[:31]), [int(c) for c in _perm64[31:]]),  # Db = 33
    "d64_40|24": ("d64_k34_stick", sorted(int(c) for c in _perm64[:40]), [int(c) for c in _perm64[40:]]),  # Da = 40
    "d64_1|1": ("d64_k34_stick", [5], [9]),
    # cond_draws_kernel works in panels of 64 targets, chunks of 64 given columns (the ones column included) and chunks of
    # 64 normals: Db = 70 runs a second panel, whose normals and factor rows start at column 64; Da = 70 (Dae = 72) a
    # second chunk of given columns; Db = 129 a third panel whose last chunk holds one column
    "d140_10|70": ("d140_stick", sorted(int(c) for c in _perm140[:10]), [int(c) for c in _perm140[10:80]]),
    "d140_70|70": ("d140_stick", sorted(int(c) for c in _perm140[:70]), [int(c) for c in _perm140[70:]]),
    "d140_11|129": ("d140_stick", sorted(int(c) for c in _perm140[:11]), None),
}


def _centres(D, K):
    c = np.zeros((K, D))
    for k in range(K):
        c[k, k % D] = 12.0 * (1 + k // D)
        c[k, (k + 1) % D] -= 7.0 * k
    return c


@functools.lru_cache(maxsize=None)
def _model(name):
    """-> (model, training context, centres): fitted once, shared by the tests and never changed"""
    wk, D, sizes, cp = MODELS[name]
    rng = np.random.default_rng(1700 + D + len(sizes))
    K = len(sizes)
    cen = _centres(D, K)
    z = np.repeat(np.arange(K), sizes)
    X = cen[z] + rng.normal(size=(z.size, D))
    q = np.ones((z.size, 1))
    if K > 1:
        q = np.full((z.size, K), 0.02 / (K - 1))
        q[np.arange(z.size), z] = 0.98
    ctx = capi.Context(0)
    ctx.set_data(X)
    ctx.set_qz(q)
    _, _, m = ctx.vbem(wk, fixed_iters=6, clusterprior=cp)
    return m, ctx, cen


def _reference(split):
    """-> (components, weights, given, target) of a split: sample_ref's conditional components, the prior one last"""
    name, given, target = SPLITS[split]
    m, _, _ = _model(name)
    _, D, _, cp = MODELS[name]
    _, K, _ = m.dims()
    tg = list(target) if target is not None else [c for c in range(D) if c not in set(given)]
    e, rest = capi.weights_predictive(m.kinds()[0], m.weights(0)[1])
    posts = [(p["nu"], p["beta"], p["mean"], p["iW"]) for p in (m.cluster(k) for k in range(K))]
    w = list(e)
    if rest > 0:
        pr = o.GaussWish(cp, D)
        posts.append((pr.nu, pr.beta, pr.m, pr.iW))
        w.append(rest)
    return [sr.CondComponent(*p, given, tg) for p in posts], np.array(w), given, tg


def _rows(split, rng, n):
    """held-out known columns: rows of the training mixture, some of them between two clusters"""
    name, given, _ = SPLITS[split]
    _, _, cen = _model(name)
    K, D = cen.shape
    z = rng.integers(0, K, n)
    X = cen[z] + rng.normal(size=(n, D)) * 2.0
    half = rng.random(n) < 0.3
    X[half] = 0.5 * (X[half] + cen[(z[half] + 1) % K])
    return np.ascontiguousarray(X[:, given])


def test_distribution_four_rows_50000_copies():
    """4 distinct x_a, 50 000 copies each, 4 draws per copy: one near a cluster, two between clusters, one far out"""
    split = "d5_2|3"
    comps, w, given, tg = _reference(split)
    m, _, cen = _model("d5_dir")

    def between(a, b):
        """the point of the segment between two centres where, by the reference, the second largest r_k is largest"""
        line = np.array([(1 - t) * cen[a, given] + t * cen[b, given] for t in np.linspace(0.0, 1.0, 2001)])
        return line[np.argmax(np.sort(sr.responsibilities(comps, w, line), axis=1)[:, -2])]

    xa = np.array([cen[0, given] + 0.3, between(0, 1), between(1, 2), cen[2, given] + 9.0])
    copies, nd = 50_000, 4
    Xa = np.repeat(xa, copies, axis=0)
    got = m.predict_conditional(Xa, given, draws=nd, seed=77)
    plain = m.predict_conditional(Xa, given)
    assert np.array_equal(got.mean, plain.mean) and np.array_equal(got.logp, plain.logp)  # bit for bit
    assert got.draws.shape == (4 * copies, nd, 3) and got.label.shape == (4 * copies, nd)
    assert np.all(np.isfinite(got.draws))
    r = sr.responsibilities(comps, w, xa)
    var = m.predict_conditional(xa, given, variance=True)
    tally, multimodal = sr.Tally(), 0
    for i in range(4):
        rows = slice(i * copies, (i + 1) * copies)
        lab, dr = got.label[rows].reshape(-1), got.draws[rows].reshape(-1, 3)
        sr.check_frequencies(lab, r[i], f"x_a {i}")
        tested = 0
        for k, c in enumerate(comps):
            x = dr[lab == k]
            if x.shape[0] < 50_000:
                continue
            tested += 1
            wh = c.whiten(np.repeat(xa[i:i + 1], x.shape[0], axis=0), x)
            tally.add(sr.ks_whitened(wh, c.eta), f"x_a {i} component {k} (eta {c.eta:g}, {x.shape[0]} draws)")
        assert tested >= 1
        multimodal += tested >= 2
        # the average of the draws against the mean and the variance of the merged kernels
        avg = dr.mean(axis=0)
        bound = 5 * np.sqrt(var.var[i] / dr.shape[0])
        print(f"x_a {i}: |average - mean| / bound = {np.max(np.abs(avg - var.mean[i]) / bound):.3f} (bar 1)")
        assert np.all(np.abs(avg - var.mean[i]) <= bound)
    assert multimodal >= 1  # (not vacuous: some x_a draws from two experts)
    print(f"conditional draws: {tally.n} KS tests, largest statistic {tally.stat:.3e}, smallest p {tally.p:.3e}")


@pytest.mark.parametrize("split,n,nd", [("d2_1|1", 30_000, 4), ("d23_8|3", 20_000, 5), ("d5_k1", 3000, 1),
                                        ("d64_31|33", 1500, 64), ("d64_40|24", 3000, 3), ("d64_1|1", 3000, 7),
                                        ("d140_10|70", 3000, 3), ("d140_70|70", 2000, 5), ("d140_11|129", 1000, 2)])
def test_shapes_pooled_over_rows(split, n, nd):
    """Db = 1, 3, 33, 70 and 129, Da = 1, 40 and 70, Kp = 1 and 35, ndraws = 1 and 64: every draw whitened with the component its label
    names, pooled over rows per component; labels against numpy's r_k(x_a); exact labels from the documented counters"""
    comps, w, given, tg = _reference(split)
    m, _, _ = _model(SPLITS[split][0])
    rng = np.random.default_rng(len(split) + n)
    Xa = _rows(split, rng, n)
    seed = (11 << 32) + 5
    got = m.predict_conditional(Xa, given, SPLITS[split][2], draws=nd, seed=seed)
    plain = m.predict_conditional(Xa, given, SPLITS[split][2])
    assert np.array_equal(got.mean, plain.mean) and np.array_equal(got.logp, plain.logp)
    Db, Kp = len(tg), len(comps)
    assert got.draws.shape == (n, nd, Db) and np.all(np.isfinite(got.draws))
    assert got.label.min() >= 0 and got.label.max() < Kp
    r = sr.responsibilities(comps, w, Xa)
    # exact labels: u of every (row, draw) from the numpy Philox, the choice from numpy's cumulative r_k
    left = 0
    for i in range(nd):
        want, far = sr.choose(sr.choice_u(seed, 0, np.arange(n), i), r)
        assert np.array_equal(got.label[far, i], want[far]), (split, i)
        left += int((~far).sum())
    print(f"{split}: {left} of {n * nd} labels left out (within 1e-9 of a boundary)")
    assert left <= 1e-3 * n * nd
    # expected label frequencies: the mean of r_k over the rows (a sum of independent Bernoulli draws: the binomial
    # standard error of the mean weight bounds its standard error)
    sr.check_frequencies(got.label.reshape(-1), r.mean(axis=0), split)
    # every draw, whitened with the component its label names and sent through that component's CDFs: uniforms that pool
    parts = []
    for k, c in enumerate(comps):
        rows, draws = np.nonzero(got.label == k)
        if rows.size:
            parts.append((c.whiten(Xa[rows], got.draws[rows, draws]), c.eta))
    assert sum(p[0].shape[0] for p in parts) == n * nd
    sr.Tally().add(sr.ks_whitened_pooled(parts), f"{split} ({len(parts)} components drawn from, {n * nd} draws)")


def test_same_bits_and_what_a_draw_depends_on():
    split = "d23_8|3"
    comps, w, given, tg = _reference(split)
    m, _, _ = _model("d23_stick")
    rng = np.random.default_rng(3)
    Xa = _rows(split, rng, 300)  # four full waves and one of 44 rows
    a = m.predict_conditional(Xa, given, tg, draws=7, seed=1)
    b = m.predict_conditional(Xa, given, tg, draws=7, seed=1)
    assert np.array_equal(a.draws, b.draws) and np.array_equal(a.label, b.label)
    c = m.predict_conditional(Xa, given, tg, draws=7, seed=2)
    assert not np.any(np.all(a.draws.reshape(300, -1) == c.draws.reshape(300, -1), axis=1))
    # ndraws: the first 3 of 7
    d = m.predict_conditional(Xa, given, tg, draws=3, seed=1)
    assert np.array_equal(d.draws, a.draws[:, :3]) and np.array_equal(d.label, a.label[:, :3])
    # N: the first n rows of 2n, and a row's neighbours
    e = m.predict_conditional(np.vstack([Xa, Xa[::-1]]), given, tg, draws=7, seed=1)
    assert np.array_equal(e.draws[:300], a.draws) and np.array_equal(e.label[:300], a.label)
    f = m.predict_conditional(np.vstack([Xa[:100], Xa[:200][::-1]]), given, tg, draws=7, seed=1)
    assert np.array_equal(f.draws[:100], a.draws[:100])
    # blocks: block 0 does not depend on J; block 1 has its own counters
    g = m.predict_conditional([Xa, Xa], given, tg, draws=7, seed=1)
    assert np.array_equal(g[0].draws, a.draws) and np.array_equal(g[0].label, a.label)
    assert not np.array_equal(g[1].draws, a.draws)
    want, far = sr.choose(sr.choice_u(1, 1, np.arange(300), 2), sr.responsibilities(comps, w, Xa))
    assert np.array_equal(g[1].label[far, 2], want[far])


def test_two_blocks_with_different_groups():
    rng = np.random.default_rng(8)
    D, K, sizes = 3, 2, ([9, 2], [3, 8])
    cen = _centres(D, K)
    Xs, qs = [], []
    for s in sizes:
        z = np.repeat(np.arange(K), s)
        Xs.append(cen[z] + rng.normal(size=(z.size, D)))
        q = np.full((z.size, K), 0.02)
        q[np.arange(z.size), z] = 0.98
        qs.append(q)
    ctx = capi.Context(0)
    ctx.set_data(Xs)
    ctx.set_qz(qs)
    _, _, m = ctx.vbem(capi.W_GDIRICHLET, fixed_iters=6)
    given, tg = [0], [1, 2]
    posts = [(p["nu"], p["beta"], p["mean"], p["iW"]) for p in (m.cluster(k) for k in range(K))]
    comps = [sr.CondComponent(*p, given, tg) for p in posts]
    # between the clusters, where by the reference learned group 0 gives both a share: the weights decide
    line = np.array([(1 - t) * cen[0, given] + t * cen[1, given] for t in np.linspace(0.0, 1.0, 2001)])
    w0 = capi.weights_predictive(m.kinds()[0], m.weights(0)[1])[0]
    at = line[np.argmax(sr.responsibilities(comps, w0, line).min(axis=1))]
    xa = np.repeat(at[None, :], 40_000, axis=0)
    got = m.predict_conditional([xa, xa], given, tg, groups=[1, 0], draws=2, seed=4)
    for b, j in ((0, 1), (1, 0)):
        w = capi.weights_predictive(m.kinds()[0], m.weights(j)[1])[0]
        r = sr.responsibilities(comps, w, xa[:1])[0]
        sr.check_frequencies(got[b].label.reshape(-1), r, f"block {b} with learned group {j}")
    assert abs(np.mean(got[0].label) - np.mean(got[1].label)) > 0.1  # (not vacuous: the groups mix differently)


def test_device_level_calls_and_errors():
    split = "d5_2|3"
    comps, w, given, tg = _reference(split)
    m, train, _ = _model("d5_dir")
    Xa = _rows(split, np.random.default_rng(1), 100)
    with capi.Context(0) as ctx:
        ctx.set_data(Xa)
        nt = m.predict_conditional_context(ctx, given, draws=5, seed=3)
        assert nt == 3
        assert ctx.conditional_draws() == (5, 3)  # the library's own counts size the download
        with pytest.raises(ValueError):
            ctx.get_conditional(0, 0, 10, nt, draws=4)  # not the count of this prediction: refused, nothing is copied
        part = ctx.get_conditional(0, 10, 50, nt, draws=True)
        whole = m.predict_conditional(Xa, given, draws=5, seed=3)
        assert np.array_equal(part.draws, whole.draws[10:60]) and np.array_equal(part.label, whole.label[10:60])
        assert np.array_equal(part.mean, whole.mean[10:60]) and part.var is None
        with pytest.raises(ValueError):
            ctx.get_conditional(0, 0, 101, nt, draws=True)
        with pytest.raises(ValueError):
            ctx.get_conditional(0, 0, 10, nt, variance=True)  # this prediction has draws, no variance
        # a failed call leaves no prediction on the context
        for bad in (0, 65):
            with pytest.raises(ValueError):
                m.predict_conditional_context(ctx, given, draws=bad)
        rc = capi.lib().lc_model_predict_conditional_draws(m._h, ctx._h, None, (capi.C.c_int * 2)(3, 0), 2, None, 0, 0, 0)
        assert rc == capi.LC_EINVAL  # ndraws = 0 at the C boundary
        with pytest.raises(ValueError):
            ctx.get_conditional(0, 0, 10, nt)
        with pytest.raises(ValueError):
            m.predict_conditional_context(ctx, [0, 0], draws=2)  # the cases of lc_model_predict_conditional
        with pytest.raises(ValueError):
            m.predict_conditional_context(ctx, [0, 1, 2], draws=2)  # the context's width is 2
        # a plain prediction has no draws
        m.predict_conditional_context(ctx, given)
        with pytest.raises(ValueError):
            ctx.get_conditional(0, 0, 10, nt, draws=5)
        # an empty context is fine
        ctx.set_data(np.zeros((0, 2)))
        assert m.predict_conditional_context(ctx, given, draws=4) == 3
        assert ctx.get_conditional(0, 0, 0, 3, draws=True).draws.shape == (0, 4, 3)
    # a freed model
    m2, _ = _diag_model()
    handle = m2._h.value
    m2.close()
    with capi.Context(0) as ctx:
        ctx.set_data(Xa)
        gv = (capi.C.c_int * 2)(3, 0)
        assert capi.lib().lc_model_predict_conditional_draws(capi.C.c_void_p(handle), ctx._h, None, gv, 2, None, 0, 2, 0) == capi.LC_EINVAL
        assert b"freed" in capi.lib().lc_last_error()
        assert ctx.conditional_draws() == (0, 0)
    with pytest.raises(ValueError):
        m.predict_conditional(Xa, given, variance=True, draws=2)
    with pytest.raises(ValueError):
        m.predict_conditional(Xa, given, draws=0)
    with pytest.raises(ValueError):
        m.predict_conditional(Xa, given, draws=65)
    ng, _ = _diag_model()
    with pytest.raises(ValueError):
        ng.predict_conditional(Xa, given, draws=2)  # Gauss-Wishart only


def _diag_model():
    rng = np.random.default_rng(0)
    ctx = capi.Context(0)
    ctx.set_data(rng.normal(size=(30, 5)))
    ctx.set_qz(np.ones((30, 1)))
    _, _, m = ctx.vbem(capi.W_DIRICHLET, fixed_iters=2, ckind=capi.C_NORMGAMMA)
    return m, ctx


def test_impute_draws_are_multiple_imputations():
    m, _, cen = _model("d5_dir")
    rng = np.random.default_rng(6)
    X = cen[rng.integers(0, 3, 200)] + rng.normal(size=(200, 5))
    holes = X.copy()
    holes[:, [1, 4]] = np.nan
    copies = m.impute(holes, [1, 4], draws=3, seed=9)
    assert isinstance(copies, list) and len(copies) == 3
    ref = m.predict_conditional(X[:, [0, 2, 3]], [0, 2, 3], [1, 4], draws=3, seed=9)
    for i, c in enumerate(copies):
        assert c.shape == X.shape and np.array_equal(c[:, [0, 2, 3]], X[:, [0, 2, 3]])
        assert np.array_equal(c[:, [1, 4]], ref.draws[:, i, :])
    assert not np.array_equal(copies[0], copies[1])
    blocks = m.impute([holes, holes[:50]], [1, 4], draws=2, seed=9)
    assert len(blocks) == 2 and len(blocks[0]) == 2 and blocks[1][0].shape == (50, 5)
    assert np.array_equal(blocks[0][0], copies[0])
    with pytest.raises(ValueError):
        m.impute(holes, [1, 4], draws=2, return_var=True)
