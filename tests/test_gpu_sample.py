"""New rows from a learned model (lc_model_sample).

Models are fitted on few rows (fixed-K VBEM on the device from the true labels, as the _fit helpers of the prediction tests
do), so that the Student-t densities have few degrees of freedom and a wrong count shows: nu' = 1 + N_k for a Gauss-Wishart
cluster of N_k rows, nu' = 1 for the prior component of StickBreak weights.  The statistical bars are those of
tests/sample_ref.py (KS p >= 1e-4 on >= 50 000 draws per tested component, label frequencies within 5 standard errors);
tests/test_sample_host.py shows that numpy's own generators pass them.  Seeds are fixed; none had to be changed."""
import ctypes as C
import functools

import numpy as np
import pytest

import lc_oracle as o
import sample_ref as sr
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

MIN_DRAWS = 50_000
MODELS = {  # name: (family, weights, D, rows per training cluster and block, cluster prior)
    "gw_d2_stick": (capi.C_GAUSSWISH, capi.W_STICKBREAK, 2, [[5, 8, 11]], 1.0),      # nu' = 6, 9, 12 and the prior's 1
    "gw_d5_dir": (capi.C_GAUSSWISH, capi.W_DIRICHLET, 5, [[5, 9]], 1.0),              # nu' = 6, 10
    "gw_d23_stick": (capi.C_GAUSSWISH, capi.W_STICKBREAK, 23, [[5, 8, 12]], 2.5),
    "gw_d23_stick1": (capi.C_GAUSSWISH, capi.W_STICKBREAK, 23, [[2]], 2.5),           # E[pi_rest] = 1/4: the prior's nu' = 1 at D = 23
    "gw_d400": (capi.C_GAUSSWISH, capi.W_DIRICHLET, 400, [[5]], 1.0),                 # DP = 448: 56 KB of normals per block
    "gw_d520": (capi.C_GAUSSWISH, capi.W_DIRICHLET, 520, [[5]], 1.0),                 # DP = 576: 72 KB, the kernel's LDS limit is raised
    "gw_d1": (capi.C_GAUSSWISH, capi.W_DIRICHLET, 1, [[4]], 1.0),                     # K = 1, nu' = 5
    "gw_d3": (capi.C_GAUSSWISH, capi.W_DIRICHLET, 3, [[6]], 1.0),                     # an odd D: the pair's tail
    "gw_d200": (capi.C_GAUSSWISH, capi.W_DIRICHLET, 200, [[5]], 1.0),                 # DP = 256: 32 KB of normals per block
    "ng_d4_stick": (capi.C_NORMGAMMA, capi.W_STICKBREAK, 4, [[6, 10]], 1.0),          # 2 nu = 8, 12 and the prior's 2
    "eg_d3_dir": (capi.C_EXPGAMMA, capi.W_DIRICHLET, 3, [[6, 12]], 1.0),              # a = 7, 13
    "gw_d2_groups": (capi.C_GAUSSWISH, capi.W_GDIRICHLET, 2, [[9, 2, 6], [2, 8, 7]], 1.0),  # two learned groups
}
# rows drawn, so that every component meets MIN_DRAWS -- the prior component of the two small StickBreak models included
# (E[pi_rest] is 0.03 and 0.05 there); at D = 23 that would take 1.8M rows of gw_d23_stick, whose 0.03 is left to the
# frequency check: gw_d23_stick1, one cluster of two rows, gives the prior component a quarter of the rows instead
SAMPLES = {"gw_d2_stick": 2_000_000, "gw_d5_dir": 200_000, "gw_d23_stick": 340_000, "gw_d23_stick1": 230_000, "gw_d1": 60_000,
           "gw_d3": 60_000, "gw_d200": 50_000, "gw_d400": 20_000, "gw_d520": 20_000, "ng_d4_stick": 1_300_000,
           "eg_d3_dir": 200_000}
TESTED = {"gw_d2_stick": 4, "gw_d5_dir": 2, "gw_d23_stick": 3, "gw_d23_stick1": 2, "gw_d1": 1, "gw_d3": 1, "ng_d4_stick": 3,
          "eg_d3_dir": 2}


def _training(rng, family, D, sizes):
    """well-separated clusters: rows and their true labels"""
    X, z = [], []
    for k, n in enumerate(sizes):
        if family == capi.C_EXPGAMMA:
            X.append(rng.exponential(10.0 ** k, (n, D)))
        else:
            centre = np.zeros(D)
            centre[k % D] = 40.0 * (1 + k // D)
            centre[(k + 1) % D] -= 25.0 * k
            X.append(centre + rng.normal(size=(n, D)))
        z += [k] * n
    return np.vstack(X), np.array(z)


@functools.lru_cache(maxsize=None)
def _model(name):
    """-> (model, components per learned group): fitted once, shared by the tests and never changed.  A component is
    (kind, parameters...) in the order 0 ... K - 1, then the prior component when it has weight."""
    family, wk, D, blocks, cp = MODELS[name]
    rng = np.random.default_rng(1600 + D + len(blocks))
    K = len(blocks[0])
    Xs, qs = [], []
    for sizes in blocks:
        X, z = _training(rng, family, D, sizes)
        q = np.full((X.shape[0], K), 0.02 / max(K - 1, 1)) if K > 1 else np.ones((X.shape[0], 1))
        if K > 1:
            q[np.arange(z.size), z] = 0.98
        Xs.append(X)
        qs.append(q)
    ctx = capi.Context(0)
    ctx.set_data(Xs)
    ctx.set_qz(qs)
    _, _, m = ctx.vbem(wk, fixed_iters=6, ckind=family, clusterprior=cp)
    return m, ctx


def _weights(m, j):
    """E[pi_k] of learned group j, the prior component's E[pi_rest] appended when any group has one"""
    J = m.dims()[0]
    ws = [capi.weights_predictive(m.kinds()[0], m.weights(g)[1]) for g in range(J)]
    e, r = ws[j]
    return np.append(e, r) if any(w[1] > 0 for w in ws) else e


def _components(name):
    """the densities of the model's components, from its posteriors and the formulas of the header"""
    m, _ = _model(name)
    family, _, D, _, cp = MODELS[name]
    _, K, _ = m.dims()
    Kp = _weights(m, 0).size
    out = []
    for k in range(Kp):
        if family == capi.C_GAUSSWISH:
            p = m.cluster(k) if k < K else None
            pr = o.GaussWish(cp, D)
            out.append(sr.gw_student(*((p["nu"], p["beta"], p["mean"], p["iW"]) if p else (pr.nu, pr.beta, pr.m, pr.iW))))
        elif family == capi.C_NORMGAMMA:
            p = m.cluster(k) if k < K else None
            pr = o.NormGamma(cp, D)
            out.append(sr.ng_student(*((p["nu"], p["beta"], p["mean"], p["L"]) if p else (pr.nu, pr.beta, pr.m, pr.L))))
        else:
            p = m.cluster(k) if k < K else None
            pr = o.ExpGamma(cp, D)
            out.append(sr.eg_lomax(*((p["a"], p["ib"]) if p else (pr.a, pr.ib))))
    return out


def _ks(family, x, comp):
    if family == capi.C_GAUSSWISH:
        return sr.ks_student(x, *comp)
    return sr.ks_student_diag(x, *comp) if family == capi.C_NORMGAMMA else sr.ks_lomax(x, *comp)


@pytest.mark.parametrize("name", ["gw_d2_stick", "gw_d5_dir", "gw_d23_stick", "gw_d23_stick1", "gw_d1", "gw_d3", "ng_d4_stick",
                                  "eg_d3_dir"])
def test_distribution_per_component(name):
    m, _ = _model(name)
    family = MODELS[name][0]
    comps, w = _components(name), _weights(m, 0)
    s = m.sample(SAMPLES[name], seed=31)
    assert s.rows.shape == (SAMPLES[name], m.dims()[2]) and s.label.shape == (SAMPLES[name],)
    assert np.all(np.isfinite(s.rows))
    if family == capi.C_EXPGAMMA:
        assert np.all(s.rows >= 0)
    sr.check_frequencies(s.label, w, name)
    tally, tested = sr.Tally(), 0
    for k, comp in enumerate(comps):
        x = s.rows[s.label == k][:60_000]  # (>= 50 000 draws per tested component: what the bar was sized for)
        if x.shape[0] < MIN_DRAWS:
            continue
        tested += 1
        dof = comp[2] if family != capi.C_EXPGAMMA else comp[0]
        tally.add(_ks(family, x, comp), f"{name} component {k} (dof / shape {dof:g}, {x.shape[0]} draws)")
    assert tested == TESTED[name], "every learned cluster gets its test, and the prior component where SAMPLES says so"
    print(f"{name}: {tally.n} KS tests, largest statistic {tally.stat:.3e}, smallest p {tally.p:.3e}")


def test_wide_rows_d200():
    """a 200 x 200 triangular product per row, its normals in 32 KB of LDS per block: the radius over all coordinates and
    the coordinates at both ends and at the 64-column boundaries"""
    name = "gw_d200"
    m, _ = _model(name)
    loc, Scale, dof = _components(name)[0]
    s = m.sample(SAMPLES[name], seed=5)
    assert np.all(s.label == 0) and np.all(np.isfinite(s.rows))
    L = np.linalg.cholesky(Scale)
    w = np.linalg.solve(L, (s.rows - loc).T).T
    from scipy import stats

    res = [stats.kstest((w * w).sum(axis=1) / 200, stats.f(200, dof).cdf)]
    res += [stats.kstest(w[:, d], stats.t(dof).cdf) for d in (0, 1, 63, 64, 127, 128, 198, 199)]
    sr.Tally().add(res, f"{name} (dof {dof:g})")


@pytest.mark.parametrize("name", ["gw_d400", "gw_d520"])
def test_wide_rows_past_48_and_64_kb_of_lds(name):
    """16 rows of normals are 56 KB at D = 400 and 72 KB at D = 520, where the launcher has to raise the kernel's limit:
    row-group edges, and the whitened radius over all coordinates with the coordinates at both ends"""
    m, _ = _model(name)
    D = MODELS[name][2]
    loc, Scale, dof = _components(name)[0]
    s = m.sample(SAMPLES[name], seed=6)
    assert np.all(s.label == 0) and np.all(np.isfinite(s.rows))
    for n in (1, 15, 16, 17):
        e = m.sample(n, seed=6)
        assert np.array_equal(e.rows, s.rows[:n]), n
    w = np.linalg.solve(np.linalg.cholesky(Scale), (s.rows - loc).T).T
    from scipy import stats

    res = [stats.kstest((w * w).sum(axis=1) / D, stats.f(D, dof).cdf)]
    res += [stats.kstest(w[:, d], stats.t(dof).cdf) for d in (0, 1, D // 2, D - 2, D - 1)]
    sr.Tally().add(res, f"{name} (dof {dof:g}, {s.rows.shape[0]} draws)")


def test_grouped_model_blocks_use_their_groups():
    name = "gw_d2_groups"
    m, _ = _model(name)
    assert m.dims()[0] == 2
    n = 120_000
    both = m.sample([n, n], seed=9, groups=[1, 0])
    w0, w1 = _weights(m, 0), _weights(m, 1)
    assert np.max(np.abs(w0 - w1)) > 0.1  # (not vacuous: the two learned groups mix the clusters differently)
    sr.check_frequencies(both[0].label, w1, "block 0 with learned group 1")
    sr.check_frequencies(both[1].label, w0, "block 1 with learned group 0")
    comps = _components(name)
    tally = sr.Tally()
    for b in (0, 1):
        for k, comp in enumerate(comps):
            x = both[b].rows[both[b].label == k]
            if x.shape[0] >= MIN_DRAWS:
                tally.add(sr.ks_student(x[:60_000], *comp), f"{name} block {b} component {k}")
    assert tally.n > 0
    # block b's rows depend on b, not on J
    alone = m.sample([n], seed=9, groups=[1])
    assert np.array_equal(alone[0].rows, both[0].rows) and np.array_equal(alone[0].label, both[0].label)


@pytest.mark.parametrize("name", ["gw_d2_stick", "ng_d4_stick", "eg_d3_dir", "gw_d2_groups"])
def test_exact_labels_from_the_documented_counters(name):
    """u of every row from the numpy Philox and the counter table of the header, the choice from numpy's cumulative weights"""
    m, _ = _model(name)
    J = m.dims()[0]
    counts, groups, seed, off = [40_000, 1_000, 17], [J - 1, 0, 0], (7 << 32) + 12345, 3_000_000_000
    with capi.Context(0) as ctx:
        m.sample_context(ctx, counts, groups, seed=seed, row_offset=off)
        left = total = 0
        for b, n in enumerate(counts):
            lab = ctx.get_sample_labels(b, 0, n)
            u = sr.choice_u(seed, b, np.arange(n), 0, off)
            want, far = sr.choose(u, _weights(m, groups[b]))
            assert np.array_equal(lab[far], want[far]), (name, b)
            left += int((~far).sum())
            total += n
    print(f"{name}: {left} of {total} labels left out (within 1e-9 of a boundary)")
    assert left <= 1e-3 * total


def test_numpy_generator_reproduces_synth():
    """the test's Philox, u01 and Box-Muller against the generator that predates the samplers"""
    N, D, seed, off = 1000, 5, (3 << 32) + 99, 123
    with capi.Context(0) as ctx:
        ctx.synth(N, D, 1, np.zeros((1, D)), np.eye(D)[None], seed, row_offset=off)
        got = ctx.get_rows(0, 0, N)
    want = sr.synth_rows(seed, N, D, off)
    print(f"synth against numpy: max |difference| = {np.max(np.abs(got - want)):.3e} (bar 1e-12)")
    assert np.max(np.abs(got - want)) <= 1e-12


@pytest.mark.parametrize("name", ["gw_d5_dir", "ng_d4_stick", "eg_d3_dir"])
def test_same_bits_other_seed_and_shards(name):
    m, _ = _model(name)
    a, b = m.sample(1000, seed=4), m.sample(1000, seed=4)
    assert np.array_equal(a.rows, b.rows) and np.array_equal(a.label, b.label)
    c = m.sample(1000, seed=5)
    assert not np.any(np.all(a.rows == c.rows, axis=1))
    D = m.dims()[2]
    with capi.Context(0) as ctx:
        for lo, hi in ((0, 17), (17, 500), (333, 1000)):  # shards that do not start on a row group
            m.sample_context(ctx, [hi - lo], seed=4, row_offset=lo)
            assert np.array_equal(ctx.get_rows(0, 0, hi - lo), a.rows[lo:hi]), (lo, hi)
            assert np.array_equal(ctx.get_sample_labels(0, 0, hi - lo), a.label[lo:hi])
        assert ctx.dims()[1] == D


@pytest.mark.parametrize("name", ["gw_d1", "gw_d3", "gw_d23_stick", "gw_d200", "ng_d4_stick"])
def test_row_group_edges(name):
    """N = 1, 15, 16, 17 rows: a row does not depend on how many follow it"""
    m, _ = _model(name)
    full = m.sample(1000, seed=2)
    assert np.all(np.isfinite(full.rows))
    for n in (1, 15, 16, 17):
        s = m.sample(n, seed=2)
        assert np.array_equal(s.rows, full.rows[:n]) and np.array_equal(s.label, full.label[:n]), n


@pytest.mark.parametrize("name", ["gw_d2_stick", "gw_d23_stick", "ng_d4_stick", "eg_d3_dir"])
def test_predict_on_a_sampled_context(name):
    m, _ = _model(name)
    family = MODELS[name][0]
    K = m.dims()[1]
    n = 20_000
    with capi.Context(0) as ctx:
        m.sample_context(ctx, [n], seed=8)
        lab = ctx.get_sample_labels(0, 0, n)
        rows = ctx.get_rows(0, 0, n)
        m.predict_context(ctx)  # (no domain error: ExpGamma rows are >= 0)
        plab, logZ, logp = ctx.get_predictions(0, 0, n)
        assert np.array_equal(ctx.get_sample_labels(0, 0, n), lab)  # the rows still come from the sampler
    assert np.all(np.isfinite(logp)) and np.all(np.isfinite(logZ))
    if family == capi.C_EXPGAMMA:
        return
    # where the clusters are well separated: a row whose whitened radius^2 is below D / 4.  Few training rows far from the
    # prior mean leave wide posteriors, stretched towards the origin by the term beta_p N / beta (xbar - m_p)(xbar - m_p)^T
    # of iW: at D = 23 the oracle's classes on the same training rows, with numpy's draws, relabel 398 of 90 152 rows
    # inside one scale radius (radius^2 < D) and none of 2 409 inside half of it (smallest margin 29 nats).
    comps, agree, central = _components(name), 0, 0
    for k in range(K):
        x = rows[lab == k]
        if family == capi.C_GAUSSWISH:
            w = np.linalg.solve(np.linalg.cholesky(comps[k][1]), (x - comps[k][0]).T).T
        else:
            w = (x - comps[k][0]) / comps[k][1]
        near = (w * w).sum(axis=1) < w.shape[1] / 4
        central += int(near.sum())
        agree += int((plab[lab == k][near] == k).sum())
    print(f"{name}: {agree} of {central} central rows are labelled with the component they were drawn from")
    assert central >= 50 and agree == central


def test_empty_blocks_and_errors():
    """Two of lc_model_sample's LC_EINVAL cases cannot be reached here: a model without clusters and a Gauss-Wishart model
    with D > 1024 -- no learner returns the first and fitting refuses the second, so no model of either kind exists to
    hand over; lcp::sample checks both before it touches the context."""
    m, train = _model("gw_d5_dir")
    with capi.Context(0) as ctx:
        m.sample_context(ctx, [0])  # an empty context is fine
        assert ctx.dims()[:3] == (1, 5, 0) and ctx.get_sample_labels(0, 0, 0).size == 0
        m.sample_context(ctx, [0, 33, 0], groups=[0, 0, 0])
        assert ctx.get_rows(1, 0, 33).shape == (33, 5)
        ctx.set_data(np.zeros((4, 5)))
        with pytest.raises(ValueError, match="lc_model_sample"):
            ctx.get_sample_labels(0, 0, 4)
        m.sample_context(ctx, [8])
        held = ctx.get_rows(0, 0, 8)
        for counts, groups in (([], None), ([-1], None), ([4], [1]), ([4], [-1])):
            with pytest.raises(ValueError):
                m.sample_context(ctx, counts, groups)
        assert np.array_equal(ctx.get_rows(0, 0, 8), held)  # a refused call leaves the context as it was
        with pytest.raises(ValueError):
            ctx.get_sample_labels(0, 0, 9)
    with pytest.raises(ValueError, match="lc_model_sample"):
        train.get_sample_labels(0, 0, 1)  # an uploaded context
    # a freed model
    m2, _ = _fit_throwaway()
    handle = m2._h.value
    m2.close()
    with capi.Context(0) as ctx:
        nj = (C.c_int64 * 1)(4)
        assert capi.lib().lc_model_sample(C.c_void_p(handle), ctx._h, 1, nj, None, 0, 0) == capi.LC_EINVAL
        assert b"freed" in capi.lib().lc_last_error()


def _fit_throwaway():
    rng = np.random.default_rng(0)
    ctx = capi.Context(0)
    ctx.set_data(rng.normal(size=(20, 2)))
    ctx.set_qz(np.ones((20, 1)))
    _, _, m = ctx.vbem(capi.W_DIRICHLET, fixed_iters=2)
    return m, ctx
