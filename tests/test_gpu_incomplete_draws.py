"""Draws of the unknown values of rows with holes (lc_model_predict_incomplete_draws).

The reference is tests/incomplete_draws_ref.py: numpy / scipy on the model's posteriors by the direct route -- per (hole
pattern, component) the Cholesky factor of iW_aa, the Student-t marginal of the known columns, the expert M_k(x_a), the Schur
complement S_k, eta = nu' + Da and the scale c_k h_k S_k.  Never the device, never its route.  Whitened with the component its
label names, a draw has t(eta) coordinates and radius^2 / nb ~ F(nb, eta) whatever x_a and the pattern are, so the draws of
different rows pool per hole count.  Models are fitted on few rows (fixed-K VBEM on the device from the true labels), so that
eta is small.  Bars (tests/sample_ref.py, unchanged): KS p >= 1e-4, frequencies within 5 binomial standard errors;
tests/test_incomplete_draws_host.py shows on the CPU that numpy's own draws from the reference pass them at these sizes.
Seeds are fixed; none had to be changed."""
import functools

import numpy as np
import pytest
from scipy import stats

import incomplete_draws_ref as dr
import lc_oracle as o
import sample_ref as sr
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

HMAX = capi.HOLES_MAX
WK = {dr.STICK: capi.W_STICKBREAK, dr.DIRICHLET: capi.W_DIRICHLET}


@functools.lru_cache(maxsize=None)
def _model(name):
    """-> (model, training context): fitted once, shared by the tests and never changed"""
    wk, _, _, cp, _ = dr.MODELS[name]
    X, q, _ = dr.training(name)
    ctx = capi.Context(0)
    ctx.set_data(X)
    ctx.set_qz(q)
    _, _, m = ctx.vbem(WK[wk], fixed_iters=6, clusterprior=cp)
    return m, ctx


def _mixture_of(m, cp, group=0):
    _, K, D = m.dims()
    e, rest = capi.weights_predictive(m.kinds()[0], m.weights(group)[1])
    posts = [(p["nu"], p["beta"], p["mean"], p["iW"]) for p in (m.cluster(k) for k in range(K))]
    pr = o.GaussWish(cp, D)
    return dr.mixture(posts, (pr.nu, pr.beta, pr.m, pr.iW), e, rest)


@functools.lru_cache(maxsize=None)
def _mixture(name):
    """the reference of a model: its components (the prior one last) and weights"""
    return _mixture_of(_model(name)[0], dr.MODELS[name][3])


def _same_completion(a, b):
    for f in ("rows", "logp", "count", "cols"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.int64 if x.dtype == np.float64 else x.dtype),
                                                                             y.view(np.int64 if y.dtype == np.float64 else y.dtype)), f


def _structure(got, Xh, Kp, nd):
    N = Xh.shape[0]
    count = np.isnan(Xh).sum(axis=1)
    assert got.draws.shape == (N, nd, HMAX) and got.label.shape == (N, nd) and got.label.dtype == np.int32
    assert np.array_equal(got.count, count)
    assert np.all(np.isfinite(got.draws)) and np.all(np.isfinite(got.rows)) and np.all(np.isfinite(got.logp))
    beyond = np.arange(HMAX)[None, None, :] >= count[:, None, None]
    assert np.all(got.draws[np.broadcast_to(beyond, got.draws.shape)].view(np.int64) == 0)  # exactly +0.0
    assert np.all(got.label[count == 0] == -1)
    lab = got.label[count > 0]
    assert lab.size == 0 or (lab.min() >= 0 and lab.max() < Kp)


def _exact_labels(got, Xh, mix, seed, nd, what, block=0):
    """u of every (row, draw) from the numpy Philox, the choice from numpy's r_k(x_a) of the direct reference"""
    rows = np.flatnonzero(np.isnan(Xh).any(axis=1))
    r = mix.responsibilities(Xh)[rows]
    left = 0
    for i in range(nd):
        want, far = sr.choose(sr.choice_u(seed, block, rows, i), r)
        assert np.array_equal(got.label[rows[far], i], want[far]), (what, i)
        left += int((~far).sum())
    print(f"{what}: {left} of {rows.size * nd} labels left out (within 1e-9 of a boundary; share {left / max(rows.size * nd, 1):.2e})")
    assert left <= 1e-3 * rows.size * nd
    return r


def _pooled(mix, Xh, draws, label, what, tally):
    parts = mix.whitened_by_nb(Xh, draws, label)
    for nb in sorted(parts):
        tally.add(sr.ks_whitened_pooled(parts[nb]), f"{what}, {nb} holes ({len(parts[nb])} values of eta, "
                                                   f"{sum(p[0].shape[0] for p in parts[nb])} draws)")


@functools.lru_cache(maxsize=None)
def _rows300():
    """300 rows (four full waves and one of 44), a third complete, D = 23, 1 ... 8 holes"""
    rng = np.random.default_rng(3)
    Xh = dr.punch(rng, dr.rows("d23_stick", rng, 300, 0.1))
    Xh.setflags(write=False)
    return Xh


@functools.lru_cache(maxsize=None)
def _draws300():
    return _model("d23_stick")[0].predict_incomplete(_rows300(), draws=7, seed=1)


def test_same_bits_as_the_call_without_draws():
    m, _ = _model("d23_stick")
    Xh = _rows300()
    count = np.isnan(Xh).sum(axis=1)
    assert set(np.unique(count)) == set(range(9)) and 0.2 < np.mean(count == 0) < 0.45
    a = _draws300()
    assert isinstance(a, capi.CompletionDraws) and a.var is None
    _same_completion(a, m.predict_incomplete(Xh))
    b = m.predict_incomplete(Xh, draws=7, seed=1)
    assert np.array_equal(a.draws, b.draws) and np.array_equal(a.label, b.label)
    _same_completion(a, b)


def test_structure():
    m, _ = _model("d23_stick")
    Xh = _rows300()
    _structure(_draws300(), Xh, _mixture("d23_stick").Kp, 7)
    holed = np.isnan(Xh).any(axis=1)
    assert np.all(_draws300().draws[~holed] == 0.0)
    # a context with no NaN at all
    X = dr.rows("d23_stick", np.random.default_rng(4), 100)
    full = m.predict_incomplete(X, draws=3, seed=1)
    _same_completion(full, m.predict_incomplete(X))
    assert np.all(full.draws == 0.0) and np.all(full.label == -1) and np.all(full.count == 0)


def test_what_a_draw_depends_on():
    m, _ = _model("d23_stick")
    Xh = np.array(_rows300())
    a = _draws300()
    holed = np.isnan(Xh).any(axis=1)
    # ndraws: the first 3 of 7
    d = m.predict_incomplete(Xh, draws=3, seed=1)
    assert np.array_equal(d.draws, a.draws[:, :3]) and np.array_equal(d.label, a.label[:, :3])
    # N: the first n rows of 2n
    e = m.predict_incomplete(np.vstack([Xh, Xh[::-1]]), draws=7, seed=1)
    assert np.array_equal(e.draws[:300], a.draws) and np.array_equal(e.label[:300], a.label)
    # a row's neighbours: every seventh row stays where it is, all others are replaced by the rows in reverse order -- other
    # neighbours, and other rows with holes ahead of it in its wave's queue
    keep = np.arange(0, 300, 7)
    moved = Xh[::-1].copy()
    moved[keep] = Xh[keep]
    assert not np.array_equal(np.isnan(moved), np.isnan(Xh))
    f = m.predict_incomplete(moved, draws=7, seed=1)
    assert np.array_equal(f.draws[keep], a.draws[keep]) and np.array_equal(f.label[keep], a.label[keep])
    assert np.array_equal(f.rows[keep], a.rows[keep]) and np.array_equal(f.logp[keep], a.logp[keep])
    # blocks: block 0 does not depend on J; block 1 has its own counters
    g = m.predict_incomplete([Xh, Xh], draws=7, seed=1)
    assert np.array_equal(g[0].draws, a.draws) and np.array_equal(g[0].label, a.label)
    assert not np.any(np.all(g[1].draws[holed].reshape(holed.sum(), -1) == a.draws[holed].reshape(holed.sum(), -1), axis=1))
    rows = np.flatnonzero(holed)
    want, far = sr.choose(sr.choice_u(1, 1, rows, 2), _mixture("d23_stick").responsibilities(Xh)[rows])
    assert np.array_equal(g[1].label[rows[far], 2], want[far])
    # another seed changes every row with holes
    c = m.predict_incomplete(Xh, draws=7, seed=2)
    assert not np.any(np.all(a.draws[holed].reshape(holed.sum(), -1) == c.draws[holed].reshape(holed.sum(), -1), axis=1))
    assert np.all(c.draws[~holed] == 0.0)


@pytest.mark.parametrize("case", sorted(dr.CASES))
def test_shapes_pooled_over_rows(case):
    """every case crosses one loop of the kernels (tests/incomplete_draws_ref.py, CASES).  Exact labels from the documented
    counters and numpy's r_k(x_a); label frequencies; every draw whitened with the component its label names, pooled over rows
    and patterns per hole count"""
    name, n, nd, _, nbs = dr.CASES[case]
    m, _ = _model(name)
    mix = _mixture(name)
    Xh = dr.case_rows(case)
    holed = np.isnan(Xh).any(axis=1)
    got = m.predict_incomplete(Xh, draws=nd, seed=dr.CASE_SEED)
    _same_completion(got, m.predict_incomplete(Xh))
    _structure(got, Xh, mix.Kp, nd)
    r = _exact_labels(got, Xh, mix, dr.CASE_SEED, nd, case)
    sr.check_frequencies(got.label[holed].reshape(-1), r.mean(axis=0), case)
    _pooled(mix, Xh, got.draws, got.label, case, sr.Tally())
    if case == "d23_prior":
        assert np.sum(got.label == mix.Kp - 1) >= 100 and mix.posts[-1][0] + 1 - 23 == 1.0  # the prior component: nu' = 1
    if case == "d64_kp35_m64":
        assert mix.Kp == 35 and nd == 64
    if case == "d5_kp70":
        assert mix.Kp == 70 and got.label.max() >= 64  # the second chunk of clusters is drawn from
    if case == "d200_nb8_m1":
        assert np.all(got.count[holed] == 8)


def test_exact_structure_of_a_draw():
    """Without emulating the gamma draw: with z regenerated from the documented counters and the reference's L, M_k, cqnu_k and
    h_k, L^T (x_b - M_k) / sqrt(cqnu_k h_k) over z is ONE scalar 1 / sqrt(G) in every hole of a draw (|z_i| < 1e-3 left out),
    to 1e-9 relative -- a wrong slot order, pair assignment, a transposed solve or another component's tables break it -- and
    the recovered G, pooled per (component, nb), is Gamma(e_k(nb))"""
    case = "d23_prior"
    name, n, nd, _, _ = dr.CASES[case]
    m, _ = _model(name)
    mix = _mixture(name)
    Xh = dr.case_rows(case)
    got = m.predict_incomplete(Xh, draws=nd, seed=dr.CASE_SEED)
    worst, G = 0.0, {}
    for c, pat, rows, di, Xa in mix.each(Xh, got.label):
        nb = len(pat)
        if nb < 2:
            continue
        z = dr.normals(dr.CASE_SEED, 0, rows, di, (nb + 1) // 2)[:, :nb]
        ratio = c.inv_sqrt_g(Xa, got.draws[rows, di, :nb], z)
        ratio[np.abs(z) < 1e-3] = np.nan
        ok = np.sum(~np.isnan(ratio), axis=1) >= 2
        spread = np.nanmax(ratio[ok], axis=1) / np.nanmin(ratio[ok], axis=1) - 1
        assert np.all(np.nanmin(ratio[ok], axis=1) > 0)
        worst = max(worst, float(np.max(spread, initial=0.0)))
        G.setdefault((c.eta, nb), []).append(1 / np.nanmean(ratio[ok], axis=1) ** 2)
    print(f"largest relative spread of 1 / sqrt(G) over the holes of a draw: {worst:.3e} (bar 1e-9)")
    assert worst <= 1e-9
    tally, tested = sr.Tally(), 0
    for (eta, nb), g in sorted(G.items()):
        g = np.concatenate(g)
        if g.size >= 100:
            tested += 1
            tally.add([stats.kstest(g, stats.gamma(eta / 2).cdf)], f"recovered G, eta {eta:g}, {nb} holes, {g.size} draws")
    assert tested >= 8
    print(f"recovered G: {tally.n} KS tests, largest statistic {tally.stat:.3e}, smallest p {tally.p:.3e}")


def test_distribution_four_rows_50000_copies():
    """4 distinct (pattern, x_a) rows with 1, 2, 3 and 4 holes at D = 5, 50 000 copies each, 4 draws per copy"""
    m, _ = _model("d5_dir")
    mix = _mixture("d5_dir")
    X4 = dr.four_rows(mix, "d5_dir")
    copies, nd = 50_000, 4
    Xh = np.repeat(X4, copies, axis=0)
    got = m.predict_incomplete(Xh, draws=nd, seed=77)
    _same_completion(got, m.predict_incomplete(Xh))
    _structure(got, Xh, mix.Kp, nd)
    r = mix.responsibilities(X4)
    var = m.predict_incomplete(X4, variance=True)  # (Dirichlet weights, nu - 1 - nb > 0 in every cluster: it exists)
    tally, multimodal = sr.Tally(), 0
    for i in range(4):
        rows = slice(i * copies, (i + 1) * copies)
        pat = np.flatnonzero(np.isnan(X4[i]))
        lab, x = got.label[rows].reshape(-1), got.draws[rows].reshape(-1, HMAX)[:, : pat.size]
        sr.check_frequencies(lab, r[i], f"row {i}")
        tested = 0
        for k in range(mix.Kp):
            sel = lab == k
            if sel.sum() < 50_000:
                continue
            tested += 1
            c = mix.comp(k, pat)
            wh = c.whiten(np.repeat(X4[i:i + 1, c.a], sel.sum(), axis=0), x[sel])
            tally.add(sr.ks_whitened(wh, c.eta), f"row {i} ({pat.size} holes) component {k} (eta {c.eta:g}, {sel.sum()} draws)")
        assert tested >= 1
        multimodal += tested >= 2
        mean, bound = var.rows[i, pat], 5 * np.sqrt(var.var[i, : pat.size] / x.shape[0])
        print(f"row {i}: |average - mean| / bound = {np.max(np.abs(x.mean(axis=0) - mean) / bound):.3f} (bar 1)")
        assert np.all(np.abs(x.mean(axis=0) - mean) <= bound)
    assert multimodal >= 1  # (not vacuous: some row draws from two experts)
    print(f"incomplete draws: {tally.n} KS tests, largest statistic {tally.stat:.3e}, smallest p {tally.p:.3e}")


def test_one_pattern_in_every_row_against_the_fixed_split_call():
    """[3, 17] missing in every row: the labels are those of predict_conditional(..., draws=m) with the same seed -- the same
    uniforms against the same r_k, up to rounding -- and the draws of both calls pass the same whitened KS.  The draws are NOT
    the same bits: the fixed-split call multiplies z by the Cholesky factor of S_k, this one solves with the transposed factor
    of (P_k)_bb -- two factors of the same scale matrix."""
    m, _ = _model("d23_stick")
    mix = _mixture("d23_stick")
    n, nd, seed, miss = 3000, 5, (5 << 32) + 9, [3, 17]
    X = dr.rows("d23_stick", np.random.default_rng(8), n, 0.1)
    Xh = X.copy()
    Xh[:, miss] = np.nan
    given = [c for c in range(23) if c not in miss]
    a = m.predict_incomplete(Xh, draws=nd, seed=seed)
    b = m.predict_conditional(X[:, given], given, miss, draws=nd, seed=seed)
    r = mix.responsibilities(Xh)
    left = 0
    for i in range(nd):
        far = sr.choose(sr.choice_u(seed, 0, np.arange(n), i), r)[1]
        assert np.array_equal(a.label[far, i], b.label[far, i])
        left += int((~far).sum())
    print(f"{left} of {n * nd} labels left out (within 1e-9 of a boundary)")
    assert left <= 1e-3 * n * nd
    assert not np.array_equal(a.draws[:, :, :2], b.draws)
    bd = np.zeros_like(a.draws)
    bd[:, :, :2] = b.draws
    tally = sr.Tally()
    _pooled(mix, Xh, a.draws, a.label, "rows with holes", tally)
    _pooled(mix, Xh, bd, b.label, "fixed split", tally)


def test_two_blocks_with_different_groups():
    rng = np.random.default_rng(8)
    D, K, sizes = 3, 2, ([9, 2], [3, 8])
    cen = dr.centres(D, K)
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
    mixes = [_mixture_of(m, 1.0, j) for j in range(2)]
    # between the clusters, where by the reference learned group 0 gives both a share: the weights decide
    line = np.array([(1 - t) * cen[0] + t * cen[1] for t in np.linspace(0.0, 1.0, 2001)])
    line[:, 1:] = np.nan
    at = line[np.argmax(mixes[0].responsibilities(line).min(axis=1))]
    xh = np.repeat(at[None, :], 40_000, axis=0)
    got = m.predict_incomplete([xh, xh], groups=[1, 0], draws=2, seed=4)
    for b, j in ((0, 1), (1, 0)):
        sr.check_frequencies(got[b].label.reshape(-1), mixes[j].responsibilities(at[None, :])[0], f"block {b} with learned group {j}")
        _pooled(mixes[j], xh, got[b].draws, got[b].label, f"block {b}", sr.Tally())
    assert abs(np.mean(got[0].label) - np.mean(got[1].label)) > 0.1  # (not vacuous: the groups mix differently)


def test_device_level_calls_and_errors():
    m, _ = _model("d5_dir")
    rng = np.random.default_rng(1)
    Xh = dr.punch(rng, dr.rows("d5_dir", rng, 100), npat=12)
    L = capi.lib()
    i32 = capi.C.POINTER(capi.C.c_int32)
    with capi.Context(0) as ctx:
        ctx.set_data(Xh)
        assert ctx.completed_draws() == 0
        assert L.lc_ctx_get_completed_draws(ctx._h, 0, 0, 10, None, None) == capi.LC_EINVAL  # no prediction
        m.predict_incomplete_context(ctx, draws=5, seed=3)
        assert ctx.completed_draws() == 5
        whole = m.predict_incomplete(Xh, draws=5, seed=3)
        part = ctx.get_completed(0, 10, 50, draws=True)
        assert np.array_equal(part.draws, whole.draws[10:60]) and np.array_equal(part.label, whole.label[10:60])
        assert np.array_equal(part.rows, whole.rows[10:60]) and part.var is None
        with pytest.raises(ValueError):
            ctx.get_completed(0, 0, 10, draws=4)  # not the count of this prediction
        with pytest.raises(ValueError):
            ctx.get_completed(0, 0, 101, draws=True)  # out of bounds
        assert L.lc_ctx_get_completed_draws(ctx._h, 1, 0, 1, None, None) == capi.LC_EINVAL
        with pytest.raises(ValueError):
            ctx.get_completed(0, 0, 10, variance=True)  # this prediction has draws, no variance
        # NULL outputs: either, or both (the checks only)
        dbuf, lbuf = np.zeros((50, 5, HMAX)), np.zeros((50, 5), dtype=np.int32)
        assert L.lc_ctx_get_completed_draws(ctx._h, 0, 10, 50, capi.dptr(dbuf), None) == 0
        assert L.lc_ctx_get_completed_draws(ctx._h, 0, 10, 50, None, lbuf.ctypes.data_as(i32)) == 0
        assert L.lc_ctx_get_completed_draws(ctx._h, 0, 10, 50, None, None) == 0
        assert np.array_equal(dbuf, whole.draws[10:60]) and np.array_equal(lbuf, whole.label[10:60])
        assert L.lc_ctx_completed_draws(ctx._h, None) == 0
        # ndraws 0 and 65: LC_EINVAL, and no prediction is left
        for bad in (0, 65):
            ctx.set_data(Xh)
            m.predict_incomplete_context(ctx, draws=2)
            assert L.lc_model_predict_incomplete_draws(m._h, ctx._h, None, bad, 0) == capi.LC_EINVAL
            assert ctx.completed_draws() == 0
            with pytest.raises(ValueError):
                ctx.get_completed(0, 0, 10)
            with pytest.raises(ValueError):
                m.predict_incomplete_context(ctx, draws=bad)
        # after a plain or a variance call: no draws
        for variance in (False, True):
            ctx.set_data(Xh)
            m.predict_incomplete_context(ctx, variance=variance)
            assert ctx.completed_draws() == 0
            assert L.lc_ctx_get_completed_draws(ctx._h, 0, 0, 10, None, None) == capi.LC_EINVAL
            with pytest.raises(ValueError):
                ctx.get_completed(0, 0, 10, draws=True)
        # predict_clear drops them
        ctx.set_data(Xh)
        m.predict_incomplete_context(ctx, draws=2)
        m.predict_context(ctx)
        assert ctx.completed_draws() == 0
    # a row with 9 NaNs: LC_EINVAL with the NaNs intact and no prediction left
    rng = np.random.default_rng(2)
    X23 = dr.punch(rng, dr.rows("d23_stick", rng, 40), npat=8)
    X23[17, :] = 1.0
    X23[17, 2:11] = np.nan
    m23, _ = _model("d23_stick")
    with capi.Context(0) as ctx:
        ctx.set_data(X23)
        assert L.lc_model_predict_incomplete_draws(m23._h, ctx._h, None, 3, 0) == capi.LC_EINVAL
        assert b"row 17" in L.lc_last_error()
        assert ctx.completed_draws() == 0
        back = np.zeros_like(X23)
        capi.check(L.lc_ctx_get_rows(ctx._h, 0, 0, 40, capi.dptr(back)))
        assert np.array_equal(np.isnan(back), np.isnan(X23))
        with pytest.raises(ValueError):
            ctx.get_completed(0, 0, 10)
    with pytest.raises(ValueError):
        m.predict_incomplete(Xh, variance=True, draws=2)
    with pytest.raises(ValueError):
        m.predict_incomplete(Xh, draws=0)
    with pytest.raises(ValueError):
        m.predict_incomplete(Xh, draws=65)


def test_impute_takes_the_nans_of_x():
    m, _ = _model("d5_dir")
    rng = np.random.default_rng(6)
    X = dr.rows("d5_dir", rng, 200)
    Xnan = dr.punch(rng, X, npat=12)
    holes = np.isnan(Xnan)
    ref = m.predict_incomplete(Xnan, draws=5, seed=1)
    copies = m.impute(Xnan, draws=5, seed=1)
    assert isinstance(copies, list) and len(copies) == 5
    for i, c in enumerate(copies):
        assert c.shape == X.shape and np.array_equal(c[~holes], X[~holes]) and np.all(np.isfinite(c))
        for n in range(200):
            assert np.array_equal(c[n, ref.cols[n, : ref.count[n]]], ref.draws[n, i, : ref.count[n]])
        assert np.array_equal(c[~holes.any(axis=1)], copies[0][~holes.any(axis=1)])  # complete rows: identical in all copies
    assert not np.array_equal(copies[0], copies[1])
    filled = m.impute(Xnan)
    assert np.array_equal(filled, m.predict_incomplete(Xnan).rows) and np.array_equal(filled, ref.rows)
    blocks = m.impute([Xnan, Xnan[:50]], draws=2, seed=1)
    assert len(blocks) == 2 and len(blocks[0]) == 2 and blocks[1][0].shape == (50, 5)
    assert np.array_equal(blocks[0][0], copies[0])
    with pytest.raises(ValueError):
        m.impute(Xnan, return_var=True)
    # with `missing`, impute behaves as before
    one = m.impute(X, [1, 4], draws=2, seed=9)
    two = m.predict_conditional(X[:, [0, 2, 3]], [0, 2, 3], [1, 4], draws=2, seed=9)
    assert np.array_equal(one[1][:, [1, 4]], two.draws[:, 1, :])
