"""The reference of the draws for rows with holes (tests/incomplete_draws_ref.py) against itself, on the CPU:

* the route of the device (P = nu iW^-1, H = P_bb, u = (P y)_b) gives the scale matrix, the expert and h_k of the direct
  route (the Cholesky factor of iW_aa, the Schur complement) to 1e-10 relative;
* the bars of tests/test_gpu_incomplete_draws.py are passable: draws that numpy's own generators make from the reference
  distribution, at the sample sizes of the GPU tests, pass the identical statistics -- sample_ref's P_BAR and
  check_frequencies, unchanged;
* the share of labels within 1e-9 of a boundary of the reference's own running sums stays inside the cap of 1e-3;
* a draw assembled as the header documents it (x_b = M_k + sqrt(cqnu h / G) L^-T z) shows 1 / sqrt(G) in every hole through
  inv_sqrt_g(), and is a draw of the reference distribution.
"""
import numpy as np
import pytest
from scipy import stats

import incomplete_draws_ref as dr
import incomplete_ref as ref
import sample_ref as sr


@pytest.mark.parametrize("D", [2, 5, 23])
def test_route_identity(D):
    rng = np.random.default_rng(40 + D)
    worst = 0.0
    for nb in range(1, min(dr.HOLES_MAX, D - 1) + 1):
        for _ in range(3):
            nu, beta, m, iW = ref.random_posterior(rng, D)
            b = np.sort(rng.choice(D, nb, replace=False))
            x = m + rng.normal(size=D) * 3.0
            c = dr.HoleComponent(nu, beta, m, iW, b)
            xa = x[c.a][None, :]
            for fill in (m[b], rng.normal(size=nb) * 10.0):  # whatever stands in the holes
                xf = x.copy()
                xf[b] = fill
                S, M, h = dr.route(nu, beta, m, iW, xf, b)
                errs = (np.max(np.abs(S - c.S)) / np.max(np.abs(c.S)),
                        np.max(np.abs(M - c.location(xa)[0])) / np.max(np.abs(c.location(xa)[0])),
                        abs(h - c.h(xa)[0]) / c.h(xa)[0])
                worst = max(worst, *errs)
                assert max(errs) <= 1e-10, (D, nb, errs)
    print(f"D = {D}: largest relative gap between the routes {worst:.3e} (bar 1e-10)")


def _pooled(mix, Xh, draws, label, what, tally):
    parts = mix.whitened_by_nb(Xh, draws, label)
    for nb in sorted(parts):
        tally.add(sr.ks_whitened_pooled(parts[nb]), f"{what}, {nb} holes ({len(parts[nb])} values of eta, "
                                                   f"{sum(p[0].shape[0] for p in parts[nb])} draws)")


@pytest.mark.parametrize("case", sorted(dr.CASES))
def test_bars_are_passable_shapes(case):
    """the statistics of test_shapes_pooled_over_rows on numpy's draws from the reference, at its sizes"""
    name, n, nd, _, _ = dr.CASES[case]
    mix = dr.host_mixture(name)
    Xh = dr.case_rows(case)
    holed = np.isnan(Xh).any(axis=1)
    assert 0.2 < 1 - holed.mean() < 0.45  # a third complete
    draws, label = mix.draw(np.random.default_rng(5), Xh, nd)
    r = mix.responsibilities(Xh)
    sr.check_frequencies(label[holed].reshape(-1), r[holed].mean(axis=0), case)
    _pooled(mix, Xh, draws, label, case, sr.Tally())
    # the cap on labels left out: u of the documented counters against the reference's own running sums
    rows = np.flatnonzero(holed)
    left = sum(int((~sr.choose(sr.choice_u(dr.CASE_SEED, 0, rows, i), r[rows])[1]).sum()) for i in range(nd))
    print(f"{case}: {left} of {rows.size * nd} labels within 1e-9 of a boundary")
    assert left <= 1e-3 * rows.size * nd


def test_bars_are_passable_distribution():
    """the statistics of test_distribution_four_rows_50000_copies on numpy's draws from the reference"""
    mix = dr.host_mixture("d5_dir")
    X4 = dr.four_rows(mix, "d5_dir")
    copies, nd = 50_000, 4
    Xh = np.repeat(X4, copies, axis=0)
    draws, label = mix.draw(np.random.default_rng(6), Xh, nd)
    r = mix.responsibilities(X4)
    tally, multimodal = sr.Tally(), 0
    for i in range(4):
        rows = slice(i * copies, (i + 1) * copies)
        pat = np.flatnonzero(np.isnan(X4[i]))
        lab, x = label[rows].reshape(-1), draws[rows].reshape(-1, dr.HOLES_MAX)[:, : pat.size]
        sr.check_frequencies(lab, r[i], f"row {i}")
        tested, mean, second = 0, 0.0, 0.0
        for k in range(mix.Kp):
            c = mix.comp(k, pat)
            xa = X4[i, c.a][None, :]
            M = c.location(xa)[0]
            mean = mean + r[i, k] * M
            second = second + r[i, k] * (c.eta / (c.eta - 2) * c.factor(xa)[0] * np.diag(c.S) + M * M)
            sel = lab == k
            if sel.sum() < 50_000:
                continue
            tested += 1
            tally.add(sr.ks_whitened(c.whiten(np.repeat(xa, sel.sum(), axis=0), x[sel]), c.eta), f"row {i} component {k}")
        assert tested >= 1
        multimodal += tested >= 2
        bound = 5 * np.sqrt((second - mean * mean) / x.shape[0])
        assert np.all(np.abs(x.mean(axis=0) - mean) <= bound)
    assert multimodal >= 1


def test_documented_draw_shows_one_over_sqrt_g_and_is_a_reference_draw():
    mix = dr.host_mixture("d23_stick")
    rng = np.random.default_rng(7)
    X = dr.rows("d23_stick", rng, 1)
    n = 60_000
    for pat, k in (([3, 17], 1), ([0, 4, 5, 11, 22], mix.Kp - 1)):  # (the last: the prior component, nu' = 1)
        c = mix.comp(k, pat)
        Xa = np.repeat(X[:, c.a], n, axis=0)
        z = dr.normals(9, 0, np.arange(n), 2, (len(pat) + 1) // 2)[:, : len(pat)]
        assert sr.ks_whitened(z, 1e9)[0].pvalue >= sr.P_BAR  # (the counters give normals)
        G = rng.gamma(c.eta / 2, size=n)
        x = c.location(Xa) + np.sqrt(c.cqnu * c.h(Xa) / G)[:, None] * np.linalg.solve(c.L.T, z.T).T
        ratio = c.inv_sqrt_g(Xa, x, z)
        ok = np.abs(z) >= 1e-3
        want = np.broadcast_to((1 / np.sqrt(G))[:, None], ratio.shape)
        assert np.max(np.abs(ratio[ok] / want[ok] - 1)) <= 1e-9
        sr.Tally().add([stats.kstest(1 / ratio[:, 0] ** 2, stats.gamma(c.eta / 2).cdf)], f"recovered G, {len(pat)} holes")
        sr.Tally().add(sr.ks_whitened(c.whiten(Xa, x), c.eta), f"documented draw, {len(pat)} holes, eta {c.eta:g}")
