"""Host side of the samplers: the Schur complement behind the conditional draws (lc_gw_conditional_cov), the
numpy Philox the GPU tests reproduce the device with, and the statistical bars of those tests applied to a reference
sampler on numpy's own generators -- a correct sampler passes them at the sample sizes the GPU tests use."""
import numpy as np
import pytest

import sample_ref as sr
from libcluster_amd import capi

NEW_SYMBOLS = ["lc_model_sample", "lc_ctx_get_sample_labels", "lc_model_predict_conditional_draws",
               "lc_ctx_get_conditional_draws", "lc_ctx_conditional_draws", "lc_gw_conditional_cov"]


def _posterior(rng, D):
    A = rng.normal(size=(D, D + 5))
    iW = A @ A.T + 0.5 * np.eye(D)
    return D + 2.5, 1.7, rng.normal(size=D), iW


def _splits(rng, D):
    """(given, target): a contiguous split, a permuted full split, and a permuted split that leaves columns out"""
    p = rng.permutation(D)
    h = max(1, D // 2)
    out = [(list(range(h)), list(range(h, D))), ([int(c) for c in p[:h]], [int(c) for c in p[h:]])]
    if D >= 4:
        out.append(([int(c) for c in p[: D // 3]], [int(c) for c in p[D // 3 + 1:]]))
    return out


@pytest.mark.parametrize("D", [3, 5, 23])
def test_conditional_cov_against_numpy(lib, D):
    rng = np.random.default_rng(160 + D)
    nu, beta, m, iW = _posterior(rng, D)
    for given, target in _splits(rng, D):
        S, L = capi.gw_conditional_cov(nu, beta, iW, given, target)
        Waa, Wab, Wbb = iW[np.ix_(given, given)], iW[np.ix_(given, target)], iW[np.ix_(target, target)]
        want = Wbb - Wab.T @ np.linalg.solve(Waa, Wab)
        bar = 1e-12 * np.linalg.norm(iW)
        print(f"D = {D}, Da = {len(given)}: max |S - ref| = {np.max(np.abs(S - want)):.3e}, "
              f"max |L - chol| = {np.max(np.abs(L - np.linalg.cholesky(want))):.3e} (bar {bar:.3e})")
        assert np.max(np.abs(S - want)) <= bar
        assert np.max(np.abs(L - np.linalg.cholesky(want))) <= bar
        assert np.array_equal(S, S.T) and np.array_equal(L, np.tril(L))
        assert np.max(np.abs(L @ L.T - S)) <= bar
        # its diagonal is the table of the conditional variance
        Sd, _ = capi.gw_conditional_var(nu, beta, iW, given, target)
        np.testing.assert_allclose(np.diag(S), Sd, rtol=1e-13, atol=0)
    # target None: the columns that are not given, ascending
    S, _ = capi.gw_conditional_cov(nu, beta, iW, [0])
    assert S.shape == (D - 1, D - 1)


def test_conditional_cov_errors(lib):
    rng = np.random.default_rng(5)
    nu, beta, m, iW = _posterior(rng, 4)
    with pytest.raises(ValueError):
        capi.gw_conditional_cov(nu, beta, iW, [0, 0], [1])
    with pytest.raises(ValueError):
        capi.gw_conditional_cov(nu, beta, iW, [0, 1], [1, 2])
    bad = iW.copy()
    bad[3, 3] = bad[3, 0] * bad[3, 0] / bad[0, 0] - 1.0  # S = iW_33 - iW_30^2 / iW_00 = -1
    with pytest.raises(capi.DomainError):
        capi.gw_conditional_cov(nu, beta, bad, [0], [3])
    # ... whichever output is asked for: S alone, L alone, neither
    import ctypes as C

    gv, tv = (C.c_int * 1)(0), (C.c_int * 1)(3)
    S = np.zeros((1, 1))
    for s_out, l_out in ((S, None), (None, S), (None, None)):
        rc = capi.lib().lc_gw_conditional_cov(4, nu, beta, capi.dptr(bad), gv, 1, tv, 1, capi.dptr(s_out), capi.dptr(l_out))
        assert rc == capi.LC_EDOMAIN
        assert capi.lib().lc_gw_conditional_cov(4, nu, beta, capi.dptr(iW), gv, 1, tv, 1, capi.dptr(s_out), capi.dptr(l_out)) == capi.LC_OK


def test_philox_known_answers():
    z = sr.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(v) for v in z] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    o = sr.philox4x32_10(f, f, f, f, f, f)
    assert [int(v) for v in o] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # vectorised = element by element
    c0 = np.arange(5, dtype=np.uint64)
    v = sr.philox4x32_10(c0, 7, 3, 0x10, 11, 13)
    for i in range(5):
        assert [int(x[i]) for x in v] == [int(x) for x in sr.philox4x32_10(i, 7, 3, 0x10, 11, 13)]
    u = sr.u01(np.array([0, f], dtype=np.uint64), np.array([0, f], dtype=np.uint64))
    assert 0.0 < u[0] < u[1] <= 1.0  # (the largest value rounds to 1: log and the inverse CDFs take it)


def test_choose_boundaries():
    w = np.array([0.25, 0.0, 0.5, 0.25, 0.0])
    k, far = sr.choose(np.array([0.1, 0.25, 0.3, 0.74999, 0.75, 0.999999]), w)
    assert list(k) == [0, 2, 2, 2, 3, 3] and list(far) == [True, False, True, True, False, True]
    k, _ = sr.choose(np.array([0.9999999]), np.array([0.5, 0.4999, 0.0]))  # the sum is short: the last with weight
    assert list(k) == [1]


def test_bars_pass_for_a_correct_sampler():
    """numpy's generators through the formulas of the header, at the sample sizes of the GPU tests: the bars of
    sample_ref (KS p >= 1e-4, frequencies within 5 standard errors) are passable."""
    rng = np.random.default_rng(2024)
    tally = sr.Tally()
    n = 200_000
    w = np.array([0.45, 0.27, 0.25, 0.03])
    lab = rng.choice(4, n, p=w)
    sr.check_frequencies(lab, w, "reference labels")
    for D, nup in ((2, 1.0), (5, 3.0), (23, 6.0)):
        nu, beta = nup + D - 1, 9.0
        A = rng.normal(size=(D, D + 3))
        loc, Scale, dof = sr.gw_student(nu, beta, rng.normal(size=D), A @ A.T)
        assert dof == nup
        x = sr.draw_student(rng, 60_000, loc, Scale, dof)
        tally.add(sr.ks_student(x, loc, Scale, dof), f"reference Gauss-Wishart D = {D}, nu' = {nup}")
    # the conditional: eta = nu' + Da, scale c (1 + s d^2) S
    D, given, target = 5, [3, 0], [1, 2, 4]
    A = rng.normal(size=(D, D + 3))
    loc, Scale, eta = sr.gw_conditional_student(7.0, 4.0, rng.normal(size=D), A @ A.T, given, target, rng.normal(size=2))
    assert eta == 7.0 + 1 - D + 2
    x = sr.draw_student(rng, 50_000, loc, Scale, eta)
    tally.add(sr.ks_student(x, loc, Scale, eta), "reference conditional 2 | 3")
    loc, scale, dof = sr.ng_student(2.5, 4.0, rng.normal(size=4), rng.uniform(0.5, 2.0, 4))
    x = sr.draw_student_diag(rng, 60_000, loc, scale, dof)
    tally.add(sr.ks_student_diag(x, loc, scale, dof), "reference NormGamma")
    shape, scale = sr.eg_lomax(6.0, rng.uniform(0.05, 0.5, 4))
    x = sr.draw_lomax(rng, 60_000, shape, scale)
    assert np.all(x >= 0)
    tally.add(sr.ks_lomax(x, shape, scale), "reference ExpGamma")
    print(f"{tally.n} KS tests: largest statistic {tally.stat:.3e}, smallest p {tally.p:.3e}")
    # ... and the bars notice a wrong sampler: one degree of freedom too many, a scale 3 % off
    loc, Scale, dof = np.zeros(2), np.eye(2), 3.0
    wrong = sr.draw_student(rng, 200_000, loc, Scale, dof + 1)
    assert min(r.pvalue for r in sr.ks_student(wrong, loc, Scale, dof)) < 1e-50
    wrong = 1.03 * sr.draw_student(rng, 200_000, loc, Scale, dof)
    assert min(r.pvalue for r in sr.ks_student(wrong, loc, Scale, dof)) < 1e-20


def test_new_symbols_declared_and_exported(lib):
    declared = capi.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
    import libcluster_amd

    assert libcluster_amd.Sample is capi.Sample and libcluster_amd.ConditionalDraws is capi.ConditionalDraws
    assert capi.DRAWS_MAX == 64
