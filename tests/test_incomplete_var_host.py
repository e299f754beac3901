"""Predictive variance of filled values, the host arithmetic: lc_gw_precision_var gives the table g(nb) the
device pass uses, and the route that pass takes -- emulated in numpy -- gives what the direct per-row Schur-complement
reference gives.  No GPU."""
import numpy as np
import pytest

import incomplete_ref as ref
import incomplete_var_ref as vref
from libcluster_amd import capi


@pytest.mark.parametrize("D,nu", [(1, 3.5), (2, 2.25), (5, 4.5), (5, 6.0), (5, 40.0), (23, 97.0)])
def test_table_against_numpy(lib, D, nu):
    beta = 1.0 + nu
    g = capi.gw_precision_var(nu, beta, D)
    want = vref.g_table(nu, beta, D)
    assert g.shape == (ref.HOLES_MAX + 1,)
    nb = np.arange(ref.HOLES_MAX + 1)
    exists = (nb < D) & (nu - 1 - nb > 0)
    assert np.array_equal(np.isnan(g), ~exists) and np.array_equal(np.isnan(want), ~exists)
    np.testing.assert_allclose(g[exists], (1 + beta) / (beta * (nu - 1 - nb[exists])), rtol=1e-13, atol=0)
    np.testing.assert_allclose(g[exists], want[exists], rtol=1e-13, atol=0)
    # DESIGN 4.14.1's g = (1 + beta) / (beta (nu' + ngiven - 2)): with all D columns given that is g[0] ...
    nup = nu + 1 - D
    np.testing.assert_allclose(g[0], (1 + beta) / (beta * (nup + D - 2)), rtol=1e-13, atol=0)
    if D >= 2 and exists[1]:  # ... and with D - 1 given, as lc_gw_conditional_var states it, g[1]
        iW = ref.random_posterior(np.random.default_rng(D), D)[3]
        np.testing.assert_allclose(g[1], capi.gw_conditional_var(nu, beta, iW, list(range(D - 1)))[1], rtol=1e-13, atol=0)


def _raw(D, nu, beta, g):
    rc = capi.lib().lc_gw_precision_var(D, nu, beta, capi.dptr(g))
    return rc, capi.lib().lc_last_error().decode()


def test_error_cases_are_einval(lib):
    g = np.zeros(ref.HOLES_MAX + 1)
    assert _raw(5, 30.0, 31.0, g)[0] == capi.LC_OK
    rc, msg = _raw(5, 4.0, 31.0, g)  # no Student-t without degrees of freedom (lc_gw_precision's check)
    assert rc == capi.LC_EINVAL and "nu" in msg
    rc, msg = _raw(5, 30.0, 0.0, g)
    assert rc == capi.LC_EINVAL and "beta" in msg
    rc, msg = _raw(0, 30.0, 31.0, g)
    assert rc == capi.LC_EINVAL and "D must be" in msg
    assert capi.lib().lc_gw_precision_var(5, 30.0, 31.0, None) == capi.LC_EINVAL


@pytest.mark.parametrize("D", [2, 5, 23])
def test_emulated_route_equals_the_direct_reference(D):
    """identity-padded 8 x 8 Cholesky of P_bb, diag(H^-1) from L^-1, the between term from the deviations from the fill
    value: the same variance as the per-row Schur complement on iW with the mixture sum centred on the mean, to
    1e-12 V_n -- the bar tests/test_incomplete_host.py uses for the same pair of routes"""
    rng = np.random.default_rng(900 + D)
    K = 3
    cls = [ref.random_posterior(rng, D) for _ in range(K)]
    # (the prior component: nu = D; at D = 2 its variance does not exist with one hole, so it takes no part there)
    prior = (float(D), 1.0, np.zeros(D), D * np.eye(D))
    Epi, rest = (np.array([0.5, 0.3, 0.15]), 0.05) if D > 2 else (np.array([0.5, 0.3, 0.2]), 0.0)
    X = np.stack([cls[k][2] + rng.normal(size=D) * 2.0 for k in rng.integers(0, K, 60)])
    # (at most D - 2 holes where the prior component takes part: nu - 1 - nb > 0)
    Xh = ref.make_holes(rng, X, max_holes=min(ref.HOLES_MAX, D - 2) if D > 2 else 1)
    assert np.any(~np.isnan(Xh).any(axis=1)) and np.isnan(Xh).any()
    var, Vn, share, logp = vref.direct_var(Xh, cls, prior, Epi, rest)
    holed = np.isnan(Xh).any(axis=1)
    # the reference's own log density is that of incomplete_ref.direct (scipy's multivariate_t)
    np.testing.assert_allclose(logp[holed], ref.direct(Xh, cls, prior, Epi, rest)[1][holed], rtol=1e-12, atol=0)
    assert np.all(np.isnan(logp[~holed])) and not var[~holed].any()
    count = np.isnan(Xh).sum(axis=1)
    assert all(not var[n, count[n]:].any() and np.all(var[n, : count[n]] > 0) for n in range(Xh.shape[0]))
    print(f"D = {D}: share of rows with holes whose between term reaches 1 % of var = {np.mean(share[holed] >= 0.01):.2f}")
    evar = vref.emulate_var(Xh, cls, prior, Epi, rest, ref.fill_value(cls, [5.0, 3.0, 1.0]))
    ratio = float(np.max(np.abs(evar - var) / Vn[:, None]))
    print(f"D = {D}: max |emulated - direct| / V_n = {ratio:.3e}")
    assert np.all(np.abs(evar - var) <= 1e-12 * Vn[:, None]), ratio
    # the fill value cancels: another one near the data gives the same answer
    ovar = vref.emulate_var(Xh, cls, prior, Epi, rest, cls[0][2])
    assert np.all(np.abs(ovar - var) <= 1e-12 * Vn[:, None])


def test_new_symbols_are_declared_and_exported(lib):
    names = capi.declared_symbols()
    for n in ("lc_model_predict_incomplete_var", "lc_ctx_get_completed_var", "lc_gw_precision_var"):
        assert n in names, f"{n} is not declared in include/libcluster_hip.h"
        assert hasattr(lib, n)
    assert capi.CompletionVar._fields == ("rows", "logp", "count", "cols", "var")
    assert capi.Completion._fields == ("rows", "logp", "count", "cols")
    done = capi.Completion(None, None, None, None)
    assert done.var is None and len(done) == 4
