"""Rows with holes, the host arithmetic: lc_gw_precision turns one Gauss-Wishart posterior into the table
the device pass uses, and the route that pass takes -- emulated in numpy -- gives what the direct per-row reference
gives.  No GPU."""
import numpy as np
import pytest

import incomplete_ref as ref
from libcluster_amd import capi


@pytest.mark.parametrize("D", [1, 2, 5, 23])
def test_tables_against_numpy(lib, D):
    rng = np.random.default_rng(150 + D)
    nu, beta, m, iW = ref.random_posterior(rng, D)
    t = capi.gw_precision(nu, beta, m, iW)
    P, G, s, e = ref.tables(nu, beta, iW)
    assert np.array_equal(t["P"], t["P"].T)
    np.testing.assert_allclose(t["P"] @ iW, nu * np.eye(D), rtol=0, atol=1e-12 * nu)
    ok = np.arange(ref.HOLES_MAX + 1) <= D
    np.testing.assert_allclose(t["G"][ok], G[ok], rtol=1e-13, atol=0)
    assert np.all(np.isnan(t["G"][~ok]))
    np.testing.assert_allclose(t["e"], e, rtol=1e-13, atol=0)
    np.testing.assert_allclose(t["s"], s, rtol=1e-13, atol=0)
    # G[0] and e[0] are the constants of the full-width Student-t that lc_model_predict mixes
    assert e[0] == (nu + 1) / 2


def _raw(D, nu, beta, m, iW):
    rc = capi.lib().lc_gw_precision(D, nu, beta, capi.dptr(m), capi.dptr(iW), None, None, None, None)
    return rc, capi.lib().lc_last_error().decode()


def test_error_cases_are_einval(lib):
    rng = np.random.default_rng(8)
    D = 5
    nu, beta, m, iW = ref.random_posterior(rng, D)
    assert _raw(D, nu, beta, m, iW)[0] == capi.LC_OK  # (every output may be NULL)
    rc, msg = _raw(D, D - 1.0, beta, m, iW)  # no Student-t without degrees of freedom
    assert rc == capi.LC_EINVAL and "nu" in msg
    rc, msg = _raw(D, nu, 0.0, m, iW)
    assert rc == capi.LC_EINVAL and "beta" in msg
    rc, msg = _raw(0, nu, beta, m, iW)
    assert rc == capi.LC_EINVAL and "D must be" in msg
    bad = iW.copy()
    bad[0, 0] = -1.0
    rc, msg = _raw(D, nu, beta, m, bad)
    assert rc == capi.LC_EINVAL and "positive definite" in msg
    assert capi.lib().lc_gw_precision(D, nu, beta, None, capi.dptr(iW), None, None, None, None) == capi.LC_EINVAL


@pytest.mark.parametrize("D", [2, 5, 23])
def test_emulated_route_equals_the_direct_reference(D):
    """fill, full-width distance, rank-nb correction with P, identity-padded 8 x 8 Cholesky: the same log density and the
    same filled values as the per-row marginal and linear expert, to 1e-12"""
    rng = np.random.default_rng(900 + D)
    K = 3
    cls = [ref.random_posterior(rng, D) for _ in range(K)]
    prior = (float(D), 1.0, np.zeros(D), D * np.eye(D))
    Epi, rest = np.array([0.5, 0.3, 0.15]), 0.05
    X = np.stack([cls[k][2] + rng.normal(size=D) * 2.0 for k in rng.integers(0, K, 60)])
    Xh = ref.make_holes(rng, X)
    assert np.isnan(Xh[0]).sum() == min(ref.HOLES_MAX, D - 1) and np.any(~np.isnan(Xh).any(axis=1))
    rows, logp, _, S = ref.direct(Xh, cls, prior, Epi, rest)
    erows, elogp = ref.emulate(Xh, cls, prior, Epi, rest, ref.fill_value(cls, [5.0, 3.0, 1.0]))
    np.testing.assert_allclose(elogp, logp, rtol=1e-12, atol=0)
    holes = np.isnan(Xh)
    assert np.array_equal(erows[~holes], Xh[~holes]) and np.array_equal(rows[~holes], Xh[~holes])
    assert np.all(np.abs(erows - rows) <= 1e-12 * S[:, None])
    # the fill value cancels: another one gives the same answer
    orows, ologp = ref.emulate(Xh, cls, prior, Epi, rest, np.zeros(D))
    np.testing.assert_allclose(ologp, logp, rtol=1e-12, atol=0)
    assert np.all(np.abs(orows - rows) <= 1e-12 * S[:, None])


def test_new_symbols_are_declared_and_exported(lib):
    names = capi.declared_symbols()
    for n in ("lc_model_predict_incomplete", "lc_ctx_get_completed", "lc_gw_precision"):
        assert n in names, f"{n} is not declared in include/libcluster_hip.h"
        assert hasattr(lib, n)
    assert capi.Completion._fields == ("rows", "logp", "count", "cols")
    assert "#define LC_HOLES_MAX 8" in capi.HEADER.read_text() and capi.HOLES_MAX == 8 == ref.HOLES_MAX
