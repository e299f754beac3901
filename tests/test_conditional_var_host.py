"""Predictive variance of the conditional prediction, the host arithmetic: lc_gw_conditional_var turns one
Gauss-Wishart posterior and a split of the columns into the diagonal of the Schur complement and the factor g.  Checked
against numpy and against numerical integration of scipy's multivariate Student-t; no GPU."""
import ctypes as C

import numpy as np
import pytest
from scipy import integrate, stats

from libcluster_amd import capi

import cond_var_ref as ref


def _posterior(rng, D):
    """a random posterior (nu, beta, m, iW) of a cluster that saw about 3 D observations"""
    n = 3 * D + 5
    Y = rng.normal(size=(n, D)) @ rng.normal(size=(D, D)) / np.sqrt(D) + rng.normal(0, 3, D)
    iW = D * np.eye(D) + (Y - Y.mean(0)).T @ (Y - Y.mean(0))
    return D + n, 1.0 + n, Y.mean(0), (iW + iW.T) / 2


def _splits(rng, D):
    """(given, target): permuted and non-contiguous given, target explicit (permuted, a subset) and defaulted"""
    if D == 2:
        return [([1], [0]), ([0], None)]
    perm = rng.permutation(D)
    Da = max(1, D // 2)
    g1, rest = [int(c) for c in perm[:Da]], [int(c) for c in perm[Da:]]
    return [(g1, None), (g1, rest[: max(1, len(rest) // 2)]), ([int(c) for c in range(0, D, 3)][::-1], None)]


@pytest.mark.parametrize("D", [2, 5, 23, 64])
def test_tables_against_numpy(lib, D):
    rng = np.random.default_rng(140 + D)
    nu, beta, m, iW = _posterior(rng, D)
    for given, target in _splits(rng, D):
        S, g = capi.gw_conditional_var(nu, beta, iW, given, target)
        tg = target if target is not None else [c for c in range(D) if c not in given]
        _, schur, gref, _ = ref.cluster_tables(nu, beta, m, iW, given, tg, D)
        assert S.shape == (len(tg),)
        np.testing.assert_allclose(S, schur, rtol=1e-12, atol=0)
        np.testing.assert_allclose(g, gref, rtol=1e-12, atol=0)
        assert np.all(S > 0)


def test_variance_against_numerical_integration(lib):
    """D = 3, two given columns, one target: g (1 + s d^2) S against the second central moment of the joint predictive
    density along the target, by scipy.integrate.quad (rtol 1e-8: quad's default tolerance)"""
    rng = np.random.default_rng(1)
    D, nu, beta = 3, 7.5, 2.3
    A_ = rng.normal(size=(D, D))
    iW = A_ @ A_.T + D * np.eye(D)
    m = rng.normal(size=D)
    nup = nu + 1 - D
    given, target = [2, 0], [1]
    xa = np.array([1.7, -0.9])
    S, g = capi.gw_conditional_var(nu, beta, iW, given, target)
    t = capi.gw_conditional(nu, beta, m, iW, given, target)
    d2 = float(np.sum((t["A"] @ (xa - t["ma"])) ** 2))
    var = g * (1 + t["s"] * d2) * S[0]
    mean = float(t["mb"][0] + t["B"][0] @ (xa - t["ma"]))
    mt = stats.multivariate_t(loc=m, shape=(1 + beta) / (beta * nup) * iW, df=nup)

    def joint(xb):
        x = np.empty(D)
        x[given], x[target] = xa, xb
        return mt.pdf(x)

    Z = integrate.quad(joint, -np.inf, np.inf)[0]
    E1 = integrate.quad(lambda v: v * joint(v), -np.inf, np.inf)[0] / Z
    E2 = integrate.quad(lambda v: (v - E1) ** 2 * joint(v), -np.inf, np.inf, limit=200)[0] / Z
    print(f"mean {mean!r} vs quad {E1!r}; var {var!r} vs quad {E2!r}")
    np.testing.assert_allclose(mean, E1, rtol=1e-8, atol=0)
    np.testing.assert_allclose(var, E2, rtol=1e-8, atol=0)


def _raw(D, nu, beta, iW, given, target, outputs=False):
    gv = np.asarray(given, dtype=np.int32)
    tv = None if target is None else np.asarray(target, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    S, g = np.full(D, np.nan), C.c_double(np.nan)
    rc = capi.lib().lc_gw_conditional_var(D, nu, beta, capi.dptr(iW), gv.ctypes.data_as(ip), gv.size,
                                          None if tv is None else tv.ctypes.data_as(ip), 0 if tv is None else tv.size,
                                          capi.dptr(S) if outputs else None, C.byref(g) if outputs else None)
    return rc, capi.lib().lc_last_error().decode(), S, g.value


def test_domain_error_exactly_at_two_degrees_of_freedom(lib):
    rng = np.random.default_rng(3)
    D = 4
    _, beta, _, iW = _posterior(rng, D)
    nu = float(D)  # nu' = 1: the state of a cluster prior
    rc, msg, _, _ = _raw(D, nu, beta, iW, [2], [0], outputs=True)  # nu' + ngiven = 2 exactly
    assert rc == capi.LC_EDOMAIN and "does not exist" in msg, (rc, msg)
    rc, msg, _, _ = _raw(D, nu, beta, iW, [2], [0])  # ... also when no output is asked for
    assert rc == capi.LC_EDOMAIN
    with pytest.raises(capi.DomainError, match="does not exist"):
        capi.gw_conditional_var(nu, beta, iW, [2], [0])
    rc, msg, S, g = _raw(D, nu, beta, iW, [2, 3], [0], outputs=True)  # nu' + ngiven = 3
    assert rc == capi.LC_OK and np.isfinite(g) and np.isfinite(S[0]) and S[0] > 0
    np.testing.assert_allclose(g, (1 + beta) / beta, rtol=1e-15)
    # just above two: huge, finite, and not an error (the check is strict, not a threshold)
    rc, msg, S, g = _raw(D, nu + 1e-9, beta, iW, [2], [0], outputs=True)
    assert rc == capi.LC_OK and np.isfinite(g) and g > 1e8
    # the mean's tables exist either way
    assert capi.gw_conditional(nu, beta, np.zeros(D), iW, [2], [0])["B"].shape == (1, 1)


def test_error_cases_are_einval(lib):
    rng = np.random.default_rng(7)
    D = 5
    nu, beta, _, iW = _posterior(rng, D)
    assert _raw(D, nu, beta, iW, [3, 0], None)[0] == capi.LC_OK  # (either output may be NULL)
    cases = [
        ([], [1], "at least one"),          # ngiven < 1
        ([0, 1], [], "at least one"),       # no target column
        ([0, 1, 2, 3, 4], None, "every column"),  # ... by default either
        ([0, 5], [1], "outside"),           # index outside [0, D)
        ([-1], [1], "outside"),
        ([0], [7], "outside"),
        ([0, 2, 0], [1], "twice"),          # duplicate index
        ([0], [1, 3, 1], "twice"),
        ([0, 2], [1, 2], "both"),           # a column in both lists
    ]
    for given, target, word in cases:
        rc, msg, _, _ = _raw(D, nu, beta, iW, given, target)
        assert rc == capi.LC_EINVAL and word in msg, (given, target, rc, msg)
    rc, msg, _, _ = _raw(D, D - 1.0, beta, iW, [0], [1])
    assert rc == capi.LC_EINVAL and "nu" in msg
    bad = iW.copy()
    bad[0, 0] = -1.0
    rc, msg, _, _ = _raw(D, nu, beta, bad, [0, 1], [2])
    assert rc == capi.LC_EINVAL and "positive definite" in msg


def test_new_symbols_are_declared_and_exported(lib):
    names = capi.declared_symbols()
    for n in ("lc_model_predict_conditional_var", "lc_ctx_get_conditional_var", "lc_gw_conditional_var"):
        assert n in names, f"{n} is not declared in include/libcluster_hip.h"
        assert hasattr(lib, n), f"{n} is not exported by the library"
    assert capi.ConditionalVar._fields == ("mean", "logp", "var")
    assert capi.Conditional(np.zeros((1, 1)), np.zeros(1)).var is None
