"""Conditional prediction, the host arithmetic: lc_gw_conditional turns one Gauss-Wishart posterior and a
split of the columns into the tables the device pass uses.  Checked against numpy / scipy; no GPU."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

from libcluster_amd import capi


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
def test_tables_against_numpy_and_scipy(lib, D):
    rng = np.random.default_rng(40 + D)
    nu, beta, m, iW = _posterior(rng, D)
    for given, target in _splits(rng, D):
        t = capi.gw_conditional(nu, beta, m, iW, given, target)
        want_t = target if target is not None else [c for c in range(D) if c not in given]
        assert t["target"] == want_t
        Da = len(given)
        Saa, Sba = iW[np.ix_(given, given)], iW[np.ix_(want_t, given)]
        assert np.array_equal(t["ma"], m[given]) and np.array_equal(t["mb"], m[want_t])
        assert np.array_equal(t["A"], np.tril(t["A"]))
        X = m[given] + rng.normal(size=(50, Da)) * rng.uniform(0.1, 30.0, (50, 1))
        d2 = np.sum(((X - t["ma"]) @ t["A"].T) ** 2, axis=1)
        maha = np.einsum("ni,ni->n", X - m[given], np.linalg.solve(Saa, (X - m[given]).T).T)
        np.testing.assert_allclose(d2, nu * maha, rtol=1e-12, atol=0)
        Bref = np.linalg.solve(Saa, Sba.T).T
        np.testing.assert_allclose(t["B"], Bref, rtol=1e-11, atol=0)
        nup = nu + 1 - D
        ref = stats.multivariate_t(loc=m[given], shape=(1 + beta) / (beta * nup) * Saa, df=nup).logpdf(X).reshape(-1)
        got = t["G"] - t["e"] * np.log1p(t["s"] * d2)
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)


def _raw(D, nu, beta, m, iW, given, target):
    gv = np.asarray(given, dtype=np.int32)
    tv = None if target is None else np.asarray(target, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    rc = capi.lib().lc_gw_conditional(D, nu, beta, capi.dptr(m), capi.dptr(iW), gv.ctypes.data_as(ip), gv.size,
                                      None if tv is None else tv.ctypes.data_as(ip), 0 if tv is None else tv.size,
                                      None, None, None, None, None, None, None)
    return rc, capi.lib().lc_last_error().decode()


def test_error_cases_are_einval(lib):
    rng = np.random.default_rng(7)
    D = 5
    nu, beta, m, iW = _posterior(rng, D)
    assert _raw(D, nu, beta, m, iW, [3, 0], None)[0] == capi.LC_OK  # (every output may be NULL)
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
        rc, msg = _raw(D, nu, beta, m, iW, given, target)
        assert rc == capi.LC_EINVAL and word in msg, (given, target, rc, msg)
    rc, msg = _raw(D, D - 1.0, beta, m, iW, [0], [1])  # no Student-t without degrees of freedom
    assert rc == capi.LC_EINVAL and "nu" in msg
    bad = iW.copy()
    bad[0, 0] = -1.0
    rc, msg = _raw(D, nu, beta, m, bad, [0, 1], [2])
    assert rc == capi.LC_EINVAL and "positive definite" in msg


def test_new_symbols_are_declared_and_exported(lib):
    names = capi.declared_symbols()
    for n in ("lc_model_predict_conditional", "lc_ctx_get_conditional", "lc_gw_conditional"):
        assert n in names, f"{n} is not declared in include/libcluster_hip.h"
        assert hasattr(lib, n)
    assert capi.Conditional._fields == ("mean", "logp")
