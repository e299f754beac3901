"""Leave-one-out conditionals, the host side: the symbols exist, and the route the device takes -- emulated in
numpy -- gives what the direct one-hole-per-row reference gives.  No GPU."""
import numpy as np
import pytest

import incomplete_ref as ref
import incomplete_var_ref as vref
import leave_one_out_ref as loo
from libcluster_amd import capi


def test_new_symbols_are_declared_and_exported(lib):
    import libcluster_amd

    names = capi.declared_symbols()
    for n in ("lc_model_predict_leave_one_out", "lc_ctx_get_leave_one_out"):
        assert n in names, f"{n} is not declared in include/libcluster_hip.h"
        assert hasattr(lib, n)
    assert capi.LeaveOneOut._fields == ("logp", "cond_logp", "mean", "worst")
    assert capi.LeaveOneOutVar._fields == ("logp", "cond_logp", "mean", "var", "worst")
    assert libcluster_amd.LeaveOneOut is capi.LeaveOneOut and libcluster_amd.LeaveOneOutVar is capi.LeaveOneOutVar
    assert capi.LeaveOneOut(None, None, None, None).var is None
    for n in ("explain", "explain_context"):
        assert callable(getattr(capi.Model, n))
    assert callable(capi.Context.get_leave_one_out)


def test_the_kernel_hook_is_in_the_hooks_library_only(lib):
    """lcx_test_loo_rows (bound by tests/test_gpu_loo_kernels.py) is exported by the hooks library; the shipped one exports no hook"""
    import aux_hooks

    assert "lcx_test_loo_rows" in aux_hooks.exported_symbols(aux_hooks.HOOKS_LIB)
    assert not [s for s in aux_hooks.exported_symbols(aux_hooks.SHIPPED_LIB) if "test_loo" in s]


def _case(D):
    rng = np.random.default_rng(900 + D)
    K = 3
    cls = [ref.random_posterior(rng, D) for _ in range(K)]
    # (the prior component: nu = D; at D = 2 the variance with one hole needs nu > 2, so it gets nu = 3 there)
    prior = (3.0 if D == 2 else float(D), 1.0, np.zeros(D), D * np.eye(D))
    Epi, rest = np.array([0.5, 0.3, 0.15]), 0.05
    X = np.stack([cls[k][2] + rng.normal(size=D) * 2.0 for k in rng.integers(0, K, 37)])
    return cls, prior, Epi, rest, X


@pytest.mark.parametrize("D", [2, 5, 23])
def test_emulated_route_equals_the_direct_reference(D):
    """v = P (x - m), the scalar correction v_d^2 / P_dd and the between term from the deviations from x_d: the same four
    quantities as the one-hole-per-row references on iW, to 1e-12 of their scales -- with the operand centred per cluster,
    on the fill value of DESIGN 4.15 and on zeros"""
    cls, prior, Epi, rest, X = _case(D)
    want = loo.loo_direct(X, cls, prior, Epi, rest)
    assert np.all(want.var > 0) and np.all(np.isfinite(want.cond))
    share = float(np.mean(want.rmax < 0.99))
    print(f"D = {D}: share of (row, column) pairs with max_k r < 0.99 = {share:.2f}")
    assert share >= 0.15, share  # (not vacuous: the mixing over the clusters is exercised)
    cb, S, V = loo.bars(want)
    for name, fill in (("per cluster", None), ("fill value", ref.fill_value(cls, [5.0, 3.0, 1.0])), ("zeros", np.zeros(D))):
        got = loo.loo_emulate(X, cls, prior, Epi, rest, fill)
        ratios = (np.max(np.abs(got.logp - want.logp) / np.abs(want.logp)), np.max(np.abs(got.cond - want.cond) / cb),
                  np.max(np.abs(got.mean - want.mean) / S), np.max(np.abs(got.var - want.var) / V))
        print(f"D = {D}, {name}: max |emulated - direct| / scale (logp, cond, mean, var) = " + ", ".join(f"{r:.2e}" for r in ratios))
        assert np.all(np.abs(got.logp - want.logp) <= 1e-12 * np.abs(want.logp))
        assert np.all(np.abs(got.cond - want.cond) <= 1e-12 * cb)
        assert np.all(np.abs(got.mean - want.mean) <= 1e-12 * S)
        assert np.all(np.abs(got.var - want.var) <= 1e-12 * V)


@pytest.mark.parametrize("D", [2, 5, 23])
def test_grouped_variance_is_direct_var(D):
    """the reference's variance beyond D = 23 (one factor of iW_aa per column and component) is direct_var's (one per row and
    component)"""
    cls, prior, Epi, rest, X = _case(D)
    v, Vn, _, _ = vref.direct_var(loo.one_hole_rows(X), cls, prior, Epi, rest)
    var, V = loo.var_by_column(X, cls, prior, Epi, rest)
    np.testing.assert_allclose(var, v[:, 0].reshape(X.shape), rtol=1e-12, atol=0)
    np.testing.assert_allclose(V, Vn.reshape(X.shape), rtol=1e-12, atol=0)
