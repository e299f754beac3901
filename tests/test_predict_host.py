"""Expected weights of the prediction path (lc_weights_predictive) against the oracle's weight objects (CPU only).

E[pi_k] of a Dirichlet is alpha_k / sum(alpha); of a stick-breaking prior E[v_k] prod_{i before k} E[1 - v_i] with
E[v] = a1 / (a1 + a2), "before" in the order the reference's update sorts the sticks (distributions.cpp:139-165), and the
mass beyond the truncation is prod_i E[1 - v_i]; GDirichlet's last stick has v = 1 (:184-194)."""
import numpy as np
import pytest

import lc_oracle as o
from libcluster_amd import capi

CASES = {
    "random": np.array([12.5, 0.3, 40.0, 7.25, 0.0, 3.0]),
    "tied": np.array([5.0, 2.0, 5.0, 5.0, 2.0, 0.0, 5.0]),
    "zeros": np.zeros(4),
    "one": np.array([17.0]),
    # (quarters: every partial sum is exact, so numpy's pairwise N = sum(Nk) and the library's running sum agree and the
    #  leftover counts N - cumNk of the last sticks carry no rounding of their own)
    "wide": np.random.default_rng(3).integers(0, 400, 40) * 0.25,
}


def _numpy_stick(w, last_is_one):
    Epi = np.zeros(w.alpha1.size)
    rest = 1.0
    for i, k in enumerate(w.order):
        a1, a2 = w.alpha1[k], w.alpha2[k]
        if last_is_one and i == len(w.order) - 1:
            Epi[k] = rest
            rest = 0.0
            break
        Epi[k] = a1 / (a1 + a2) * rest
        rest *= a2 / (a1 + a2)
    return Epi, rest


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("prior", [1.0, 0.5, 3.0])
def test_dirichlet(lib, case, prior):
    Nk = CASES[case]
    w = o.Dirichlet(prior)
    w.update(Nk)
    Epi, rest = capi.weights_predictive(capi.W_DIRICHLET, Nk, prior)
    np.testing.assert_allclose(Epi, w.alpha / w.alpha.sum(), rtol=1e-14, atol=0)
    assert rest == 0.0
    assert abs(Epi.sum() - 1.0) <= 1e-14


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("prior", [1.0, 0.5, 3.0])
def test_stickbreak(lib, case, prior):
    Nk = CASES[case]
    w = o.StickBreak(prior)
    w.update(Nk)
    want, want_rest = _numpy_stick(w, False)
    Epi, rest = capi.weights_predictive(capi.W_STICKBREAK, Nk, prior)
    np.testing.assert_allclose(Epi, want, rtol=1e-14, atol=0)
    assert abs(rest - want_rest) <= 1e-14 * want_rest
    assert rest > 0.0
    assert abs(Epi.sum() + rest - 1.0) <= 1e-14


@pytest.mark.parametrize("case", sorted(CASES))
def test_gdirichlet(lib, case):
    Nk = CASES[case]
    w = o.GDirichlet()
    w.update(Nk)
    want, want_rest = _numpy_stick(w, True)
    Epi, rest = capi.weights_predictive(capi.W_GDIRICHLET, Nk)
    np.testing.assert_allclose(Epi, want, rtol=1e-14, atol=0)
    assert rest == want_rest == 0.0
    assert abs(Epi.sum() - 1.0) <= 1e-14


def test_tied_counts_follow_the_sort(lib):
    """Equal counts: the sticks are taken in the reference's (unstable) sort order, which the oracle reproduces --
    the expected weights of tied clusters differ, and by which of them comes first."""
    Nk = CASES["tied"]
    w = o.StickBreak()
    w.update(Nk)
    Epi, _ = capi.weights_predictive(capi.W_STICKBREAK, Nk)
    tied = [k for k in w.order if Nk[k] == 5.0]
    assert all(Epi[a] > Epi[b] for a, b in zip(tied, tied[1:]))


def test_errors(lib):
    with pytest.raises(ValueError):
        capi.weights_predictive(7, np.ones(3))
    with pytest.raises(ValueError):
        capi.weights_predictive(capi.W_DIRICHLET, np.ones(3), wprior=0.0)
    with pytest.raises(ValueError):
        capi.weights_predictive(capi.W_DIRICHLET, np.ones(0))
