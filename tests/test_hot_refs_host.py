"""The references of tests/test_gpu_hot_kernels.py (tests/hot_refs.py) have to be right on their own: no GPU here."""
import math

import numpy as np
import pytest

import hot_refs as hr
import lc_oracle as o
from test_gpu_parity import RTOL_F, RTOL_Q


def _posterior(rng, N, D, K):
    X = rng.normal(size=(N, D)) * 1.5 + rng.integers(0, K, (N, 1))
    q0 = rng.dirichlet(np.ones(K) * 0.3, N)
    w = o.StickBreak()
    cl = [o.GaussWish(1.0, D) for _ in range(K)]
    w.update(o.updateSS(X, q0, cl))
    for c in cl:
        c.update()
    return X, w, cl


def _device_params(w, cl, D):
    """what the host hands the kernels: A_k = sqrt(nu_k) chol(iW_k)^-1, m_k, c_k = E[log pi_k] + the constant of Eloglike"""
    A = np.stack([math.sqrt(c.nu) * np.linalg.inv(np.linalg.cholesky(c.iW)) for c in cl])
    m = np.stack([c.m for c in cl])
    cst = np.array([0.5 * (c.sumpsi() + c.logdW - D * (1 / c.beta + math.log(math.pi))) for c in cl])
    return A, m, (w.Elogweight() + cst)[None, :]


@pytest.mark.parametrize("N,D,K", [(200, 5, 3), (150, 23, 4), (120, 64, 3), (64, 150, 2)])
def test_longdouble_estep_from_packed_parameters_agrees_with_the_oracle(N, D, K):
    rng = np.random.default_rng(7 * D + K)
    X, w, cl = _posterior(rng, N, D, K)
    A, m, ctab = _device_params(w, cl, D)
    DP = hr.padded_dim(D)
    DC = hr.active_width(D, DP)
    P = hr.pack_params(A, m, DP, DC)
    assert P.shape == (K, hr.pstride(DP, DC))
    Au, bneg = hr.unpack_params(P, DP, DC)
    Xp = np.zeros((N, DP))
    Xp[:, :D] = X
    lq, _ = hr.estep_ref(Xp, Au, bneg, ctab, np.zeros(N, dtype=int))
    logZ, q, _ = hr.normalise_ref(lq)
    qref, Fzref = o.vbexpectation(X, w, cl)
    got = q.T.astype(np.float64)
    big = qref > 1e-12
    assert np.max(np.abs(got[big] - qref[big]) / qref[big]) < RTOL_Q
    assert np.max(np.abs(got - qref)) < 1e-11
    assert abs(float(-logZ.sum()) - Fzref) <= RTOL_F * abs(Fzref)


@pytest.mark.parametrize("D,DP,DC", [(3, 16, 16), (16, 16, 16), (17, 32, 20), (23, 32, 24), (28, 32, 28), (32, 32, 32), (37, 48, 40),
                                      (55, 64, 56), (64, 64, 64), (70, 80, 72), (100, 112, 104), (128, 128, 128), (129, 192, 192),
                                      (192, 192, 192), (200, 256, 256), (300, 320, 320)])
def test_unpacking_returns_the_whitener_and_minus_A_m(D, DP, DC):
    assert hr.padded_dim(D) == DP and hr.active_width(D, DP) == DC
    rng = np.random.default_rng(D)
    K = 2
    A = np.tril(rng.normal(size=(K, D, D)))
    m = rng.normal(size=(K, D))
    P = hr.pack_params(A, m, DP, DC)
    assert P.shape == (K, hr.pstride(DP, DC))
    Au, bneg = hr.unpack_params(P, DP, DC)
    W = Au.shape[1]
    assert W == (DP if DP > 128 else DC)
    assert np.array_equal(Au[:, :D, :D], A) and not Au[:, D:, :].any() and not Au[:, :, D:].any()
    ref = -np.einsum("kij,kj->ki", A.astype(np.longdouble), m.astype(np.longdouble))
    assert np.max(np.abs(bneg[:, :D] - ref)) <= D * hr.EPS * np.max(np.abs(A)) * np.max(np.abs(m)) * D
    assert not bneg[:, D:].any()
    # every slot of the stream is either an entry of A / -b or a structural zero: as many non-zeros as the inputs have
    assert np.count_nonzero(P) >= np.count_nonzero(A) + np.count_nonzero(bneg)
    if DP <= 128:
        assert np.count_nonzero(P) == np.count_nonzero(A) + np.count_nonzero(bneg)


def test_exact_inputs_are_exact():
    """int64 sums equal the float64 sums in several shuffled orders, and every magnitude stays below 2^53"""
    rng = np.random.default_rng(5)
    NP, D, DP, K = 4096, 61, 64, 5
    X = hr.exact_X(rng, NP, D, DP)
    q = hr.exact_q(rng, K, NP, zero_steps=True)
    assert np.array_equal(X, np.rint(X)) and np.array_equal(q * 1024, np.rint(q * 1024)) and q.min() >= 0 and q.max() <= 1
    Xi, qi = X.astype(np.int64), np.rint(q * 1024).astype(np.int64)
    ref = hr.stats_ref(X, q)
    Sint = np.einsum("kn,ni,nj->kij", qi, Xi, Xi)
    assert np.abs(Sint).max() < 2 ** 53 and np.abs(Xi).max() ** 2 * 1024 * (1 << 22) < 2 ** 53  # (up to 4M rows)
    assert np.array_equal(ref[:, 1 + DP:].reshape(K, DP, DP) * 1024, Sint.astype(np.float64))
    assert np.array_equal(ref[:, 0] * 1024, qi.sum(axis=1).astype(np.float64))
    assert np.array_equal(ref[:, 1:1 + DP] * 1024, (qi @ Xi).astype(np.float64))
    for seed in range(4):
        p = np.random.default_rng(seed).permutation(NP)
        assert np.array_equal(hr.stats_ref(X[p], q[:, p]), ref)
        parts = sum(hr.stats_ref(X[p], q[:, p], slice(a, a + 512)) for a in range(0, NP, 512))
        assert np.array_equal(parts, ref)
    # the E-step: y, its squares and log q~ in integers (doubled: c and d^2 / 2 are multiples of 1/2)
    A, m = hr.exact_params(rng, K, D)
    ctab = hr.exact_ctab(rng, 3, K)
    grp = rng.integers(0, 3, size=NP)
    P = hr.pack_params(A, m, DP, DP)
    Au, bneg = hr.unpack_params(P, DP, DP)
    lq, _ = hr.estep_ref(X, Au, bneg, ctab, grp, exact=True)
    Ai, bi = Au.astype(np.int64), bneg.astype(np.int64)
    assert np.array_equal(Ai, Au) and np.array_equal(bi, bneg)
    y = np.einsum("kij,nj->kni", Ai, Xi) + bi[:, None, :]
    d2 = (y * y).sum(axis=2)
    assert d2.max() < 2 ** 52 and np.abs(Ai).max() <= 3
    lq2 = np.rint(2 * ctab).astype(np.int64)[grp].T - d2
    assert np.array_equal(lq * 2, lq2.astype(np.float64))
    for seed in range(3):  # any order of the columns gives the same squares' sum
        p = np.random.default_rng(seed).permutation(DP)
        y2 = (np.einsum("kij,nj->kni", Au[:, :, p], X[:, p]) + bneg[:, None, :])[:, :, p]
        assert np.array_equal((y2 * y2).sum(axis=2), d2.astype(np.float64))


@pytest.mark.parametrize("G,ntile,yshare", [(512, 2047, 410), (512, 2048, 410), (512, 2049, 410), (512, 2048 + 259, 410), (512, 2048, 0),
                                            (511, 4000, 410), (2, 8, 410), (2, 7, 410), (4, 16, 999), (4, 17, 1), (6, 100, 500),
                                            (3, 3, 0), (1, 5, 410), (208, 4 * 208 + 107, 410), (16, 3, 410)])
def test_fused_deal_visits_every_tile_exactly_once(G, ntile, yshare):
    seen = np.zeros(ntile, dtype=int)
    counts = []
    for b in range(G):
        t = hr.fused_deal(b, G, ntile, yshare)
        assert all(0 <= x < ntile for x in t), (b, t[:4])
        np.add.at(seen, t, 1)
        counts.append(len(t))
    assert (seen == 1).all()
    uneven = yshare > 0 and G % 2 == 0 and ntile >= 4 * G
    if uneven:  # every second block the same share, never more than a first block's
        H = G // 2
        assert set(counts[H:]) == {ntile * 2 * yshare // (1000 * G)} and max(counts[:H]) - min(counts[:H]) <= 1
    else:
        assert max(counts) - min(counts) <= 1


def test_region_masks_partition_a_record():
    for DP, DC in ((16, 16), (32, 20), (64, 56), (192, 192)):
        low = hr.lower_mask(DP, DC)
        s_idle, S_idle, upper = hr.region_masks(DP, DC)
        tot = low.astype(int) + s_idle + S_idle + upper
        assert (tot == 1).all() and low.sum() == 1 + DC + DC * (DC + 1) // 2
