"""The references of tests/test_gpu_diag_kernels.py (tests/diag_refs.py) have to be right on their own, and the host packer of
the matrix-pipe E-step (estep_diag_centre / estep_diag_pack, csrc/lc_ctx.cpp) has to be what they restate: no GPU here."""
import numpy as np
import pytest
from scipy.special import digamma

import aux_hooks as ah
import diag_refs as dr
import hot_refs as hr
import lc_oracle as o
from test_gpu_parity import RTOL_F, RTOL_Q

u64 = np.uint64


def _posterior(rng, family, N, D, K):
    eg = family == "ExpGamma"
    X = rng.normal(size=(N, D)) * 1.5 + rng.integers(0, K, (N, 1))
    if eg:
        X = np.abs(X) + 0.1
    q0 = rng.dirichlet(np.ones(K) * 0.3, N)
    w = o.StickBreak()
    cl = [(o.ExpGamma if eg else o.NormGamma)(1.0, D) for _ in range(K)]
    w.update(o.updateSS(X, q0, cl))
    for c in cl:
        c.update()
    return X, w, cl


def _device_params(cl):
    """(a, w2, w1, constant) of the device E-step for oracle clusters (include/libcluster_hip.h, lc_estep_diag)"""
    K, D = len(cl), cl[0].D
    a, w2, w1, cst = np.zeros((K, D)), np.zeros((K, D)), np.zeros((K, D)), np.zeros(K)
    for k, c in enumerate(cl):
        if isinstance(c, o.NormGamma):
            a[k], w2[k] = c.m, -0.5 * c.nu / c.L
            cst[k] = 0.5 * (D * (digamma(c.nu) - np.log(2 * np.pi) - 1.0 / c.beta) - c.logL)
        else:
            w1[k] = -c.a * c.ib
            cst[k] = D * digamma(c.a) - c.logb
    return a, w2, w1, cst


@pytest.mark.parametrize("family", ["NormGamma", "ExpGamma"])
@pytest.mark.parametrize("N,D,K", [(200, 5, 3), (150, 23, 4), (120, 64, 3), (64, 150, 2)])
def test_both_longdouble_forms_agree_with_the_oracle(family, N, D, K):
    rng = np.random.default_rng(11 * D + K)
    X, w, cl = _posterior(rng, family, N, D, K)
    a, w2, w1, cst = _device_params(cl)
    mode = 2 if family == "ExpGamma" else 1
    DP = hr.padded_dim(D)
    Xp = np.zeros((N, DP))
    Xp[:, :D] = X
    P = dr.pad_params(a, w2, w1, DP)
    grp = np.zeros(N, dtype=int)
    zero = np.zeros((1, K))
    forms = [dr.diff_ref(Xp, P, zero, grp)[0]]
    if dr.mfma_weights(DP, K, mode) > 0:  # (D = 150: the wide layout has the difference form only)
        mu, ck, wt = dr.pack_diag(a, w2, w1, DP, mode)
        W2, WL = dr.unpack_diag(wt, DP, K, mode)
        if mode == 1:
            assert np.array_equal(W2[:, :D], w2) and not W2[:, D:].any() and not WL[:, D:].any()
        else:
            assert np.array_equal(WL[:, :D], w1) and not W2.any() and not mu.any() and not ck.any()
        lqb, SQ, SL = dr.bilinear_ref(Xp, mu, ck, W2, WL, zero, grp)
        forms.append(lqb)
        err = np.abs(lqb - forms[0]).astype(np.float64)
        assert (err <= dr.packing_bar(Xp, P, mu, W2, WL)).all(), "the two forms differ by more than the packer's roundings"
    else:
        assert D == 150
    qref, Fzref = o.vbexpectation(X, w, cl)
    for lq in forms:
        # Eloglike itself (no constant, no weights): log q~ - the cluster's constant
        for k, c in enumerate(cl):
            ref = c.Eloglike(X) - cst[k]
            got = lq[k].astype(np.float64)
            assert np.max(np.abs(got - ref)) <= 1e-11 * np.max(np.abs(ref))
        lqc = lq + (w.Elogweight() + cst).astype(hr.LD)[:, None]
        logZ, q, _ = hr.normalise_ref(lqc)
        got = q.T.astype(np.float64)
        big = qref > 1e-12
        assert np.max(np.abs(got[big] - qref[big]) / qref[big]) < RTOL_Q
        assert np.max(np.abs(got - qref)) < 1e-11
        assert abs(float(-logZ.sum()) - Fzref) <= RTOL_F * abs(Fzref)


def _same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(u64), np.ascontiguousarray(y).view(u64))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("D,DP,K", [(5, 16, 3), (16, 16, 4), (23, 32, 5), (45, 48, 9), (64, 64, 32), (77, 80, 33), (96, 96, 7), (100, 112, 12),
                                    (128, 128, 1)])
def test_host_packer_equals_the_restated_layout(mode, D, DP, K):
    """Same bits: the library's host code is built without fused multiply-adds, so a1 - (2 a2) a' and (a2 a') a' + a1 mu round as
    numpy rounds them.  (Were a compiler to contract them, the values would still have to sit within the packer's bars; this
    test would then say which entries differ.)"""
    rng = np.random.default_rng(100 * mode + D + K)
    a = rng.normal(scale=1.5, size=(K, D))
    w2 = -0.5 * rng.uniform(0.3, 3.0, size=(K, D))
    w1 = rng.normal(size=(K, D))
    if mode == 1:
        w1[:] = 0.0
    if mode == 2:
        a[:], w2[:] = 0.0, 0.0
    assert ah.diag_weights(DP, K, mode) == dr.mfma_weights(DP, K, mode) > 0
    rc, mu, ck, wt, cond = ah.diag_pack(a, w2, w1, DP, mode)
    assert rc == 0
    rmu, rck, rwt = dr.pack_diag(a, w2, w1, DP, mode)
    _, rcond = dr.centre(a, w2, DP, mode)
    assert _same_bits(mu, rmu), np.nonzero(mu != rmu)
    assert _same_bits(wt, rwt), np.nonzero(wt != rwt)
    assert _same_bits(ck, rck), (ck - rck)
    assert cond == rcond or abs(cond - rcond) <= 4 * hr.EPS * rcond  # (sqrt and the products: libm against numpy)
    print(f"cond {cond:.6g} (restated {rcond:.6g})")
    # the tiles hold every weight exactly once and zeros elsewhere; the kernel's lane map reads them back
    W2, WL = dr.unpack_diag(wt, DP, K, mode)
    if mode == 2:
        assert np.array_equal(WL[:, :D], w1)
    else:
        assert np.array_equal(W2[:, :D], w2)
        assert np.array_equal(WL[:, :D], w1 - (2.0 * w2) * (a - rmu[:D]))
    assert not W2[:, D:].any() and not WL[:, D:].any()


def test_packer_refuses_a_shape_without_a_path():
    a = np.zeros((200, 128))
    rc, *_ = ah.diag_pack(a, a - 1.0, a, 128, 1)
    assert rc == -1


def test_weights_are_zero_exactly_where_the_lds_formula_exceeds_the_limit():
    """estep_diag_mfma_weights against the restated LDS budget, every width, every K up to 300, all modes; and per width the
    largest K that still has a matrix-pipe path"""
    largest = {}
    for DP in (16, 32, 48, 64, 80, 96, 112, 128):
        NT = DP // 4
        for mode in (0, 1, 2):
            NTF = NT if mode == 2 else 2 * NT
            for K in range(1, 301):
                KT = (K + 3) // 4
                fits = dr.edm_lds_bytes(NT, NTF, KT, dr.edm_r(NT), K > 32) <= 150 * 1024
                got = ah.diag_weights(DP, K, mode)
                assert got == (KT * NTF * 16 if fits else 0), (DP, K, mode, got)
                if fits:
                    largest[(DP, mode)] = K
    assert ah.diag_weights(144, 4, 1) == 0 and ah.diag_weights(192, 4, 1) == 0 and ah.diag_weights(24, 4, 1) == 0
    assert ah.diag_weights(64, 0, 1) == 0
    print("largest K with a matrix-pipe path:", largest)
    # the slots of K > 32 cost KT R 256 doubles: two row groups per wave (DP <= 64) reach the limit sooner
    assert largest[(16, 1)] == largest[(16, 0)] and largest[(128, 2)] > largest[(128, 1)]
    for DP in (16, 32, 48, 64, 80, 96, 112, 128):
        assert largest[(DP, 1)] >= 32, "every width has the register instances"
        assert largest[(DP, 1)] % 4 == 0 or largest[(DP, 1)] == 300, "the budget is one of whole cluster tiles"


@pytest.mark.parametrize("DP,K,second", [(16, 1, 1), (48, 17, 0), (64, 33, 1), (64, 32, 1), (96, 50, 1), (112, 5, 0), (128, 130, 1), (192, 5, 1),
                                         (256, 40, 1), (320, 16, 0)])
def test_statistics_plan_equals_its_restatement(DP, K, second):
    got = ah.suffstat_diag_plan(DP, K, second)
    assert got == dr.stat_plan_ref(DP, K, second)


def test_statistics_plan_refuses_widths_without_an_instance():
    for DP in (8, 24, 144, 200):
        assert ah.suffstat_diag_plan(DP, 4, 1)["ok"] == 0


@pytest.mark.parametrize("DP,K,mode", [(16, 1, 1), (48, 5, 0), (80, 9, 2), (128, 64, 1), (128, 65, 1), (192, 3, 0), (256, 17, 1), (192, 65, 2)])
def test_valu_estep_plan_equals_its_restatement(DP, K, mode):
    for nrg in (1, 3, 4, 9):
        got = ah.estep_diag_plan(DP, K, mode, nrg, mfma=False)
        ref = dr.estep_plan_ref(DP, K, mode, nrg, mfma=False)
        assert {k: got[k] for k in ref} == ref


def test_exact_inputs_are_exact():
    """the exact inputs of the E-step and of the statistics give the same bits in any order of summation"""
    rng = np.random.default_rng(3)
    NP, D, DP, K = 128, 45, 48, 5
    X = dr.distinct_X(rng, NP, D, DP)
    for r0 in (0, 64):
        t = X[r0:r0 + 64, :D].reshape(-1)
        assert np.unique(t).size == t.size and np.array_equal(t, np.rint(t))
    for mode in (0, 1, 2):
        a, w2, w1 = dr.exact_diag_params(rng, K, D, mode)
        ctab = dr.exact_ctab(rng, 2, K)
        grp = rng.integers(0, 2, size=NP)
        P = dr.pad_params(a, w2, w1, DP)
        lq, S2, S1 = dr.diff_ref(X, P, ctab, grp, exact=True)
        assert np.abs(lq).max() < 2.0 ** 40 and np.array_equal(lq * 1024, np.rint(lq * 1024))
        p = rng.permutation(DP)
        lq2, _, _ = dr.diff_ref(X[:, p], P[:, :, p], ctab, grp, exact=True)
        assert np.array_equal(lq, lq2)
        mu = np.zeros(DP)
        mu[:D] = rng.integers(-2, 3, size=D) if mode != 2 else 0
        mu_, ck, wt = dr.pack_diag(a, w2, w1, DP, mode, mu=mu)
        W2, WL = dr.unpack_diag(wt, DP, K, mode)
        lqb, _, _ = dr.bilinear_ref(X, mu, ck, W2, WL, ctab, grp, exact=True)
        assert np.array_equal(lq, lqb), "the expansion around an integer centre is exact on exact inputs"
        lql, _, _ = dr.bilinear_ref(X, mu, ck, W2, WL, ctab, grp, exact=False)
        assert np.array_equal(lql.astype(np.float64), lq)
    q = hr.exact_q(rng, K, NP)
    rec = dr.stat_records_ref(X, q, 64, 2, 2, nstage=False, second=1)
    whole = dr.stat_records_ref(X, q, 128, 1, 1, nstage=True, second=1)
    assert np.array_equal(rec.sum(axis=(0, 1)), whole[0, 0]) and np.abs(whole).max() < 2.0 ** 40
    ld = dr.stat_records_ref(X, q, 64, 2, 2, nstage=False, second=1, dtype=hr.LD)
    assert np.array_equal(ld.astype(np.float64), rec)
    st = dr.stat_records_ref(X, q, 64, 2, 2, nstage=True, second=0)
    assert not st[:, 1, :, 0].any() and np.array_equal(st[:, 0, :, 0], rec[:, :, :, 0].sum(axis=1)) and not st[..., 1 + DP:].any()
