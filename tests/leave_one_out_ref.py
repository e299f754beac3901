"""References for the leave-one-out conditionals (lc_model_predict_leave_one_out), numpy / scipy only.  A
helper of tests/test_leave_one_out_host.py, tests/test_gpu_loo_kernels.py and tests/test_gpu_leave_one_out.py, not a test.

loo_direct():  the (N D, D) array with one NaN per row through incomplete_ref.direct (scipy's multivariate_t marginal and the
               linear expert on iW, rows grouped by hole pattern: D solves per component) and the variance on iW as
               incomplete_var_ref.direct_var forms it -- by direct_var itself up to D = 23, by the same arithmetic grouped
               by pattern beyond (direct_var factors iW_aa once per row and component; the host test holds the two
               against each other).
loo_emulate(): the route the device takes -- the full-width distance, v = P (x - m), the scalar correction v_d^2 / P_dd,
               the between term from the deviations from x_d -- in numpy.  fill: None forms x - m_k per cluster, a vector c
               centres x on it once and starts from -P_k (m_k - c) (both are routes DESIGN 4.17 allows).
"""
from typing import NamedTuple

import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.special import gammaln, logsumexp

import incomplete_ref as ref
import incomplete_var_ref as vref


class Loo(NamedTuple):
    logp: np.ndarray   # (N,) log p(x)
    rest: np.ndarray   # (N, D) log p(x_-d)
    cond: np.ndarray   # (N, D) logp - rest
    mean: np.ndarray   # (N, D)
    var: np.ndarray    # (N, D), or None
    rmax: np.ndarray   # (N, D) largest responsibility of the (row, column) pair, or None
    S: np.ndarray      # (N, D) max_k |M_k,d|: the scale of the bar on mean, or None
    V: np.ndarray      # (N, D) max_k [Cov_k,d + (M_k,d - mean_d)^2]: the scale of the bar on var, or None


def one_hole_rows(X):
    """(N D, D): row n D + d is row n with a NaN in column d"""
    N, D = X.shape
    Xh = np.repeat(X, D, axis=0)
    Xh[np.arange(N * D), np.tile(np.arange(D), N)] = np.nan
    return Xh


def var_by_column(X, cls, prior, Epi, rest):
    """direct_var's arithmetic for the one-hole patterns, one Cholesky factor of iW_aa per (column, component) -> var (N, D),
    V (N, D)"""
    N, D = X.shape
    comps = ref._components(cls, prior, Epi, rest)
    var, V = np.zeros((N, D)), np.zeros((N, D))
    for d in range(D):
        a = np.setdiff1d(np.arange(D), [d])
        T, M, C = [], [], []
        for lw, (nu, beta, mm, iW) in comps:
            nup, Da = nu + 1 - D, D - 1
            Sab = iW[a, d]
            cf = cho_factor(iW[np.ix_(a, a)], lower=True)
            sol = cho_solve(cf, Sab)
            Ya = X[:, a] - mm[a]
            q = np.einsum("na,an->n", Ya, cho_solve(cf, Ya.T))
            c = (1 + beta) / (beta * nup)
            logdet = 2 * np.sum(np.log(np.diag(cf[0]))) + Da * np.log(c)
            T.append(lw + gammaln((nup + Da) / 2) - gammaln(nup / 2) - Da / 2 * np.log(nup * np.pi) - logdet / 2
                     - (nup + Da) / 2 * np.log1p(q / (c * nup)))
            M.append(mm[d] + Ya @ sol)
            schur = iW[d, d] - Sab @ sol
            g = (1 + beta) / (beta * (nup + Da - 2))
            C.append(g * (1 + beta / (1 + beta) * q) * schur)
        T, M, C = np.stack(T, 1), np.stack(M, 1), np.stack(C, 1)  # (N, Kp)
        r = np.exp(T - logsumexp(T, axis=1)[:, None])
        mean = np.sum(r * M, axis=1)
        dev = (M - mean[:, None]) ** 2
        var[:, d] = np.sum(r * (C + dev), axis=1)
        V[:, d] = (C + dev).max(axis=1)
    return var, V


def loo_direct(X, cls, prior, Epi, rest, variance=True):
    N, D = X.shape
    Xh = one_hole_rows(X)
    rows, lrest, rmax, S = ref.direct(Xh, cls, prior, Epi, rest)
    logp = ref.direct(X, cls, prior, Epi, rest)[1]
    mean = rows[np.arange(N * D), np.tile(np.arange(D), N)].reshape(N, D)
    lrest = lrest.reshape(N, D)
    var = V = None
    if variance:
        if D <= 23:
            v, Vn, _, _ = vref.direct_var(Xh, cls, prior, Epi, rest)
            var, V = v[:, 0].reshape(N, D), Vn.reshape(N, D)
        else:
            var, V = var_by_column(X, cls, prior, Epi, rest)
    return Loo(logp, lrest, logp[:, None] - lrest, mean, var, rmax.reshape(N, D), S.reshape(N, D), V)


def loo_tables(cls, prior, Epi, rest):
    """per component: (log weight, nu, m, P, G(0), G(1), s, e(0), e(1), g(1) nu, chol(iW))"""
    out = []
    for lw, (nu, beta, mm, iW) in ref._components(cls, prior, Epi, rest):
        P, G, s, e = ref.tables(nu, beta, iW)
        g1 = vref.g_table(nu, beta, iW.shape[0])[1] * nu
        out.append((lw, nu, mm, P, G[0], G[1], s, e[0], e[1], g1, np.linalg.cholesky(iW)))
    return out


def loo_emulate(X, cls, prior, Epi, rest, fill=None, variance=True):
    """the device's route in numpy -> Loo (rmax, S, V None)"""
    N, D = X.shape
    tabs = loo_tables(cls, prior, Epi, rest)
    T0, T1, DL, CV = [], [], [], []
    for lw, nu, mm, P, G0, G1, s, e0, e1, g1, Lc in tabs:
        Y = X - mm
        d2 = nu * np.sum(np.linalg.solve(Lc, Y.T) ** 2, axis=0)  # ||A y||^2 with the whitener A = sqrt(nu) chol(iW)^-1
        Vk = Y @ P if fill is None else (X - fill) @ P - (mm - fill) @ P
        pd = np.diag(P)
        d2a = np.maximum(d2[:, None] - Vk ** 2 / pd, 0.0)
        T0.append(lw + G0 - e0 * np.log1p(s * d2))
        T1.append(lw + G1 - 0.5 * np.log(pd) - e1 * np.log1p(s * d2a))
        DL.append(-Vk / pd)
        CV.append(g1 * (1 + s * d2a) / pd)
    logp = logsumexp(np.stack(T0, 1), axis=1)
    T1, DL, CV = np.stack(T1, 1), np.stack(DL, 1), np.stack(CV, 1)  # (N, Kp, D)
    lrest = logsumexp(T1, axis=1)
    r = np.exp(T1 - lrest[:, None, :])
    dm = np.sum(r * DL, axis=1)
    var = None
    if variance:
        var = np.sum(r * (np.where(r > 0, CV, 0.0) + DL ** 2), axis=1) - dm ** 2
    return Loo(logp, lrest, logp[:, None] - lrest, X + dm, var, None, None, None)


def bars(want):
    """the project's bars of DESIGN 4.15 / 4.15.1 per (row, column): (cond, mean, var) absolute tolerances at unit factor"""
    cb = np.maximum(np.abs(want.logp)[:, None], np.abs(want.rest))
    return cb, want.S, want.V
