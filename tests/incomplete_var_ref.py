"""References for the predictive variance of filled values (lc_model_predict_incomplete_var), numpy / scipy.

direct_var():  per row, on iW itself (one Cholesky factor of iW_aa per component): the Student-t marginal of the known
               columns, the linear expert and the diagonal of the conditional covariance
               g (1 + s d_a^2) diag(iW_bb - iW_ba iW_aa^-1 iW_ab) of every component, then the
               mixture's variance CENTRED on its mean, var = sum_k r_k [Cov_k,ii + (M_k,i - mean_i)^2] -- the reference
               of the tests.
emulate_var(): the route the device takes -- the identity-padded 8 x 8 Cholesky of H = P_bb, diag(H^-1) from L^-1, the
               between term from the deviations from the fill value -- in numpy.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.special import gammaln, logsumexp

import incomplete_ref as ref

HOLES_MAX = ref.HOLES_MAX


def g_table(nu, beta, D):
    """g[nb] = (1 + beta) / (beta (nu - 1 - nb)) for nb = 0 ... HOLES_MAX; NaN where nb >= D or nu - 1 - nb <= 0"""
    nb = np.arange(HOLES_MAX + 1)
    dof2 = nu - 1.0 - nb
    g = np.full(HOLES_MAX + 1, np.nan)
    ok = (nb < D) & (dof2 > 0)
    g[ok] = (1 + beta) / (beta * dof2[ok])
    return g


def direct_var(Xh, cls, prior, Epi, rest):
    """-> var (N, HOLES_MAX) in the order of the row's holes, ascending (0 beyond them), V_n (N,) =
    max_{k,i} [Cov_k,ii + (M_k,i - mean_i)^2] (1 without holes), share (N,) = the largest share of the between term in var
    over the row's holes (0 without holes), logp (N,) = log p(x_known) of the rows with holes (NaN without), which
    tests/test_incomplete_var_host.py holds against incomplete_ref.direct's (scipy's multivariate_t)"""
    N, D = Xh.shape
    comps = ref._components(cls, prior, Epi, rest)
    var, Vn, share, logp = np.zeros((N, HOLES_MAX)), np.ones(N), np.zeros(N), np.full(N, np.nan)
    for n in range(N):
        b = np.flatnonzero(np.isnan(Xh[n]))
        if not b.size:
            continue
        a = np.setdiff1d(np.arange(D), b)
        xa = Xh[n, a]
        T, M, V = [], [], []
        for lw, (nu, beta, mm, iW) in comps:
            nup = nu + 1 - D
            Da = a.size
            Sab = iW[np.ix_(a, b)]
            cf = cho_factor(iW[np.ix_(a, a)], lower=True)  # one factor of iW_aa per (row, component)
            sol = cho_solve(cf, Sab)
            ya = xa - mm[a]
            q = ya @ cho_solve(cf, ya)  # (x_a - m_a)^T iW_aa^-1 (x_a - m_a)
            c = (1 + beta) / (beta * nup)  # the Student-t marginal of x_a: nu' degrees of freedom, shape c iW_aa
            logdet = 2 * np.sum(np.log(np.diag(cf[0]))) + Da * np.log(c)
            T.append(lw + gammaln((nup + Da) / 2) - gammaln(nup / 2) - Da / 2 * np.log(nup * np.pi) - logdet / 2
                     - (nup + Da) / 2 * np.log1p(q / (c * nup)))
            M.append(mm[b] + ya @ sol)
            schur = np.diag(iW[np.ix_(b, b)]) - np.einsum("ab,ab->b", Sab, sol)
            g = (1 + beta) / (beta * (nup + Da - 2))
            V.append(g * (1 + beta / ((1 + beta) * nu) * nu * q) * schur)
        T, M, V = np.array(T), np.array(M), np.array(V)  # (Kp,), (Kp, nb), (Kp, nb)
        logp[n] = logsumexp(T)
        r = np.exp(T - logp[n])
        mean = r @ M
        dev = (M - mean) ** 2
        within, between = r @ V, r @ dev
        var[n, : b.size] = within + between
        Vn[n] = (V + dev).max()
        share[n] = (between / (within + between)).max()
    return var, Vn, share, logp


def emulate_var(Xh, cls, prior, Epi, rest, fill):
    """the device's route in numpy -> var (N, HOLES_MAX)"""
    N, D = Xh.shape
    comps = ref._components(cls, prior, Epi, rest)
    tabs = [ref.tables(nu, beta, iW) for _, (nu, beta, _, iW) in comps]
    gtab = [g_table(nu, beta, D) * nu for _, (nu, beta, _, _) in comps]
    chol = [np.linalg.cholesky(iW) for _, (_, _, _, iW) in comps]
    var = np.zeros((N, HOLES_MAX))
    for n in range(N):
        b = np.flatnonzero(np.isnan(Xh[n]))
        nb = b.size
        if not nb:
            continue
        x = Xh[n].copy()
        x[b] = fill[b]
        t, W, C = [], [], []
        for (lw, (nu, beta, mm, iW)), (P, G, s, e), gn, Lc in zip(comps, tabs, gtab, chol):
            y = x - mm
            d2 = nu * np.sum(np.linalg.solve(Lc, y) ** 2)
            H, u = np.eye(HOLES_MAX), np.zeros(HOLES_MAX)
            H[:nb, :nb] = P[np.ix_(b, b)]
            u[:nb] = P[b] @ y
            L = np.linalg.cholesky(H)
            z = np.linalg.solve(L, u)
            w = np.linalg.solve(L.T, z)
            d2a = max(d2 - z @ z, 0.0)
            t.append(lw + G[nb] - np.log(np.prod(np.diag(L))) - e[nb] * np.log1p(s * d2a))
            Li = np.linalg.solve(L, np.eye(HOLES_MAX))
            hd = np.sum(Li ** 2, axis=0)  # (H^-1)_ii = ||L^-1 e_i||^2
            W.append(w[:nb])
            C.append(gn[nb] * (1 + s * d2a) * hd[:nb])
        t, W, C = np.array(t), np.array(W), np.array(C)
        r = np.exp(t - logsumexp(t))
        rw = r @ W  # fill - mean
        var[n, :nb] = r @ (C + W ** 2) - rw ** 2
    return var
