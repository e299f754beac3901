"""Reference of the conditional prediction with variance, numpy / scipy on the posteriors.

Per component (the K clusters and, for a weight distribution with a rest, the cluster prior): the Student-t marginal of the
given columns, the linear expert M_k(x_a) = m_b + iW_ba iW_aa^-1 (x_a - m_a) and the diagonal of the conditional covariance
g (1 + s d^2) diag(iW_bb - iW_ba iW_aa^-1 iW_ab); then the mixture's variance CENTRED on its mean,
    var = sum_k r_k [Cov_k,tt + (M_k,t - mean_t)^2] = within + between.
reference_mp states the same in mpmath at 50 digits (for the offset case, where float64 itself has to be measured)."""
import numpy as np
from scipy import stats
from scipy.special import logsumexp


def components(cls, prior, Epi, rest):
    """[(log weight, (nu, beta, m, iW))] of the components that take part"""
    comps = [(np.log(Epi[k]), c) for k, c in enumerate(cls)]
    if rest > 0:
        comps.append((np.log(rest), prior))
    return comps


def cluster_tables(nu, beta, mm, iW, given, target, D):
    """-> solve = iW_aa^-1 iW_ab (Da, Db), diag of the Schur complement (Db,), g, s"""
    Da = len(given)
    Saa, Sab, Sbb = iW[np.ix_(given, given)], iW[np.ix_(given, target)], iW[np.ix_(target, target)]
    sol = np.linalg.solve(Saa, Sab)
    schur = np.diag(Sbb) - np.einsum("ab,ab->b", Sab, sol)
    nup = nu + 1 - D
    return sol, schur, (1 + beta) / (beta * (nup + Da - 2)), beta / ((1 + beta) * nu)


def reference(Xa, given, target, D, cls, prior, Epi, rest):
    """-> mean (N, Db), var (N, Db), logp (N,), r (N, Kp), within (N, Db), between (N, Db), V_n (N,) with
    V_n = max_{k,b} [Cov_k,bb(x_n) + (M_k,b - mean_b)^2]"""
    T, M, V = [], [], []
    for lw, (nu, beta, mm, iW) in components(cls, prior, Epi, rest):
        nup = nu + 1 - D
        Saa = iW[np.ix_(given, given)]
        lp = stats.multivariate_t(loc=mm[given], shape=(1 + beta) / (beta * nup) * Saa, df=nup).logpdf(Xa)
        T.append(lw + np.asarray(lp).reshape(-1))
        sol, schur, g, s = cluster_tables(nu, beta, mm, iW, given, target, D)
        ya = Xa - mm[given]
        M.append(mm[target] + ya @ sol)
        d2 = nu * np.einsum("na,na->n", ya, np.linalg.solve(Saa, ya.T).T)
        V.append(g * (1 + s * d2)[:, None] * schur[None, :])
    T, M, V = np.stack(T, axis=1), np.stack(M, axis=1), np.stack(V, axis=1)  # (N, Kp), (N, Kp, Db), (N, Kp, Db)
    logp = logsumexp(T, axis=1)
    r = np.exp(T - logp[:, None])
    mean = np.einsum("nk,nkb->nb", r, M)
    dev = (M - mean[:, None, :]) ** 2
    within = np.einsum("nk,nkb->nb", r, V)
    between = np.einsum("nk,nkb->nb", r, dev)
    return mean, within + between, logp, r, within, between, (V + dev).max(axis=(1, 2))


def reference_mp(Xa, given, target, D, cls, prior, Epi, rest, dps=50):
    """var (N, Db) of reference(), every step in mpmath at `dps` digits from the same float64 inputs, rounded at the end"""
    import mpmath as mp

    with mp.workdps(dps):
        f = mp.mpf
        Da, Db, N = len(given), len(target), Xa.shape[0]
        tabs = []
        for lw_w, (nu, beta, mm, iW) in [(w, c) for w, c in zip(list(Epi) + [rest], list(cls) + [prior]) if w > 0]:
            nu, beta = f(float(nu)), f(float(beta))
            nup = nu + 1 - D
            Saa = mp.matrix([[f(float(iW[a, c])) for c in given] for a in given])
            Sab = mp.matrix([[f(float(iW[a, t])) for t in target] for a in given])
            Pin = Saa ** -1
            sol = Pin * Sab
            schur = [f(float(iW[t, t])) - sum(Sab[a, i] * sol[a, i] for a in range(Da)) for i, t in enumerate(target)]
            c = (1 + beta) / (beta * nup)
            G = (mp.loggamma((nup + Da) / 2) - mp.loggamma(nup / 2) - f(Da) / 2 * mp.log(nup * mp.pi)
                 - (Da * mp.log(c) + mp.log(mp.det(Saa))) / 2)
            tabs.append((mp.log(f(float(lw_w))) + G, (nup + Da) / 2, beta / (1 + beta), (1 + beta) / (beta * (nup + Da - 2)),
                         [f(float(mm[a])) for a in given], [f(float(mm[t])) for t in target], Pin, sol, schur))
        out = np.zeros((N, Db))
        for n in range(N):
            xa = [f(float(v)) for v in Xa[n]]
            T, M, V = [], [], []
            for tl, e, sq, g, ma, mb, Pin, sol, schur in tabs:
                y = [xa[a] - ma[a] for a in range(Da)]
                Py = [sum(Pin[a, c] * y[c] for c in range(Da)) for a in range(Da)]
                u = 1 + sq * sum(y[a] * Py[a] for a in range(Da))  # 1 + s d^2
                T.append(tl - e * mp.log(u))
                M.append([mb[i] + sum(y[a] * sol[a, i] for a in range(Da)) for i in range(Db)])
                V.append([g * u * schur[i] for i in range(Db)])
            top = max(T)
            w = [mp.exp(t - top) for t in T]
            tot = sum(w)
            r = [v / tot for v in w]
            for i in range(Db):
                mean = sum(rk * Mk[i] for rk, Mk in zip(r, M))
                out[n, i] = float(sum(rk * (Vk[i] + (Mk[i] - mean) ** 2) for rk, Mk, Vk in zip(r, M, V)))
        return out
