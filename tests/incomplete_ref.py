"""References for the prediction of rows with holes (lc_model_predict_incomplete), numpy / scipy only.

direct():  per row the Student-t marginal of its observed columns (scipy's multivariate_t) and the linear expert
           m_b + iW_ba iW_aa^-1 (x_a - m_a) of every cluster, mixed by the responsibilities -- the reference of the tests.
emulate(): the route the device takes -- fill the holes, the full-width distance, the rank-nb correction with
           P = nu iW^-1 and one 8 x 8 Cholesky padded with the identity -- in numpy.  tests/test_incomplete_host.py holds it
           against direct(); the d23_offset case of tests/test_gpu_incomplete.py takes its bar from the gap between the two.
"""
import numpy as np
from scipy import stats
from scipy.special import gammaln, logsumexp

HOLES_MAX = 8


def random_posterior(rng, D, offset=0.0):
    """a random posterior (nu, beta, m, iW) of a cluster that saw about 3 D observations"""
    n = 3 * D + 5
    Y = rng.normal(size=(n, D)) @ rng.normal(size=(D, D)) / np.sqrt(D) + rng.normal(0, 3, D) + offset
    iW = D * np.eye(D) + (Y - Y.mean(0)).T @ (Y - Y.mean(0))
    return float(D + n), 1.0 + n, Y.mean(0), (iW + iW.T) / 2


def make_holes(rng, X, complete_share=1 / 3, max_holes=HOLES_MAX):
    """a copy of X with NaNs: about complete_share of the rows stay complete, the others get 1 ... min(max_holes, D - 1)
    holes; row 0 has exactly min(max_holes, D - 1) holes, row 1 a hole in column 0, row 2 a hole in column D - 1"""
    N, D = X.shape
    top = min(max_holes, D - 1)
    Xh = X.copy()
    for n in range(N):
        if n > 2 and rng.random() < complete_share:
            continue
        nb = top if n == 0 else int(rng.integers(1, top + 1))
        cols = rng.choice(D, nb, replace=False)
        if n == 1 and 0 not in cols:
            cols[0] = 0
        if n == 2 and D - 1 not in cols:
            cols[0] = D - 1
        Xh[n, cols] = np.nan
    return Xh


def _components(cls, prior, Epi, rest):
    comps = [(np.log(Epi[k]), c) for k, c in enumerate(cls)]
    if rest > 0:
        comps.append((np.log(rest), prior))
    return comps


def direct(Xh, cls, prior, Epi, rest):
    """-> rows (N, D) completed, logp (N,), largest responsibility (N,), S_n (N,) = max_k |M_k(x_n)_b| (1 without holes)"""
    N, D = Xh.shape
    comps = _components(cls, prior, Epi, rest)
    rows, logp, rmax, S = Xh.copy(), np.zeros(N), np.zeros(N), np.ones(N)
    patterns = {}  # the rows of one hole pattern are scored together (most patterns have one row)
    for n in range(N):
        patterns.setdefault(tuple(np.flatnonzero(np.isnan(Xh[n]))), []).append(n)
    for pat, members in patterns.items():
        b, idx = np.array(pat, dtype=int), np.array(members)
        a = np.setdiff1d(np.arange(D), b)
        Xa = Xh[np.ix_(idx, a)]
        T, M = [], []
        for lw, (nu, beta, mm, iW) in comps:
            nup = nu + 1 - D
            Saa = iW[np.ix_(a, a)]
            lp = stats.multivariate_t(loc=mm[a], shape=(1 + beta) / (beta * nup) * Saa, df=nup).logpdf(Xa)
            T.append(lw + np.asarray(lp).reshape(-1))
            if b.size:
                M.append(mm[b] + (Xa - mm[a]) @ np.linalg.solve(Saa, iW[np.ix_(a, b)]))
        T = np.stack(T, axis=1)  # (n, Kp)
        logp[idx] = logsumexp(T, axis=1)
        r = np.exp(T - logp[idx][:, None])
        rmax[idx] = r.max(axis=1)
        if b.size:
            M = np.stack(M, axis=1)  # (n, Kp, nb)
            rows[np.ix_(idx, b)] = np.einsum("nk,nkb->nb", r, M)
            S[idx] = np.abs(M).max(axis=(1, 2))
    return rows, logp, rmax, S


def tables(nu, beta, iW):
    """P, G[nb], s, e[nb] of one posterior by the formulas of the header (lc_gw_precision), in numpy"""
    D = iW.shape[0]
    nup = nu + 1 - D
    P = nu * np.linalg.inv(iW)
    P = (P + P.T) / 2
    logdet = np.linalg.slogdet(iW)[1]
    nb = np.arange(HOLES_MAX + 1)
    Da = D - nb
    e = (nup + Da) / 2
    with np.errstate(invalid="ignore"):
        G = gammaln(e) - gammaln(nup / 2) - Da / 2 * np.log(nup * np.pi) + 0.5 * (
            Da * np.log(nup * beta / (1 + beta)) - (logdet - nb * np.log(nu)))
    G[Da < 0] = np.nan
    return P, G, beta / ((1 + beta) * nu), e


def fill_value(cls, Nk):
    """the N_k-weighted mean of the cluster means"""
    w = np.asarray(Nk, dtype=float)
    w = w / w.sum() if w.sum() > 0 else np.full(len(cls), 1.0 / len(cls))
    return sum(wk * c[2] for wk, c in zip(w, cls))


def emulate(Xh, cls, prior, Epi, rest, fill):
    """the device's route in numpy -> rows (N, D), logp (N,)"""
    N, D = Xh.shape
    comps = _components(cls, prior, Epi, rest)
    tabs = [tables(nu, beta, iW) for _, (nu, beta, _, iW) in comps]
    chol = [np.linalg.cholesky(iW) for _, (_, _, _, iW) in comps]
    rows, logp = Xh.copy(), np.zeros(N)
    for n in range(N):
        b = np.flatnonzero(np.isnan(Xh[n]))
        nb = b.size
        x = Xh[n].copy()
        x[b] = fill[b]
        t, M = [], []
        for (lw, (nu, beta, mm, iW)), (P, G, s, e), Lc in zip(comps, tabs, chol):
            y = x - mm
            d2 = nu * np.sum(np.linalg.solve(Lc, y) ** 2)  # ||A y||^2 with the whitener A = sqrt(nu) chol(iW)^-1
            H, u = np.eye(HOLES_MAX), np.zeros(HOLES_MAX)
            H[:nb, :nb] = P[np.ix_(b, b)]
            u[:nb] = P[b] @ y
            L = np.linalg.cholesky(H)
            z = np.linalg.solve(L, u)
            w = np.linalg.solve(L.T, z)
            d2a = max(d2 - z @ z, 0.0)
            t.append(lw + G[nb] - np.log(np.prod(np.diag(L))) - e[nb] * np.log1p(s * d2a))
            M.append(x[b] - w[:nb])
        t = np.array(t)
        logp[n] = logsumexp(t)
        if nb:
            rows[n, b] = np.exp(t - logp[n]) @ np.array(M)
    return rows, logp
