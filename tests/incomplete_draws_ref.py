"""What the tests of the draws for rows with holes share (lc_model_predict_incomplete_draws), numpy / scipy.

HoleComponent: one posterior and one hole pattern b by the DIRECT route of incomplete_ref.direct / incomplete_var_ref.direct_var
               -- the Cholesky factor of iW_aa, the expert M_k(x_a), the Schur complement S_k = iW_bb - iW_ba iW_aa^-1 iW_ab,
               eta = nu' + Da and the scale c_k h_k S_k -- vectorised over the rows of the pattern.  whiten() maps a draw
               labelled k to (x_b - M_k) over the lower Cholesky factor of that scale: what sample_ref.ks_whitened(_pooled) takes.
HoleMixture:   the components of a model (the prior one last) with their weights; responsibilities and whitening of a whole
               block of rows, pattern by pattern.
route():       the device's route for one (row, component) -- P = nu iW^-1, H = P_bb, u = (P y)_b -- for the identity test.
normals():     the normals of (row, draw) from the documented counters; inv_sqrt_g(): the scalar 1 / sqrt(G) every hole of a
               draw has to show.
The models of the tests (small, trained from the true labels so that eta is small) and their rows are built here as well,
so that the CPU tests run the statistics of the GPU tests at the GPU tests' sizes.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.special import gammaln

import lc_oracle as o
import sample_ref as sr

HOLES_MAX = 8


class HoleComponent:
    """one component's conditional Student-t of the holes b for many rows x_a: location M(x_a), scale c h(x_a) S, eta"""

    def __init__(self, nu, beta, m, iW, b):
        m, iW = np.asarray(m, dtype=np.float64), np.asarray(iW, dtype=np.float64)
        D = len(m)
        self.b = np.asarray(b, dtype=int)
        self.a = np.setdiff1d(np.arange(D), self.b)
        Da = self.a.size
        self.nu, self.beta = nu, beta
        self.nup = nu + 1 - D
        self.eta = self.nup + Da
        self.ma, self.mb = m[self.a], m[self.b]
        self.cf = cho_factor(iW[np.ix_(self.a, self.a)], lower=True)  # one factor of iW_aa
        Wab = iW[np.ix_(self.a, self.b)]
        self.B = cho_solve(self.cf, Wab)  # (Da, nb): M = m_b + (x_a - m_a) B
        self.S = iW[np.ix_(self.b, self.b)] - Wab.T @ self.B
        self.S = (self.S + self.S.T) / 2
        self.LS = np.linalg.cholesky(self.S)
        c = (1 + beta) / (beta * self.nup)  # the marginal of x_a: nu' degrees of freedom, shape c iW_aa
        self.c = c
        logdet = 2 * np.sum(np.log(np.diag(self.cf[0]))) + Da * np.log(c)
        self.logc = gammaln((self.nup + Da) / 2) - gammaln(self.nup / 2) - Da / 2 * np.log(self.nup * np.pi) - logdet / 2
        self.cqnu = (1 + beta) * nu / (2 * beta)
        H = nu * np.linalg.inv(self.S)  # = (P_k)_bb
        self.L = np.linalg.cholesky((H + H.T) / 2)

    def maha(self, Xa):  # (x_a - m_a)^T iW_aa^-1 (x_a - m_a)
        y = Xa - self.ma
        return np.einsum("na,na->n", y, cho_solve(self.cf, y.T).T)

    def log_marginal(self, Xa):
        return self.logc - 0.5 * self.eta * np.log1p(self.maha(Xa) / (self.c * self.nup))

    def location(self, Xa):
        return self.mb + (Xa - self.ma) @ self.B

    def h(self, Xa):  # 1 + s d_a^2 with d_a^2 = nu maha and s = beta / ((1 + beta) nu)
        return 1 + self.beta / (1 + self.beta) * self.maha(Xa)

    def factor(self, Xa):  # c_k h_k: the scale matrix is factor S
        return (1 + self.beta) / (self.beta * self.eta) * self.h(Xa)

    def whiten(self, Xa, x):
        """draws x (n, nb) of rows Xa (n, Da) -> whitened coordinates: t(eta) each, radius^2 / nb ~ F(nb, eta)"""
        w = np.linalg.solve(self.LS, (x - self.location(Xa)).T).T
        return w / np.sqrt(self.factor(Xa))[:, None]

    def draw(self, rng, Xa):
        """one draw per row on numpy's generators: the reference distribution itself"""
        n = Xa.shape[0]
        z = rng.standard_normal((n, self.b.size))
        return self.location(Xa) + (z @ self.LS.T) * np.sqrt(self.factor(Xa) * self.eta / rng.chisquare(self.eta, n))[:, None]

    def inv_sqrt_g(self, Xa, x, z):
        """L^T (x_b - M_k) / sqrt(cqnu h) over z, elementwise: 1 / sqrt(G) in every hole of a draw made as documented"""
        v = (x - self.location(Xa)) @ self.L  # (rows of) L^T (x_b - M_k)
        return v / np.sqrt(self.cqnu * self.h(Xa))[:, None] / z


def route(nu, beta, m, iW, x, b):
    """the device's route for one row x (its holes b filled with anything finite) -> S_k = nu (P_bb)^-1, M_k, h_k"""
    b = np.asarray(b, dtype=int)
    P = nu * np.linalg.inv(iW)
    P = (P + P.T) / 2
    L = np.linalg.cholesky(P[np.ix_(b, b)])
    y = x - m
    u = P[b] @ y
    w = cho_solve((L, True), u)
    d2a = y @ P @ y - u @ w
    Li = np.linalg.inv(L)
    return nu * Li.T @ Li, x[b] - w, 1 + beta / ((1 + beta) * nu) * d2a


class HoleMixture:
    """posts: [(nu, beta, m, iW)] with the prior component last when it has weight; weights: their E[pi]"""

    def __init__(self, posts, weights):
        self.posts, self.w = list(posts), np.asarray(weights, dtype=np.float64)
        self.Kp = len(self.posts)
        self._comp = {}

    def comp(self, k, pat):
        key = (k, tuple(int(c) for c in pat))
        if key not in self._comp:
            self._comp[key] = HoleComponent(*self.posts[k], key[1])
        return self._comp[key]

    @staticmethod
    def patterns(Xh):
        """{hole pattern: rows} of the rows with holes"""
        pats = {}
        for n in np.flatnonzero(np.isnan(Xh).any(axis=1)):
            pats.setdefault(tuple(np.flatnonzero(np.isnan(Xh[n]))), []).append(n)
        return {p: np.array(r) for p, r in pats.items()}

    def responsibilities(self, Xh):
        """r_k(x_a) per row, (N, Kp); NaN in rows without holes"""
        r = np.full((Xh.shape[0], self.Kp), np.nan)
        for pat, rows in self.patterns(Xh).items():
            a = self.comp(0, pat).a
            with np.errstate(divide="ignore"):
                t = np.stack([np.log(self.w[k]) + self.comp(k, pat).log_marginal(Xh[np.ix_(rows, a)]) for k in range(self.Kp)], axis=1)
            t -= t.max(axis=1, keepdims=True)
            e = np.exp(t)
            r[rows] = e / e.sum(axis=1, keepdims=True)
        return r

    def each(self, Xh, label):
        """yields (component, pattern, rows, draw indices, x_a) for every (pattern, component) that label names"""
        for pat, rows in self.patterns(Xh).items():
            lab = label[rows]
            for k in np.unique(lab):
                ri, di = np.nonzero(lab == k)
                c = self.comp(int(k), pat)
                yield c, pat, rows[ri], di, Xh[np.ix_(rows[ri], c.a)]

    def whitened_by_nb(self, Xh, draws, label):
        """{nb: [(whitened draws (n, nb), eta)]}: every draw whitened with the component its label names"""
        parts = {}  # (eta depends on the component and nb, not on the pattern: one part per (nb, eta))
        for c, pat, rows, di, Xa in self.each(Xh, label):
            parts.setdefault(len(pat), {}).setdefault(c.eta, []).append(c.whiten(Xa, draws[rows, di, : len(pat)]))
        return {nb: [(np.concatenate(w), eta) for eta, w in by_eta.items()] for nb, by_eta in parts.items()}

    def draw(self, rng, Xh, nd):
        """nd reference draws per row on numpy's generators -> draws (N, nd, HOLES_MAX), label (N, nd) (-1: no holes)"""
        N = Xh.shape[0]
        r = self.responsibilities(Xh)
        label = np.full((N, nd), -1, dtype=np.int32)
        holed = np.flatnonzero(~np.isnan(r[:, 0]))
        label[holed] = sr.choose(rng.random(holed.size * nd), np.repeat(r[holed], nd, axis=0))[0].reshape(-1, nd)
        draws = np.zeros((N, nd, HOLES_MAX))
        for c, pat, rows, di, Xa in self.each(Xh, label):
            draws[rows, di, : len(pat)] = c.draw(rng, Xa)
        return draws, label


def normals(seed, block, rows, draw, npairs):
    """z (n, 2 npairs) of (row, draw): tag 0x11, c2 = draw, sub = pair p -> z[2p], z[2p + 1]"""
    c0, c1 = sr.row_counters(block, rows)
    z = np.zeros((len(rows), 2 * npairs))
    for p in range(npairs):
        z[:, 2 * p], z[:, 2 * p + 1] = sr.box_muller(sr.philox4x32_10(c0, c1, draw, sr.TAG_NORMAL | (p << 8), seed & 0xFFFFFFFF, seed >> 32))
    return z


# ---- the models of the tests and their rows -----------------------------------------------------------------------------------
STICK, DIRICHLET = "stickbreak", "dirichlet"
MODELS = {  # name: (weights, D, rows per training cluster, cluster prior, offset)
    "d2_stick": (STICK, 2, [5, 8, 11], 1.0, 0.0),       # one hole, one known; the prior component has nu' = 1
    "d5_dir": (DIRICHLET, 5, [5, 9, 7], 1.0, 0.0),
    "d5_k1": (DIRICHLET, 5, [9], 1.0, 0.0),             # Kp = 1
    "d23_stick": (STICK, 23, [5, 8, 12], 2.5, 0.0),
    "d23_offset": (STICK, 23, [5, 8, 12], 2.5, 1e3),    # 1e3 from the origin
    "d64_k34_stick": (STICK, 64, [6] * 34, 1.0, 0.0),   # Kp = 35 with the prior component
    "d5_k69_stick": (STICK, 5, [4, 5, 6] * 23, 1.0, 0.0),  # Kp = 70: two chunks of 64 clusters
    "d200_stick": (STICK, 200, [5, 8, 12], 1.0, 0.0),   # several 64-column steps
}


def centres(D, K):
    c = np.zeros((K, D))
    for k in range(K):
        c[k, k % D] = 12.0 * (1 + k // D)
        c[k, (k + 1) % D] -= 7.0 * k
    return c


def training(name):
    """-> (X, q, centres): the training rows of a model and the responsibilities its fit starts from (the true labels)"""
    _, D, sizes, _, offset = MODELS[name]
    rng = np.random.default_rng(4161 + D + len(sizes))
    K = len(sizes)
    cen = centres(D, K) + offset
    z = np.repeat(np.arange(K), sizes)
    X = cen[z] + rng.normal(size=(z.size, D))
    q = np.ones((z.size, 1))
    if K > 1:
        q = np.full((z.size, K), 0.02 / (K - 1))
        q[np.arange(z.size), z] = 0.98
    return X, q, cen


def expected_weights(w):
    """E[pi_k], E[pi_rest] from the oracle's weight object"""
    if isinstance(w, o.Dirichlet):
        return w.alpha / w.alpha.sum(), 0.0
    Epi, rest = np.zeros(w.alpha1.size), 1.0
    for i, k in enumerate(w.order):
        if isinstance(w, o.GDirichlet) and i == len(w.order) - 1:
            Epi[k], rest = rest, 0.0
            break
        Epi[k] = w.alpha1[k] / (w.alpha1[k] + w.alpha2[k]) * rest
        rest *= w.alpha2[k] / (w.alpha1[k] + w.alpha2[k])
    return Epi, rest


def mixture(posts, prior, Epi, rest):
    """HoleMixture of K posteriors and, when it has weight, the cluster prior"""
    posts, w = list(posts), list(Epi)
    if rest > 0:
        posts.append(prior)
        w.append(rest)
    return HoleMixture(posts, w)


def host_mixture(name):
    """the model of `name` after ONE update from the true labels by the oracle's own classes: what the CPU tests draw from
    (the GPU tests take the posteriors of the model the device fitted in six iterations: the same family and sizes)"""
    wk, D, sizes, cp, _ = MODELS[name]
    X, q, _ = training(name)
    posts = []
    for k in range(len(sizes)):
        g = o.GaussWish(cp, D)
        g.addobs(q[:, k], X)
        g.update()
        posts.append((g.nu, g.beta, g.m, g.iW))
    w = o.StickBreak() if wk == STICK else o.Dirichlet()
    w.update(q.sum(axis=0))
    pr = o.GaussWish(cp, D)
    return mixture(posts, (pr.nu, pr.beta, pr.m, pr.iW), *expected_weights(w))


def rows(name, rng, n, far_share=0.0):
    """held-out full rows: rows of the training mixture at twice its spread, 30 % of them pulled half way to another
    cluster, far_share of them far out (where the prior component of StickBreak weights takes over)"""
    _, D, sizes, _, offset = MODELS[name]
    K = len(sizes)
    cen = centres(D, K) + offset
    z = rng.integers(0, K, n)
    X = cen[z] + rng.normal(size=(n, D)) * 2.0
    half = rng.random(n) < 0.3
    X[half] = 0.5 * (X[half] + cen[(z[half] + 1) % K])
    far = rng.random(n) < far_share
    X[far] = cen[z[far]] + rng.normal(size=(int(far.sum()), D)) * 25.0
    return X


def punch(rng, X, npat=40, complete_share=1 / 3, nbs=None):
    """a copy of X with NaNs: about complete_share of the rows stay complete, every other row takes one of npat patterns
    (few patterns: the reference factors iW_aa once per pattern and component); the patterns cycle through the hole counts
    nbs (default 1 ... min(HOLES_MAX, D - 1)), the first has the most holes, the second holds column 0, the third D - 1"""
    N, D = X.shape
    nbs = list(nbs) if nbs is not None else list(range(min(HOLES_MAX, D - 1), 0, -1))
    pats = []
    for i in range(npat):
        cols = rng.choice(D, nbs[i % len(nbs)], replace=False)
        if i == 1 and 0 not in cols:
            cols[0] = 0
        if i == 2 and D - 1 not in cols:
            cols[0] = D - 1
        pats.append(np.sort(cols))
    Xh = X.copy()
    for n in range(N):
        if n >= npat and rng.random() < complete_share:
            continue
        Xh[n, pats[n if n < npat else int(rng.integers(0, npat))]] = np.nan
    return Xh


CASES = {  # name: (model, rows, draws per row, share of far rows, hole counts of the patterns or None for all)
    "d2": ("d2_stick", 3000, 4, 0.1, None),                    # D = 2: one hole, one known
    "d5_k1": ("d5_k1", 2000, 1, 0.0, None),                    # K = 1
    "d23_prior": ("d23_stick", 3000, 5, 0.15, None),           # the StickBreak prior component (nu' = 1) is drawn from
    "d64_kp35_m64": ("d64_k34_stick", 1000, 64, 0.05, None),   # Kp = 35, every lane draws
    "d5_kp70": ("d5_k69_stick", 2000, 3, 0.05, None),          # two chunks of clusters
    "d200_nb8_m1": ("d200_stick", 1000, 1, 0.0, [8]),          # several 64-column steps, one draw
    "d23_offset": ("d23_offset", 2000, 3, 0.05, None),         # 1e3 from the origin
}
CASE_SEED = (11 << 32) + 5


def case_rows(case):
    """the rows with holes of a case: the same on every call"""
    name, n, _, far_share, nbs = CASES[case]
    rng = np.random.default_rng(4160 + n + len(case))
    return punch(rng, rows(name, rng, n, far_share), nbs=nbs)


def four_rows(mix, name):
    """the four (pattern, x_a) rows of the distribution test at D = 5, patterns of 1, 2, 3 and 4 holes: near a cluster, two
    between clusters (where, by the reference, the second largest r_k is largest on the segment between two centres), one
    far out"""
    _, D, sizes, _, offset = MODELS[name]
    cen = centres(D, len(sizes)) + offset
    pats = [[2], [0, 3], [1, 2, 4], [0, 1, 3, 4]]

    def between(a, b, pat):
        line = np.array([(1 - t) * cen[a] + t * cen[b] for t in np.linspace(0.0, 1.0, 2001)])
        line[:, pat] = np.nan
        return line[np.argmax(np.sort(mix.responsibilities(line), axis=1)[:, -2])]

    X = np.array([cen[0] + 0.3, between(0, 1, pats[1]), between(1, 2, pats[2]), cen[2] + 9.0])
    for i, p in enumerate(pats):
        X[i, p] = np.nan
    return X
