"""What the tests of the samplers share: a numpy restatement of Philox-4x32-10 and of the counter table in
include/libcluster_hip.h, reference samplers on numpy's own generators (from the formulas of the header, nothing from the
device), and the statistical checks with their bar.

The bar: every Kolmogorov-Smirnov p-value >= P_BAR = 1e-4 on >= 50 000 draws per tested component, label frequencies within
5 binomial standard errors."""
import numpy as np
from scipy import stats

P_BAR = 1e-4
MASK = np.uint64(0xFFFFFFFF)
TAG_CHOICE, TAG_NORMAL = 0x10, 0x11


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox-4x32-10 on arrays (or scalars) of 32-bit words -> four uint64 arrays holding 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & MASK, (p0 >> s32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def u01(a, b):
    """the 53-bit uniform in (0, 1) of two output words"""
    v = ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) | np.asarray(b, dtype=np.uint64)) >> np.uint64(11)
    return (v.astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def box_muller(o):
    u1, u2 = u01(o[0], o[1]), u01(o[2], o[3])
    rad = np.sqrt(-2.0 * np.log(u1))
    return rad * np.cos(6.283185307179586476925 * u2), rad * np.sin(6.283185307179586476925 * u2)


def row_counters(block, rows, row_offset=0):
    """(c0, c1) of g = (block << 40) + row_offset + row for the rows of one block"""
    g = (np.uint64(block) << np.uint64(40)) + np.uint64(row_offset) + np.asarray(rows, dtype=np.uint64)
    return g & MASK, g >> np.uint64(32)


def choice_u(seed, block, rows, draw=0, row_offset=0):
    """the uniform of the component choice of (row, draw): tag 0x10, c2 = draw"""
    c0, c1 = row_counters(block, rows, row_offset)
    o = philox4x32_10(c0, c1, draw, TAG_CHOICE, seed & 0xFFFFFFFF, seed >> 32)
    return u01(o[0], o[1])


def choose(u, weights):
    """-> (component, far): the first k whose running sum exceeds u (the sum short: the last with weight); far = u is
    farther than 1e-9 from every boundary.  weights: (Kp,) or (n, Kp)."""
    w = np.asarray(weights, dtype=np.float64)
    cdf = np.cumsum(np.broadcast_to(w, (u.size, w.shape[-1])), axis=1)
    k = (cdf > u[:, None]).argmax(axis=1)
    short = ~(cdf > u[:, None]).any(axis=1)
    last = w.shape[-1] - 1 - (np.broadcast_to(w, cdf.shape)[:, ::-1] > 0).argmax(axis=1)
    k = np.where(short, last, k)
    far = np.all(np.abs(cdf - u[:, None]) > 1e-9, axis=1)
    return k.astype(np.int32), far


def synth_rows(seed, n, D, row_offset=0):
    """lc_ctx_synth with K = 1, mu = 0, L = I: the normals of tag 1 (c2 = pair)"""
    c0, c1 = row_counters(0, np.arange(n), row_offset)
    X = np.zeros((n, D))
    for p in range((D + 1) // 2):
        z0, z1 = box_muller(philox4x32_10(c0, c1, p, 1, seed & 0xFFFFFFFF, seed >> 32))
        X[:, 2 * p] = z0
        if 2 * p + 1 < D:
            X[:, 2 * p + 1] = z1
    return X


# ---- the densities, as (location, scale matrix or scales, degrees of freedom) ----------------------------------------------
def gw_student(nu, beta, m, iW):
    """the predictive Student-t of a Gauss-Wishart posterior: nu' = nu + 1 - D, scale (1 + beta) / (beta nu') iW"""
    D = len(m)
    nup = nu + 1 - D
    return np.asarray(m, dtype=np.float64), (1 + beta) / (beta * nup) * np.asarray(iW, dtype=np.float64), nup


def gw_conditional_student(nu, beta, m, iW, given, target, xa):
    """the conditional of that Student-t for one x_a: location M(x_a), scale c (1 + s d^2) S, eta = nu' + Da"""
    m, iW = np.asarray(m, dtype=np.float64), np.asarray(iW, dtype=np.float64)
    D, Da = len(m), len(given)
    nup = nu + 1 - D
    Waa, Wba, Wbb = iW[np.ix_(given, given)], iW[np.ix_(target, given)], iW[np.ix_(target, target)]
    ya = np.asarray(xa, dtype=np.float64) - m[given]
    sol = np.linalg.solve(Waa, ya)
    eta = nup + Da
    sd2 = beta / (1 + beta) * float(ya @ sol)  # s d^2 with d^2 = nu maha and s = beta / ((1 + beta) nu)
    S = Wbb - Wba @ np.linalg.solve(Waa, Wba.T)
    return m[target] + Wba @ sol, (1 + beta) / (beta * eta) * (1 + sd2) * S, eta


def ng_student(nu, beta, m, L):
    """NormGamma: per column a Student-t with 2 nu degrees of freedom, from (1 + w (x - m)^2)^-(nu + 1/2), w = beta / (2 (1 + beta) L)"""
    w = beta / (2 * (1 + beta) * np.asarray(L, dtype=np.float64))
    return np.asarray(m, dtype=np.float64), np.sqrt(1.0 / (2 * nu * w)), 2 * nu


def eg_lomax(a, ib):
    """ExpGamma: per column a Lomax with shape a and scale 1 / ib, from (1 + ib x)^-(a + 1)"""
    return a, 1.0 / np.asarray(ib, dtype=np.float64)


# ---- reference samplers on numpy's generators -------------------------------------------------------------------------------
def draw_student(rng, n, loc, Scale, dof):
    L = np.linalg.cholesky(Scale)
    z = rng.standard_normal((n, len(loc)))
    return loc + (z @ L.T) * np.sqrt(dof / rng.chisquare(dof, n))[:, None]


def draw_student_diag(rng, n, loc, scale, dof):
    z = rng.standard_normal((n, len(loc)))
    return loc + scale * z * np.sqrt(dof / rng.chisquare(dof, (n, len(loc))))


def draw_lomax(rng, n, shape, scale):
    return scale * (rng.random((n, len(scale))) ** (-1.0 / shape) - 1.0)


# ---- the checks -----------------------------------------------------------------------------------------------------------------
def ks_student(x, loc, Scale, dof):
    """p-values of the whitened radius against F(Db, dof) and of every whitened coordinate against t(dof)"""
    L = np.linalg.cholesky(Scale)
    w = np.linalg.solve(L, (x - loc).T).T
    Db = len(loc)
    out = [stats.kstest((w * w).sum(axis=1) / Db, stats.f(Db, dof).cdf)]
    out += [stats.kstest(w[:, d], stats.t(dof).cdf) for d in range(Db)]
    return out


def ks_student_diag(x, loc, scale, dof):
    w = (x - loc) / scale
    return [stats.kstest(w[:, d], stats.t(dof).cdf) for d in range(x.shape[1])]


def ks_lomax(x, shape, scale):
    return [stats.kstest(x[:, d], stats.lomax(shape, scale=scale[d]).cdf) for d in range(x.shape[1])]


class Tally:
    """collects KS results: the largest statistic and the smallest p-value seen, for the report"""

    def __init__(self):
        self.stat, self.p, self.n = 0.0, 1.0, 0

    def add(self, results, what):
        for r in results:
            self.stat, self.p, self.n = max(self.stat, float(r.statistic)), min(self.p, float(r.pvalue)), self.n + 1
        worst = min(results, key=lambda r: r.pvalue)
        print(f"{what}: {len(results)} KS tests, largest statistic {max(r.statistic for r in results):.3e}, "
              f"smallest p {worst.pvalue:.3e} (bar {P_BAR:.0e})")
        assert worst.pvalue >= P_BAR, (what, worst)


def check_frequencies(label, weights, what):
    """label counts within 5 binomial standard errors of the weights, every component (the prior one included)"""
    n = label.size
    w = np.asarray(weights, dtype=np.float64)
    cnt = np.bincount(label, minlength=w.size)[: w.size]
    assert cnt.sum() == n, (what, "a label outside the components")
    se = np.sqrt(np.maximum(w * (1 - w), 0.0) / n)
    dev = np.abs(cnt / n - w)
    print(f"{what}: largest deviation of a label frequency {np.max(dev / np.maximum(se, 1e-300)):.2f} standard errors (bar 5)")
    assert np.all(dev <= 5 * se + 1e-15), (what, cnt / n, w)


# ---- the conditional mixture, vectorised over rows (tests/test_gpu_conditional_draws.py) -----------------------------------------
class CondComponent:
    """one component's conditional Student-t for many rows x_a: location M(x_a), scale f(x_a) S, eta degrees of freedom"""

    def __init__(self, nu, beta, m, iW, given, target):
        from scipy.special import gammaln

        m, iW = np.asarray(m, dtype=np.float64), np.asarray(iW, dtype=np.float64)
        D, Da = len(m), len(given)
        self.nup = nu + 1 - D
        self.eta = self.nup + Da
        self.beta, self.ma, self.mb = beta, m[given], m[target]
        self.Waa = iW[np.ix_(given, given)]
        Wba = iW[np.ix_(target, given)]
        self.B = np.linalg.solve(self.Waa, Wba.T).T
        self.S = iW[np.ix_(target, target)] - Wba @ np.linalg.solve(self.Waa, Wba.T)
        self.LS = np.linalg.cholesky(self.S)
        Sig = (1 + beta) / (beta * self.nup) * self.Waa  # the marginal's scale
        self.logc = (gammaln((self.nup + Da) / 2) - gammaln(self.nup / 2) - 0.5 * Da * np.log(self.nup * np.pi)
                     - 0.5 * np.linalg.slogdet(Sig)[1])

    def maha(self, Xa):  # (x_a - m_a)^T iW_aa^-1 (x_a - m_a)
        y = Xa - self.ma
        return np.einsum("na,na->n", y, np.linalg.solve(self.Waa, y.T).T)

    def log_marginal(self, Xa):
        q = self.beta * self.nup / (1 + self.beta) * self.maha(Xa)  # the distance under the marginal's scale
        return self.logc - 0.5 * self.eta * np.log1p(q / self.nup)

    def location(self, Xa):
        return self.mb + (Xa - self.ma) @ self.B.T

    def factor(self, Xa):  # c (1 + s d^2)
        return (1 + self.beta) / (self.beta * self.eta) * (1 + self.beta / (1 + self.beta) * self.maha(Xa))

    def whiten(self, Xa, x):
        """draws x (n, Db) of rows Xa (n, Da) -> whitened coordinates: t(eta) each, radius^2 / Db ~ F(Db, eta)"""
        w = np.linalg.solve(self.LS, (x - self.location(Xa)).T).T
        return w / np.sqrt(self.factor(Xa))[:, None]

    def variance(self, Xa):  # diagonal of the conditional covariance (eta > 2)
        return (self.eta / (self.eta - 2) * self.factor(Xa))[:, None] * np.diag(self.S)[None, :]


def responsibilities(comps, weights, Xa):
    """r_k(x_a) of the mixture of the components' marginals, rows x components"""
    with np.errstate(divide="ignore"):
        t = np.stack([np.log(w) + c.log_marginal(Xa) for c, w in zip(comps, weights)], axis=1)
    t -= t.max(axis=1, keepdims=True)
    r = np.exp(t)
    return r / r.sum(axis=1, keepdims=True)


def ks_whitened(w, eta):
    Db = w.shape[1]
    out = [stats.kstest((w * w).sum(axis=1) / Db, stats.f(Db, eta).cdf)]
    return out + [stats.kstest(w[:, d], stats.t(eta).cdf) for d in range(Db)]


def ks_whitened_pooled(parts):
    """parts: [(whitened draws (n_k, Db), eta_k)] of several components.  Every value goes through its own component's CDF
    (radius^2 / Db through F(Db, eta_k), a coordinate through t(eta_k)), which leaves uniforms whatever eta_k is: they
    pool into one KS test per coordinate and one for the radius, however many components there are."""
    Db = parts[0][0].shape[1]
    rad = np.concatenate([stats.f(Db, eta).cdf((w * w).sum(axis=1) / Db) for w, eta in parts])
    out = [stats.kstest(rad, "uniform")]
    for d in range(Db):
        out.append(stats.kstest(np.concatenate([stats.t(eta).cdf(w[:, d]) for w, eta in parts]), "uniform"))
    return out
