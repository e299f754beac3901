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


# ---- exact values on the documented streams (include/libcluster_hip.h; tests/test_gpu_sample_kernels.py) ---------------------
# Everything below is written from the counter table of the header and DESIGN 4.16.  `xp` is the arithmetic the values are
# formed in: F64 (numpy) or MP (40-digit mpmath on object arrays, tests/test_sample_exact_refs_host.py); the Philox words,
# the uniforms (exact in float64 by construction) and every DECISION (which attempt is accepted, which component is chosen)
# are float64's either way, so the two evaluations differ by rounding alone.
TAG_GAMMA_N, TAG_GAMMA_U, TAG_GAMMA_B, TAG_LOMAX = 0x12, 0x13, 0x14, 0x15
GAMMA_ATTEMPTS = 64  # RNG_GAMMA_ATTEMPTS
NEAR = 1e-9          # a decision closer than this to its boundary is left out of a comparison (cap: EXCLUDED_SHARE)
EXCLUDED_SHARE = 1e-3


class F64:
    log, exp, expm1, sqrt, cos, sin = np.log, np.exp, np.expm1, np.sqrt, np.cos, np.sin
    two_pi = 6.283185307179586476925

    @staticmethod
    def lift(x):
        return np.asarray(x, dtype=np.float64)

    @staticmethod
    def zeros(shape):
        return np.zeros(shape)


def mp_backend(digits=40):
    """the same operations at `digits` decimal digits: object arrays of mpmath.mpf"""
    import mpmath

    mpmath.mp.dps = digits
    f = lambda fn: np.frompyfunc(fn, 1, 1)  # noqa: E731

    class MP:
        log, exp, expm1, sqrt, cos, sin = f(mpmath.log), f(mpmath.exp), f(mpmath.expm1), f(mpmath.sqrt), f(mpmath.cos), f(mpmath.sin)
        two_pi = 2 * mpmath.pi

        @staticmethod
        def lift(x):
            return np.frompyfunc(lambda v: mpmath.mpf(float(v)), 1, 1)(np.asarray(x, dtype=np.float64))

        @staticmethod
        def zeros(shape):
            z = np.empty(shape, dtype=object)
            z.fill(mpmath.mpf(0))
            return z

    return MP


def _words(seed, c0, c1, c2, tag, sub=0):
    return philox4x32_10(c0, c1, c2, tag | (sub << 8), seed & 0xFFFFFFFF, seed >> 32)


def box_muller_xp(o, xp=F64):
    u1, u2 = xp.lift(u01(o[0], o[1])), xp.lift(u01(o[2], o[3]))
    rad = xp.sqrt(-2 * xp.log(u1))
    return rad * xp.cos(xp.two_pi * u2), rad * xp.sin(xp.two_pi * u2)


def normals_xp(seed, c0, c1, c2, ncols, xp=F64):
    """z (n, ncols): tag 0x11, sub = pair p -> z[2p] (cos), z[2p + 1] (sin)"""
    z = xp.zeros((len(c0), ncols))
    for p in range((ncols + 1) // 2):
        z0, z1 = box_muller_xp(_words(seed, c0, c1, c2, TAG_NORMAL, p), xp)
        z[:, 2 * p] = z0
        if 2 * p + 1 < ncols:
            z[:, 2 * p + 1] = z1
    return z


def gamma_draw_counters(seed, c0, c1, c2, shape, xp=F64):
    """Marsaglia-Tsang on the streams of (c0, c1, c2): attempt t takes its normal x (the cos value) from block (0x12, t) and its
    uniform u from (0x13, t); with d = a - 1/3, c = 1 / sqrt(9 d), w = 1 + c x, v = w^3 it is accepted when w > 0 and
    log u < x^2 / 2 + d - d v + d log v, and gives d v; a = shape + 1 and a factor U^(1 / shape) (block (0x14, 0)) for a
    shape below 1.  -> (G, attempts, margin): margin = the smallest distance of a decision of the row from its boundary."""
    c0, c1 = np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64)
    n = c0.size
    shape = np.broadcast_to(np.asarray(shape, dtype=np.float64), (n,))
    c2 = np.broadcast_to(np.asarray(c2, dtype=np.uint64), (n,))
    a = np.where(shape < 1.0, shape + 1.0, shape)
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    attempts, margin, taken = np.zeros(n, dtype=np.int64), np.full(n, np.inf), np.zeros(n, dtype=np.int64)
    live = np.arange(n)
    for t in range(GAMMA_ATTEMPTS):
        if live.size == 0:
            break
        x = box_muller(_words(seed, c0[live], c1[live], c2[live], TAG_GAMMA_N, t))[0]
        w = 1.0 + c[live] * x
        pos = w > 0.0
        v = w * w * w
        u = u01(*_words(seed, c0[live], c1[live], c2[live], TAG_GAMMA_U, t)[:2])
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = np.log(u) - (0.5 * x * x + d[live] - d[live] * v + d[live] * np.log(v))
        margin[live] = np.minimum(margin[live], np.where(pos, np.minimum(np.abs(w), np.abs(gap)), np.abs(w)))
        acc = pos & (gap < 0.0)
        attempts[live], taken[live] = t + 1, t
        live = live[~acc]
    assert live.size == 0, "a rejection run of 64 attempts (probability below 1e-80)"
    # the value, from the accepted attempt's words, in xp
    G = xp.zeros(n)
    for t in np.unique(taken):
        m = taken == t
        x = box_muller_xp(_words(seed, c0[m], c1[m], c2[m], TAG_GAMMA_N, int(t)), xp)[0]
        dx = xp.lift(a[m]) - xp.lift(np.ones(m.sum())) / 3
        cx = 1 / xp.sqrt(9 * dx)
        w = 1 + cx * x
        G[m] = dx * w * w * w
    low = shape < 1.0
    if low.any():
        ub = xp.lift(u01(*_words(seed, c0[low], c1[low], c2[low], TAG_GAMMA_B)[:2]))
        G[low] = G[low] * xp.exp(xp.log(ub) / xp.lift(shape[low]))
    return G, attempts, margin


def gamma_draw(seed, block, rows, c2, shape, row_offset=0, xp=F64):
    c0, c1 = row_counters(block, rows, row_offset)
    return gamma_draw_counters(seed, c0, c1, c2, shape, xp)


def choose_cdf(u, cdf, klast):
    """the component of u under running sums cdf (Kp,): the first k with cdf[k] > u, else klast -> (k, far)"""
    over = cdf[None, :] > u[:, None]
    k = np.where(over.any(axis=1), over.argmax(axis=1), klast)
    return k.astype(np.int32), np.all(np.abs(cdf[None, :] - u[:, None]) > NEAR, axis=1)


class Exact:
    """values with what a comparison needs: mag = the magnitude of each entry's summed terms, nsum = the length of its sum,
    label_far / value_far = the row's decisions are farther than NEAR from their boundaries"""

    def __init__(self, x, mag, nsum, label, label_far, value_far):
        self.x, self.mag, self.nsum, self.label, self.label_far, self.value_far = x, mag, nsum, label, label_far, value_far


def sample_rows(mode, seed, block, rows, cdf, klast, loc, fac, shape, row_offset=0, xp=F64):
    """lc_model_sample's rows of one block (i = 0): mode 0 Gauss-Wishart loc + F eps / sqrt(G) (one gamma per row, slot 0), mode
    1 NormGamma loc_d + fac_d eps_d / sqrt(G_d) (slot = column), mode 2 ExpGamma fac_d expm1(-log u_d / shape) (c2 = pair)"""
    rows = np.asarray(rows)
    c0, c1 = row_counters(block, rows, row_offset)
    k, lfar = choose_cdf(choice_u(seed, block, rows, 0, row_offset), np.asarray(cdf, dtype=np.float64), klast)
    fac = np.asarray(fac, dtype=np.float64)
    D = fac.shape[1]
    n = rows.size
    sh = np.asarray(shape, dtype=np.float64)[k]
    x, mag = xp.zeros((n, D)), xp.zeros((n, D))
    vfar = np.ones(n, dtype=bool)
    if mode == 0:
        G, _, margin = gamma_draw_counters(seed, c0, c1, 0, sh, xp)
        vfar = margin > NEAR
        eps = normals_xp(seed, c0, c1, 0, D, xp)
        rs = 1 / xp.sqrt(G)
        L, Fk = xp.lift(np.asarray(loc, dtype=np.float64)[k]), fac[k]
        for i in range(D):
            nz = np.flatnonzero(np.any(Fk[:, i, : i + 1] != 0, axis=0))  # (a product with an exact zero adds nothing)
            terms = xp.lift(Fk[:, i, nz]) * eps[:, nz]
            x[:, i] = L[:, i] + rs * terms.sum(axis=1)
            mag[:, i] = abs(L[:, i]) + rs * abs(terms).sum(axis=1)
        nsum = np.broadcast_to(np.arange(D) + 2, (n, D))
    elif mode == 1:
        eps = normals_xp(seed, c0, c1, 0, D, xp)
        L, F = xp.lift(np.asarray(loc, dtype=np.float64)[k]), xp.lift(fac[k])
        for d in range(D):
            G, _, margin = gamma_draw_counters(seed, c0, c1, d, sh, xp)
            vfar &= margin > NEAR
            t = F[:, d] * eps[:, d] / xp.sqrt(G)
            x[:, d], mag[:, d] = L[:, d] + t, abs(L[:, d]) + abs(t)
        nsum = np.full((n, D), 2)
    else:
        F = xp.lift(fac[k])
        for p in range((D + 1) // 2):
            o = _words(seed, c0, c1, p, TAG_LOMAX)
            for h, u in enumerate((u01(o[0], o[1]), u01(o[2], o[3]))):
                d = 2 * p + h
                if d < D:
                    x[:, d] = F[:, d] * xp.expm1(-xp.log(xp.lift(u)) / xp.lift(sh))
                    mag[:, d] = abs(x[:, d])
        nsum = np.full((n, D), 1)
    return Exact(x, mag, nsum, k, lfar, vfar)


def cond_draws(seed, block, rows, ndraws, Xa, t, logp, ttab, pexp, mext, T, Lt, cq, Db, xp=F64):
    """lc_model_predict_conditional_draws' rows of one block from the launch's own tables: per (row, draw i) the component k by
    inverse CDF over r_k = exp(t_k - logp) (the sum short: the last k with r_k > 0), then
      x_b = M_k(x_a) + sqrt(cq_k exp((ttab_k - t_k) / e_k) / G) L_k z,  M_k = [x_a - m_a,k, 1] T_k,  G ~ Gamma(e_k)  (c2 = i)
    Xa (n, Da); t (n, Kp); logp (n,); ttab (Kp,) of the block; mext (Kp, Dae); T (Kp, Dae, Dbp); Lt (Kp, Dbp, Dbp) with
    Lt[k][j][c] = L_k[c][j].  -> Exact with x, mag, nsum (n, ndraws, Db) and label, label_far, value_far (n, ndraws)"""
    rows = np.asarray(rows)
    n, Da = Xa.shape
    c0, c1 = row_counters(block, rows)
    r = np.exp(t - logp[:, None])
    cum = np.cumsum(r, axis=1)
    last = r.shape[1] - 1 - (r[:, ::-1] > 0).argmax(axis=1)
    x, mag = xp.zeros((n, ndraws, Db)), xp.zeros((n, ndraws, Db))
    label = np.zeros((n, ndraws), dtype=np.int32)
    lfar, vfar = np.zeros((n, ndraws), dtype=bool), np.zeros((n, ndraws), dtype=bool)
    Xl, ml, Tl, Ll = xp.lift(Xa), xp.lift(mext), xp.lift(T), xp.lift(Lt)
    for i in range(ndraws):
        u = choice_u(seed, block, rows, i)
        over = (cum > u[:, None]) & (r > 0)
        k = np.where(over.any(axis=1), over.argmax(axis=1), last)
        label[:, i], lfar[:, i] = k, np.all(np.abs(cum - u[:, None]) > NEAR, axis=1)
        e = pexp[k]
        G, _, margin = gamma_draw_counters(seed, c0, c1, i, e, xp)
        vfar[:, i] = margin > NEAR
        z = normals_xp(seed, c0, c1, i, Db, xp)
        tk = t[np.arange(n), k]
        f = xp.sqrt(xp.lift(cq[k]) * xp.exp((xp.lift(ttab[k]) - xp.lift(tk)) / xp.lift(e)) / G)
        dv = Xl - ml[k][:, :Da]
        for c in range(Db):
            mt = dv * Tl[k][:, :Da, c]
            lt = Ll[k][:, : c + 1, c] * z[:, : c + 1]
            x[:, i, c] = mt.sum(axis=1) + Tl[k][:, Da, c] + f * lt.sum(axis=1)
            mag[:, i, c] = abs(mt).sum(axis=1) + abs(Tl[k][:, Da, c]) + f * abs(lt).sum(axis=1)
    nsum = np.broadcast_to(Da + 1 + np.arange(Db) + 1, (n, ndraws, Db))
    return Exact(x, mag, nsum, label, lfar, vfar)


def scaled_error(got, want, mag):
    """|got - want| / mag per entry as float64 (0 where both the error and the magnitude are 0)"""
    err = np.abs(got - want)
    out = np.zeros(np.shape(err))
    nz = np.asarray(mag != 0, dtype=bool)
    out[nz] = np.asarray(err[nz] / mag[nz], dtype=np.float64)
    out[~nz & np.asarray(err != 0, dtype=bool)] = np.inf
    return out


def value_bar(nsum, e_ref):
    """the bar of a drawn value: the forward bound of a recursive sum of nsum products plus 8 times the reference's own error"""
    return (np.asarray(nsum) + 2) * 2.0 ** -53 + 8 * e_ref
