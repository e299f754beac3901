"""The inputs of tests/test_gpu_holes_kernels.py (the launchers of lc_kernels_holes.hip on synthetic tables, no model fit) and
their references, shared with tests/test_holes_kernels_refs_host.py, which holds the inputs to the conditions the GPU file
relies on without a device.  numpy / scipy only; a plain helper module, no fixtures.

Tables:     Kp posteriors (incomplete_ref.random_posterior) and what the kernels read of them (incomplete_ref.tables,
            incomplete_var_ref.g_table, cqnu as incomplete_draws_ref.HoleComponent forms it), padded to DP.
Layout:     blocks of rows on the padded row axis (rginfo words, valid rows, block of a row).
reference:  incomplete_ref.direct, incomplete_var_ref.direct_var and incomplete_draws_ref.HoleMixture per block -- the direct
            route, never the device's.
CASES:      the shapes of the prediction tests with their rows; DRAW_CASES those of the draws.
"""
import functools

import numpy as np

import incomplete_draws_ref as dr
import incomplete_ref as ref
import incomplete_var_ref as vref

RG, HMAX, NH = 16, ref.HOLES_MAX, ref.HOLES_MAX + 1
BAR_LOGP, BAR_FILL, BAR_VAR, BAR_T = 1e-10, 1e-9, 1e-9, 1e-10


def dp(D):
    """the padded width of a context with D columns"""
    return (D + 15) // 16 * 16 if D <= 128 else (D + 63) // 64 * 64


def lpr(D):
    """lanes per row of holes_scan_kernel"""
    return 16 if dp(D) <= 16 else 32 if dp(D) <= 32 else 64


class Tables:
    """Kp posteriors at width D and the device tables of them; posts replaces the random ones"""

    def __init__(self, D, Kp, seed, posts=None):
        rng = np.random.default_rng(seed)
        self.D, self.Kp, self.DP = D, Kp, dp(D)
        self.posts = list(posts) if posts is not None else [ref.random_posterior(rng, D) for _ in range(Kp)]
        DP = self.DP
        self.mean, self.P = np.zeros((Kp, DP)), np.zeros((Kp, DP, DP))
        self.s, self.cqnu = np.zeros(Kp), np.zeros(Kp)
        self.e, self.G, self.gnu = np.zeros((NH, Kp)), np.zeros((NH, Kp)), np.zeros((NH, Kp))
        self.chol, self.sd = [], np.zeros((Kp, D))
        for k, (nu, beta, m, iW) in enumerate(self.posts):
            P, G, s, e = ref.tables(nu, beta, iW)
            self.mean[k, :D], self.P[k, :D, :D] = m, P
            self.s[k], self.e[:, k], self.G[:, k] = s, e, G  # (G is NaN where nb > D: no row reads it there)
            self.gnu[:, k] = np.nan_to_num(vref.g_table(nu, beta, D) * nu, nan=0.0)  # 0: the variance does not exist
            self.cqnu[k] = (1 + beta) * nu / (2 * beta)
            self.chol.append(np.linalg.cholesky(iW))
            self.sd[k] = np.sqrt(np.diag(iW) / nu)

    def weights(self, rng):
        w = rng.random(self.Kp) + 0.05
        return w / w.sum()

    def rows(self, rng, n):
        """rows near a component (1.5 of its spread), every other one pulled 40 ... 60 % of the way to another component"""
        X = np.zeros((n, self.D))
        for i in range(n):
            k, k2 = rng.integers(0, self.Kp, 2)
            X[i] = self.posts[k][2] + 1.5 * self.sd[k] * rng.normal(size=self.D)
            if i % 2:
                t = rng.uniform(0.4, 0.6)
                X[i] = (1 - t) * X[i] + t * self.posts[k2][2]
        return X

    def fill(self, w):
        """the weighted mean of the component means"""
        return np.asarray(w) @ self.mean[:, : self.D]

    def raw_column(self, Xf):
        """-d_full^2 / 2 of filled rows (n, D) -> (Kp, n), as the raw E-step leaves it"""
        return np.stack([-0.5 * nu * np.sum(np.linalg.solve(L, (Xf - m).T) ** 2, axis=0) for (nu, _, m, _), L in zip(self.posts, self.chol)])

    def ttab(self, weights):
        """[J x NH x Kp]: log w_jk + G_k(nb)"""
        return np.stack([np.log(w)[None, :] + self.G for w in weights])


def punch(rng, X, complete, nbs=None):
    """a copy of X with NaNs in the rows that are not `complete` (bool mask): the hole counts cycle through nbs (default
    min(8, D - 1) ... 1); the first such row holds column 0, the second column D - 1"""
    n, D = X.shape
    nbs = list(nbs) if nbs is not None else list(range(min(HMAX, D - 1), 0, -1))
    Xh, i = X.copy(), 0
    for r in range(n):
        if complete[r]:
            continue
        cols = rng.choice(D, nbs[i % len(nbs)], replace=False)
        if i == 0 and 0 not in cols:
            cols[0] = 0
        if i == 1 and D - 1 not in cols:
            cols[0] = D - 1
        Xh[r, cols] = np.nan
        i += 1
    return Xh


def balance(tab, w, xh, k, k2):
    """the row on the segment between the means of components k and k2, with the holes of xh, where by the direct route these
    two (with their weights) have the same responsibility to within a step of 1 / 2000 of the segment"""
    pat = np.flatnonzero(np.isnan(xh))
    line = np.array([(1 - t) * tab.posts[k][2] + t * tab.posts[k2][2] for t in np.linspace(0.0, 1.0, 2001)])
    line[:, pat] = np.nan
    r = dr.HoleMixture([tab.posts[k], tab.posts[k2]], [w[k], w[k2]]).responsibilities(line)
    return line[np.argmin(np.abs(r[:, 0] - 0.5))]


def third_complete(n):
    """every third row complete, between rows with holes"""
    return np.arange(n) % 3 == 1


class Layout:
    """blocks of counts[j] rows, each padded to whole row groups, then `empty` row groups of count 0 (of the last block)"""

    def __init__(self, counts, empty=0):
        self.counts, self.J = list(counts), len(counts)
        npad = [(c + RG - 1) // RG * RG for c in counts]
        self.goff = np.concatenate([[0], np.cumsum(npad)]).astype(np.int64)
        self.NP = int(self.goff[-1]) + RG * empty
        self.nrg = self.NP // RG
        self.valid, self.block = np.zeros(self.NP, bool), np.full(self.NP, self.J - 1)
        words = []
        for j, c in enumerate(counts):
            self.valid[self.goff[j]:self.goff[j] + c] = True
            self.block[self.goff[j]:self.goff[j + 1]] = j
            words += [(j << 5) | min(RG, c - g * RG) for g in range(npad[j] // RG)]  # lck::rginfo_pack
        words += [(self.J - 1) << 5] * empty
        self.words = np.array(words, dtype=np.int32)
        self.rginfo = self.words if self.J > 1 or empty else None  # (a single block goes by nrows)
        self.nrows = counts[0]

    def place(self, parts, pad):
        """the blocks' arrays on the padded row axis, `pad` elsewhere"""
        shape = (self.NP,) + parts[0].shape[1:]
        out = np.full(shape, pad, dtype=parts[0].dtype)
        for j, p in enumerate(parts):
            out[self.goff[j]:self.goff[j] + p.shape[0]] = p
        return out


def host_scan(Xh):
    """count (n,), cols (n, 8) of rows with NaNs: what holes_scan_kernel records"""
    nan = np.isnan(Xh)
    count = nan.sum(axis=1).astype(np.int32)
    cols = np.full((Xh.shape[0], HMAX), -1, dtype=np.int32)
    for r in np.flatnonzero(count):
        c = np.flatnonzero(nan[r])[:HMAX]
        cols[r, : c.size] = c
    return count, cols


def t_reference(mix, Xh):
    """t_k = log w_k + log p_k(x_a) by the direct route, (n, Kp); NaN in rows without holes"""
    t = np.full((Xh.shape[0], mix.Kp), np.nan)
    for pat, rows in mix.patterns(Xh).items():
        a = mix.comp(0, pat).a
        t[rows] = np.stack([np.log(mix.w[k]) + mix.comp(k, pat).log_marginal(Xh[np.ix_(rows, a)]) for k in range(mix.Kp)], axis=1)
    return t


def direct_var_table(Xh, posts, w, gnu):
    """incomplete_var_ref.direct_var's route with g_k(nb) nu_k taken from the table the device reads (gnu [NH x Kp], 0 where the
    variance of a component does not exist) -> var (n, 8), V_n (n,)"""
    n, D = Xh.shape
    var, Vn = np.zeros((n, HMAX)), np.ones(n)
    for r in range(n):
        b = np.flatnonzero(np.isnan(Xh[r]))
        if not b.size:
            continue
        a = np.setdiff1d(np.arange(D), b)
        T, M, V = [], [], []
        for k, (nu, beta, mm, iW) in enumerate(posts):
            c = dr.HoleComponent(nu, beta, mm, iW, b)
            xa = Xh[r:r + 1, a]
            T.append(np.log(w[k]) + c.log_marginal(xa)[0])
            M.append(c.location(xa)[0])
            V.append(gnu[b.size, k] / nu * c.h(xa)[0] * np.diag(c.S))
        T, M, V = np.array(T), np.array(M), np.array(V)
        rk = np.exp(T - T.max())
        rk /= rk.sum()
        dev = (M - rk @ M) ** 2
        var[r, : b.size] = rk @ V + rk @ dev
        Vn[r] = (V + dev).max()
    return var, Vn


class Reference:
    """the direct route for blocks [(Xh (n, D), weights (Kp,))], rows of all blocks one after the other"""

    def __init__(self, tab, blocks, table_g=False):
        rows, logp, S, var, Vn, t, r = [], [], [], [], [], [], []
        self.mixes = []
        for Xh, w in blocks:
            a, lp, _, s = ref.direct(Xh, tab.posts, None, w, 0.0)
            v, vn = direct_var_table(Xh, tab.posts, w, tab.gnu) if table_g else vref.direct_var(Xh, tab.posts, None, w, 0.0)[:2]
            mix = dr.HoleMixture(tab.posts, w)
            self.mixes.append(mix)
            rows.append(a), logp.append(lp), S.append(s), var.append(v), Vn.append(vn)
            t.append(t_reference(mix, Xh)), r.append(mix.responsibilities(Xh))
        self.rows, self.logp, self.S = np.concatenate(rows), np.concatenate(logp), np.concatenate(S)
        self.var, self.Vn, self.t, self.r = np.concatenate(var), np.concatenate(Vn), np.concatenate(t), np.concatenate(r)


def ratios(ref_, rows, logp, var=None, t=None):
    """largest |value - reference| over its bar's scale, per output: {"logp", "fill", "var", "t"}"""
    out = {"logp": float(np.max(np.abs(logp - ref_.logp) / np.abs(ref_.logp))),
           "fill": float(np.max(np.abs(rows - ref_.rows).max(axis=1) / ref_.S))}
    if var is not None:
        out["var"] = float(np.max(np.abs(var - ref_.var).max(axis=1) / ref_.Vn))
    if t is not None:
        holed = ~np.isnan(ref_.t[:, 0])
        out["t"] = float(np.max(np.abs(t[holed] - ref_.t[holed]) / np.maximum(1.0, np.abs(ref_.t[holed])), initial=0.0))
    return out


BARS = {"logp": BAR_LOGP, "fill": BAR_FILL, "var": BAR_VAR, "t": BAR_T}


# ---- the prediction cases -------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, tab, blocks, **notes):
        self.tab, self.blocks, self.notes = tab, blocks, notes
        self.Xh = np.concatenate([b[0] for b in blocks])
        for b in blocks:
            b[0].setflags(write=False)

    @functools.cached_property
    def ref(self):
        return Reference(self.tab, self.blocks, table_g=self.notes.get("table_g", False))


def _plain(D, Kp, N, seed, complete=None, nbs=None):
    tab = Tables(D, Kp, seed)
    rng = np.random.default_rng(seed + 1)
    X = tab.rows(rng, N)
    complete = third_complete(N) if complete is None else complete
    Xh, w = punch(rng, X, complete, nbs), tab.weights(rng)
    if Kp > 1:  # every fourth row: between two components, so that the mixture of the experts is a mixture
        for r in range(3, N, 4):
            if not complete[r]:
                k = int(rng.integers(0, Kp))
                Xh[r] = balance(tab, w, Xh[r], k, (k + 1 + int(rng.integers(0, Kp - 1))) % Kp)
    return Case(tab, [(Xh, w)])


def _chunks():
    """Kp = 130 at D = 23: rows 0, 1, 2 sit on components of chunk 0, 1 and 2; row 3 lies between a component of chunk 0 and one of a
    later chunk where, by the reference, the two have about the same responsibility"""
    tab = Tables(23, 130, 4153)
    rng = np.random.default_rng(4154)
    w = tab.weights(rng)
    X = tab.rows(rng, 20)
    placed = [(0, 5), (1, 70), (2, 129)]
    for r, k in placed:
        X[r] = tab.posts[k][2] + 0.3 * tab.sd[k] * rng.normal(size=23)
    Xh = punch(rng, X, third_complete(20) & (np.arange(20) > 3))
    # the pairs (chunk 0, a later chunk) by the distance of their means, closest first: the first whose balanced row has, in
    # the whole mixture, these two on top with a fifth of the mass or more for the second
    m = tab.mean[:, :23]
    dist = np.linalg.norm(m[:64, None, :] - m[None, 64:, :], axis=2)
    mix = dr.HoleMixture(tab.posts, w)
    for flat in np.argsort(dist, axis=None)[:20]:
        k, k2 = int(flat // dist.shape[1]), 64 + int(flat % dist.shape[1])
        x = balance(tab, w, Xh[3], k, k2)
        r = mix.responsibilities(x[None, :])[0]
        if set(np.argsort(r)[-2:]) == {k, k2} and min(r[k], r[k2]) >= 0.2:
            Xh[3] = x
            return Case(tab, [(Xh, w)], placed=placed, between=(3, k, k2))
    raise AssertionError("no pair of components in different chunks shares a row")


def _edges():
    """D = 23, Kp = 5, 135 rows = 8 row groups and one of 7: wave 0 has its only row with holes at lane 0, wave 1 at lane 63;
    row 128 has x_a exactly on component 2's m_a, row 129 lies 50 spreads from component 0 in every column, row 134 is the last
    valid row of the partly filled row group"""
    tab = Tables(23, 5, 4155)
    rng = np.random.default_rng(4156)
    X = tab.rows(rng, 135)
    X[128] = tab.posts[2][2]
    X[129] = tab.posts[0][2] + 50.0 * tab.sd[0] * np.where(rng.random(23) < 0.5, -1.0, 1.0)
    complete = np.ones(135, bool)
    complete[[0, 127, 128, 129, 134]] = False
    return Case(tab, [(punch(rng, X, complete, nbs=[3, 8, 5, 4, 2]), tab.weights(rng))], on_mean=(128, 2), far=129)


def _gnu0():
    """D = 3, Kp = 2: component 1 has nu = 2.5, so its variance does not exist with two holes (nu - 1 - nb <= 0) and the table
    holds 0 there; the reference takes the same table"""
    rng = np.random.default_rng(4157)
    posts = [ref.random_posterior(rng, 3), (2.5, 1.5, np.array([0.5, -1.0, 2.0]), np.array([[2.0, 0.3, 0.1], [0.3, 1.5, -0.2], [0.1, -0.2, 1.0]]))]
    tab = Tables(3, 2, 0, posts=posts)
    X = tab.rows(rng, 12)
    return Case(tab, [(punch(rng, X, third_complete(12), nbs=[2, 1]), np.array([0.6, 0.4]))], table_g=True)


def _d23_k5():
    """one wave with all 64 rows holed, one ragged wave of 6"""
    complete = np.zeros(70, bool)
    complete[[65, 68]] = True
    return _plain(23, 5, 70, 4144, complete)


def _blocks3():
    """J = 3: 5, 30 and 20 rows -- the second block starts at padded row 16, inside the first wave"""
    tab = Tables(23, 5, 4158)
    rng = np.random.default_rng(4159)
    blocks = []
    for n in (5, 30, 20):
        blocks.append((punch(rng, tab.rows(rng, n), third_complete(n)), tab.weights(rng)))
    return Case(tab, blocks)


BUILDERS = {
    "d2_k1_n1": lambda: _plain(2, 1, 1, 4140, np.zeros(1, bool)),  # Kp = 1: the filled value is M_1 itself
    "d3_k2_n17": lambda: _plain(3, 2, 17, 4141),
    "d9_k3_n40": lambda: _plain(9, 3, 40, 4142),                   # nb = 1 ... 8: Da down to 1
    "d23_k5_n70": _d23_k5,
    "d64_k35_n33": lambda: _plain(64, 35, 33, 4145),               # DP = 64: one column step exactly
    "d72_k64_n20": lambda: _plain(72, 64, 20, 4146),               # DP = 80: lanes 0 - 15 take a second step; one full chunk
    "d72_k65_n20": lambda: _plain(72, 65, 20, 4147),               # ... and one cluster in a second chunk
    "d23_k130_n20": _chunks,                                       # three chunks
    "d200_k3_n20": lambda: _plain(200, 3, 20, 4148),
    "d5_k3_n260": lambda: _plain(5, 3, 260, 4149),                 # a second 256-thread block
    "edges": _edges,
    "gnu0": _gnu0,
    "blocks3": _blocks3,
}
SHAPES = [n for n in BUILDERS if n[0] == "d"]


@functools.lru_cache(maxsize=None)
def case(name):
    """built once, shared by the tests and never changed"""
    return BUILDERS[name]()


# ---- the draws --------------------------------------------------------------------------------------------------------------------
DRAW_SEED = (7 << 32) + 3
DRAW_CASES = {  # name: (builder, draws per row)
    "d23_k5_n70_m1": ("d23_k5_n70", 1),
    "d23_k5_n70_m7": ("d23_k5_n70", 7),
    "d23_k5_n70_m64": ("d23_k5_n70", 64),
    "d5_k70_n40_m64": ("d5_k70_n40", 64),   # the second chunk of clusters is drawn from
    "d72_k3_n20_m7": ("d72_k3_n20", 7),
    "d5_k1_n120_m64": ("d5_k1_n120", 64),   # Kp = 1: the recovered G pooled per nb
    "blocks2_m7": ("blocks2", 7),           # J = 2 with goff
}


def _k70():
    """Kp = 70 at D = 5 with the weights of the last six components raised, so that they take a good share of the rows"""
    tab = Tables(5, 70, 4161)
    rng = np.random.default_rng(4162)
    w = tab.weights(rng)
    w[64:] *= 40.0
    w /= w.sum()
    return Case(tab, [(punch(rng, tab.rows(rng, 40), third_complete(40)), w)])


def _blocks2():
    tab = Tables(23, 5, 4163)
    rng = np.random.default_rng(4164)
    return Case(tab, [(punch(rng, tab.rows(rng, n), third_complete(n)), tab.weights(rng)) for n in (21, 30)])


BUILDERS.update({"d5_k70_n40": _k70, "d72_k3_n20": lambda: _plain(72, 3, 20, 4165), "d5_k1_n120": lambda: _plain(5, 1, 120, 4166),
                 "blocks2": _blocks2})


def label_reference(c, seed, nd):
    """-> want (n, nd), far (n, nd) for the rows of all blocks: sample_ref.choose on the documented uniforms and the reference's
    responsibilities; rows without holes: -1, far"""
    import sample_ref as sr

    want, far, at = np.full((c.Xh.shape[0], nd), -1, dtype=np.int32), np.ones((c.Xh.shape[0], nd), bool), 0
    for j, (Xh, _) in enumerate(c.blocks):
        rows = np.flatnonzero(np.isnan(Xh).any(axis=1))
        r = c.ref.r[at + rows]
        for i in range(nd):
            want[at + rows, i], far[at + rows, i] = sr.choose(sr.choice_u(seed, j, rows, i), r)
        at += Xh.shape[0]
    return want, far
