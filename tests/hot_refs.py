"""References for the hot-path launchers (tests/test_gpu_hot_kernels.py, tests/test_hot_refs_host.py): the packer of the
E-step parameter stream (both layouts, restated from the comments of csrc/lc_kernels.h and Context::pack_estep_params),
np.longdouble restatements of the E-step, the statistics and the fused record that take the PACKED doubles as exact, the
tile deal of fused_small_kernel, the input generators and the error bars.  A plain helper module: no fixtures, no hooks.

Two kinds of input.  EXACT inputs (small integers, q a multiple of 2^-10) make every product and partial sum a multiple of
a power of two far below 2^53: any order of summation gives the same bits, float64 numpy IS the reference and the
comparison is bit for bit.  ROUNDING inputs (normal data plus cluster offsets) are compared against first-order bars in
EPS = 2^-52 that count every rounded operation of the kernel's path once, relative to the sum of absolute values."""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -52
TINY = np.finfo(np.float64).tiny
LD = np.longdouble
WIDE_CHUNK = 256 * 16 + 64
FUSED_ROWS = 256


# ---- layouts (lc_kernels.h) --------------------------------------------------------------------------------------------------
def padded_dim(D):
    if D <= 128:
        return (D + 15) // 16 * 16
    return (D + 63) // 64 * 64


def active_width(D, DP):
    """estep_active_width"""
    if DP < 32 or DP > 128:
        return DP
    g, lo = (4, DP - 12) if DP <= 48 else (8, DP - 8)
    dc = (D + g - 1) // g * g
    return max(dc, lo) if dc < DP else DP


def ntiles(DP):
    nt = DP // 4
    return nt * (nt + 1) // 2


def pstride(DP, DC=None):
    DC = DP if DC is None else DC
    if DP > 128:
        npan = DP // 64
        return npan * (npan + 1) // 2 * WIDE_CHUNK
    return ntiles(DC) * 16 + DC


def stat_stride(DP):
    return 1 + DP + DP * DP


def fused_record(K, DP=16):
    return K * stat_stride(DP) + 1 + K


# ---- the parameter stream ----------------------------------------------------------------------------------------------------
def pack_params(A, m, DP, DC=None):
    """A [K x D x D] (lower triangular), m [K x D] -> [K x pstride(DP, DC)].
    Narrow layouts: the 4 x 4 tiles (it, jt <= it) of the active width in consumption order, element (lo, hi) of a tile at
    lo + 4 hi = A[4 it + lo][4 jt + hi]; then -b = -A m (DC entries).  Wide layouts: 64 x 64 blocks (I, J <= I) row-major, per
    block 16 x 16 tiles whose tile column jt = 4 q + jr holds the columns 16 q + jr + 4 h, then the 64 entries of -b_I."""
    A, m = np.asarray(A, dtype=np.float64), np.asarray(m, dtype=np.float64)
    K, D, _ = A.shape
    DC = DP if DC is None else DC
    W = DP if DP > 128 else DC
    assert D <= W
    Af = np.zeros((K, DP, DP))
    Af[:, :D, :D] = np.tril(A)
    bneg = np.zeros((K, DP))
    for k in range(K):
        for i in range(D):
            s = 0.0
            for j in range(i + 1):
                s += A[k, i, j] * m[k, j]
            bneg[k, i] = -s
    P = np.zeros((K, pstride(DP, DC)))
    if DP <= 128:
        NT = DC // 4
        for it in range(NT):
            for jt in range(it + 1):
                t = it * (it + 1) // 2 + jt
                tile = Af[:, 4 * it:4 * it + 4, 4 * jt:4 * jt + 4]           # [K][lo][hi]
                P[:, 16 * t:16 * t + 16] = tile.transpose(0, 2, 1).reshape(K, 16)  # index lo + 4 hi
        P[:, ntiles(DC) * 16:] = bneg[:, :DC]
    else:
        c = 0
        for I in range(DP // 64):
            for Jb in range(I + 1):
                C = P[:, c * WIDE_CHUNK:(c + 1) * WIDE_CHUNK]
                for it in range(16):
                    for jt in range(16):
                        cols = [64 * Jb + 16 * (jt // 4) + 4 * h + (jt % 4) for h in range(4)]
                        tile = Af[:, 64 * I + 4 * it:64 * I + 4 * it + 4, :][:, :, cols]  # [K][lo][h]
                        C[:, (it * 16 + jt) * 16:(it * 16 + jt) * 16 + 16] = tile.transpose(0, 2, 1).reshape(K, 16)
                C[:, 4096:4160] = bneg[:, 64 * I:64 * I + 64]
                c += 1
    return P


def unpack_params(P, DP, DC=None):
    """-> A [K x W x W] and -b [K x W] as the stream holds them (W = DC, or DP for the wide layouts).  The wide stream
    repeats -b_I in every chunk of block row I: all copies must agree."""
    P = np.asarray(P, dtype=np.float64)
    K = P.shape[0]
    DC = DP if DC is None else DC
    W = DP if DP > 128 else DC
    A, b = np.zeros((K, W, W)), np.zeros((K, W))
    if DP <= 128:
        for it in range(DC // 4):
            for jt in range(it + 1):
                t = it * (it + 1) // 2 + jt
                A[:, 4 * it:4 * it + 4, 4 * jt:4 * jt + 4] = P[:, 16 * t:16 * t + 16].reshape(K, 4, 4).transpose(0, 2, 1)
        b[:] = P[:, ntiles(DC) * 16:]
    else:
        c = 0
        for I in range(DP // 64):
            for Jb in range(I + 1):
                C = P[:, c * WIDE_CHUNK:(c + 1) * WIDE_CHUNK]
                for it in range(16):
                    for jt in range(16):
                        tile = C[:, (it * 16 + jt) * 16:(it * 16 + jt) * 16 + 16].reshape(K, 4, 4)  # [h][lo]
                        for h in range(4):
                            A[:, 64 * I + 4 * it:64 * I + 4 * it + 4, 64 * Jb + 16 * (jt // 4) + 4 * h + (jt % 4)] = tile[:, h, :]
                bI = C[:, 4096:4160]
                if Jb == 0:
                    b[:, 64 * I:64 * I + 64] = bI
                else:
                    assert np.array_equal(b[:, 64 * I:64 * I + 64], bI)
                c += 1
    return A, b


# ---- the E-step --------------------------------------------------------------------------------------------------------------
def estep_ref(X, A, bneg, ctab, grp, exact=False):
    """log q~ = c - |A x + (-b)|^2 / 2 for all rows of X (pad rows included) and T = sum_i (|A| |x| + |b|)_i^2, the scale of
    its error bar.  X [NP x >= W]; A [K x W x W], bneg [K x W] as unpacked; ctab [J x K]; grp [NP] group of every row.
    exact: float64 throughout (for the exact inputs: every operation is exact); else np.longdouble."""
    dt = np.float64 if exact else LD
    K, W, _ = A.shape
    Xw = np.asarray(X)[:, :W].astype(dt)
    NP = Xw.shape[0]
    lq, T = np.empty((K, NP), dtype=dt), np.empty((K, NP))
    c = np.asarray(ctab, dtype=dt)[np.asarray(grp)]  # [NP x K]
    for k in range(K):
        Ak, bk = A[k].astype(dt), bneg[k].astype(dt)
        y = Xw @ Ak.T + bk
        lq[k] = c[:, k] - (y * y).sum(axis=1) / 2
        if not exact:
            S = np.abs(Xw) @ np.abs(Ak).T + np.abs(bk)
            T[k] = (S * S).sum(axis=1).astype(np.float64)
    return lq, T


def lq_bar(T, c, W):
    """|log q~ - ref| <= EPS ((1.5 W + 2) T + |c|).  y_i: the accumulator starts at -b_i and takes W products, each product-add
    of the matrix pipe rounded once: (W + 1) EPS S_i with S_i = |b_i| + sum_j |a_ij| |x_j| >= |y_i|.  d^2 = sum y_i^2: the error
    of y_i enters as 2 |y_i| (W + 1) EPS S_i <= 2 (W + 1) EPS S_i^2; the W squares-and-adds (fma chain per lane, the four lanes'
    sum on the matrix pipe) add at most W EPS sum y_i^2 <= W EPS T.  log q~ = c - d^2 / 2 halves that ((1.5 W + 1) EPS T) and
    rounds once more: EPS |log q~| <= EPS (|c| + T / 2)."""
    return EPS * ((1.5 * W + 2) * np.asarray(T, dtype=np.float64) + np.abs(np.asarray(c, dtype=np.float64)))


def normalise_ref(lq, lqbar=None):
    """log-sum-exp over the clusters (axis 0) of log q~ [K x NP] in longdouble -> logZ [NP], q [K x NP] and, with the bars of
    log q~, bar(logZ) [NP].  Rows whose log q~ are all -inf give logZ = -inf, q = nan (the caller masks pad rows).

    bar(logZ) = sum_k q_k (bar(log q~_k) + EPS |log q~_k - max| + 2 EPS) + (K - 1) EPS + 2 EPS |log s| + EPS |logZ|:
    logZ as a function of the computed log q~ does not depend on which of them serves as the maximum, so their errors enter
    with the weights q_k; each exponential's argument is rounded once (EPS |log q~_k - max|, a relative error of e_k) and the
    exponential is good to one unit in the last place (2 EPS); K - 1 additions form s; the logarithm (2 EPS |log s|) and the
    final addition of the maximum (EPS |logZ|) round once each."""
    lq = np.asarray(lq, dtype=LD)
    K = lq.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        mx = lq.max(axis=0)
        d = lq - mx
        d[np.isnan(d)] = -np.inf
        e = np.exp(d)
        s = e.sum(axis=0)
        logZ = np.log(s) + mx
        q = e / s
        bar = None
        if lqbar is not None:
            qf = q.astype(np.float64)
            dd = np.where(np.isfinite(d), np.abs(d), 0.0).astype(np.float64)
            per = np.where(qf > 0, qf * (lqbar + EPS * dd + 2 * EPS), 0.0)
            bar = per.sum(axis=0) + (K - 1) * EPS + 2 * EPS * np.abs(np.log(s)).astype(np.float64) + EPS * np.abs(logZ).astype(np.float64)
    return logZ, q, bar


def q_bar(q_ref, lqbar, lzbar):
    """the issue's bar of a responsibility: q_ref (bar(log q~) + bar(logZ) + 2 EPS) + the smallest normal double"""
    return np.asarray(q_ref, dtype=np.float64) * (lqbar + lzbar + 2 * EPS) + TINY


def block_sums_ref(lq, logZ, q, ctab, grp, valid, blk, nblk, lqbar, lzbar):
    """per block (blk [NP]: the block that owns every row): fz_part = -sum logZ and ll_part[k] = sum q (log q~ - c) over the
    valid rows, with bars.
    bar(fz) = sum bar(logZ) + n EPS sum |logZ| (n valid rows of the block: the additions).
    bar(ll_k) = sum [ |t| (bar_rel(q) + 2 EPS) + q bar(log q~) ] + n EPS sum |t|, t = q (log q~ - c): q's relative bar, the
    subtraction and the product round once each, the error of log q~ enters with weight q, then n additions."""
    K, NP = lq.shape
    c = np.asarray(ctab, dtype=LD)[np.asarray(grp)].T  # [K x NP]
    fz, fzb = np.zeros(nblk, dtype=LD), np.zeros(nblk)
    ll, llb = np.zeros((nblk, K), dtype=LD), np.zeros((nblk, K))
    with np.errstate(invalid="ignore"):
        t = np.where(q > 0, q * (lq - c), LD(0))
    t = np.where(valid[None, :], t, LD(0))
    qrel = lqbar + lzbar[None, :] + 2 * EPS
    qf = np.where(valid[None, :], q.astype(np.float64), 0.0)
    with np.errstate(invalid="ignore"):
        tb = np.abs(t).astype(np.float64) * (qrel + 2 * EPS) + np.where(qf > 0, qf * lqbar, 0.0)
    for b in range(nblk):
        v = valid & (blk == b)
        n = int(v.sum())
        z = logZ[v]
        fz[b] = -z.sum()
        fzb[b] = lzbar[v].sum() + n * EPS * float(np.abs(z).sum())
        ll[b] = t[:, v].sum(axis=1)
        llb[b] = tb[:, v].sum(axis=1) + n * EPS * np.abs(t[:, v]).sum(axis=1).astype(np.float64)
    return fz, fzb, ll, llb


# ---- statistics ---------------------------------------------------------------------------------------------------------------
def stats_ref(X, q, rows=None, dtype=np.float64):
    """N_k = sum q, s_k = sum q x, S_k = sum q x x^T over `rows` (a slice; default all) -> records [K x stat_stride(DP)] with
    the full symmetric S; dtype float64 (exact inputs) or longdouble."""
    X, q = np.asarray(X), np.asarray(q)
    rows = slice(None) if rows is None else rows
    Xc, qc = X[rows].astype(dtype), q[:, rows].astype(dtype)
    K, DP = qc.shape[0], Xc.shape[1]
    rec = np.zeros((K, stat_stride(DP)), dtype=dtype)
    rec[:, 0] = qc.sum(axis=1)
    rec[:, 1:1 + DP] = qc @ Xc
    for k in range(K):
        rec[k, 1 + DP:] = ((Xc * qc[k][:, None]).T @ Xc).reshape(-1)
    return rec


def stats_abs(X, q):
    """the same sums over absolute values (the scale of the statistics' bars), float64"""
    return stats_ref(np.abs(X), np.abs(q))


def stats_bar(absrec, n):
    """|stat - ref| <= (n + 2) EPS sum |q x_i x_j|: every row's term is formed with at most two roundings (q x, then the
    product-add of the matrix pipe) and the n rows (+ the chunks' partial sums: fewer additions than rows) are added once each."""
    return (n + 2) * EPS * absrec


def lower_mask(DP, DC=None):
    """Boolean mask over a record: N, s[0 .. DC) and the lower triangle of the DC x DC corner -- what the host reads"""
    DC = DP if DC is None else DC
    m = np.zeros(stat_stride(DP), dtype=bool)
    m[0] = True
    m[1:1 + DC] = True
    S = np.zeros((DP, DP), dtype=bool)
    S[:DC, :DC] = np.tril(np.ones((DC, DC), dtype=bool))
    m[1 + DP:] = S.reshape(-1)
    return m


def region_masks(DP, DC):
    """the regions of a record nobody reads: s of the idle / pad columns, S rows and columns of the idle / pad columns, the
    strict upper triangle of the active corner"""
    s_idle = np.zeros(stat_stride(DP), dtype=bool)
    s_idle[1 + DC:1 + DP] = True
    S = np.zeros((DP, DP), dtype=bool)
    S[DC:, :] = True
    S[:, DC:] = True
    S_idle = np.zeros(stat_stride(DP), dtype=bool)
    S_idle[1 + DP:] = S.reshape(-1)
    U = np.zeros((DP, DP), dtype=bool)
    U[:DC, :DC] = np.triu(np.ones((DC, DC), dtype=bool), 1)
    upper = np.zeros(stat_stride(DP), dtype=bool)
    upper[1 + DP:] = U.reshape(-1)
    return s_idle, S_idle, upper


# ---- the fused pass's tile deal (fused_small_kernel) --------------------------------------------------------------------------------
def fused_deal(b, G, ntile, yshare):
    """tiles of block b of G, in the order the block walks them.  Plain deal: every G-th tile from b on.  With yshare > 0,
    an even G and ntile >= 4 G: every second block (b >= H = G / 2) takes xy = ntile * 2 * yshare // (1000 G) tiles -- from
    Te + (b - H) on, every H-th --, and the first blocks deal the tiles 0 .. Te - 1 = ntile - H xy - 1 among themselves, every
    H-th from b on."""
    H = G // 2
    if yshare > 0 and G % 2 == 0 and ntile >= 4 * G:
        xy = ntile * 2 * yshare // (1000 * G)
        Te = ntile - H * xy
        if b < H:
            return list(range(b, Te, H))
        return [Te + (b - H) + i * H for i in range(xy)]
    return list(range(b, ntile, G))


def fused_yshare(grid, cus, share=410):
    """launch_fused: the uneven deal only when the grid is two blocks per compute unit"""
    return share if grid == 2 * cus else 0


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def exact_X(rng, NP, D, DP, valid=None, amp=7):
    """small integers in the first D columns; pad columns and pad rows zero (the layout's contract)"""
    X = np.zeros((NP, DP))
    X[:, :D] = rng.integers(-amp, amp + 1, size=(NP, D))
    if valid is not None:
        X[~valid] = 0.0
    return X


def exact_params(rng, K, D, amp=3, mamp=4):
    """A: integer lower-triangular with |a| <= 3 and a non-zero diagonal; m integer; -> A [K x D x D], m [K x D]"""
    A = np.tril(rng.integers(-amp, amp + 1, size=(K, D, D))).astype(np.float64)
    for k in range(K):
        d = rng.integers(1, amp + 1, size=D) * rng.choice([-1, 1], size=D)
        A[k][np.arange(D), np.arange(D)] = d
    m = rng.integers(-mamp, mamp + 1, size=(K, D)).astype(np.float64)
    return A, m


def exact_ctab(rng, J, K):
    """multiples of 1/2"""
    return rng.integers(-40, 41, size=(J, K)) / 2.0


def exact_q(rng, K, NP, zero_steps=False):
    """multiples of 2^-10 in [0, 1]; zero_steps: whole 4-row steps of a cluster all zero, others with a single non-zero"""
    q = rng.integers(0, 1025, size=(K, NP)) / 1024.0
    if zero_steps:
        steps = NP // 4
        kind = rng.integers(0, 3, size=(K, steps))  # 0: all zero, 1: one non-zero, 2: as drawn
        for k in range(K):
            for s in np.nonzero(kind[k] == 0)[0]:
                q[k, 4 * s:4 * s + 4] = 0.0
            for s in np.nonzero(kind[k] == 1)[0]:
                keep = rng.integers(0, 4)
                v = q[k, 4 * s + keep] or 1.0 / 1024
                q[k, 4 * s:4 * s + 4] = 0.0
                q[k, 4 * s + keep] = v
    return q


def rounding_problem(rng, K, D, NP, DP, valid=None, J=1):
    """normal data around K cluster offsets, whiteners near the identity -> X [NP x DP], A, m, ctab [J x K].  The offsets
    shrink with the width (|mu_k - mu_l|^2 of about 8 at every D) so that the clusters overlap and q takes every size."""
    mu = rng.normal(scale=2.0 / np.sqrt(D), size=(K, D))
    lab = rng.integers(0, K, size=NP)
    X = np.zeros((NP, DP))
    X[:, :D] = mu[lab] + rng.normal(size=(NP, D))
    if valid is not None:
        X[~valid] = 0.0
    A = np.tril(rng.normal(scale=0.2, size=(K, D, D)))
    A[:, np.arange(D), np.arange(D)] = rng.uniform(0.7, 1.4, size=(K, D))
    ctab = rng.normal(scale=2.0, size=(J, K)) - 0.5 * D
    return X, A, mu, ctab
