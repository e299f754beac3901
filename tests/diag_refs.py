"""References for the launchers of csrc/lc_kernels_diag.hip (tests/test_gpu_diag_kernels.py, tests/test_diag_refs_host.py): the
packer of the matrix-pipe E-step's operands restated from the comments of estep_diag_mfma_kernel and estep_diag_pack, np.longdouble
restatements of both forms of log q~ and of the statistics records that take the PACKED doubles as exact, the restated launch
plans, the input generators and the error bars.  A plain helper module: no fixtures, no hooks.

EXACT / ROUNDING inputs as in tests/hot_refs.py.  EXACT: x, a, mu small integers, w2 and w1 multiples of 1/8, c and q multiples
of 2^-10 -- every product and partial sum is a multiple of 2^-10 far below 2^43, so any order of summation gives the same bits
and float64 numpy IS the reference.  ROUNDING: normal data plus cluster offsets against first-order bars in EPS = 2^-52 that
count every rounded operation of the kernel's path once, relative to the sum of absolute values."""
from __future__ import annotations

import numpy as np

import hot_refs as hr

EPS, TINY, LD = hr.EPS, hr.TINY, hr.LD

# (csrc/lc_kernels_diag.hip, lc_kernels.h; tests/test_host.py compares them with the sources)
DIAG_MAXT = 4
SD_QMAX = 64
EDM_CT_CAP = 1024
EDM_KTM = 8
EDM_LDS_LIMIT = 150 * 1024
EDM_LDS_TWO_BLOCKS = 80 * 1024
EDI = ("none", "generic", "plain", "tabled", "one_group")  # DiagEstepInstance, in the order of the enum


def edm_r(NT):
    return 2 if NT <= 16 else 1


# ---- launch plans, restated ----------------------------------------------------------------------------------------------------
def edm_lds_bytes(NT, NTF, KT, R, slots, table=False):
    """weights [KT][NTF][16], constants [4 KT], centre [4 NT], four F_z sums, every lane's LL_k sums [KT][256], (K > 32) every
    lane's log q~ slots [KT][R][256], (tabled) the table c_jk, the 64-entry exponential table -- doubles"""
    return (KT * NTF * 16 + 4 * KT + 4 * NT + 4 + KT * 256 + (KT * R * 256 if slots else 0) + (EDM_CT_CAP if table else 0) + 64) * 8


def mfma_weights(DP, K, mode):
    """estep_diag_mfma_weights: doubles of the packed tiles, 0 when the shape has no matrix-pipe path"""
    if DP > 128 or DP % 16 or K < 1:
        return 0
    NT = DP // 4
    NTF = NT if mode == 2 else 2 * NT
    KT = (K + 3) // 4
    if edm_lds_bytes(NT, NTF, KT, edm_r(NT), K > 4 * EDM_KTM) > EDM_LDS_LIMIT:
        return 0
    return KT * NTF * 16


def estep_plan_ref(DP, K, mode, nrg, mfma, raw=False, want_ll=False, grouped=False, ngroups=1, cus=None):
    """estep_diag_plan restated; cus: compute units of the device (matrix-pipe path)"""
    nslots = (nrg * 16 + 63) // 64
    if not mfma:
        DC = min(DP, 128)
        return dict(ok=1, mfma=0, mode=mode, grid=nslots, lds_bytes=(64 * (DC + 1) + 256 + K) * 8, wide=int(DP > 128),
                    KT=1 if K <= 4 else 2 if K <= 8 else 4, REG=int(K <= 4 * DIAG_MAXT * 4), nslots=nslots,
                    name="estep_diag_wide_kernel" if DP > 128 else "estep_diag_kernel")
    NT = DP // 4
    QUAD = mode != 2
    NTF = 2 * NT if QUAD else NT
    R, KT = edm_r(NT), (K + 3) // 4
    KTM = EDM_KTM if K <= 4 * EDM_KTM else 0
    plain = KTM > 0 and not raw and not want_ll
    tabled = plain and grouped and ngroups * K <= EDM_CT_CAP and edm_lds_bytes(NT, NTF, KT, R, KTM == 0, True) <= EDM_LDS_LIMIT
    inst = "one_group" if plain and not grouped else "tabled" if tabled else "plain" if plain else "generic"
    lds = edm_lds_bytes(NT, NTF, KT, R, KTM == 0, tabled)
    per_cu = 2 if lds <= EDM_LDS_TWO_BLOCKS else 1
    ntile = (nrg + 4 * R - 1) // (4 * R)
    return dict(ok=1, mfma=1, mode=mode, grid=min(ntile, nslots, cus * per_cu), lds_bytes=lds, NT=NT, QUAD=int(QUAD), R=R, KTM=KTM,
                instance=inst, nslots=nslots, per_cu=per_cu, block_cap=cus * per_cu, name="estep_diag_mfma_kernel")


def sd_br(DP):
    return 32 if DP <= 64 else 16


def sd_rsplit(K):
    groups = (min(K, SD_QMAX) + 15) // 16
    return 1 if groups >= 3 else 2 if groups == 2 else 4


def stat_plan_ref(DP, K, second):
    """suffstat_diag_plan restated"""
    RS = sd_rsplit(K)
    w = min(DP, 128)
    lw = (64 if DP % 128 else 128) if DP > 128 else DP

    def nstage(dp):
        return int(dp <= 96 and not (dp >= 64 and RS == 1))

    return dict(ok=1, nslice=(K + SD_QMAX - 1) // SD_QMAX, rsplit=RS, second=int(bool(second)), nblocks=(DP + 127) // 128 if DP > 128 else 1,
                width=w, last_width=lw, BR=sd_br(w), BR_last=sd_br(lw), nstage=nstage(w), nstage_last=nstage(lw), deep=int(w <= 96),
                deep_last=int(lw <= 96), lds_bytes=(2 * sd_br(w) * lds_row_stride(w) + 2 * SD_QMAX * (sd_br(w) + 4)) * 8,
                name="suffstat_diag_kernel")


def lds_row_stride(DP):
    return 16 if DP == 16 else DP + 32 if (DP + 16) % 32 != 16 else DP + 16


# ---- the packed operands of the matrix-pipe path -------------------------------------------------------------------------------
def centre(a, w2, DP, mode):
    """mu [DP]: the mean of the cluster centres, summed in cluster order and divided by K (pad columns, mode 2: zero); cond =
    max_d max_k |w2| reach_d^2 with reach_d the farthest 6-sigma edge (sigma = sqrt(0.5 / |w2|)) of any cluster from mu_d"""
    a, w2 = np.asarray(a, dtype=np.float64), np.asarray(w2, dtype=np.float64)
    K, D = a.shape
    mu = np.zeros(DP)
    if mode == 2:
        return mu, 0.0
    m = np.zeros(D)
    for k in range(K):
        m = m + a[k]
    m = m / K
    mu[:D] = m
    w = np.abs(w2)
    with np.errstate(divide="ignore"):
        sig = np.where(w > 0, np.sqrt(0.5 / w), 0.0)
    reach = (np.abs(a - m) + 6.0 * sig).max(axis=0)
    cond = float((w.max(axis=0) * reach * reach).max(initial=0.0))
    return mu, cond


def tile_slot(k, half, d, NT, NTF):
    """where W[k][half][d] sits: cluster tile it = k / 4 holds NTF feature tiles of 16 doubles; column d of a half belongs to the
    feature tile jt = half NT + 4 (d / 16) + d % 4 (a tile stands for the columns {16 q + jr + 4 h}), element lo + 4 hh with
    lo = k % 4, hh = (d % 16) / 4"""
    it, lo = k // 4, k % 4
    jt = half * NT + 4 * (d // 16) + d % 4
    hh = (d % 16) // 4
    return (it * NTF + jt) * 16 + lo + 4 * hh


def pack_diag(a, w2, w1, DP, mode, mu=None):
    """a / w2 / w1 [K x D] -> mu [DP], constk [K], wt [ceil(K / 4) NTF 16].
    The features of a row around the centre are [x'^2 (half 0), x' (half 1)], x' = x - mu; mode 2 has the linear half only, around
    zero.  Weights: w2 on x'^2, w1 - 2 w2 a' on x' with a' = a - mu; constk_k = sum_d (w2 a'^2 + w1 mu), each term formed as
    (w2 a') a' + w1 mu and added in column order.  Everything else is zero."""
    a, w2, w1 = (np.asarray(v, dtype=np.float64) for v in (a, w2, w1))
    K, D = a.shape
    if mu is None:
        mu, _ = centre(a, w2, DP, mode)
    mu = np.asarray(mu, dtype=np.float64)
    NT = DP // 4
    NTF = NT if mode == 2 else 2 * NT
    wt = np.zeros((K + 3) // 4 * NTF * 16)
    ck = np.zeros(K)
    for k in range(K):
        cs = 0.0
        for d in range(D):
            if mode == 2:
                wt[tile_slot(k, 0, d, NT, NTF)] = w1[k, d]
                continue
            ac = a[k, d] - mu[d]
            wt[tile_slot(k, 0, d, NT, NTF)] = w2[k, d]
            wt[tile_slot(k, 1, d, NT, NTF)] = w1[k, d] - (2.0 * w2[k, d]) * ac
            cs = cs + ((w2[k, d] * ac) * ac + w1[k, d] * mu[d])
        ck[k] = cs
    return mu, ck, wt


def unpack_diag(wt, DP, K, mode):
    """-> W2 [K x DP] (zeros in mode 2), WL [K x DP] as the tiles hold them; every other slot must be zero"""
    NT = DP // 4
    NTF = NT if mode == 2 else 2 * NT
    W2, WL = np.zeros((K, DP)), np.zeros((K, DP))
    used = np.zeros(wt.size, dtype=bool)
    for k in range(K):
        for d in range(DP):
            if mode == 2:
                s = tile_slot(k, 0, d, NT, NTF)
                WL[k, d] = wt[s]
                used[s] = True
            else:
                s2, s1 = tile_slot(k, 0, d, NT, NTF), tile_slot(k, 1, d, NT, NTF)
                W2[k, d], WL[k, d] = wt[s2], wt[s1]
                used[s2] = used[s1] = True
    assert used.sum() == K * DP * (1 if mode == 2 else 2) and not wt[~used].any()
    return W2, WL


def pad_params(a, w2, w1, DP):
    """[3][K][DP]: a, w2, w1 with zero pad columns (what launch_estep_diag takes)"""
    K, D = np.asarray(a).shape
    P = np.zeros((3, K, DP))
    P[0, :, :D], P[1, :, :D], P[2, :, :D] = a, w2, w1
    return P


# ---- log q~, both forms ----------------------------------------------------------------------------------------------------------
def diff_ref(X, P, ctab, grp, exact=False):
    """difference form: log q~[k, n] = c_jk + sum_d (w2 (x - a)^2 + w1 x); P [3][K][DP].  -> lq [K x NP], and the scales of its
    bar: S2 = sum |w2| (x - a)^2, S1 = sum |w1 x| (float64)"""
    dt = np.float64 if exact else LD
    X = np.asarray(X).astype(dt)
    a, w2, w1 = (np.asarray(P[i]).astype(dt) for i in range(3))
    K = a.shape[0]
    c = np.asarray(ctab, dtype=dt)[np.asarray(grp)]  # [NP x K]
    lq = np.empty((K, X.shape[0]), dtype=dt)
    S2, S1 = np.empty(lq.shape), np.empty(lq.shape)
    for k in range(K):
        t = X - a[k]
        q2, l1 = (t * t) * w2[k], X * w1[k]
        lq[k] = c[:, k] + (q2 + l1).sum(axis=1)
        S2[k], S1[k] = np.abs(q2).sum(axis=1), np.abs(l1).sum(axis=1)
    return lq, S2, S1


def bilinear_ref(X, mu, ck, W2, WL, ctab, grp, exact=False):
    """bilinear form: log q~ = c_jk + constk_k + sum_d (W2 x'^2 + WL x'), x' = x - mu.  -> lq, SQ = sum |W2| x'^2, SL = sum |WL x'|"""
    dt = np.float64 if exact else LD
    f = np.asarray(X).astype(dt) - np.asarray(mu).astype(dt)
    K = W2.shape[0]
    c = np.asarray(ctab, dtype=dt)[np.asarray(grp)]
    lq = np.empty((K, f.shape[0]), dtype=dt)
    SQ, SL = np.empty(lq.shape), np.empty(lq.shape)
    for k in range(K):
        q2, l1 = (f * f) * W2[k].astype(dt), f * WL[k].astype(dt)
        lq[k] = c[:, k] + dt(ck[k]) + (q2 + l1).sum(axis=1)
        SQ[k], SL[k] = np.abs(q2).sum(axis=1), np.abs(l1).sum(axis=1)
    return lq, SQ, SL


def _absc(ctab, grp):
    c = np.abs(np.asarray(ctab, dtype=np.float64))[np.asarray(grp)].T
    return np.where(np.isfinite(c), c, 0.0)


def valu_bar(S2, S1, ctab, grp, DP, mode, nonreg_wide=False):
    """|log q~ - ref| of the difference-form kernels.  Per column: t = x - a rounds once (2 EPS of t^2), t w2 rounds once -- 3 EPS
    S2; every fma rounds its sum once, nf = DP (modes 1, 2) or 2 DP (mode 0) of them, each at most EPS S with S = S2 + S1 the sum of
    absolute terms.  Wide observations add the chunks' sums one by one (nch more additions of at most |c| + S: in registers on top of
    each other and then on c, or -- more than 64 clusters -- as the running sum c + acc_0 + acc_1 ... kept in qZ).  The last
    addition of c rounds |log q~| <= |c| + S once."""
    S = S2 + S1
    nf = DP * (2 if mode == 0 else 1)
    nch = (DP + 127) // 128 if DP > 128 else 0
    c = _absc(ctab, grp)
    return EPS * (3 * S2 + nf * S + (nch + 1) * (c + S))


def mfma_bar(SQ, SL, ck, ctab, grp, DP, mode):
    """|log q~ - ref| of the matrix-pipe kernel.  x' = x - mu rounds once (EPS |WL x'|, 2 EPS W2 x'^2) and its square once more
    (EPS W2 x'^2): the double rounding of the quadratic feature, 3 EPS SQ + EPS SL.  The accumulator starts at constk + c (one
    rounded addition) and takes DP product-adds per half, each rounded once at no more than EPS A, A = |c| + |constk| + SQ + SL."""
    n = DP * (1 if mode == 2 else 2)
    A = _absc(ctab, grp) + np.abs(np.asarray(ck, dtype=np.float64))[:, None] + SQ + SL
    return EPS * (3 * SQ + SL + (n + 1) * A)


def packing_bar(X, P, mu, W2, WL):
    """|difference form - bilinear form| in exact arithmetic on the packed doubles: the roundings of the packer.  a' = a - mu
    rounds once (da <= EPS |a'|); WL = w1 - 2 w2 a' carries 2 |w2| da, the product's and the subtraction's rounding:
    EPS (4 |w2 a'| + |WL|) |x'| per column; constk's term (w2 a') a' + w1 mu carries 2 EPS from a', two products and w1 mu's product
    and the sum -- EPS (4 |w2 a'^2| + |w1 mu| + |term|) -- and the D additions EPS sum |terms| each."""
    a, w2, w1 = (np.asarray(P[i], dtype=np.float64) for i in range(3))
    ac = np.abs(a - mu)
    f = np.abs(np.asarray(X, dtype=np.float64)[None, :, :] - mu)          # [1 x NP x DP]
    lin = (EPS * (4 * np.abs(w2) * ac + np.abs(WL)))[:, None, :] * f        # [K x NP x DP]
    t2, t1 = np.abs(w2) * ac * ac, np.abs(w1 * mu)
    D = a.shape[1]
    ckb = EPS * (4 * t2 + t1 + (t2 + t1)).sum(axis=1) + D * EPS * (t2 + t1).sum(axis=1)
    return lin.sum(axis=2) + ckb[:, None] + TINY


def q_bar_full(qref, lq, logZ, lqbar, lzbar):
    """hot_refs.q_bar + q EPS (|log q~ - logZ| + 3): the rounding of the exponential's argument, the reciprocal and the product
    (tests/test_gpu_hot_kernels.py derives it; exp_nonpos and rcp_pos are inside the 2 EPS the formulas grant an exponential and a
    reciprocal: 1.27 ulp and 0.50 ulp measured, docs/NOTEBOOK.md)"""
    with np.errstate(invalid="ignore"):
        d = np.where(qref > 0, np.abs(lq - logZ[None, :]), 0).astype(np.float64)
    return hr.q_bar(qref, lqbar, lzbar[None, :]) + np.asarray(qref, dtype=np.float64) * EPS * (d + 3)


def mfma_block_of_rows(NP, R, grid):
    """the persistent deal: tile t (4 waves x R row groups = 64 R rows) belongs to block t mod grid"""
    return (np.arange(NP) // (64 * R)) % grid


# ---- statistics ------------------------------------------------------------------------------------------------------------------
def stat_records_ref(X, q, chunk_rows, nchunks, RS, nstage, second, dtype=np.float64, scale=False):
    """records [nchunks x RS x K x (1 + 2 DP)]: record (chunk, row class r) sums the 4-row steps st = r (mod RS) of every batch
    of the chunk (batches start at the chunk's first row and hold a multiple of 4 RS rows, so row i of a chunk is of class
    (i / 4) mod RS); layout [N | x_s | xx_s].  nstage: N_k of the whole chunk in class 0, exactly 0 in the others.  second = 0:
    xx_s = 0.  scale: sums of absolute values (float64) and the rows per record, for the bars."""
    X, q = np.asarray(X), np.asarray(q)
    NP, DP = X.shape
    K = q.shape[0]
    rec = np.zeros((nchunks, RS, K, 1 + 2 * DP), dtype=dtype)
    rows = np.zeros((nchunks, RS), dtype=np.int64)
    if scale:
        X, q = np.abs(X), np.abs(q)
    for c in range(nchunks):
        r0, r1 = c * chunk_rows, min((c + 1) * chunk_rows, NP)
        cls = (np.arange(r1 - r0) // 4) % RS
        for r in range(RS):
            sel = np.arange(r0, r1)[cls == r]
            Xc, qc = X[sel].astype(dtype), q[:, sel].astype(dtype)
            rows[c, r] = sel.size
            rec[c, r, :, 1:1 + DP] = qc @ Xc
            if second:
                rec[c, r, :, 1 + DP:] = qc @ (Xc * Xc)
            if not nstage:
                rec[c, r, :, 0] = qc.sum(axis=1)
        if nstage:
            rec[c, 0, :, 0] = q[:, r0:r1].astype(dtype).sum(axis=1)
    return (rec, rows) if scale else rec


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def distinct_X(rng, NP, D, DP, tile_rows=64):
    """integers, every element of a tile_rows x D tile different from every other (a misplaced element shows); pad columns zero"""
    X = np.zeros((NP, DP))
    n = tile_rows * D
    for r0 in range(0, NP, tile_rows):
        rows = min(tile_rows, NP - r0)
        X[r0:r0 + rows, :D] = (rng.permutation(n) - n // 2).reshape(tile_rows, D)[:rows]
    return X


def exact_diag_params(rng, K, D, mode, amp=3):
    """a integers, w2 negative multiples of 1/8, w1 multiples of 1/8 (mode 1: w1 = 0; mode 2: a = w2 = 0)"""
    a = rng.integers(-amp, amp + 1, size=(K, D)).astype(np.float64)
    w2 = -rng.integers(1, 9, size=(K, D)) / 8.0
    w1 = rng.integers(-8, 9, size=(K, D)) / 8.0
    if mode == 1:
        w1[:] = 0.0
    if mode == 2:
        a[:], w2[:] = 0.0, 0.0
    return a, w2, w1


def exact_ctab(rng, J, K):
    """multiples of 2^-10"""
    return rng.integers(-40 * 1024, 40 * 1024 + 1, size=(J, K)) / 1024.0


def rounding_diag_problem(rng, K, D, NP, DP, mode, valid=None, J=1):
    """normal data around K cluster offsets (mode 2: exponential data), widths near one -> X [NP x DP], a, w2, w1 [K x D], ctab.
    Well conditioned: |w2| reach^2 stays far below the switch of Context::estep_diag."""
    X = np.zeros((NP, DP))
    lab = rng.integers(0, K, size=NP)
    if mode == 2:
        rate = rng.uniform(0.7, 1.4, size=(K, D))
        X[:, :D] = rng.exponential(size=(NP, D)) / rate[lab] * (2.0 / np.sqrt(D) + 1) / 2
        a, w2, w1 = np.zeros((K, D)), np.zeros((K, D)), -rate
    else:
        mu = rng.normal(scale=2.0 / np.sqrt(D), size=(K, D))
        X[:, :D] = mu[lab] + rng.normal(size=(NP, D))
        a, w2 = mu, -0.5 * rng.uniform(0.6, 1.5, size=(K, D))
        w1 = np.zeros((K, D)) if mode == 1 else rng.normal(scale=0.05, size=(K, D))
    if valid is not None:
        X[~valid] = 0.0
    ctab = rng.normal(scale=2.0, size=(J, K)) - 0.5 * D
    return X, a, w2, w1, ctab
