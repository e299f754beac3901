"""launch_estep, launch_suffstat (with launch_fold_extra) and launch_fused, launcher by launcher, through the lc_test_* hooks
of libcluster_hip_testhooks.so (csrc/lc_testhooks.hip, tests/aux_hooks.py) against the references of tests/hot_refs.py.

Every launch runs twice and must repeat its bits; every destination holds SENT (a NaN) before the launch and is downloaded
whole: rows past the launch, columns past K, partial slots past the grid and the guard behind the last record must keep it.
Every case asserts the plan it expects, so no case can drift onto another kernel.

EXACT inputs (small integers; hot_refs) are compared value for value with no bar (np.array_equal, and no NaN: the only freedom
is the sign of a zero).  ROUNDING inputs are compared against the bars derived in hot_refs (lq_bar, normalise_ref, q_bar,
block_sums_ref, stats_bar), each a first-order count of the rounded operations in EPS = 2^-52; the worst ratio of error to bar
of every test is printed (pytest -s) and recorded in docs/NOTEBOOK.md.  q's bar is q_ref (bar(log q~) + bar(logZ) + 2 EPS) + the
smallest normal double, plus the operations that formula leaves out: q_ref EPS (|log q~ - logZ| + 3) (see q_bar_full)."""
import numpy as np
import pytest

import aux_hooks as ah
import hot_refs as hr

pytestmark = pytest.mark.gpu

SENT = np.nan
EPS = hr.EPS
u64 = np.uint64
RATIOS = {}


def note(name, ratio):
    """the worst ratio of error to bar seen under `name`; printed, and asserted <= 1 by the caller"""
    ratio = float(ratio)
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"ratio {name}: {ratio:.3g}")
    return ratio


def ratio_of(err, bar):
    err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    assert err.shape == bar.shape and np.isfinite(err).all(), "an error is not finite"
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return float(np.max(r, initial=0.0))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u64), np.ascontiguousarray(b).view(u64))


def exact_equal(got, ref):
    got, ref = np.asarray(got), np.asarray(ref, dtype=np.float64)
    return got.shape == ref.shape and not np.isnan(got).any() and np.array_equal(got, ref)


def untouched(a):
    return bool(np.isnan(np.asarray(a)).all())


# ---- row layouts ---------------------------------------------------------------------------------------------------------------
def layout_nrows(nrg, nrows):
    NP = nrg * 16
    return dict(rginfo=None, nrows=nrows, valid=np.arange(NP) < nrows, grp=np.zeros(NP, dtype=np.int64), J=1, NP=NP)


def layout_groups(rgs):
    """rgs: (group, nvalid) per row group"""
    info = np.array([(g << 5) | n for g, n in rgs], dtype=np.int32)
    valid = np.concatenate([np.arange(16) < n for _, n in rgs])
    grp = np.repeat(np.array([g for g, _ in rgs], dtype=np.int64), 16)
    return dict(rginfo=info, nrows=0, valid=valid, grp=grp, J=max(g for g, _ in rgs) + 1, NP=16 * len(rgs))


def layout_three_groups(nrg):
    """three groups of row groups, with nvalid 0, 1, 15 and 16 in the middle of the launch"""
    rgs = [((3 * i) // nrg, 16) for i in range(nrg)]
    mid = max(0, nrg // 2 - 2)
    for t, n in enumerate((0, 1, 15, 16)):
        if mid + t < nrg:
            rgs[mid + t] = (rgs[mid + t][0], n)
    rgs[-1] = (rgs[-1][0], 7)
    return layout_groups(rgs)


def layout_sparse(nrg, R, rgpb):
    """groups for the sparse E-step: the first wave's R row groups of block 0 -> group 1, the rest of block 0 -> group 0, later
    blocks -> group 2, the very last row group (when it lies beyond block 0) -> group 3"""
    rgs = []
    for i in range(nrg):
        g = 1 if i < R else 0 if i < rgpb else 3 if i == nrg - 1 else 2
        rgs.append((g, 16 if i % 5 else 9))
    lay = layout_groups(rgs)
    lay["J"] = 4
    return lay


def sparse_ctab(rng, K):
    """cluster 0 inactive in all of block 0 (groups 0, 1: the block's list starts at cluster 1), cluster 1 inactive for the
    first wave's group only, group 3 with the single active cluster K - 1"""
    c = hr.exact_ctab(rng, 4, K)
    c[0, 0] = c[1, 0] = -np.inf
    c[1, 1] = -np.inf
    c[3, :K - 1] = -np.inf
    return c


# ---- the E-step ------------------------------------------------------------------------------------------------------------------
NARROW = [(16, 16)] + [(dp, dc) for dp in (32, 48) for dc in (dp, dp - 4, dp - 8, dp - 12)] + \
         [(dp, dc) for dp in (64, 80, 96, 112, 128) for dc in (dp, dp - 8)]
ES_K = (1, 3, 4, 5, 9)


def run_estep(X, DC, P, ctab, K, lay, plan, raw, sparse, want_ll):
    NP, grid = X.shape[0], plan["grid"]
    outs = []
    for _ in range(2):
        q = np.full((K + 2, NP + 48), SENT)
        fz = np.full(grid + 3, SENT)
        ll = np.full(grid * K + 5, SENT) if want_ll else None
        rc = ah.estep(X, DC, P, ctab, K, q, fz, ll, rginfo=lay["rginfo"], nrows=lay["nrows"], raw=raw, sparse=sparse)
        assert rc == 0, rc
        outs.append((q, fz, ll))
    for a, b in zip(outs[0], outs[1]):
        assert (a is None and b is None) or same_bits(a, b), "a second launch gave other bits"
    q, fz, ll = outs[0]
    assert untouched(q[K:]) and untouched(q[:, NP:]), "a store outside the K columns / NP rows"
    assert untouched(fz[grid:]) and (ll is None or untouched(ll[grid * K:])), "a partial sum outside the grid"
    if raw:
        assert untouched(fz) and (ll is None or untouched(ll)), "a raw launch wrote partial sums"
    return q[:K, :NP], fz[:grid], None if ll is None else ll[:grid * K].reshape(grid, K)


def q_bar_full(qref, lq, logZ, lqbar, lzbar):
    """hot_refs.q_bar (the issue's formula) + q EPS (|log q~ - logZ| + 3): the operations that formula does not count.
    Measured with the formula alone: up to 2.05 x the bar (exact inputs at 16 and 32 columns, where bar(log q~) is zero and the
    normalisation's own roundings are all there is).  Two paths form q.  (a) q = exp(log q~ - logZ): the exponential's
    argument is a difference of two doubles, rounded once before the exponential sees it -- EPS |log q~ - logZ|, which
    dominates for small q.  (b) where log q~ waits in LDS and LL_k is not asked for (and in the fused pass) q = e / s with
    e = exp(log q~ - max) kept from the sum: the argument's rounding is EPS |log q~ - max| <= EPS |log q~ - logZ|, the Newton
    reciprocal of s is good to a unit in the last place (2 EPS) and the product rounds once more (EPS)."""
    with np.errstate(invalid="ignore"):
        d = np.where(qref > 0, np.abs(lq - logZ[None, :]), 0).astype(np.float64)
    return hr.q_bar(qref, lqbar, lzbar[None, :]) + np.asarray(qref, dtype=np.float64) * EPS * (d + 3)


def check_normalised(tag, q, fz, ll, lq, lqbar, ctab, lay, blk, nblk):
    """q, the rows' sums, fz_part and ll_part of a normalising launch against the longdouble reference built on lq (exact
    inputs: lqbar = 0, the bars are those of the normalisation alone)"""
    K, NP = lq.shape
    valid = lay["valid"]
    lqbar = np.where(np.isfinite(lq.astype(np.float64)), lqbar, 0.0)
    logZ, qref, lzbar = hr.normalise_ref(lq, lqbar)
    assert exact_equal(q[:, ~valid], np.zeros((K, int((~valid).sum())))), "q of a pad row is not exactly 0.0"
    qv, qr = q[:, valid], qref[:, valid]
    assert np.isfinite(qv).all() and (qv >= 0).all()
    bar = q_bar_full(qr, lq[:, valid], logZ[valid], lqbar[:, valid], lzbar[valid])
    err = np.abs(qv.astype(hr.LD) - qr).astype(np.float64)
    r = [note(f"{tag} q", ratio_of(err, bar))]
    print(f"info {tag} q against the issue's formula alone: {ratio_of(err, hr.q_bar(qr, lqbar[:, valid], lzbar[valid][None, :])):.3g}")
    rs = np.abs(qv.astype(hr.LD).sum(axis=0) - 1).astype(np.float64)
    r.append(note(f"{tag} row sums", ratio_of(rs, bar.sum(axis=0) + (K - 1) * EPS)))
    fzr, fzb, llr, llb = hr.block_sums_ref(lq, logZ, qref, ctab, lay["grp"], valid, blk, nblk, lqbar, lzbar)
    r.append(note(f"{tag} fz_part", ratio_of(np.abs(fz.astype(hr.LD) - fzr).astype(np.float64), fzb)))
    if ll is not None:
        assert np.isfinite(ll).all(), "ll_part is not finite"
        r.append(note(f"{tag} ll_part", ratio_of(np.abs(ll.astype(hr.LD) - llr).astype(np.float64), llb + hr.TINY)))
    assert max(r) <= 1.0, r


def near_params(rng, K, D):
    """exact parameters whose clusters lie close: one integer whitener for all (diagonal +-1, a sub-diagonal of -1 / 0 / 1),
    centres one step apart in two coordinates -- log q~ of the clusters a few halves apart, so that the normalisation has q of
    every size to form"""
    A = np.diag(rng.choice([-1.0, 1.0], size=D))
    if D > 1:
        A[np.arange(1, D), np.arange(D - 1)] = rng.integers(-1, 2, size=D - 1)
    m0 = rng.integers(-2, 3, size=D).astype(np.float64)
    A, m = np.repeat(A[None], K, axis=0), np.repeat(m0[None], K, axis=0)
    for k in range(1, K):
        m[k, rng.integers(0, D, size=2)] += rng.integers(-1, 2, size=2)
    return A, m


def estep_case(rng, DP, DC, D, K, nrg, lay, raw, sparse, want_ll, kind, expect):
    plan = ah.estep_plan(DP, DC, K, nrg, raw=raw, sparse=sparse)
    assert plan["ok"] == 1 and plan["DC"] == DC and plan["pstride"] == hr.pstride(DP, DC)
    for key, v in expect.items():
        assert plan[key] == v, (key, plan)
    rpb = plan["rows_per_block"]
    assert plan["grid"] == (nrg * 16 + rpb - 1) // rpb
    NP = nrg * 16
    W = DP if DP > 128 else DC
    if kind == "exact":
        X = hr.exact_X(rng, NP, D, DP, lay["valid"], amp=2 if not raw else 7)
        A, m = hr.exact_params(rng, K, D) if raw else near_params(rng, K, D)
        ctab = sparse_ctab(rng, K) if sparse else hr.exact_ctab(rng, lay["J"], K)
    else:
        X, A, m, ctab = hr.rounding_problem(rng, K, D, NP, DP, lay["valid"], lay["J"])
    P = hr.pack_params(A, m, DP, DC)
    Au, bneg = hr.unpack_params(P, DP, DC)
    q, fz, ll = run_estep(X, DC, P, ctab, K, lay, plan, raw, sparse, want_ll)
    lq, T = hr.estep_ref(X, Au, bneg, ctab, lay["grp"], exact=kind == "exact")
    tag = f"estep {DP}/{DC} {kind}"
    if raw:
        if kind == "exact":
            assert exact_equal(q, lq), "raw log q~ of exact inputs differs"
        else:
            fin = np.isfinite(lq.astype(np.float64))
            assert np.array_equal(np.isfinite(q), fin)
            bar = hr.lq_bar(T, ctab[lay["grp"]].T, W)
            assert note(f"{tag} raw log q~", ratio_of(np.abs(q.astype(hr.LD) - lq).astype(np.float64)[fin], bar[fin])) <= 1.0
        return
    lqbar = np.zeros((K, NP)) if kind == "exact" else hr.lq_bar(T, np.where(np.isfinite(ctab), ctab, 0.0)[lay["grp"]].T, W)
    blk = np.arange(NP) // rpb
    check_normalised(tag, q, fz, ll, lq.astype(hr.LD), lqbar, ctab, lay, blk, plan["grid"])


def nrg_set(rpb):
    n = rpb // 16
    return (n - 1, n, n + 1, 2 * n + 1)


def expect_for(DP, K, raw, sparse):
    """the instance of a narrow launch: four row groups per wave at 64 / 80 columns for dense normalising launches from six
    clusters on (the K of these cases lie below the cap of the table); log q~ waits in LDS wherever a wave has four row groups
    and the launch normalises"""
    four = DP in (64, 80) and not raw and not sparse and K >= 6
    R, WAVES = (4, 4) if four else (ah.estep_cfg_r(DP), ah.estep_cfg_waves(DP))
    return dict(four_groups=int(four), lq_lds=int(R == 4 and not raw), rows_per_block=R * WAVES * 16), R


@pytest.mark.parametrize("DP,DC", NARROW)
def test_estep_narrow(DP, DC):
    """Every (DP, DC) instance estep_plan accepts; K in {1, 3, 4, 5, 9}; nrg one row group short of a block, a block, one more
    and two blocks + 1 (the last block then has missing row groups); one group with nrows no multiple of 16 / three groups
    with nvalid 0, 1, 15, 16 mid-launch; raw (exact inputs: all NP rows value for value, the pad rows too -- X is zero there by
    the layout's contract) and normalising (exact inputs whose clusters lie close: the normalisation alone against its bars;
    rounding inputs: the whole path); ll_part null and set; sparse tables at K >= 3."""
    rng = np.random.default_rng(1000 * DP + DC)
    D = DC - 1 if DC < DP else DP - 3
    for K in ES_K:
        for raw in (True, False):
            e, R = expect_for(DP, K, raw, False)
            n = e["rows_per_block"] // 16
            for i, nrg in enumerate(nrg_set(e["rows_per_block"])):
                lay = layout_nrows(nrg, nrg * 16 - 5) if i < 2 else layout_three_groups(nrg)
                estep_case(rng, DP, DC, D, K, nrg, lay, raw, False, want_ll=bool((i + K) & 1), kind="exact", expect=e)
            if K in (4, 9):
                estep_case(rng, DP, DC, D, K, n + 1, layout_three_groups(n + 1), raw, False, want_ll=True, kind="rounding", expect=e)
            if K >= 3:
                es, Rs = expect_for(DP, K, raw, True)
                ns = es["rows_per_block"] // 16
                for n2 in (ns + 1, 2 * ns + 1):
                    estep_case(rng, DP, DC, D, K, n2, layout_sparse(n2, Rs, ns), raw, True, want_ll=not raw, kind="exact", expect=es)


@pytest.mark.parametrize("DP", (64, 80))
def test_estep_four_row_groups_and_the_lq_lds_cap(DP):
    """D = 64 / 80: three row groups per wave below K = 6, four (log q~ in LDS) from 6 up to the cap of the table, three again
    beyond -- both sides of both thresholds, found by asking the plan (21 / 22 and 12 / 13 today), both active widths"""
    kcap = max(K for K in range(6, 64) if ah.estep_plan(DP, DP, K, 1)["four_groups"])
    assert ah.estep_plan(DP, DP, kcap + 1, 1)["four_groups"] == 0 and ah.estep_plan(DP, DP, 6, 1)["four_groups"] == 1
    assert ah.estep_plan(DP, DP, kcap, 1)["lds_bytes"] <= ah.ES_LQ_LDS_CAP < ah.estep_plan(DP, DP, kcap, 1)["lds_bytes"] + 2200  # (a cluster more: 256 + 4 doubles, 2 ints)
    rng = np.random.default_rng(DP)
    for DC in (DP, DP - 8):
        kc = max(K for K in range(6, 64) if ah.estep_plan(DP, DC, K, 1)["four_groups"])
        for K in (5, 6, kc, kc + 1):
            four = 6 <= K <= kc
            e = dict(four_groups=int(four), lq_lds=int(four), rows_per_block=256 if four else 192)
            for i, nrg in enumerate(nrg_set(e["rows_per_block"])):
                lay = layout_nrows(nrg, nrg * 16 - 3) if i % 2 else layout_three_groups(nrg)
                estep_case(rng, DP, DC, DC - 2, K, nrg, lay, False, False, want_ll=bool(i & 1), kind="exact", expect=e)
            nrg = e["rows_per_block"] // 16 + 1
            estep_case(rng, DP, DC, DC - 2, K, nrg, layout_three_groups(nrg), False, False, want_ll=K == 6, kind="rounding", expect=e)
            # raw and sparse launches never take the four-row-group instance
            e3 = dict(four_groups=0, lq_lds=0, rows_per_block=192)
            estep_case(rng, DP, DC, DC - 2, K, 13, layout_three_groups(13), True, False, want_ll=False, kind="exact", expect=e3)
            estep_case(rng, DP, DC, DC - 2, K, 13, layout_sparse(13, 3, 12), False, True, want_ll=True, kind="exact", expect=e3)


@pytest.mark.parametrize("DP,D", [(192, 129), (192, 192), (256, 190), (320, 300)])
def test_estep_wide(DP, D):
    """The register-resident instances (192, 256) and the streaming one (320); K in {1, 2, 5}; nrg around the 8 row groups of a
    block; the checks of the narrow layouts"""
    rng = np.random.default_rng(DP + D)
    rpb = ah.WIDE_R * ah.WIDE_WAVES * 16
    e = dict(four_groups=0, lq_lds=0, rows_per_block=rpb)
    for K in (1, 2, 5):
        for i, nrg in enumerate(nrg_set(rpb)):
            lay = layout_nrows(nrg, nrg * 16 - 5) if i < 2 else layout_three_groups(nrg)
            estep_case(rng, DP, DP, D, K, nrg, lay, True, False, want_ll=False, kind="exact", expect=e)
            estep_case(rng, DP, DP, D, K, nrg, lay, False, False, want_ll=bool((i + K) & 1), kind="exact", expect=e)
    nrg = rpb // 16 + 1
    for raw in (True, False):
        estep_case(rng, DP, DP, D, 2, nrg, layout_three_groups(nrg), raw, False, want_ll=True, kind="rounding", expect=e)


# ---- the statistics pass ---------------------------------------------------------------------------------------------------------
# what a launch leaves in the record entries of the idle columns DC .. DP - 1 (s, and the rows and columns of S): zeros, or
# nothing at all (SENT stays); the strict upper triangle of the active corner is the mirror image of the lower one everywhere
IDLE = {"per_cluster": "zero", "wide": "zero", "quad": "sent", "feat": "sent"}
#            DP   DC   K  route
SS_SHAPES = [(16, 16, 5, "per_cluster"), (16, 16, 33, "per_cluster"), (32, 28, 2, "per_cluster"), (48, 48, 1, "per_cluster"),
             (64, 64, 2, "per_cluster"), (64, 64, 33, "per_cluster"), (64, 64, 34, "per_cluster"), (80, 80, 5, "per_cluster"),
             (96, 96, 9, "per_cluster"), (112, 104, 3, "per_cluster"), (128, 128, 12, "per_cluster"), (128, 120, 4, "per_cluster"),
             (32, 32, 3, "quad"), (32, 20, 6, "quad"), (32, 32, 13, "quad"), (32, 24, 16, "quad"), (48, 40, 12, "quad"),
             (48, 48, 16, "quad"), (64, 64, 9, "quad"), (64, 56, 5, "quad"),
             (64, 64, 20, "feat"), (64, 64, 32, "feat"), (64, 56, 20, "feat"), (96, 96, 13, "feat"), (96, 88, 16, "feat"),
             (80, 72, 7, "feat"), (128, 128, 64, "feat"),
             (192, 192, 3, "wide"), (320, 320, 2, "wide")]
SS_NP = (16, 32, 48, 240, 256, 272, 1008, 1024, 1040, 2320)


def run_suffstat(X, DC, q, K, mode, nrec_of, fold=True, **kw):
    """-> plan, partial records [nrec x SS], folded [K x SS] (or None); nrec_of(plan) = records of the launch"""
    DP = X.shape[1]
    SS = hr.stat_stride(DP)
    plan0 = ah.suffstat_plan(DP, DC, X.shape[0], K, mode)
    nrec = nrec_of(plan0)
    qbuf = np.full((K, X.shape[0] + 48), SENT)  # ldq = NP + 48: a read past the rows poisons the sums
    qbuf[:, :X.shape[0]] = q
    q = qbuf
    outs = []
    for _ in range(2):
        part = np.full(nrec * SS + 64, SENT)
        fo = np.full(K * SS + 64, SENT) if fold else None
        rc, plan = ah.suffstat(X, DC, q, K, mode, part, folded=fo, **kw)
        assert rc == 0, (rc, plan)
        assert all(plan[k] == plan0[k] for k in plan), (plan, plan0)
        outs.append((part, fo))
    assert same_bits(outs[0][0], outs[1][0]) and (not fold or same_bits(outs[0][1], outs[1][1])), "a second launch gave other bits"
    part, fo = outs[0]
    assert untouched(part[nrec * SS:]) and (fo is None or untouched(fo[K * SS:])), "the guard behind the last record was written"
    return plan0, part[:nrec * SS].reshape(nrec, SS), None if fo is None else fo[:K * SS].reshape(K, SS)


def check_regions(rec, ref, DP, DC, route):
    """one record against the exact sums `ref` (full symmetric S): what the host reads, and what it never reads"""
    low = hr.lower_mask(DP, DC)
    s_idle, S_idle, upper = hr.region_masks(DP, DC)
    assert exact_equal(rec[low], ref[low]), "N, s or the lower triangle differ from the exact sums"
    assert exact_equal(rec[upper], ref[upper]), "the strict upper triangle is not the mirror image of the lower one"
    for m in (s_idle, S_idle):
        if IDLE[route] == "zero":
            assert exact_equal(rec[m], np.zeros(int(m.sum()))), "idle columns: zeros expected"
        else:
            assert untouched(rec[m]), "idle columns: expected to be left alone"


def dense_case(rng, DP, DC, D, K, route, NP, mode, seen):
    """dense grid (dense, masked dense, zero-skip with / without mask): every chunk's records, the extra records, the fold"""
    zs = mode.startswith("zero_skip")
    masked = mode in ("masked_dense", "zero_skip_masked")
    hmode = "zero_skip" if zs else mode
    lay = layout_three_groups(NP // 16) if masked else layout_nrows(NP // 16, NP - 3)
    X = hr.exact_X(rng, NP, D, DP, lay["valid"])
    q = hr.exact_q(rng, K, NP, zero_steps=zs)
    q[:, ~lay["valid"]] = 0.0
    kw, qeff = {}, q
    if masked:
        smask = rng.integers(0, 2, size=(3, K)).astype(np.uint8)
        smask[1] = 0
        smask[0, 0] = 1
        kw = dict(rginfo=lay["rginfo"], smask=smask)
        qeff = q * smask[lay["grp"]].T
    plan, part, fo = run_suffstat(X, DC, q, K, hmode, lambda p: p["nchunks"] * p["KR"], **kw)
    assert plan["route"] == (route if hmode == "dense" or route == "wide" else "per_cluster"), plan
    nch, cr, KR, extra, kl0 = plan["nchunks"], plan["chunk_rows"], plan["KR"], plan["extra"], plan["klast0"]
    assert cr % ah.SS_BR == 0 and (nch - 1) * cr < NP <= nch * cr and KR == K + extra
    seen.add((nch > 1, NP - (nch - 1) * cr - cr, extra > 0))
    wrote = plan["route"]
    nlast = K - kl0
    for c in range(nch):
        ref = hr.stats_ref(X, qeff, slice(c * cr, min(NP, (c + 1) * cr)))
        recs = part[c * KR:(c + 1) * KR]
        for k in range(K):
            if extra and k >= kl0:  # the row classes of the last slice add up to the chunk's sums
                assert extra % nlast == 0
                tot = recs[k].copy()
                for rc in range(extra // nlast):
                    tot = tot + recs[K + rc * nlast + (k - kl0)]
                low = hr.lower_mask(DP, DC)
                assert exact_equal(tot[low], ref[k][low]), "the regular and the extra records do not add up to the chunk's sums"
                for r2 in [recs[k]] + [recs[K + rc * nlast + (k - kl0)] for rc in range(extra // nlast)]:
                    S = r2[1 + DP:].reshape(DP, DP)
                    assert not np.isnan(r2).any() and np.array_equal(S, S.T) and not r2[1 + DC:1 + DP].any() and not S[DC:].any()
            else:
                check_regions(recs[k], ref[k], DP, DC, wrote)
    low = hr.lower_mask(DP, DC)
    assert exact_equal(fo[:, low], hr.stats_ref(X, qeff)[:, low]), "the folded result is not the exact total"


@pytest.mark.parametrize("DP,DC,K,route", SS_SHAPES)
def test_suffstat_dense_exact(DP, DC, K, route):
    """Exact inputs, the dense pass at every NP of SS_NP (one to three row groups; a chunk short of, equal to and beyond
    chunk_rows; several chunks with a ragged last one): every chunk's records equal the exact sums over that chunk's rows --
    N, s[0 .. DC), lower triangle --, the extra records of a ragged last slice add up with the regular ones, the fold is the
    exact total.  Regions nobody reads, pinned: the strict upper triangle is the MIRROR of the lower one on every route; the
    entries of the idle columns DC .. DP - 1 (s, rows and columns of S) are ZEROS after the per-cluster and wide kernels and
    UNTOUCHED after the feature-GEMM and the few-cluster (quad) kernels."""
    rng = np.random.default_rng(DP * 100 + DC + K)
    D = DC - 1 if DP <= 128 else DP - 9
    seen = set()
    for NP in SS_NP:
        dense_case(rng, DP, DC, D, K, route, NP, "dense", seen)
    assert any(multi and short < 0 for multi, short, _ in seen), "no ragged last chunk among the cases"
    assert any(short == -16 for _, short, _ in seen) and any(short == 0 for _, short, _ in seen), seen
    ragged = route == "per_cluster" and ah.suffstat_plan(DP, DC, 1040, K, "dense")["extra"] > 0
    assert ragged == any(x for _, _, x in seen)


def test_suffstat_ragged_k_cases_cover_two_and_four_row_classes():
    """remainders of one and two waves in the last cluster slice: 4 and 2 row classes, extra > 0 -- the shapes of SS_SHAPES"""
    classes = set()
    for DP, DC, K, route in SS_SHAPES:
        p = ah.suffstat_plan(DP, DC, 1040, K, "dense")
        assert p["route"] == route, (DP, DC, K, p)
        if p["extra"]:
            classes.add(p["extra"] // (K - p["klast0"]) + 1)
    assert classes == {2, 4}, classes


@pytest.mark.parametrize("DP,DC,K,route", SS_SHAPES)
@pytest.mark.parametrize("mode", ("masked_dense", "zero_skip", "zero_skip_masked"))
def test_suffstat_masked_and_zero_skip_exact(DP, DC, K, route, mode):
    """masked dense (three groups, a mask with an all-zero row), zero-skip with and without the mask (q with whole all-zero 4-row
    steps and steps with a single non-zero): the per-cluster kernel (panel launches beyond 128 columns) on the chunking of the
    shape's route"""
    rng = np.random.default_rng(DP * 100 + DC + K + len(mode))
    D = DC - 1 if DP <= 128 else DP - 9
    seen = set()
    for NP in (48, 272, 1040):
        dense_case(rng, DP, DC, D, K, route, NP, mode, seen)


def worklist(goff, smask, cpb, rows):
    """Context::build_sparse_worklist: items (r0, r1, kofs, kcnt, rec0), klist, nrec"""
    J, K = smask.shape
    klist, kofs = [], [0]
    for j in range(J):
        klist += [k for k in range(K) if smask[j, k]]
        kofs.append(len(klist))
    items, nrec = [], 0
    for j in range(J):
        na = kofs[j + 1] - kofs[j]
        for b0 in range(int(goff[j]), int(goff[j + 1]), rows):
            b1 = min(b0 + rows, int(goff[j + 1]))
            for s0 in range(0, na, cpb):
                kc = min(cpb, na - s0)
                items.append((b0, b1, kofs[j] + s0, kc, nrec))
                nrec += kc
    return items, np.array(klist, dtype=np.int32), nrec


@pytest.mark.parametrize("DP,DC,K", [(16, 16, 5), (32, 28, 9), (64, 64, 6), (64, 56, 20), (96, 96, 9), (128, 128, 3), (192, 192, 5)])
@pytest.mark.parametrize("skip", (False, True))
def test_suffstat_work_list_exact(DP, DC, K, skip):
    """the sparse work list (row ranges of one group x slices of that group's active clusters), with and without skip_listed:
    every record equals the exact sums of its rows and cluster, the fold (launch_reduce_records) the exact totals; a wrong
    list is refused by the hook before anything is launched"""
    rng = np.random.default_rng(DP + K + skip)
    D = DC - 1 if DP <= 128 else DP - 9
    counts = [260, 16 * 5 - 2, 300, 33]
    goff = ah.padded_offsets(counts)
    NP = int(goff[-1])
    valid = ah.valid_rows(counts)
    X = hr.exact_X(rng, NP, D, DP, valid)
    q = hr.exact_q(rng, K, NP, zero_steps=skip)
    q[:, ~valid] = 0.0
    smask = rng.integers(0, 2, size=(4, K)).astype(np.uint8)
    smask[1] = 0
    smask[0] = 1
    smask[2, K - 1] = 1
    plan0 = ah.suffstat_plan(DP, DC, NP, K, "work_list")
    assert plan0["route"] == ("wide" if DP > 128 else "per_cluster") and plan0["extra"] == 0
    items, klist, nrec = worklist(goff, smask, plan0["clusters_per_block"], 256)
    plan, part, fo = run_suffstat(X, DC, q, K, "work_list", lambda p: nrec, items=items, klist=klist, nrec=nrec, skip_listed=skip)
    route = plan["route"]
    tot = np.zeros((K, hr.stat_stride(DP)))
    for r0, r1, ko, kc, rec0 in items:
        ref = hr.stats_ref(X, q, slice(r0, r1))
        for t in range(kc):
            k = int(klist[ko + t])
            check_regions(part[rec0 + t], ref[k], DP, DC, route)
            tot[k] += ref[k]
    low = hr.lower_mask(DP, DC)
    assert exact_equal(fo[:, low], tot[:, low])
    # refusals: a row range past NP, a cluster past K, too many clusters for a block, overlapping records
    SS = hr.stat_stride(DP)
    r0, r1, ko, kc, rec0 = items[0]
    bad_lists = [[(r0, NP + 16, ko, kc, rec0)], [(r0 + 3, r1, ko, kc, rec0)], [(r0, r1, ko, plan0["clusters_per_block"] + 1, rec0)],
                 [(r0, r1, ko, kc, rec0), (r0, r1, ko, kc, rec0)], [(r0, r1, len(klist), 1, rec0)], [(r0, r1, ko, kc, nrec)]]
    for bad in bad_lists:
        part2 = np.full(nrec * SS + 64, SENT)
        rc, _ = ah.suffstat(X, DC, q, K, "work_list", part2, items=bad, klist=klist, nrec=nrec)
        assert rc == -1 and untouched(part2)
    kl2 = klist.copy()
    kl2[0] = K
    part2 = np.full(nrec * SS + 64, SENT)
    assert ah.suffstat(X, DC, q, K, "work_list", part2, items=items, klist=kl2, nrec=nrec)[0] == -1 and untouched(part2)


@pytest.mark.parametrize("DP,DC,K,route", SS_SHAPES)
def test_suffstat_rounding(DP, DC, K, route):
    """rounding inputs: the folded result within (n + 2) EPS sum |q x_i x_j| of the longdouble sums (hot_refs.stats_bar)"""
    rng = np.random.default_rng(DP + DC + K)
    D = DC - 1 if DP <= 128 else DP - 9
    NP = 1040 if K * DP * DP <= 50_000 else 272 if K * DP * DP <= 400_000 else 48
    valid = np.arange(NP) < NP - 3
    X, _, _, _ = hr.rounding_problem(rng, K, D, NP, DP, valid)
    q = rng.dirichlet(np.ones(K) * 0.3, NP).T.copy() if K > 1 else rng.uniform(size=(1, NP))
    q[:, ~valid] = 0.0
    plan, part, fo = run_suffstat(X, DC, q, K, "dense", lambda p: p["nchunks"] * p["KR"])
    assert plan["route"] == route
    low = hr.lower_mask(DP, DC)
    ref = hr.stats_ref(X, q, dtype=hr.LD)[:, low]
    bar = hr.stats_bar(hr.stats_abs(X, q)[:, low], NP)
    assert np.isfinite(fo[:, low]).all()
    assert note(f"suffstat {route} {DP}/{DC} K={K} folded", ratio_of(np.abs(fo[:, low].astype(hr.LD) - ref).astype(np.float64), bar + hr.TINY)) <= 1.0


def test_fold_extra_alone():
    """launch_fold_extra on synthetic integer records: rec[klast0 + e % nlast] += rec[K + e] for e = 0 .. extra - 1, nothing
    else moves -- one, two and three extra row classes, a last slice of one to three clusters"""
    rng = np.random.default_rng(3)
    for K, kl0, classes, SS in ((7, 4, 4, 37), (5, 4, 4, 273), (10, 8, 2, 1057), (3, 0, 3, 5), (4, 3, 1, 9)):
        nlast, extra = K - kl0, (classes - 1) * (K - kl0)
        rec0 = rng.integers(-1000, 1000, size=((K + extra), SS)).astype(np.float64)
        outs = []
        for _ in range(2):
            buf = np.concatenate([rec0.reshape(-1), np.full(16, SENT)])
            assert ah.fold_extra(buf, SS, K, kl0, extra) == 0
            outs.append(buf)
        assert same_bits(outs[0], outs[1]) and untouched(outs[0][rec0.size:])
        got = outs[0][:rec0.size].reshape(K + extra, SS)
        want = rec0.copy()
        for e in range(extra):
            want[kl0 + e % nlast] += rec0[K + e]
        assert exact_equal(got, want)
    buf = np.full(10, SENT)
    assert ah.fold_extra(buf, 5, 2, 1, 1) == -1 and ah.fold_extra(buf, 5, 1, 1, 1) == -1 and untouched(buf)


# ---- the fused pass -------------------------------------------------------------------------------------------------------------
def fused_blocks(NP, grid, cus):
    """-> block of every row under the restated deal, number of 256-row tiles"""
    ntile = (NP + ah.FUSED_ROWS - 1) // ah.FUSED_ROWS
    ys = hr.fused_yshare(grid, cus, ah.FUSED_YSHARE)
    tile_blk = np.full(ntile, -1, dtype=np.int64)
    for b in range(grid):
        t = hr.fused_deal(b, grid, ntile, ys)
        assert (tile_blk[t] == -1).all()
        tile_blk[t] = b
    assert (tile_blk >= 0).all()
    return np.repeat(tile_blk, ah.FUSED_ROWS)[:NP], ntile


def run_fused(X, D, P, ctab, K, lay, want_ll, grid):
    NP = X.shape[0]
    fp = ah.fused_plan(NP // 16, K)
    assert fp["eligible"] == 1 and fp["record"] == hr.fused_record(K)
    g = grid if grid else fp["grid"]
    W = fp["record"]
    outs = []
    for _ in range(2):
        q = np.full((K + 2, NP + 48), SENT)
        part = np.full(g * W + 32, SENT)
        rc, used = ah.fused(X, D, P, ctab, K, q, part, want_ll=want_ll, grid=grid, rginfo=lay["rginfo"], nrows=lay["nrows"])
        assert rc == 0 and used == g, (rc, used, g)
        outs.append((q, part))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), "a second launch gave other bits"
    q, part = outs[0]
    assert untouched(q[K:]) and untouched(q[:, NP:]) and untouched(part[g * W:])
    assert not np.isnan(part[:g * W]).any(), "a block left part of its record unwritten"
    return q[:K, :NP], part[:g * W].reshape(g, W), g, fp["cus"]


def fused_case(rng, D, K, NP, grid, groups, want_ll, kind):
    nrg = NP // 16
    SS = hr.stat_stride(16)
    if groups == "one":
        lay = layout_nrows(nrg, NP - 5)
    else:
        J = 3 if groups == "three" else ah.FUSED_CT_CAP // K + 3
        rgs = [((i * 7) % J if groups == "many" else (3 * i) // nrg, 16 if i % 4 else 11) for i in range(nrg)]
        lay = layout_groups(rgs)
        lay["J"] = J
        assert (J * K > ah.FUSED_CT_CAP) == (groups == "many")
    valid = lay["valid"]
    if kind == "exact":  # centres 64 apart on one axis, A = I: every q is exactly 0.0 or 1.0
        X = hr.exact_X(rng, NP, D, 16, valid, amp=7)
        lab = rng.integers(0, K, size=NP)
        X[:, 0] += 64.0 * lab
        X[~valid] = 0.0
        A = np.repeat(np.eye(D)[None], K, axis=0)
        m = np.zeros((K, D))
        m[:, 0] = 64.0 * np.arange(K)
        ctab = hr.exact_ctab(rng, lay["J"], K)
    else:
        X, A, m, ctab = hr.rounding_problem(rng, K, D, NP, 16, valid, lay["J"])
    P = hr.pack_params(A, m, 16, 16)
    Au, bneg = hr.unpack_params(P, 16, 16)
    q, part, g, cus = run_fused(X, D, P, ctab, K, lay, want_ll, grid)
    blk, ntile = fused_blocks(NP, g, cus)
    lq, T = hr.estep_ref(X, Au, bneg, ctab, lay["grp"], exact=kind == "exact")
    fz, ll = part[:, K * SS], part[:, K * SS + 1:]
    if not want_ll:
        assert exact_equal(ll, np.zeros((g, K))), "LL_k slots of a launch without LL_k are not zero"
    tag = f"fused D={D} K={K} {kind}"
    if kind == "exact":
        logZ, qref, _ = hr.normalise_ref(lq.astype(hr.LD))
        qref = np.where(valid[None, :], qref.astype(np.float64), 0.0)
        assert set(np.unique(qref)) <= {0.0, 1.0} and (K == 1 or (qref.sum(axis=0)[valid] == 1).all())
        assert exact_equal(q, qref), "q of the exact inputs is not exactly 0.0 / 1.0"
        logZ = logZ.astype(np.float64)
        for b in range(g):
            v = valid & (blk == b)
            assert fz[b] == -logZ[v].sum(), "Fz of a block"
            if want_ll:
                c = ctab[lay["grp"]].T
                assert exact_equal(ll[b], np.where(qref[:, v] > 0, lq[:, v] - c[:, v], 0.0).sum(axis=1)), "LL_k of a block"
    else:
        lqbar = hr.lq_bar(T, ctab[lay["grp"]].T, 16)
        check_normalised(tag, q, fz, ll if want_ll else None, lq, lqbar, ctab, lay, blk, g)
    # every block's statistics: the sums of the q the kernel returned over the block's tiles
    low = hr.lower_mask(16, 16)
    rmax = 0.0
    for b in range(g):
        rows = np.nonzero(blk == b)[0]
        recs = part[b, :K * SS].reshape(K, SS)
        S = recs[:, 17:].reshape(K, 16, 16)
        assert np.array_equal(S, S.transpose(0, 2, 1)), "S of a fused record is not symmetric"
        if kind == "exact":
            assert exact_equal(recs, hr.stats_ref(X, q, rows)), "a block's record differs from the exact sums of its tiles"
        else:
            ref = hr.stats_ref(X, q, rows, dtype=hr.LD)
            bar = hr.stats_bar(hr.stats_abs(X[rows], q[:, rows]), rows.size) + hr.TINY
            rmax = max(rmax, ratio_of(np.abs(recs.astype(hr.LD) - ref).astype(np.float64), bar))
    if kind != "exact":
        assert note(f"{tag} records", rmax) <= 1.0
    return ntile


FUSED_D, FUSED_K = (2, 4, 5, 8, 9, 16), (1, 4, 5, 8, 9, 16)


@pytest.mark.parametrize("D", FUSED_D)
@pytest.mark.parametrize("K", FUSED_K)
def test_fused(D, K):
    """All three NTA instances (D <= 4, <= 8, beyond) x the three CPW (K <= 4, <= 8, beyond); one group, three groups with the
    table in LDS, many small groups with J K > FUSED_CT_CAP; want_ll 0 and 1; NP in {16, 240, 256, 272, 3 x 256 + 16};
    grid in {1, 2, 3, ntile} (as far as the tiles go).  q, Fz and LL_k against the references, every block's record against
    the restated deal.  (A block without tiles cannot be launched through the hook: the grid never exceeds the tiles.)"""
    rng = np.random.default_rng(100 * D + K)
    idx = FUSED_D.index(D) * len(FUSED_K) + FUSED_K.index(K)
    for i, NP in enumerate((16, 240, 256, 272, 3 * 256 + 16)):
        ntile = (NP + 255) // 256
        grid = min((1, 2, 3, ntile)[(i + idx) % 4], ntile)
        groups = ("one", "three", "many")[(i + idx) % 3]
        for want_ll in (False, True):
            for kind in ("exact", "rounding"):
                fused_case(rng, D, K, NP, grid, groups, want_ll, kind)
    for grid in (1, 2, 3, 4):
        fused_case(rng, D, K, 3 * 256 + 16, grid, ("one", "three", "many")[(grid + idx) % 3], bool(grid & 1), "exact")


@pytest.mark.parametrize("which", range(4))
def test_fused_uneven_tile_deal(which):
    """G = 2 x CUs blocks (fused_plan) and 4 G - 1, 4 G, 4 G + 1, 4 G + G / 2 + 3 tiles: the first below the threshold of the
    uneven deal (every G-th tile), the others on it (a CU's second block takes 41 % of its tiles).  Exact inputs, D = 4,
    K = 2, centres 64 apart: every q exactly 0.0 or 1.0 and every block's record value for value the sums of the tiles the
    restated deal gives it."""
    cus = ah.fused_plan(16, 2)["cus"]
    G = 2 * cus
    ntile = (4 * G - 1, 4 * G, 4 * G + 1, 4 * G + G // 2 + 3)[which]
    NP = ntile * 256 - (240 if which == 3 else 0)
    fp = ah.fused_plan(NP // 16, 2)
    assert fp["grid"] == G, fp
    K, D, SS = 2, 4, hr.stat_stride(16)
    rng = np.random.default_rng(which)
    nrows = NP - 7
    valid = np.arange(NP) < nrows
    X = np.zeros((NP, 16))
    X[:, :D] = rng.integers(-7, 8, size=(NP, D))
    lab = rng.integers(0, K, size=NP)
    X[:, 0] += 64.0 * lab
    X[~valid] = 0.0
    m = np.zeros((K, D))
    m[:, 0] = 64.0 * np.arange(K)
    ctab = np.array([[1.5, -2.0]])
    P = hr.pack_params(np.repeat(np.eye(D)[None], K, axis=0), m, 16, 16)
    lay = layout_nrows(NP // 16, nrows)
    q, part, g, _ = run_fused(X, D, P, ctab, K, lay, True, 0)
    assert g == G
    ys = hr.fused_yshare(G, cus, ah.FUSED_YSHARE)
    assert ys == ah.FUSED_YSHARE and (ntile >= 4 * G) == (which > 0)
    # exact reference: log q~ = c - |x - m|^2 / 2 in float64 (integers and halves)
    d2 = np.stack([((X[:, :D] - m[k]) ** 2).sum(axis=1) for k in range(K)])
    lq = ctab[0][:, None] - d2 / 2
    qref = (lq == lq.max(axis=0)).astype(np.float64) * valid
    assert (qref.sum(axis=0)[valid] == 1).all() and np.abs(lq[0] - lq[1]).min() > 800
    assert exact_equal(q, qref), "q is not exactly 0.0 / 1.0"
    # per-tile sums (exact in float64 whatever the order), then per block by the restated deal
    pad = ntile * 256 - NP
    Xt = np.concatenate([X, np.zeros((pad, 16))]).reshape(ntile, 256, 16)
    qt = np.concatenate([qref, np.zeros((K, pad))], axis=1).reshape(K, ntile, 256)
    lzt = np.concatenate([np.where(valid, lq.max(axis=0), 0.0), np.zeros(pad)]).reshape(ntile, 256).sum(axis=1)
    llt = np.concatenate([qref * (-d2 / 2), np.zeros((K, pad))], axis=1).reshape(K, ntile, 256).sum(axis=2)
    rec_t = np.zeros((ntile, K, SS))
    for k in range(K):
        rec_t[:, k, 0] = qt[k].sum(axis=1)
        rec_t[:, k, 1:17] = np.einsum("tn,tni->ti", qt[k], Xt)
        rec_t[:, k, 17:] = np.matmul((Xt * qt[k][:, :, None]).transpose(0, 2, 1), Xt).reshape(ntile, 256)
    seen = np.zeros(ntile, dtype=int)
    for b in range(G):
        t = hr.fused_deal(b, G, ntile, ys)
        seen[t] += 1
        assert exact_equal(part[b, :K * SS].reshape(K, SS), rec_t[t].sum(axis=0)), f"record of block {b}"
        assert part[b, K * SS] == -lzt[t].sum() and exact_equal(part[b, K * SS + 1:], llt[:, t].sum(axis=1)), f"Fz / LL_k of block {b}"
    assert (seen == 1).all()


def test_hooks_refuse_what_would_be_an_address():
    """a wrong test comes back as -1 and nothing is launched"""
    rng = np.random.default_rng(0)
    X = hr.exact_X(rng, 32, 16, 16)
    P = hr.pack_params(np.eye(16)[None], np.zeros((1, 16)), 16, 16)
    c = np.zeros((1, 1))
    q, fz = np.full((1, 32), SENT), np.full(1, SENT)
    assert ah.estep(X, 16, P, c, 1, np.full((1, 16), SENT), fz) == -1          # ldq below the rows
    assert ah.estep(X, 16, P, c, 1, q, np.full(0, SENT)) == -1                  # no slot for the block's partial sum
    assert ah.estep(X, 16, P, c, 1, q, fz, nrows=33) == -1                      # more valid rows than rows
    assert ah.estep(X, 16, P, c, 1, q, fz, rginfo=np.array([16, (1 << 5) | 16], dtype=np.int32)) == -1  # a group past ctab
    assert ah.estep(X, 12, P, c, 1, q, fz) == -1                                # no such active width
    assert ah.estep(X, 16, P, c, 1, q, fz, ll_part=np.full(0, SENT)) == -1
    part = np.full(hr.fused_record(1) - 1, SENT)
    assert ah.fused(X, 16, P, c, 1, q, part)[0] == -1                           # a record does not fit
    part = np.full(4 * hr.fused_record(1), SENT)
    assert ah.fused(X, 16, P, c, 1, q, part, grid=2)[0] == -1                   # more blocks than tiles
    assert ah.fused(X, 17, P, c, 1, q, part)[0] == -1
    sp = np.full(hr.stat_stride(16), SENT)
    assert ah.suffstat(X, 16, np.zeros((1, 31)), 1, "dense", sp)[0] == -1       # ldq below NP
    assert ah.suffstat(X, 16, np.zeros((1, 32)), 1, "dense", sp[:-1].copy())[0] == -1
    assert ah.suffstat(X, 16, np.zeros((1, 32)), 1, "masked_dense", sp)[0] == -1  # no mask
    assert untouched(q) and untouched(fz) and untouched(part) and untouched(sp)


def test_zz_report_ratios():
    """the worst ratio of error to bar of every comparison of this file (pytest -s shows the table; docs/NOTEBOOK.md keeps it)"""
    for name in sorted(RATIOS):
        print(f"worst ratio {name}: {RATIOS[name]:.3g}")
    assert all(r <= 1.0 for r in RATIOS.values())
