"""launch_estep_diag (the difference-form VALU kernels and the matrix-pipe kernel) and launch_suffstat_diag, launcher by launcher,
through the lc_test_* hooks of libcluster_hip_testhooks.so (csrc/lc_testhooks.hip, tests/aux_hooks.py) against the references
of tests/diag_refs.py.

Every launch runs twice and must repeat its bits; every destination holds SENT (a NaN) before the launch, has ldq = NP + 16 and
is downloaded whole: rows past NP, columns past K, partial slots past nslots, fz_part / ll_part of a raw launch, the guard behind
the 256 sink entries and the guard behind the last record must keep it.  Every case asserts the plan it expects against the
restated plan (diag_refs.estep_plan_ref / stat_plan_ref), so no case can drift onto another kernel.

EXACT inputs are compared value for value (np.array_equal and no NaN); ROUNDING inputs against the bars of diag_refs / hot_refs,
each a first-order count of the rounded operations in EPS = 2^-52; the worst ratio of error to bar of every test is printed
(pytest -s), asserted <= 1 and recorded in docs/NOTEBOOK.md."""
import numpy as np
import pytest

import aux_hooks as ah
import diag_refs as dr
import hot_refs as hr
from test_gpu_hot_kernels import (check_normalised, exact_equal, layout_groups, layout_nrows, layout_three_groups, note, ratio_of,
                                  same_bits, untouched)

pytestmark = pytest.mark.gpu

SENT = np.nan
EPS = hr.EPS
GARBAGE = 3.0e5  # pad-row X: finite, far from anything a valid row holds


# ---- the E-step: one launch, twice, with every guard -----------------------------------------------------------------------------
def run_estep(X, P, mode, ctab, K, lay, raw, want_ll, packed=None, expect=None):
    """-> q [K x NP], fz [nslots], ll [nslots x K] or None, the plan.  packed = (mu, constk, wt): the matrix-pipe path."""
    NP = X.shape[0]
    nslots = (NP + 63) // 64
    outs = []
    for _ in range(2):
        q = np.full((K + 2, NP + 16), SENT)
        fz = np.full(nslots + 3, SENT)
        ll = np.full(nslots * K + 5, SENT) if want_ll else None
        sink = np.full(ah.DIAG_SINK + ah.DIAG_SINK_GUARD, SENT) if packed else None
        kw = dict(mu=packed[0], constk=packed[1], wt=packed[2], sink=sink) if packed else {}
        rc, plan = ah.estep_diag(X, P, mode, ctab, K, q, fz, ll, rginfo=lay["rginfo"], nrows=lay["nrows"], raw=raw, **kw)
        assert rc == 0, (rc, plan)
        outs.append((q, fz, ll, sink))
    for a, b in zip(outs[0], outs[1]):
        assert (a is None and b is None) or same_bits(a, b), "a second launch gave other bits"
    q, fz, ll, sink = outs[0]
    DP = X.shape[1]
    ref = dr.estep_plan_ref(DP, K, mode, NP // 16, mfma=packed is not None, raw=raw, want_ll=want_ll, grouped=lay["rginfo"] is not None,
                            ngroups=lay["J"], cus=(plan["block_cap"] // plan["per_cu"]) if packed else None)
    assert {k: plan[k] for k in ref} == ref, (plan, ref)
    for key, v in (expect or {}).items():
        assert plan[key] == v, (key, v, plan)
    assert untouched(q[K:]) and untouched(q[:, NP:]), "a store outside the K columns / NP rows"
    assert untouched(fz[nslots:]) and (ll is None or untouched(ll[nslots * K:])), "a partial sum outside the slots"
    if raw:
        assert untouched(fz) and (ll is None or untouched(ll)), "a raw launch wrote partial sums"
    if sink is not None:
        assert untouched(sink[ah.DIAG_SINK:]), "a store behind the 256 sink entries"
        s = sink[:ah.DIAG_SINK]
        assert (np.isnan(s) | (s == 0.0)).all(), "the sink holds something else than zeros"
        if raw:
            assert untouched(s), "a raw launch stored to the sink"
    return q[:K, :NP], fz[:nslots], None if ll is None else ll[:nslots * K].reshape(nslots, K), plan


def split_slots(plan, fz, ll):
    """matrix-pipe launches: the slots of the grid, after asserting that the slots past it are exactly 0.0"""
    g = plan["grid"]
    assert exact_equal(fz[g:], np.zeros(fz.size - g)), "fz_part past the grid is not 0.0"
    if ll is not None:
        assert exact_equal(ll[g:], np.zeros_like(ll[g:])), "ll_part past the grid is not 0.0"
    return fz[:g], None if ll is None else ll[:g]


def garbage_pad_rows(rng, X, valid):
    X = X.copy()
    n = int((~valid).sum())
    X[~valid] = GARBAGE * rng.choice([-1.0, 1.0], size=(n, 1)) * (1 + rng.random((n, X.shape[1])))
    return X


def with_ninf(ctab, lay, K):
    """c = -inf for one column in one group only (several groups, K >= 2)"""
    ctab = ctab.copy()
    if lay["J"] >= 2 and K >= 2:
        ctab[1, K // 2] = -np.inf
    return ctab


def check_ninf(q, ctab, lay):
    for j, k in zip(*np.nonzero(np.isneginf(ctab))):
        assert exact_equal(q[k, lay["grp"] == j], np.zeros(int((lay["grp"] == j).sum()))), "q of a column with c = -inf is not exactly 0"


def valu_exact_raw(rng, DP, D, mode, K, lay, want_ll):
    NP = lay["NP"]
    X = dr.distinct_X(rng, NP, D, DP)
    a, w2, w1 = dr.exact_diag_params(rng, K, D, mode)
    P = dr.pad_params(a, w2, w1, DP)
    ctab = dr.exact_ctab(rng, lay["J"], K)
    q, _, _, _ = run_estep(X, P, mode, ctab, K, lay, True, want_ll)
    lq, _, _ = dr.diff_ref(X, P, ctab, lay["grp"], exact=True)
    assert exact_equal(q, lq), f"raw log q~ of exact inputs differs ({DP}, {mode}, {K}, {NP})"


def valu_rounding(rng, tag, DP, D, mode, K, lay, want_ll, raw=False):
    NP = lay["NP"]
    X, a, w2, w1, ctab = dr.rounding_diag_problem(rng, K, D, NP, DP, mode, lay["valid"], lay["J"])
    ctab = ctab if raw else with_ninf(ctab, lay, K)
    P = dr.pad_params(a, w2, w1, DP)
    Xg = X if raw else garbage_pad_rows(rng, X, lay["valid"])
    q, fz, ll, plan = run_estep(Xg, P, mode, ctab, K, lay, raw, want_ll)
    lq, S2, S1 = dr.diff_ref(X, P, ctab, lay["grp"])
    bar = dr.valu_bar(S2, S1, ctab, lay["grp"], DP, mode)
    if raw:
        err = np.abs(q.astype(hr.LD) - lq).astype(np.float64)
        assert note(f"{tag} raw log q~", ratio_of(err, bar)) <= 1.0
        return
    check_normalised(tag, q, fz, ll, lq, bar, ctab, lay, np.arange(NP) // 64, plan["grid"])
    check_ninf(q, ctab, lay)


VALU_NP = (16, 48, 64, 144)


def layouts_of(NP):
    nrg = NP // 16
    return (layout_nrows(nrg, NP - 5), layout_three_groups(nrg))


@pytest.mark.parametrize("K", (1, 3, 4, 5, 8, 9, 64, 65))
@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("DP", (16, 48, 80, 112, 128))
def test_estep_valu(DP, mode, K):
    """estep_diag_kernel: KT = 1 / 2 / 4 (K <= 4, <= 8, beyond), waves without a tile (K = 1, 3, 5), a ragged last tile, all 16
    register slots full (K = 64) and the path that re-reads its columns from L2 (K = 65); 16, 48, 64 and 144 rows (a partial last
    block, a whole one, two and a quarter); one group with nrows no multiple of 16 and three groups with counts 0, 1, 15, 16.
    Raw launches on exact inputs with distinct X per tile, with and without ll_part (which a raw launch must leave alone);
    normalising launches on rounding inputs with garbage in the pad rows of X and a column with c = -inf in one group."""
    rng = np.random.default_rng(10000 * DP + 100 * mode + K)
    D = DP - 3
    exp = dict(KT=1 if K <= 4 else 2 if K <= 8 else 4, REG=int(K <= 64), wide=0, name="estep_diag_kernel")
    assert {k: ah.estep_diag_plan(DP, K, mode, 9, mfma=False)[k] for k in exp} == exp
    for i, NP in enumerate(VALU_NP):
        for j, lay in enumerate(layouts_of(NP)):
            valu_exact_raw(rng, DP, D, mode, K, lay, want_ll=bool((i + j) & 1))
            valu_rounding(rng, f"valu {DP} mode {mode}", DP, D, mode, K, lay, want_ll=bool((i + j + K) & 1))


@pytest.mark.parametrize("K", (3, 17, 65))
@pytest.mark.parametrize("DP", (192, 256))
def test_estep_valu_wide(DP, K):
    """estep_diag_wide_kernel: a whole and a half last chunk of 128 columns; registers (K = 3, 17) and the running sum
    c + acc_0 + acc_1 kept in qZ (K = 65), raw and normalising"""
    rng = np.random.default_rng(DP + K)
    D = DP - 7
    for mode in (0, 1, 2):
        for NP in (48, 144):
            for j, lay in enumerate(layouts_of(NP)):
                valu_exact_raw(rng, DP, D, mode, K, lay, want_ll=bool(j))
                valu_rounding(rng, f"valu wide {DP}", DP, D, mode, K, lay, want_ll=not j)
        valu_rounding(rng, f"valu wide {DP}", DP, D, mode, K, layout_three_groups(5), want_ll=False, raw=True)


# ---- the matrix-pipe kernel ----------------------------------------------------------------------------------------------------------
def int_centre(rng, D, DP, mode):
    mu = np.zeros(DP)
    if mode != 2:
        mu[:D] = rng.integers(-2, 3, size=D)
    return mu


def mfma_exact_raw(rng, DP, D, mode, K, lay, want_ll, expect=None):
    NP = lay["NP"]
    X = dr.distinct_X(rng, NP, D, DP, tile_rows=64 * dr.edm_r(DP // 4))
    a, w2, w1 = dr.exact_diag_params(rng, K, D, mode)
    P = dr.pad_params(a, w2, w1, DP)
    ctab = dr.exact_ctab(rng, lay["J"], K)
    packed = dr.pack_diag(a, w2, w1, DP, mode, mu=int_centre(rng, D, DP, mode))
    q, _, _, _ = run_estep(X, P, mode, ctab, K, lay, True, want_ll, packed=packed, expect=expect)
    lq, _, _ = dr.diff_ref(X, P, ctab, lay["grp"], exact=True)
    assert exact_equal(q, lq), f"raw log q~ of exact inputs differs ({DP}, {mode}, {K}, {NP})"


def mfma_problem(rng, DP, D, mode, K, lay, ninf=True):
    """a rounding input, its packed operands, the longdouble bilinear form on them and its bar"""
    NP = lay["NP"]
    X, a, w2, w1, ctab = dr.rounding_diag_problem(rng, K, D, NP, DP, mode, lay["valid"], lay["J"])
    ctab = with_ninf(ctab, lay, K) if ninf else ctab
    P = dr.pad_params(a, w2, w1, DP)
    mu, ck, wt = dr.pack_diag(a, w2, w1, DP, mode)
    W2, WL = dr.unpack_diag(wt, DP, K, mode)
    lq, SQ, SL = dr.bilinear_ref(X, mu, ck, W2, WL, ctab, lay["grp"])
    bar = dr.mfma_bar(SQ, SL, ck, ctab, lay["grp"], DP, mode)
    return dict(X=X, Xg=garbage_pad_rows(rng, X, lay["valid"]), P=P, ctab=ctab, packed=(mu, ck, wt), lq=lq, bar=bar, mode=mode, K=K)


def mfma_check(tag, pb, lay, want_ll, expect=None, raw=False):
    NP, K = lay["NP"], pb["K"]
    q, fz, ll, plan = run_estep(pb["X"] if raw else pb["Xg"], pb["P"], pb["mode"], pb["ctab"], K, lay, raw, want_ll, packed=pb["packed"],
                                expect=expect)
    if raw:
        err = np.abs(q.astype(hr.LD) - pb["lq"]).astype(np.float64)
        assert note(f"{tag} raw log q~", ratio_of(err, pb["bar"])) <= 1.0
        return plan
    fz, ll = split_slots(plan, fz, ll)
    check_normalised(tag, q, fz, ll, pb["lq"], pb["bar"], pb["ctab"], lay, dr.mfma_block_of_rows(NP, plan["R"], plan["grid"]), plan["grid"])
    check_ninf(q, pb["ctab"], lay)
    return plan


def mfma_rounding(rng, tag, DP, D, mode, K, lay, want_ll, expect=None, raw=False, ninf=True):
    return mfma_check(tag, mfma_problem(rng, DP, D, mode, K, lay, ninf=ninf and not raw), lay, want_ll, expect=expect, raw=raw)


@pytest.mark.parametrize("K", (1, 4, 5, 8, 12, 29, 32, 33, 40))
@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("DP", (16, 48, 64, 80, 128))
def test_estep_mfma(DP, mode, K):
    """estep_diag_mfma_kernel: R = 2 (DP <= 64) and 1, ring depths 4 (DP = 48, 80) and 8, the quadratic + linear halves (mode 1)
    and the linear half alone (mode 2); K with paired cluster tiles (8), an odd last tile on its own ring (12 = 3 tiles, 5 and 29
    with padding clusters as well), one tile (1, 4), all eight register tiles (32) and the per-lane LDS slots (33, 40: KTM = 0).
    nrg = 4 R + 3: the second tile lacks row groups.  The generic instance raw (exact inputs, value for value) and with ll_part;
    the one-group instance with nrows ending mid row group and at 0 rows of the last group; the plain / tabled instances with
    three groups (counts 0, 1, 15, 16)."""
    rng = np.random.default_rng(20000 * DP + 100 * mode + K)
    D = DP - 3
    R = dr.edm_r(DP // 4)
    nrg = 4 * R + 3
    regs = K <= 32
    base = dict(R=R, KTM=8 if regs else 0, QUAD=int(mode != 2), NT=DP // 4, grid=2)
    one, three = layout_nrows(nrg, nrg * 16 - 5), layout_three_groups(nrg)
    tag = f"mfma {DP} mode {mode}"
    for lay in (one, three):
        mfma_exact_raw(rng, DP, D, mode, K, lay, want_ll=lay is three, expect=dict(base, instance="generic"))
        mfma_rounding(rng, tag + " ll", DP, D, mode, K, lay, want_ll=True, expect=dict(base, instance="generic"))
    mfma_rounding(rng, tag, DP, D, mode, K, three, want_ll=False, raw=True, expect=dict(base, instance="generic"))
    inst = "one_group" if regs else "generic"
    mfma_rounding(rng, tag + " one group", DP, D, mode, K, one, want_ll=False, expect=dict(base, instance=inst))
    mfma_rounding(rng, tag + " one group", DP, D, mode, K, layout_nrows(nrg, (nrg - 1) * 16), want_ll=False, expect=dict(base, instance=inst))
    mfma_rounding(rng, tag + " groups", DP, D, mode, K, three, want_ll=False, expect=dict(base, instance="tabled" if regs else "generic"))


@pytest.mark.parametrize("DP,mode", [(16, 0), (80, 0), (64, 0)])
def test_estep_mfma_general_mode(DP, mode):
    """mode 0 (a, w2 and w1 all present) on the matrix pipe: the linear weights w1 - 2 w2 a' and constk's w1 mu term"""
    rng = np.random.default_rng(DP)
    R = dr.edm_r(DP // 4)
    for K in (5, 12, 33):
        lay = layout_three_groups(4 * R + 1)
        mfma_exact_raw(rng, DP, DP - 1, mode, K, lay, want_ll=False)
        mfma_rounding(rng, f"mfma {DP} mode 0", DP, DP - 1, mode, K, lay, want_ll=True)
        mfma_rounding(rng, f"mfma {DP} mode 0", DP, DP - 1, mode, K, lay, want_ll=False)


def spread_groups(nrg, J):
    """nrg row groups over J groups, ascending, the last row group in group J - 1; a few counts below 16"""
    rgs = [(min(J - 1, i * J // nrg), 16) for i in range(nrg)]
    rgs[-1] = (J - 1, 9)
    rgs[1] = (rgs[1][0], 0)
    rgs[2] = (rgs[2][0], 15)
    return layout_groups(rgs)


@pytest.mark.parametrize("K,J,instance", [(32, 32, "tabled"), (8, 128, "tabled"), (25, 41, "plain"), (5, 205, "plain"), (32, 33, "plain"),
                                          (1, 1024, "tabled"), (1, 1025, "plain")])
@pytest.mark.parametrize("DP", (16, 80))
def test_estep_mfma_table_in_lds_up_to_the_cap(DP, K, J, instance):
    """the tabled instance at J K = EDM_CT_CAP = 1024 exactly, the plain untabled one at 1025: rows of the highest group read
    the last entries of the table"""
    assert (J * K <= dr.EDM_CT_CAP) == (instance == "tabled")
    rng = np.random.default_rng(DP + K + J)
    R = dr.edm_r(DP // 4)
    lay = spread_groups(4 * R + 3, J)
    assert lay["J"] == J
    mfma_rounding(rng, f"mfma {DP} {instance}", DP, DP - 3, 1, K, lay, want_ll=False, expect=dict(instance=instance), ninf=K > 1)
    mfma_rounding(rng, f"mfma {DP} {instance}", DP, DP - 3, 2, K, lay, want_ll=False, expect=dict(instance=instance), ninf=K > 1)


@pytest.mark.parametrize("DP", (16, 80))
def test_estep_mfma_blocks_run_several_tiles(DP):
    """Persistent blocks: ntile = 2 cap + cap / 2 tiles on cap blocks (the plan's block cap), so that the first half of the blocks
    runs three tiles and the rest two: the prefetch across tiles and the zeroing of the slots past the grid, value for value on
    exact inputs (raw) and block by block against the bars (one-group, normalising)."""
    rng = np.random.default_rng(DP)
    K, mode, D = 3, 1, DP - 3
    R = dr.edm_r(DP // 4)
    cap = ah.estep_diag_plan(DP, K, mode, 1 << 20, mfma=True)["block_cap"]
    assert cap >= 2 and cap % 2 == 0
    ntile = 2 * cap + cap // 2
    nrg = ntile * 4 * R
    exp = dict(grid=cap, R=R, nslots=nrg // 4)
    assert exp["nslots"] > cap
    lay = layout_nrows(nrg, nrg * 16 - 21)
    mfma_exact_raw(rng, DP, D, mode, K, lay, want_ll=False, expect=dict(exp, instance="generic"))
    pb = mfma_problem(rng, DP, D, mode, K, lay)
    mfma_check(f"mfma {DP} several tiles", pb, lay, want_ll=False, expect=dict(exp, instance="one_group"))
    mfma_check(f"mfma {DP} several tiles ll", pb, lay, want_ll=True, expect=dict(exp, instance="generic"))


@pytest.mark.parametrize("DP,K,mode", [(16, 5, 1), (48, 9, 1), (64, 32, 1), (80, 12, 0), (128, 8, 1), (112, 40, 1), (96, 3, 2)])
def test_both_estep_paths_on_one_input(DP, K, mode):
    """One well-conditioned rounding input through both paths, raw: each against its own longdouble form and bar, and the two
    longdouble forms against each other within the packer's roundings"""
    rng = np.random.default_rng(7 * DP + K)
    D = DP - 2
    lay = layout_three_groups(9)
    NP = lay["NP"]
    X, a, w2, w1, ctab = dr.rounding_diag_problem(rng, K, D, NP, DP, mode, lay["valid"], lay["J"])
    P = dr.pad_params(a, w2, w1, DP)
    mu, cond = dr.centre(a, w2, DP, mode)
    assert cond <= 4096.0, "not a case Context::estep_diag would hand to the matrix pipe"
    mu, ck, wt = dr.pack_diag(a, w2, w1, DP, mode)
    W2, WL = dr.unpack_diag(wt, DP, K, mode)
    lqd, S2, S1 = dr.diff_ref(X, P, ctab, lay["grp"])
    lqb, SQ, SL = dr.bilinear_ref(X, mu, ck, W2, WL, ctab, lay["grp"])
    tag = f"both paths {DP}"
    r = [note(tag + " forms against the packing bar", ratio_of(np.abs(lqd - lqb).astype(np.float64), dr.packing_bar(X, P, mu, W2, WL)))]
    qv, _, _, _ = run_estep(X, P, mode, ctab, K, lay, True, False)
    qm, _, _, _ = run_estep(X, P, mode, ctab, K, lay, True, False, packed=(mu, ck, wt))
    r.append(note(tag + " valu", ratio_of(np.abs(qv.astype(hr.LD) - lqd).astype(np.float64), dr.valu_bar(S2, S1, ctab, lay["grp"], DP, mode))))
    r.append(note(tag + " mfma", ratio_of(np.abs(qm.astype(hr.LD) - lqb).astype(np.float64), dr.mfma_bar(SQ, SL, ck, ctab, lay["grp"], DP, mode))))
    assert max(r) <= 1.0, r


def test_estep_hook_refuses_wrong_calls():
    """everything the kernels would use as an address is checked on the host: -1, and the destinations keep their sentinels"""
    rng = np.random.default_rng(1)
    DP, K, NP = 16, 3, 32
    lay = layout_nrows(2, 30)
    X = dr.distinct_X(rng, NP, DP, DP)
    a, w2, w1 = dr.exact_diag_params(rng, K, DP, 1)
    P = dr.pad_params(a, w2, w1, DP)
    ctab = dr.exact_ctab(rng, 1, K)
    mu, ck, wt = dr.pack_diag(a, w2, w1, DP, 1, mu=np.zeros(DP))

    def call(**kw):
        args = dict(X=X, P=P, mode=1, ctab=ctab, K=K, q=np.full((K, NP + 16), SENT), fz=np.full(1, SENT), ll=None, rginfo=None,
                    nrows=30, wt=None, mu=None, ck=None, sink=None)
        args.update(kw)
        rc, _ = ah.estep_diag(args["X"], args["P"], args["mode"], args["ctab"], args["K"], args["q"], args["fz"], args["ll"],
                              rginfo=args["rginfo"], nrows=args["nrows"], wt=args["wt"], mu=args["mu"], constk=args["ck"], sink=args["sink"])
        assert untouched(args["q"]) and untouched(args["fz"])
        return rc

    sink = np.full(320, SENT)
    assert call(q=np.full((K, NP - 16), SENT)) == -1                       # nrg * 16 > ldq
    assert call(fz=np.full(0, SENT)) == -1                                 # fewer slots than blocks
    assert call(ll=np.full(K - 1, SENT)) == -1                             # ll_part below nslots * K
    assert call(nrows=NP + 1) == -1
    assert call(rginfo=np.array([16, (1 << 5) | 16], dtype=np.int32)) == -1  # a group index beyond the table
    assert call(rginfo=np.array([16, 17], dtype=np.int32)) == -1            # 17 rows in a row group
    assert call(wt=wt[:-16], mu=mu, ck=ck, sink=sink) == -1                 # not estep_diag_mfma_weights doubles
    assert call(wt=wt, mu=mu, ck=ck, sink=None) == -1
    assert call(mu=mu) == -1                                                # operands of the other path
    X24 = np.zeros((NP, 24))
    assert call(X=X24, P=np.zeros((3, K, 24))) == -1                       # a width without an instance
    assert untouched(sink)


# ---- the statistics pass -------------------------------------------------------------------------------------------------------------
def run_stat(X, q, K, chunk_rows, second, lay=None, smask=None, fold=True):
    """-> records [nchunks x RS x K x SS], the folded record [K x SS] or None, the plan"""
    NP, DP = X.shape
    SS = 1 + 2 * DP
    nchunks = (NP + chunk_rows - 1) // chunk_rows
    RS = dr.sd_rsplit(K)
    qbuf = np.full((K, NP + 16), SENT)  # (rows past NP: nobody may read them)
    qbuf[:, :NP] = q
    n = nchunks * RS * K * SS
    outs = []
    for _ in range(2):
        part = np.full(n + 7, SENT)
        folded = np.full(K * SS + 3, SENT) if fold else None
        rc, plan = ah.suffstat_diag(X, qbuf, K, nchunks, chunk_rows, second, part, rginfo=None if smask is None else lay["rginfo"],
                                    smask=smask, folded=folded)
        assert rc == 0, (rc, plan)
        outs.append((part, folded))
    for a, b in zip(outs[0], outs[1]):
        assert (a is None and b is None) or same_bits(a, b), "a second launch gave other bits"
    part, folded = outs[0]
    ref = dr.stat_plan_ref(DP, K, second)
    assert {k: plan[k] for k in ref if k != "name"} == {k: v for k, v in ref.items() if k != "name"}, (plan, ref)
    assert untouched(part[n:]), "a store behind the last record"
    assert not np.isnan(part[:n]).any(), "an entry of a record was left unwritten"
    if fold:
        assert untouched(folded[K * SS:])
        folded = folded[:K * SS].reshape(K, SS)
    return part[:n].reshape(nchunks, RS, K, SS), folded, plan


def stat_exact(rng, DP, K, chunk_rows, second, NP=None, masked=False, garbage=False):
    NP = 2 * chunk_rows - 16 if NP is None else NP
    D = DP - 3
    lay = layout_three_groups(NP // 16)
    X = hr.exact_X(rng, NP, D, DP, lay["valid"] if garbage else None)
    q = hr.exact_q(rng, K, NP)
    smask = None
    if garbage:  # pad rows: q = 0 against finite garbage in X must change no bit
        q[:, ~lay["valid"]] = 0.0
        Xg = garbage_pad_rows(rng, X, lay["valid"])
    qeff = q
    if masked:
        smask = (rng.random((lay["J"], K)) < 0.6).astype(np.uint8)
        smask[0, K - 1], smask[1, K - 1], smask[lay["J"] - 1, 0] = 0, 1, 0
        qeff = np.where(smask[lay["grp"]].T != 0, q, 0.0)
    rec, folded, plan = run_stat(Xg if garbage else X, q, K, chunk_rows, second, lay, smask)
    ref = dr.stat_records_ref(X, qeff, chunk_rows, rec.shape[0], plan["rsplit"], plan["nstage"], second)
    assert exact_equal(rec, ref), f"a statistics record differs ({DP}, {K}, {chunk_rows}, {second})"
    # N_k: the sum over a chunk's row-class records, value for value; summed at staging: the classes >= 1 hold exactly 0
    for c in range(rec.shape[0]):
        r0, r1 = c * chunk_rows, min((c + 1) * chunk_rows, NP)
        assert exact_equal(rec[c, :, :, 0].sum(axis=0), qeff[:, r0:r1].sum(axis=1))
    if plan["nstage"] and plan["rsplit"] > 1:
        assert exact_equal(rec[:, 1:, :, 0], np.zeros_like(rec[:, 1:, :, 0]))
    if not second:
        assert exact_equal(rec[..., 1 + DP:], np.zeros_like(rec[..., 1 + DP:])), "second = 0 must store xx_s = 0.0"
    assert exact_equal(folded, ref.sum(axis=(0, 1))), "the folded record differs"
    return plan


STAT_DP = (16, 48, 64, 80, 96, 112, 128)
STAT_K = (1, 5, 16, 17, 32, 33, 50, 64, 65, 130)
STAT_CHUNKS = (32, 64, 96, 160, 224)


@pytest.mark.parametrize("K", STAT_K)
@pytest.mark.parametrize("DP", STAT_DP)
def test_suffstat_diag_every_width_and_cluster_count(DP, K):
    """RS = 4 (K <= 16), 2 (17 .. 32) and 1; ragged groups of 16 and of 4 clusters, inactive waves (K = 1, 5, 33), a second and a
    third slice (65, 130); two chunk lengths per case, NP = 2 chunk_rows - 16: a whole chunk and a short one whose last batch is
    half full; second = 0 where the exponential family runs"""
    rng = np.random.default_rng(1000 * DP + K)
    i = STAT_DP.index(DP) + STAT_K.index(K)
    plan = stat_exact(rng, DP, K, STAT_CHUNKS[i % 5], 1)
    assert plan["rsplit"] == (4 if K <= 16 else 2 if K <= 32 else 1) and plan["BR"] == (32 if DP <= 64 else 16)
    stat_exact(rng, DP, K, STAT_CHUNKS[(i + 2) % 5], int(DP not in (16, 64, 112)), garbage=True)


@pytest.mark.parametrize("chunk_rows", STAT_CHUNKS)
@pytest.mark.parametrize("DP", STAT_DP)
def test_suffstat_diag_every_chunk_length(DP, chunk_rows):
    """the three batch loops at every chunk length: 1, 2, 3, 5, 7 batches of 32 rows (2 ... 14 of 16): a single batch, one pair,
    pair + odd, the whole-batch loop entered once and twice with both tails; for every row split"""
    rng = np.random.default_rng(DP + chunk_rows)
    for K in (5, 17, 33):
        stat_exact(rng, DP, K, chunk_rows, 1)
    stat_exact(rng, DP, 5, chunk_rows, 0)
    stat_exact(rng, DP, 9, chunk_rows, 1, NP=3 * chunk_rows)  # whole chunks only


@pytest.mark.parametrize("K", (5, 70))
@pytest.mark.parametrize("DP", (16, 64, 96, 128))
def test_suffstat_diag_masked(DP, K):
    """rginfo + smask: masked pairs in the first and (K = 70) in the second slice are staged as zeros"""
    rng = np.random.default_rng(DP + K)
    for chunk_rows in (64, 160):
        stat_exact(rng, DP, K, chunk_rows, 1, masked=True)
        stat_exact(rng, DP, K, chunk_rows, 0, masked=True, garbage=True)


@pytest.mark.parametrize("DP", (192, 256, 320))
def test_suffstat_diag_wide(DP):
    """one launch per block of 128 columns, the last one of 64 at 192 and 320: every column block of every record"""
    rng = np.random.default_rng(DP)
    for K, chunk_rows in ((5, 96), (17, 160), (33, 64), (70, 224)):
        plan = stat_exact(rng, DP, K, chunk_rows, 1)
        assert plan["nblocks"] == (DP + 127) // 128 and plan["last_width"] == (64 if DP % 128 else 128) and plan["BR"] == 16
    stat_exact(rng, DP, 5, 64, 0, masked=True)


@pytest.mark.parametrize("DP,K,chunk_rows", [(16, 5, 224), (64, 17, 160), (80, 33, 96), (128, 8, 64), (192, 5, 160)])
def test_suffstat_diag_rounding(DP, K, chunk_rows):
    """normal data and responsibilities of every size against (n + 2) EPS sum |q x| (|q x^2|): q x^2 is formed with two roundings
    (the square, the matrix pipe's product-add), the n rows of a record are added once each"""
    rng = np.random.default_rng(DP + K)
    NP = 2 * chunk_rows - 16
    X = np.zeros((NP, DP))
    X[:, :DP - 3] = rng.normal(size=(NP, DP - 3)) * 1.5 + 0.5
    q = rng.dirichlet(np.ones(K) * 0.3, NP).T.copy()
    rec, folded, plan = run_stat(X, q, K, chunk_rows, 1)
    ref = dr.stat_records_ref(X, q, chunk_rows, rec.shape[0], plan["rsplit"], plan["nstage"], 1, dtype=hr.LD)
    sc, rows = dr.stat_records_ref(X, q, chunk_rows, rec.shape[0], plan["rsplit"], plan["nstage"], 1, scale=True)
    bar = (chunk_rows + 2) * EPS * sc + hr.TINY
    r = [note(f"stat {DP} records", ratio_of(np.abs(rec.astype(hr.LD) - ref).astype(np.float64), bar))]
    fbar = bar.sum(axis=(0, 1)) + rec.shape[0] * rec.shape[1] * EPS * sc.sum(axis=(0, 1))
    r.append(note(f"stat {DP} folded", ratio_of(np.abs(folded.astype(hr.LD) - ref.sum(axis=(0, 1))).astype(np.float64), fbar)))
    assert max(r) <= 1.0, r


def test_suffstat_hook_refuses_wrong_calls():
    rng = np.random.default_rng(2)
    DP, K, NP = 16, 3, 48
    X = hr.exact_X(rng, NP, DP, DP)
    q = hr.exact_q(rng, K, NP)
    SS = 1 + 2 * DP

    def call(nchunks=2, chunk_rows=32, npart=2 * 4 * K * SS, rginfo=None, smask=None, Xa=X):
        part = np.full(npart, SENT)
        rc, _ = ah.suffstat_diag(Xa, q, K, nchunks, chunk_rows, 1, part, rginfo=rginfo, smask=smask, NP=NP)
        assert untouched(part)
        return rc

    assert call(chunk_rows=48) == -1                       # not whole batches
    assert call(nchunks=1) == -1 and call(nchunks=3) == -1  # the chunks do not tile NP
    assert call(npart=2 * 4 * K * SS - 1) == -1            # a record too few
    assert call(smask=np.ones((1, K), dtype=np.uint8)) == -1  # a mask without the row groups
    assert call(rginfo=np.array([16, 16, 16], dtype=np.int32)) == -1
    assert call(rginfo=np.array([16, 16, (1 << 5) | 16], dtype=np.int32), smask=np.ones((1, K), dtype=np.uint8)) == -1
    assert call(Xa=np.zeros((NP, 24))) == -1
