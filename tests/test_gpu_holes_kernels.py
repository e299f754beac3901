"""The six launchers of lc_kernels_holes.hip through three hooks of the hooks library, bound here
as tests/test_gpu_loo_kernels.py binds its own: lcx_test_holes_scan (launch_holes_scan, launch_holes_fill),
lcx_test_predict_holes (launch_predict_holes / _var / _keep) and lcx_test_holes_draws (launch_predict_holes_keep,
launch_holes_draws).  Synthetic tables, no model fit (tests/holes_kernel_cases.py; tests/test_holes_kernels_refs_host.py holds
these inputs to their conditions without a device): what lc_model_predict_incomplete* never hands the kernels -- any fill value,
any ldq, canaries in pad rows, tables with the dominant component in a later chunk of 64 clusters -- is handed to them here.
The reference is the direct route (incomplete_ref.direct, incomplete_var_ref.direct_var, incomplete_draws_ref.HoleMixture),
never an emulation of the device's; the raw E-step column is numpy's -d_full^2 / 2 of the filled row.  Bars: the project's own
of DESIGN 4.15 / 4.15.1 (logp 1e-10 relative, filled values 1e-9 S_n, var 1e-9 V_n, t_k 1e-10 max(1, |t|))."""
import ctypes as C
import functools

import numpy as np
import pytest
from scipy import stats

import aux_hooks as ah
import holes_kernel_cases as hc
import incomplete_draws_ref as dr
import sample_ref as sr

pytestmark = pytest.mark.gpu

RG, HMAX, GUARD = hc.RG, hc.HMAX, 64
CANARY, ICANARY = -7.25e77, -77  # (no result has these values; pad rows, column tails and the guards keep them)
NONE64 = (1 << 64) - 1

_P, _I, _L = ah._P, ah._I, ah._L
SCAN_ARGS = [_P, _I, _I, _L, _P, _L, _I, _P, _L, _P, _P, _P]
PREDICT_ARGS = [_I, _P, _I, _I, _I, _P, _L, _L, _P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P, _P]
DRAWS_ARGS = [_P, _I, _I, _I, _P, _L, _L, _P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, C.c_ulonglong, _L, _P, _P, _P]


def _hook(name, args):
    fn = getattr(ah.hooks(), name)
    fn.argtypes, fn.restype = args, C.c_int
    return fn


def _guarded(a, canary):
    g = np.full(GUARD, canary, dtype=a.dtype)
    return np.concatenate([g, a.ravel(), g])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _inner(buf, canary, what):
    assert np.all(buf[:GUARD] == canary) and np.all(buf[-GUARD:] == canary), f"{what}: a guard was written"
    return buf[GUARD:-GUARD]


# ---- scan and fill ------------------------------------------------------------------------------------------------------------------
NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000BEEF01]


def _scan_input(D, N, holes=True):
    """block 0: N rows, block 1: 5 rows (a partly filled last row group), then a row group of count 0.  Row r takes pattern
    (r + 1) % 9, so neighbouring rows -- the rows of one wave step -- differ"""
    rng = np.random.default_rng(1000 * D + N)
    lay, DP, lp = hc.Layout([N, 5], empty=1), hc.dp(D), hc.lpr(D)
    n = N + 5
    X = rng.normal(size=(n, D))
    flat = X.reshape(-1)
    flat[::7], flat[3::11], flat[5::13], flat[1::17] = np.inf, -np.inf, -0.0, 5e-324  # none of these is a hole
    Xb = X.view(np.uint64)
    k = 0
    for r in range(n if holes else 0):
        p = (r + 1) % 9
        cols = [[], [0], [D - 1], [63, 64], [3 % D, 3 % D + lp], rng.choice(D, min(8, D), replace=False),
                rng.choice(D, min(9, D), replace=False), np.delete(np.arange(D), rng.integers(0, D)), np.arange(D)][p]
        for c in cols:
            if c < D:
                Xb[r, c] = NANS[k % len(NANS)]
                k += 1
    full = np.full((lay.NP, DP), np.nan)  # pad rows and pad columns: full of NaN, and never read
    full[lay.valid, :D] = X
    return lay, full, X


def _scan(lay, X, D, fill=None):
    DP = X.shape[1]
    Xg, cnt, cols = _guarded(X, CANARY), _guarded(np.full(lay.NP, ICANARY, np.int32), ICANARY), _guarded(
        np.full((lay.NP, HMAX), ICANARY, np.int32), ICANARY)
    out = np.array([5, 5, 5], dtype=np.uint64)
    rc = _hook("lcx_test_holes_scan", SCAN_ARGS)(ah._p(Xg), DP, D, lay.nrg, ah._p(lay.rginfo), lay.nrows, lay.J, ah._p(fill), GUARD,
                                                 ah._p(cnt), ah._p(cols), ah._p(out))
    assert rc == 0, rc
    return (_inner(Xg, CANARY, "X").reshape(lay.NP, DP), _inner(cnt, ICANARY, "count"), _inner(cols, ICANARY, "cols").reshape(lay.NP, HMAX),
            [int(v) for v in out])


@pytest.mark.parametrize("D", [1, 5, 16, 17, 32, 33, 64, 65, 130, 200])
def test_scan_and_fill(D):
    """exact: the records of every row, the three integers, and what the fill touches"""
    per = {16: 1024, 32: 512, 64: 256}[hc.lpr(D)]  # rows one block scans
    fill = np.random.default_rng(D).normal(size=D)
    for N in (1, 17, per + 5):
        lay, X, Xv = _scan_input(D, N)
        want_count, want_cols = hc.host_scan(Xv)
        Xs, cnt, cols, out = _scan(lay, X, D)
        assert _same(Xs, X)  # the scan writes nothing into X
        assert np.array_equal(cnt[lay.valid], want_count) and np.array_equal(cols[lay.valid], want_cols), (D, N)
        assert np.all(cnt[~lay.valid] == ICANARY) and np.all(cols[~lay.valid] == ICANARY)  # pad rows
        bad = np.flatnonzero(lay.valid)[(want_count > HMAX) | (want_count >= D)]
        assert out == [int(np.sum(want_count > 0)), int(want_count.max()), int(bad.min()) if bad.size else NONE64], (D, N, out)
        if N > per:  # offending rows in two blocks of the grid: the smallest position wins
            assert np.any(bad < per) and np.any(bad >= per)
        if hc.lpr(D) == 16 and N >= 17:
            assert want_count[3] > 0 and want_count[7] > 0  # the fourth row of a step: ballot bits 48 - 63
        again = _scan(lay, X, D)
        assert _same(again[1], cnt) and _same(again[2], cols) and again[3] == out
        # the fill: only the recorded positions change, to fill[c]
        Xf, cnt2, cols2, out2 = _scan(lay, X, D, fill)
        assert _same(cnt2, cnt) and _same(cols2, cols) and out2 == out
        want = X.copy()
        for r, row in zip(np.flatnonzero(lay.valid), range(N + 5)):
            c = want_cols[row][want_cols[row] >= 0]
            want[r, c] = fill[c]
        assert _same(Xf, want), (D, N)  # (the ninth NaN of a row, pad rows and pad columns as they were)
        if D >= 10:
            assert np.any(np.isnan(Xf[lay.valid, :D]))  # a row with nine holes keeps its ninth
        # no NaN at all: nothing found, nothing filled
        lay0, X0, _ = _scan_input(D, N, holes=False)
        Xz, cz, colz, outz = _scan(lay0, X0, D, fill)
        assert _same(Xz, X0) and outz == [0, 0, NONE64]
        assert np.all(cz[lay0.valid] == 0) and np.all(colz[lay0.valid] == -1)


# ---- predict_holes: the three instances -------------------------------------------------------------------------------------------
class Inputs:
    """the device arrays of blocks [(Xh, weights)] on the tables of `tab`"""

    def __init__(self, tab, blocks, fill=None, ldq_extra=16, empty=0):
        self.tab, self.blocks = tab, blocks
        lay = self.lay = hc.Layout([b[0].shape[0] for b in blocks], empty)
        D, DP, Kp = tab.D, tab.DP, tab.Kp
        Xh = np.concatenate([b[0] for b in blocks])
        self.count_v, self.cols_v = hc.host_scan(Xh)
        self.fill = tab.fill(blocks[0][1]) if fill is None else fill
        Xf = np.where(np.isnan(Xh), self.fill[None, :], Xh)
        self.X = np.full((lay.NP, DP), CANARY)
        self.X[lay.valid, :D], self.X[lay.valid, D:] = Xf, 0.0  # (a context pads valid rows with zeros)
        self.ldq = lay.NP + ldq_extra
        self.col = np.full((Kp, self.ldq), CANARY)
        self.col[:, np.flatnonzero(lay.valid)] = tab.raw_column(Xf)
        self.count, self.cols = np.full(lay.NP, ICANARY, np.int32), np.full((lay.NP, HMAX), ICANARY, np.int32)
        self.count[lay.valid], self.cols[lay.valid] = self.count_v, self.cols_v
        self.ttab = tab.ttab([b[1] for b in blocks])
        self.holed = self.count_v > 0


class Out:
    pass


def _run(inp, mode, nd=0, seed=0, goff=None, count=None, cols=None, ldq=None, expect=0, drop=None):
    """mode 0 / 1 / 2: lcx_test_predict_holes; mode 3: lcx_test_holes_draws with nd draws.  Checks the guards, the pad rows and
    the column tails; -> the outputs of the valid rows"""
    tab, lay = inp.tab, inp.lay
    D, DP, Kp, NP = tab.D, tab.DP, tab.Kp, lay.NP
    Xg, colg, logpg = _guarded(inp.X, CANARY), _guarded(inp.col, CANARY), _guarded(np.full(NP, CANARY), CANARY)
    varg = _guarded(np.full((NP, HMAX), CANARY), CANARY) if mode == 1 else None
    count = inp.count if count is None else count
    cols = inp.cols if cols is None else cols
    a = {"X": ah._p(Xg), "col": ah._p(colg), "count": ah._p(count), "cols": ah._p(cols), "ttab": ah._p(inp.ttab), "pscale": ah._p(tab.s),
         "pexp": ah._p(tab.e), "mean": ah._p(tab.mean), "P": ah._p(tab.P), "logp": ah._p(logpg), "gnu": ah._p(tab.gnu) if mode == 1 else None,
         "var": ah._p(varg), "cqnu": ah._p(tab.cqnu)}
    nd1 = max(nd, 1)
    drawsg = _guarded(np.zeros((NP, nd1, HMAX)), 0.0) if mode == 3 else None
    labelg = _guarded(np.full((NP, nd1), -1, np.int32), -1) if mode == 3 else None
    a["draws"], a["label"] = ah._p(drawsg), ah._p(labelg)
    if drop:
        a[drop] = None
    rows = (ldq if ldq is not None else inp.ldq, lay.nrg, ah._p(lay.rginfo), lay.nrows, lay.J)
    tabs = (a["count"], a["cols"], a["ttab"], a["pscale"], a["pexp"], a["mean"], a["P"])
    if mode == 3:
        rc = _hook("lcx_test_holes_draws", DRAWS_ARGS)(a["X"], DP, D, Kp, a["col"], *rows, *tabs, ah._p(goff), a["cqnu"], nd, seed, GUARD,
                                                       a["logp"], a["draws"], a["label"])
    else:
        rc = _hook("lcx_test_predict_holes", PREDICT_ARGS)(mode, a["X"], DP, D, Kp, a["col"], *rows, *tabs, a["gnu"], GUARD, a["logp"], a["var"])
    assert rc == expect, rc
    o = Out()
    v = lay.valid
    Xo, colo = _inner(Xg, CANARY, "X").reshape(NP, DP), _inner(colg, CANARY, "col").reshape(Kp, inp.ldq)
    logpo = _inner(logpg, CANARY, "logp")
    if rc != 0:  # refused: nothing was launched, every buffer is as it went in
        assert _same(Xo, inp.X) and _same(colo, inp.col) and np.all(logpo == CANARY)
        assert varg is None or np.all(varg == CANARY)
        assert drawsg is None or (np.all(_bits(drawsg) == 0) and np.all(labelg == -1))
        return o
    assert np.all(Xo[~v] == CANARY) and np.all(Xo[v][:, D:] == 0.0) and np.all(logpo[~v] == CANARY)  # pad rows, pad columns
    known = np.ones((int(v.sum()), D), bool)
    for r in np.flatnonzero(inp.holed):
        known[r, inp.cols_v[r, : inp.count_v[r]]] = False
    assert np.array_equal(_bits(Xo[v][:, :D])[known], _bits(inp.X[v][:, :D])[known])  # only the holes are written
    assert np.all(colo[:, NP:] == CANARY) and np.all(colo[:, :NP][:, ~v] == CANARY)  # column tails, pad rows
    assert _same(colo[:, np.flatnonzero(v)[~inp.holed]], inp.col[:, np.flatnonzero(v)[~inp.holed]])  # complete rows: raw columns
    o.rows, o.logp, o.t = Xo[v][:, :D].copy(), logpo[v].copy(), colo[:, np.flatnonzero(v)].T.copy()
    if mode < 2:
        assert _same(colo, inp.col)  # read only
    if mode == 1:
        var = _inner(varg, CANARY, "var").reshape(NP, HMAX)
        assert np.all(var[~v] == CANARY)
        o.var = var[v].copy()
        dead = np.arange(HMAX)[None, :] >= inp.count_v[:, None]
        assert np.all(_bits(o.var)[dead] == 0) and np.all(o.var[~dead] > 0)  # exactly +0.0 beyond the count; positive in live slots
    if mode == 3:
        draws, label = _inner(drawsg, 0.0, "draws").reshape(NP, nd1, HMAX), _inner(labelg, -1, "label").reshape(NP, nd1)
        assert np.all(_bits(draws[~v]) == 0) and np.all(label[~v] == -1)
        o.draws, o.label = draws[v].copy(), label[v].copy()
        dead = np.broadcast_to((np.arange(HMAX)[None, :] >= inp.count_v[:, None])[:, None, :], o.draws.shape)
        assert np.all(_bits(o.draws)[dead] == 0) and np.all(o.label[~inp.holed] == -1)
        lab = o.label[inp.holed]
        assert lab.size == 0 or (lab.min() >= 0 and lab.max() < Kp)
        assert np.all(np.isfinite(o.draws))
    return o


def _inputs(name, **kw):
    c = hc.case(name)
    return Inputs(c.tab, c.blocks, **kw)


def _three_modes(inp):
    """the three instances: the same bits in X and logp; -> (mean, variance, keep) outputs"""
    o = [_run(inp, m) for m in (0, 1, 2)]
    for x in o[1:]:
        assert _same(x.rows, o[0].rows) and _same(x.logp, o[0].logp)
    assert _same(o[0].t, o[1].t)
    return o


def _against_direct(c, o, what, table=None):
    got = hc.ratios(c.ref, o[0].rows, o[0].logp, o[1].var, o[2].t)
    print(f"{what}: largest |device - direct| over the bar's scale: " + ", ".join(f"{k} {v:.2e} (bar {hc.BARS[k]:.0e})" for k, v in got.items()))
    assert np.all(np.isfinite(o[0].rows)) and np.all(np.isfinite(o[0].logp)) and np.all(np.isfinite(o[1].var))
    for k, v in got.items():
        assert v <= hc.BARS[k], (what, k, v)
    return got


@pytest.mark.parametrize("name", hc.SHAPES + ["edges", "gnu0"])
def test_predict_holes_against_the_direct_reference(name):
    c = hc.case(name)
    inp = _inputs(name)
    o = _three_modes(inp)
    _against_direct(c, o, name)
    again = _three_modes(inp)  # the same bits on every run
    for x, y in zip(o, again):
        assert _same(x.rows, y.rows) and _same(x.logp, y.logp) and _same(x.t, y.t)
    assert _same(o[1].var, again[1].var)
    if name == "d2_k1_n1":  # Kp = 1: the filled value is the one expert
        assert abs(o[0].rows[0, 0] - c.ref.rows[0, 0]) <= 1e-9 * c.ref.S[0] and c.ref.r[0, 0] == 1.0
    if name == "d23_k130_n20":  # the dominant component in chunk 0, 1, 2 in turn, and two comparable ones in different chunks
        row, k, k2 = c.notes["between"]
        for r in [p[0] for p in c.notes["placed"]] + [row]:
            s = slice(r, r + 1)
            one = {"logp": abs(o[0].logp[r] - c.ref.logp[r]) / abs(c.ref.logp[r]), "fill": np.abs(o[0].rows[s] - c.ref.rows[s]).max() / c.ref.S[r],
                   "var": np.abs(o[1].var[s] - c.ref.var[s]).max() / c.ref.Vn[r]}
            print(f"  row {r} (largest r in chunk {int(np.argmax(c.ref.r[r])) // 64}): " + ", ".join(f"{k_} {v:.2e}" for k_, v in one.items()))
    if name == "gnu0":
        assert np.any(inp.tab.gnu[inp.count_v[inp.holed]] == 0.0)  # a live slot whose component has no variance


@pytest.mark.parametrize("name", ["d3_k2_n17", "d23_k5_n70"])
def test_the_fill_value_cancels(name):
    """the weighted mean of the means, and that + 3 spreads per column: both within the bars (bits may differ)"""
    c = hc.case(name)
    w = c.blocks[0][1]
    moved = Inputs(c.tab, c.blocks, fill=c.tab.fill(w) + 3.0 * (w @ c.tab.sd))
    o = _three_modes(moved)
    _against_direct(c, o, f"{name}, fill + 3 spreads")
    assert not np.array_equal(moved.col, _inputs(name).col)  # (the raw column does see the fill value)


def test_three_blocks_with_their_own_weight_tables():
    c = hc.case("blocks3")
    inp = _inputs("blocks3")
    assert inp.lay.goff[1] == 16 and inp.lay.J == 3  # the second block starts inside the first wave
    o = _three_modes(inp)
    _against_direct(c, o, "three blocks")
    at = 0
    for j, (Xh, w) in enumerate(c.blocks):  # each block equals the same block alone, bit for bit
        alone = _three_modes(Inputs(c.tab, [(Xh, w)], fill=inp.fill))
        s = slice(at, at + Xh.shape[0])
        for x, y in zip(alone, o):
            assert _same(x.rows, y.rows[s]) and _same(x.logp, y.logp[s]) and _same(x.t[inp.holed[s]], y.t[s][inp.holed[s]]), j
        assert _same(alone[1].var, o[1].var[s])
        at += Xh.shape[0]
    swapped = Inputs(c.tab, [(c.blocks[0][0], c.blocks[1][1]), (c.blocks[1][0], c.blocks[0][1]), c.blocks[2]], fill=inp.fill)
    s = _run(swapped, 0)
    assert not np.array_equal(s.logp[:35], o[0].logp[:35]) and _same(s.logp[35:], o[0].logp[35:])  # (the tables do differ)


@pytest.mark.parametrize("D", [5, 64, 72])
def test_a_row_gives_the_same_bits_wherever_it_sits(D):
    """another lane (21), another wave (70) and another block (260): every output, the draws included (goff moves the row's
    counter along with it)"""
    tab = hc.Tables(D, 3, 4170 + D)
    rng = np.random.default_rng(4171 + D)
    w = tab.weights(rng)
    first = hc.punch(rng, tab.rows(rng, 3), np.zeros(3, bool))
    other = hc.punch(rng, tab.rows(rng, 300), hc.third_complete(300))
    fill = tab.fill(w)
    base = Inputs(tab, [(first, w)], fill=fill)
    a = _three_modes(base) + [_run(base, 3, nd=7, seed=hc.DRAW_SEED)]
    for pos in (21, 70, 260):
        moved = other.copy()
        moved[pos] = first[0]
        inp = Inputs(tab, [(moved, w)], fill=fill)
        b = _three_modes(inp) + [_run(inp, 3, nd=7, seed=hc.DRAW_SEED, goff=np.array([pos, 0], dtype=np.int64))]
        for x, y in zip(a, b):
            assert _same(x.rows[0], y.rows[pos]) and _same(x.logp[:1], y.logp[pos:pos + 1]), pos
        assert _same(a[1].var[0], b[1].var[pos]) and _same(a[2].t[0], b[2].t[pos]) and _same(a[3].t[0], b[3].t[pos]), pos
        assert _same(a[3].draws[0], b[3].draws[pos]) and _same(a[3].label[0], b[3].label[pos]), pos


# ---- holes_draws ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _draws(name):
    """one launch per case, shared by the tests and never changed"""
    build, nd = hc.DRAW_CASES[name]
    inp = _inputs(build)
    o = _run(inp, 3, nd=nd, seed=hc.DRAW_SEED, goff=inp.lay.goff if inp.lay.J > 1 else None)
    return inp, o


def _recovered_g_bar(comp, Xa, x, z, D, t, S):
    """The bar of |G_recovered / gamma_draw - 1| per draw, G_recovered = 1 / mean_i(ratio_i)^2 over the holes i with
    |z_i| >= 1e-3, ratio_i = v_i / (sqrt(cqnu h) z_i), v_i = sum_c (x_c - M_c) L_ci.  First order, every term relative to ratio_i:
      * the device's x_c carries the value bar of the samplers, (n + 2) 2^-53 + 8 E_REF (n = D + 2 nb: a row of P times y, two
        triangular solves), of |x_c| + |M_c|, and the subtraction x_c - M_c cancels: (|x| + |M|) |L| over |v_i|;
      * the reference's location M_c is the direct route's, which this file holds to BAR_FILL S_n: BAR_FILL S_n |L| over |v_i|;
      * the scale's h_k = exp((... - t_k) / e) inherits the error of t_k, which this file holds to BAR_T max(1, |t_k|): half of
        that over e for the square root;
      * a normal is wrong by at most rad (2 pi + 2) 2^-53, rad <= 8.65 (the angle's rounding times 2 pi, a sincos of an ulp),
        on the device and in the reference, each allowed twice that: 4 * 8.65 (2 pi + 2) 2^-53 over |z_i|.
    G takes twice the largest of these over its holes, plus 8 E_REF for the two gamma values themselves."""
    import sample_kernel_cases as sc

    nb = x.shape[1]
    M = comp.location(Xa)
    v = np.abs((x - M) @ comp.L)
    aL = np.abs(comp.L)
    e = comp.eta / 2
    per = (sr.value_bar(D + 2 * nb, sc.E_REF["gamma"]) * ((np.abs(x) + np.abs(M)) @ aL) + hc.BAR_FILL * S[:, None] * aL.sum(axis=0)) / v
    per = per + (0.5 * hc.BAR_T * np.maximum(1.0, np.abs(t)) / e)[:, None] + 4 * 8.65 * (2 * np.pi + 2) * 2.0 ** -53 / np.abs(z)
    per[np.abs(z) < 1e-3] = np.nan
    return 2 * np.nanmax(per, axis=1) + 8 * sc.E_REF["gamma"]


@pytest.mark.parametrize("name", sorted(hc.DRAW_CASES))
def test_draws(name):
    build, nd = hc.DRAW_CASES[name]
    c = hc.case(build)
    inp, o = _draws(name)
    keep = _run(inp, 2)
    assert _same(o.rows, keep.rows) and _same(o.logp, keep.logp) and _same(o.t, keep.t)  # the draws pass reads, never writes these
    # labels: the documented uniforms against the reference's responsibilities
    want, far = hc.label_reference(c, hc.DRAW_SEED, nd)
    assert np.array_equal(o.label[far], want[far]), name
    left, total = int((~far[inp.holed]).sum()), int(inp.holed.sum()) * nd
    print(f"{name}: {left} of {total} labels left out (within 1e-9 of a boundary; share {left / total:.2e})")
    assert left <= 1e-3 * total
    if build == "d5_k70_n40":
        assert o.label.max() >= 64  # the second chunk of clusters is drawn from
    # the structure of a draw: L^T (x_b - M_k) / sqrt(cqnu_k h_k) over z is one positive scalar 1 / sqrt(G) over its holes
    worst, G, at = 0.0, {}, 0
    gworst, gleft, gtotal = 0.0, 0, 0
    for j, (Xh, _) in enumerate(c.blocks):
        s = slice(at, at + Xh.shape[0])
        for comp, pat, rows, di, Xa in c.ref.mixes[j].each(Xh, o.label[s]):
            nb = len(pat)
            z = dr.normals(hc.DRAW_SEED, j, rows, di, (nb + 1) // 2)[:, :nb]
            x = o.draws[s][rows, di, :nb]
            ratio = comp.inv_sqrt_g(Xa, x, z)
            ratio[np.abs(z) < 1e-3] = np.nan
            ok = np.sum(~np.isnan(ratio), axis=1) >= 1
            lo, hi = np.nanmin(ratio[ok], axis=1), np.nanmax(ratio[ok], axis=1)
            assert np.all(lo > 0), (name, pat)
            worst = max(worst, float(np.max(hi / lo - 1, initial=0.0)))
            g = 1 / np.nanmean(ratio[ok], axis=1) ** 2
            G.setdefault((comp.eta, nb), []).append(g)
            # the recovered G against the restated gamma draw on the draw's own stream (c2 = draw, shape e_k(nb))
            want, _, margin = sr.gamma_draw(hc.DRAW_SEED, j, rows[ok], di[ok], comp.eta / 2)
            k = o.label[s][rows[ok], di[ok]]
            bar = _recovered_g_bar(comp, Xa[ok], x[ok], z[ok], c.Xh.shape[1], o.t[s][rows[ok], k], c.ref.S[at + rows[ok]])
            far = margin > sr.NEAR
            gleft, gtotal = gleft + int((~far).sum()), gtotal + far.size
            gworst = max(gworst, float(np.max((np.abs(g / want - 1) / bar)[far], initial=0.0)))
        at += Xh.shape[0]
    print(f"{name}: largest error of the recovered G against gamma_draw over its bar {gworst:.3e}; {gleft} of {gtotal} draws left out")
    assert gleft <= (1 if gtotal < 1000 else sr.EXCLUDED_SHARE * gtotal)
    assert gworst <= 1.0, name
    print(f"{name}: largest relative spread of 1 / sqrt(G) over the holes of a draw: {worst:.3e} (bar 1e-9)")
    assert worst <= 1e-9
    if build == "d5_k1_n120":  # Kp = 1: the recovered G, pooled per hole count, is Gamma(e(nb))
        tally = sr.Tally()
        assert sorted(nb for _, nb in G) == [1, 2, 3, 4]
        for (eta, nb), g in sorted(G.items()):
            g = np.concatenate(g)
            assert g.size >= 100 and eta / 2 == c.tab.e[nb, 0]
            tally.add([stats.kstest(g, stats.gamma(eta / 2).cdf)], f"recovered G, eta {eta:g}, {nb} holes, {g.size} draws")
    again = _run(inp, 3, nd=nd, seed=hc.DRAW_SEED, goff=inp.lay.goff if inp.lay.J > 1 else None)
    assert _same(again.draws, o.draws) and _same(again.label, o.label)


def test_draw_i_does_not_depend_on_the_number_of_draws():
    a, b, one = _draws("d23_k5_n70_m7")[1], _draws("d23_k5_n70_m64")[1], _draws("d23_k5_n70_m1")[1]
    assert _same(a.draws, b.draws[:, :7]) and _same(a.label, b.label[:, :7])
    assert _same(one.draws, b.draws[:, :1]) and _same(one.label, b.label[:, :1])


def test_blocks_have_their_own_counters():
    inp, o = _draws("blocks2_m7")
    c = hc.case("blocks2")
    alone = Inputs(c.tab, [c.blocks[1]], fill=inp.fill)  # block 1 run alone is block 0 of its launch: other uniforms
    x = _run(alone, 3, nd=7, seed=hc.DRAW_SEED)
    assert _same(x.rows, o.rows[21:]) and not np.array_equal(x.draws[alone.holed], o.draws[21:][alone.holed])


@pytest.mark.parametrize("nd", [0, 65])
def test_the_launcher_refuses_a_draw_count_outside_1_to_64(nd):
    inp = _inputs("d3_k2_n17")
    _run(inp, 3, nd=nd, seed=1, expect=ah.HIP_ERROR_INVALID_VALUE)


# ---- refusals: -1, and nothing is launched ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_hooks_refuse_what_a_kernel_could_not_address(mode):
    inp = _inputs("d3_k2_n17")
    kw = {"nd": 3, "seed": 1} if mode == 3 else {}
    row = np.flatnonzero(inp.lay.valid)[np.flatnonzero(inp.holed)[0]]
    for drop in ("X", "col", "count", "cols", "ttab", "pscale", "pexp", "mean", "P", "logp") + (("cqnu", "draws", "label") if mode == 3 else ()):
        _run(inp, mode, expect=-1, drop=drop, **kw)
    if mode == 1:
        _run(inp, 1, expect=-1, drop="gnu")
        _run(inp, 1, expect=-1, drop="var")
    for bad in (9, 3):  # more than HOLES_MAX; no known column (D = 3)
        count = inp.count.copy()
        count[row] = bad
        cols = inp.cols.copy()
        cols[row, :3] = [0, 1, 2]
        _run(inp, mode, expect=-1, count=count, cols=cols, **kw)
    for bad in (3, -1):  # a column outside [0, D)
        cols = inp.cols.copy()
        cols[row, 0] = bad
        _run(inp, mode, expect=-1, cols=cols, **kw)
    cols = inp.cols.copy()
    two = np.flatnonzero(inp.lay.valid)[np.flatnonzero(inp.count_v == 2)[0]]
    cols[two, :2] = cols[two, 1::-1]  # descending
    _run(inp, mode, expect=-1, cols=cols, **kw)
    _run(inp, mode, expect=-1, ldq=inp.lay.NP - 1, **kw)


def test_scan_hook_refusals():
    lay, X, _ = _scan_input(5, 17)
    fn = _hook("lcx_test_holes_scan", SCAN_ARGS)
    Xg, cnt, cols = _guarded(X, CANARY), _guarded(np.full(lay.NP, ICANARY, np.int32), ICANARY), _guarded(np.full((lay.NP, HMAX), ICANARY, np.int32), ICANARY)
    out = np.array([5, 5, 5], dtype=np.uint64)
    args = [ah._p(Xg), 16, 5, lay.nrg, ah._p(lay.rginfo), lay.nrows, lay.J, None, GUARD, ah._p(cnt), ah._p(cols), ah._p(out)]
    for i in (0, 9, 10, 11):  # a missing array
        assert fn(*[None if k == i else v for k, v in enumerate(args)]) == -1
    assert fn(*[{1: 8, 2: 9}.get(k, v) for k, v in enumerate(args)]) == -1  # DP < D, DP no multiple of 16
    assert fn(*[{3: 0}.get(k, v) for k, v in enumerate(args)]) == -1  # no row group
    assert fn(*[{6: 1}.get(k, v) for k, v in enumerate(args)]) == -1  # rginfo names a block beyond J
    assert np.all(cnt == ICANARY) and np.all(cols == ICANARY) and out.tolist() == [5, 5, 5]
