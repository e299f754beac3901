"""launch_sample and launch_predict_cond_draws (lc_kernels_sample.hip) through the lcx_test_sample and
lcx_test_cond_draws hooks of the hooks library (bound here): synthetic tables, no model fit (tests/sample_kernel_cases.py).
Every drawn VALUE is compared with the float64 restatement of the documented streams (tests/sample_ref.py): labels exactly, values
within (n + 2) 2^-53 + 8 E_REF of the magnitude of the entry's summed terms, n the length of its sum and E_REF the reference's own
error against 40-digit arithmetic on these inputs (tests/test_sample_exact_refs_host.py).  Rows with a decision within 1e-9 of its
boundary are left out, at most 1e-3 of a case's rows (at most one row of a case under 1000 rows)."""
import ctypes as C

import numpy as np
import pytest

import aux_hooks as ah
import sample_kernel_cases as sc
import sample_ref as sr

pytestmark = pytest.mark.gpu

RG, GUARD = 16, 64
CANARY = -7.25e77  # (no result has this value)
LCANARY = -77
_P, _I, _L, _U = ah._P, ah._I, ah._L, C.c_ulonglong
SAMPLE_ARGS = [_I, _I, _I, _I, _L, _L, _L, _U, _P, _P, _I, _P, _P, _P, _P, _P, _L, _P, _P]
COND_ARGS = [_P, _I, _I, _I, _I, _I, _I, _P, _L, _L, _P, _L, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _U, _L, _P, _P]


def _hook(name, args):
    fn = getattr(ah.hooks(), name)
    fn.argtypes, fn.restype = args, C.c_int
    return fn


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


# ---- launch_sample ------------------------------------------------------------------------------------------------------------
def run_sample(c, expect=0, **kw):
    """one launch of case c (keywords replace its arguments) -> X [NP x DP], label [NP]; the guards are checked here"""
    a = dict(mode=c.mode, D=c.D, DP=c.DP, Kp=c.Kp, NP=c.NP, nrows=c.nrows, row_offset=c.row_offset, seed=sc.SEED, rginfo=c.rginfo,
             goff=c.goff, J=c.J, cdf=c.cdf, klast=c.klast, loc=None if c.mode == 2 else c.loc, fac=c.fac, shape=c.shape)
    a.update(kw)
    NP, DP = a["NP"], max(a["DP"], 1)
    X = np.full(NP * DP + 2 * GUARD, CANARY)
    label = np.full(NP + 2 * GUARD, LCANARY, dtype=np.int32)
    keep = [np.ascontiguousarray(a[k], dtype=np.float64) if a[k] is not None else None for k in ("cdf", "loc", "fac", "shape")]
    rgi, goff, klast = _i32(a["rginfo"]), None if a["goff"] is None else np.ascontiguousarray(a["goff"], dtype=np.int64), _i32(a["klast"])
    rc = _hook("lcx_test_sample", SAMPLE_ARGS)(a["mode"], a["D"], a["DP"], a["Kp"], NP, a["nrows"], a["row_offset"], a["seed"], ah._p(rgi),
                                               ah._p(goff), a["J"], ah._p(keep[0]), ah._p(klast), ah._p(keep[1]), ah._p(keep[2]),
                                               ah._p(keep[3]), GUARD, ah._p(X), ah._p(label))
    assert rc == expect, rc
    assert np.all(X[:GUARD] == CANARY) and np.all(X[-GUARD:] == CANARY), "a write outside X"
    assert np.all(label[:GUARD] == LCANARY) and np.all(label[-GUARD:] == LCANARY), "a write outside label"
    if expect != 0:
        assert np.all(X == CANARY) and np.all(label == LCANARY)  # a refusal launches nothing
        return None, None
    return X[GUARD:-GUARD].reshape(NP, DP), label[GUARD:-GUARD]


def check_sample(c, X, label, exact, valid):
    """every byte written; pad rows and columns +0.0, pad labels -1; labels exact and values within the bar on the valid rows"""
    assert not np.any(X == CANARY) and not np.any(label == LCANARY), "an entry the launch owes was not written"
    assert np.all(_bits(X[~valid]) == 0) and np.all(_bits(X[:, c.D:]) == 0), "pad rows and pad columns are +0.0"
    assert np.all(label[~valid] == -1)
    worst, left, total = 0.0, 0, 0
    for at, e in exact:
        n = e.label.size
        lab, x = label[at:at + n], X[at:at + n, : c.D]
        assert np.array_equal(lab[e.label_far], e.label[e.label_far]), c.name
        ok = e.label_far & e.value_far
        left, total = left + int((~ok).sum()), total + n
        ratio = sr.scaled_error(x, e.x, e.mag) / sr.value_bar(e.nsum, sc.E_REF[sc.FAMILY[c.mode]])
        worst = max(worst, float(np.max(ratio[ok], initial=0.0)))
        assert np.all(np.isfinite(x))
    print(f"{c.name}: largest error over its bar {worst:.3f}; {left} of {total} rows left out")
    assert left <= (1 if total < 1000 else sr.EXCLUDED_SHARE * total)
    assert worst <= 1.0, c.name


def _valid(c):
    v = np.zeros(c.NP, dtype=bool)
    for _, at, n in c.block_rows():
        v[at:at + n] = True
    return v


@pytest.mark.parametrize("name", list(sc.SAMPLE_CASES) + [sc.WIDE_CASE.name])
def test_sample_values_are_the_documented_streams(name):
    c = sc.SAMPLE_CASES.get(name, sc.WIDE_CASE)
    X, label = run_sample(c)
    check_sample(c, X, label, c.exact(), _valid(c))
    X2, label2 = run_sample(c)
    assert np.array_equal(_bits(X), _bits(X2)) and np.array_equal(label, label2)  # the same bits on every call
    if c.J == 1:  # a shard generated alone is that part of the whole, bitwise
        a, b = 7, min(30, c.nrows)
        n = b - a
        Xs, ls = run_sample(c, NP=(n + RG - 1) // RG * RG, nrows=n, row_offset=c.row_offset + a)
        assert np.array_equal(_bits(Xs[:n]), _bits(X[a:b])) and np.array_equal(ls[:n], label[a:b])
        assert np.all(_bits(Xs[n:]) == 0) and np.all(ls[n:] == -1)


def test_sample_refusals():
    c = sc.SAMPLE_CASES["gw_d3_dp4"]
    inv = ah.HIP_ERROR_INVALID_VALUE
    run_sample(c, expect=inv, DP=5)   # odd
    run_sample(c, expect=inv, DP=2)   # below D
    run_sample(c, expect=inv, Kp=0)
    run_sample(c, expect=inv, mode=3)
    run_sample(c, expect=inv, mode=-1)
    for table in ("cdf", "klast", "loc", "fac", "shape"):
        run_sample(c, expect=inv, **{table: None})
    e = sc.SAMPLE_CASES["eg_d4"]
    X, label = run_sample(e, loc=None)  # (ExpGamma has no location)
    assert not np.any(X == CANARY)


# ---- launch_predict_cond_draws --------------------------------------------------------------------------------------------------
def run_cond(c, ndraws=None, expect=0, **kw):
    nd = c.ndraws if ndraws is None else ndraws
    a = dict(Dae=c.Dae, Dbp=c.Dbp)
    a.update(kw)
    ndb = max(nd, 1)
    draws = np.full(c.NP * ndb * c.Db + 2 * GUARD, CANARY)
    label = np.full(c.NP * ndb + 2 * GUARD, LCANARY, dtype=np.int32)
    rc = _hook("lcx_test_cond_draws", COND_ARGS)(
        ah._p(c.X), c.DP, c.Da, a["Dae"], c.Db, a["Dbp"], c.Kp, ah._p(c.t), c.ldq, c.nrg, ah._p(c.rginfo), 0, c.J, ah._p(c.ttab),
        ah._p(c.pexp), ah._p(c.mext), ah._p(c.T), ah._p(c.logp), ah._p(c.goff), ah._p(c.Lt), ah._p(c.cq), nd, sc.SEED, GUARD,
        ah._p(draws), ah._p(label))
    assert rc == expect, rc
    assert np.all(draws[:GUARD] == CANARY) and np.all(draws[-GUARD:] == CANARY), "a write outside draws"
    assert np.all(label[:GUARD] == LCANARY) and np.all(label[-GUARD:] == LCANARY), "a write outside label"
    if expect != 0:
        assert np.all(draws == CANARY) and np.all(label == LCANARY)
        return None, None
    draws, label = draws[GUARD:-GUARD].reshape(c.NP, nd, c.Db), label[GUARD:-GUARD].reshape(c.NP, nd)
    assert np.all(draws[~c.valid] == CANARY) and np.all(label[~c.valid] == LCANARY), "pad rows write nothing"
    assert not np.any(draws[c.valid] == CANARY) and not np.any(label[c.valid] == LCANARY)
    return draws, label


@pytest.mark.parametrize("name", list(sc.COND_CASES))
def test_cond_draws_are_the_documented_streams(name):
    c = sc.COND_CASES[name]
    draws, label = run_cond(c)
    worst, left, total = 0.0, 0, 0
    for pos, e in c.exact():
        assert np.array_equal(label[pos][e.label_far], e.label[e.label_far]), name
        ok = e.label_far & e.value_far
        left, total = left + int((~ok).sum()), total + ok.size
        ratio = sr.scaled_error(draws[pos], e.x, e.mag) / sr.value_bar(e.nsum, sc.E_REF["cond"])
        worst = max(worst, float(np.max(ratio[ok], initial=0.0)))
    print(f"{name}: largest error over its bar {worst:.3f}; {left} of {total} draws left out")
    assert left <= (1 if total < 1000 else sr.EXCLUDED_SHARE * total)
    assert worst <= 1.0, name
    if c.planted:
        assert np.all(label[c.planted["under"]] == 2)
        for p in c.planted["hard"]:
            assert np.all(label[p] == p % c.Kp)
    again = run_cond(c)
    assert np.array_equal(_bits(again[0]), _bits(draws)) and np.array_equal(again[1], label)


def test_draw_i_does_not_depend_on_the_number_of_draws():
    c = sc.COND_CASES["k7_m4_8x3"]
    d64, l64 = run_cond(c, 64)
    for nd in (1, 4, 5):
        d, lab = run_cond(c, nd)
        assert np.array_equal(_bits(d[c.valid]), _bits(d64[c.valid][:, :nd])) and np.array_equal(lab[c.valid], l64[c.valid][:, :nd])


def test_cond_draws_refusals():
    c = sc.COND_CASES["k7_m4_8x3"]
    inv = ah.HIP_ERROR_INVALID_VALUE
    run_cond(c, 0, expect=inv)
    run_cond(c, 65, expect=inv)
    run_cond(c, expect=inv, Dae=c.Dae + 1)
    run_cond(c, expect=inv, Dbp=c.Dbp + 2)
