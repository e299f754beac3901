"""launch_top_rows (lc_kernels_rank.hip) and launch_score_select, launch_score_counts, launch_rows_beyond
(lc_kernels_select.hip) through their hooks of the hooks library (bound here): synthetic columns
(tests/rank_select_cases.py), sized to enter the loops the C ABI's tests never enter -- the second trip of the merge kernel, the
second chunk of a histogram block, the carry of the scan -- and launcher arguments the API never varies (ld > NP, label0 != 0,
row groups with no or an odd number of rows anywhere).  The references are numpy (tests/score_select_ref.py and the ranking
reference of tests/rank_select_cases.py).  Every comparison is exact: positions, ranks, counts and totals equal, scores and
values bitwise equal."""
import ctypes as C

import numpy as np
import pytest

import aux_hooks as ah
import rank_select_cases as rc
import score_select_ref as ssr

pytestmark = pytest.mark.gpu

RG, GUARD, CH = 16, 64, rc.TOP_CHUNK_ROWS
CANARY, ICANARY = -7.25e77, -7777777
INV = ah.HIP_ERROR_INVALID_VALUE
_P, _I, _L, _D = ah._P, ah._I, ah._L, ah._D
TOP_ARGS = [_P, _L, _I, _L, _P, _L, _P, _I, _I, _I, _L, _P, _P, _P, _P]
SELECT_ARGS = [_P, _L, _I, _L, _P, _L, _P, _I, _I, _P, _L, _P, _P, _P]
COUNTS_ARGS = [_P, _L, _I, _L, _P, _L, _P, _I, _I, _P, _L, _P]
BEYOND_ARGS = [_P, _L, _I, _L, _P, _L, _P, _I, _D, _I, _L, _I, _L, _P, _P, _P, _P]


def _hook(name, args):
    fn = getattr(ah.hooks(), name)
    fn.argtypes, fn.restype = args, C.c_int
    return fn


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _chunks(NP):
    return (NP + CH - 1) // CH


def _guarded(n, fill, dtype):
    return np.full(n + 2 * GUARD, fill, dtype=dtype)


def _mid(buf, fill, what):
    assert np.all(buf[:GUARD] == fill) and np.all(buf[-GUARD:] == fill), f"a write outside {what}"
    return buf[GUARD:-GUARD] if GUARD else buf


def _columns(col, lay, ld=None, slack=None):
    """col [C x NP] -> [C x ld] with `slack` behind every column"""
    col = np.atleast_2d(col)
    out = np.full((col.shape[0], ld or lay.NP), 0.0 if slack is None else slack)
    out[:, : lay.NP] = col
    return out


# ---- launch_top_rows -------------------------------------------------------------------------------------------------------------
def run_top(col, lay, m, largest, label=None, expect=0, **kw):
    col = np.ascontiguousarray(col, dtype=np.float64)
    a = dict(ld=col.shape[1], C=col.shape[0], NP=lay.NP, m=m, nchunks=_chunks(lay.NP))
    a.update(kw)
    nch, mm, Cn = _chunks(lay.NP), min(max(m, 1), 64), col.shape[0]
    pkey, ppos = _guarded(nch * Cn * mm, CANARY, np.float64), _guarded(nch * Cn * mm, ICANARY, np.int64)
    score, pos = _guarded(Cn * mm, CANARY, np.float64), _guarded(Cn * mm, ICANARY, np.int64)
    lab = None if label is None else np.ascontiguousarray(label, dtype=np.int32)
    rc_ = _hook("lcx_test_top_rows", TOP_ARGS)(ah._p(col), a["ld"], a["C"], a["NP"], ah._p(lay.rginfo), lay.nrows, ah._p(lab), a["m"],
                                               int(largest), a["nchunks"], GUARD, ah._p(pkey), ah._p(ppos), ah._p(score), ah._p(pos))
    assert rc_ == expect, rc_
    if expect != 0:
        assert np.all(pkey == CANARY) and np.all(ppos == ICANARY) and np.all(score == CANARY) and np.all(pos == ICANARY)
        return None
    return (_mid(pos, ICANARY, "out_pos").reshape(Cn, m), _mid(score, CANARY, "out_score").reshape(Cn, m),
            _mid(pkey, CANARY, "pkey").reshape(nch, Cn, m), _mid(ppos, ICANARY, "ppos").reshape(nch, Cn, m))


def check_top(col, lay, m, largest, label=None, lists=True):
    pos, score, pkey, ppos = run_top(col, lay, m, largest, label)
    wpos, wscore = rc.top_ref_padded(col, lay, m, largest, label)
    assert np.array_equal(pos, wpos), (pos, wpos)
    has = wpos >= 0
    assert np.array_equal(_bits(score)[has], _bits(wscore)[has]) and np.all(np.isnan(score[~has]))
    if lists:  # each chunk's own best m, best first; unused slots hold no row
        wkey, wp = rc.chunk_lists_ref(col, lay, m, largest, label)
        assert np.array_equal(ppos, wp)
        used = wp != np.iinfo(np.int64).max
        assert np.array_equal(_bits(pkey[used]), _bits(wkey[used]))
    return pos, score


NP_ADV = 2 * CH + 16


@pytest.mark.parametrize("m", [1, 2, 63, 64])
@pytest.mark.parametrize("largest", [True, False])
def test_top_rows_adversarial_orders(m, largest):
    lay = rc.Layout(NP_ADV, nrows=NP_ADV - 3)
    cols = rc.adversarial_columns(NP_ADV)
    col = np.stack(list(cols.values()))
    pos, score = check_top(col, lay, m, largest)
    names = list(cols)
    assert np.array_equal(pos[names.index("constant")], np.arange(m))  # ties: the position decides
    inf = pos[names.index("neg_inf" if largest else "pos_inf")]  # keys that equal the empty list's threshold
    assert np.array_equal(inf, np.arange(m))


@pytest.mark.parametrize("largest", [True, False])
def test_top_rows_slack_pad_rows_and_ragged_groups(largest):
    rng = np.random.default_rng(11)
    NP = CH + 7 * RG
    win = 1e9 if largest else -1e9
    lay = rc.Layout(NP, fill=rc.ragged_fill(NP, rng))
    col = rng.standard_normal((3, NP))
    col[:, ~lay.valid] = win  # pad rows hold values that would win
    wide = _columns(col, lay, ld=NP + 16, slack=win)  # ... and so does the slack behind every column
    for m in (1, 5, 64):
        check_top(wide, lay, m, largest)
    one = rc.Layout(NP, nrows=NP - 11)
    col[:, one.valid] = rng.standard_normal((3, NP - 11))
    col[:, ~one.valid] = win
    check_top(_columns(col, one, ld=NP + 16, slack=win), one, 64, largest)


def test_top_rows_label_filter():
    rng = np.random.default_rng(12)
    NP = CH + 3 * RG
    lay = rc.Layout(NP, fill=rc.ragged_fill(NP, rng))
    col = rng.standard_normal((3, NP))
    label = rng.choice(np.array([-1, 0, 1, 2, 3, 7], dtype=np.int32), NP)
    for c in range(3):
        padlab = label.copy()
        padlab[~lay.valid] = c  # pad rows labelled c never take part
        col[:, ~lay.valid] = 1e9
        pos, _ = check_top(col, lay, 64, True, padlab)
        assert np.all(lay.valid[pos[c][pos[c] >= 0]])
    rare = np.where(np.arange(NP) % 1000 == 1, 1, 5).astype(np.int32)  # fewer candidates than m: the slots behind them are empty
    pos, score = check_top(col, lay, 64, False, rare)
    assert np.all(pos[0] == -1) and np.all(pos[2] == -1) and np.all(np.isnan(score[0])) and 0 < (pos[1] >= 0).sum() < 64


@pytest.mark.parametrize("nch,m", [(64, 64), (65, 64), (66, 63)])
def test_top_rows_merge_kernel_second_trip(nch, m):
    """the partial lists hold nch * m entries: exactly one trip of the merge loop (4096), and 64 or 62 more"""
    NP = nch * CH
    assert (nch * m > rc.MERGE_TRIP) == (nch > 64)
    lay = rc.Layout(NP, nrows=NP)
    rising = np.arange(NP, dtype=np.float64)[None, :] * 0.125 - 7.0  # the winners are the last entries of the last list
    pos, _ = check_top(rising, lay, m, True, lists=False)
    assert np.array_equal(pos[0], NP - 1 - np.arange(m))
    planted = np.random.default_rng(nch).standard_normal((1, NP))
    chunks = np.unique(np.concatenate([[nch - 1, 0], np.arange(nch)[-64:]]))[-64:]  # the best rows one per chunk, the last included
    at = chunks * CH + (chunks * 37) % CH
    planted[0, at] = 100.0 + np.arange(at.size)
    pos, _ = check_top(planted, lay, m, True, lists=False)
    assert np.array_equal(pos[0], at[::-1][:m])
    pos, _ = check_top(-planted, lay, m, False, lists=False)
    assert np.array_equal(pos[0], at[::-1][:m])


def test_top_rows_empty_and_refusals():
    lay = rc.Layout(0, nrows=0)
    pos, score, _, _ = run_top(np.zeros((2, 0)), lay, 5, True)
    assert np.all(pos == -1) and np.all(np.isnan(score))
    lay = rc.Layout(32, nrows=30)
    col = np.arange(64, dtype=np.float64).reshape(2, 32)
    for kw in (dict(m=0), dict(m=65), dict(NP=24), dict(ld=16), dict(nchunks=2), dict(nchunks=0), dict(C=0), dict(C=65536)):
        run_top(col, lay, kw.pop("m", 3), True, expect=INV, **kw)


# ---- launch_score_select and launch_score_counts -----------------------------------------------------------------------------------
def run_select(col, lay, probs, label=None, label0=0, expect=0, junk=True, **kw):
    col = np.ascontiguousarray(col, dtype=np.float64)
    Cn = col.shape[0]
    a = dict(NP=lay.NP, nprobs=len(probs), hist=True, state=True)
    a.update(kw)
    P = max(len(probs), 1)
    hist = np.full(Cn * rc.SEL_HIST_WORDS, 0xFFFFFFFFFFFFFFFF if junk else 0, dtype=np.uint64)  # the launcher zeroes it itself
    state = np.full(Cn * rc.SEL_STATE_WORDS, -1 if junk else 0, dtype=np.int64)                 # ... and needs no initial state
    out = _guarded(Cn + 2 * Cn * P, ICANARY, np.int64)
    pr = np.ascontiguousarray(list(probs) + [0.0], dtype=np.float64)
    lab = None if label is None else np.ascontiguousarray(label, dtype=np.int32)
    rc_ = _hook("lcx_test_score_select", SELECT_ARGS)(ah._p(col), col.shape[1], Cn, a["NP"], ah._p(lay.rginfo), lay.nrows, ah._p(lab), label0,
                                                     a["nprobs"], ah._p(pr), GUARD, ah._p(hist) if a["hist"] else None,
                                                     ah._p(state) if a["state"] else None, ah._p(out))
    assert rc_ == expect, rc_
    if expect != 0:
        assert np.all(out == ICANARY)
        return None
    assert not hist.any(), "the histograms are zero again after the call"
    o = _mid(out, ICANARY, "out")
    return o[:Cn], o[Cn:Cn + Cn * P].reshape(Cn, P), o[Cn + Cn * P:].reshape(Cn, P).view(np.float64), state.reshape(Cn, -1)


def run_counts(col, lay, thr, label=None, label0=0, expect=0, **kw):
    col = np.ascontiguousarray(col, dtype=np.float64)
    Cn = col.shape[0]
    a = dict(NP=lay.NP, nthr=len(thr))
    a.update(kw)
    T = max(len(thr), 1)
    out = _guarded(Cn * (1 + T), 0xA5A5A5A5A5A5A5A5, np.uint64)  # junk: the launcher zeroes what it owns
    th = np.ascontiguousarray(list(thr) + [0.0], dtype=np.float64)
    lab = None if label is None else np.ascontiguousarray(label, dtype=np.int32)
    rc_ = _hook("lcx_test_score_counts", COUNTS_ARGS)(ah._p(col), col.shape[1], Cn, a["NP"], ah._p(lay.rginfo), lay.nrows, ah._p(lab), label0,
                                                     a["nthr"], ah._p(th), GUARD, ah._p(out))
    assert rc_ == expect, rc_
    if expect != 0:
        return None
    o = _mid(out, 0xA5A5A5A5A5A5A5A5, "out").reshape(Cn, 1 + T).astype(np.int64)
    return o[:, 0], o[:, 1:]


def _valid_cols(col, lay, label=None, label0=0):
    cols = col[:, : lay.NP][:, lay.valid].T
    return cols, None if label is None else label[: lay.NP][lay.valid] - label0


def check_select(col, lay, probs, label=None, label0=0):
    n, rank, value, state = run_select(col, lay, probs, label, label0)
    cols, lab = _valid_cols(col, lay, label, label0)
    wn, wrank, wvalue = ssr.quantiles(cols, probs, lab)
    assert np.array_equal(n, wn), (n, wn)
    assert np.array_equal(rank, wrank), (rank, wrank)
    ok = wrank >= 0
    assert np.array_equal(_bits(value)[ok], _bits(wvalue)[ok]) and np.all(_bits(value)[~ok] == 0)
    return n, rank, value, state


def check_counts(col, lay, thr, label=None, label0=0):
    n, atmost = run_counts(col, lay, thr, label, label0)
    cols, lab = _valid_cols(col, lay, label, label0)
    wn, wat = ssr.counts(cols, thr, lab)
    assert np.array_equal(n, wn) and np.array_equal(atmost, wat), (atmost, wat)


def _thresholds(col):
    s = np.unique(col[np.isfinite(col)])
    pick = s[np.linspace(0, s.size - 1, min(s.size, 5)).astype(int)] if s.size else np.zeros(0)
    t = [-np.inf, np.inf, -0.0, np.nan] + list(pick) + list((pick[:-1] + pick[1:]) / 2)
    return (t + [0.5, -0.5, 1e300, -1e300])[:16]


@pytest.mark.parametrize("p", range(8))
def test_select_follows_sixteen_prefixes_from_pass(p):
    rng = np.random.default_rng(20 + p)
    NP = CH + 21 * RG
    lay = rc.Layout(NP, fill=rc.ragged_fill(NP, rng))
    n = int(lay.valid.sum()) // 16 * 16
    col = np.full((3, NP), -1e300)
    take = lay.pos[:n]
    for c in range(3):
        col[c, take] = rc.pass_family(p, n, rng)
    col[:, lay.pos[n:]] = np.nan  # (the valid rows left over take no part)
    wide = _columns(col, lay, ld=NP + 32, slack=-1e300)
    cnt, rank, value, state = check_select(wide, lay, rc.PASS_PROBS)
    assert np.all(cnt == n) and np.all(state.view(np.int32)[:, rc.STATE_NACT_INT] == 16)
    assert all(np.unique(ssr.key_map(value[c]) >> np.uint64(56 - 8 * p)).size == 16 for c in range(3))
    check_select(wide, lay, [0.5])
    check_counts(wide, lay, _thresholds(col[0, take]))


def test_select_duplicates_empty_column_labels_and_clamped_probabilities():
    rng = np.random.default_rng(31)
    NP = CH + 5 * RG
    lay = rc.Layout(NP, fill=rc.ragged_fill(NP, rng))
    dup = rng.integers(0, 3, NP) / 4.0
    zeros = np.where(rng.random(NP) < 0.5, 0.0, -0.0)
    col = np.stack([dup, np.full(NP, np.nan), rng.standard_normal(NP), zeros])  # an empty column between full ones
    col[:, ~lay.valid] = -1e300
    n = int(lay.valid.sum())
    probs16 = [0.0, 1.0, -0.5, 1.5, 0.25, 0.5, 8.0 / n, 1.0 / n, (n - 1.0) / n, 0.999, 1e-12, 0.5, 0.75, 2.0 / 3.0, 0.1, 0.9]
    for probs in ([0.5], probs16):
        cnt, rank, value, _ = check_select(col, lay, probs)
        assert cnt[1] == 0 and np.all(rank[1] == -1) and np.all(_bits(value[1]) == 0)
    cnt, rank, _, _ = check_select(col, lay, probs16)
    assert rank[0][2] == 0 and rank[0][3] == n - 1  # the documented clamp
    check_counts(col, lay, _thresholds(dup))
    check_counts(col, lay, [-0.0])
    check_counts(col, lay, [np.nan])
    for label0 in (0, 5, -3):
        label = (rng.integers(-1, 5, NP) + label0).astype(np.int32)
        label[~lay.valid] = label0  # (pad rows with a fitting label still take no part)
        check_select(col, lay, probs16, label, label0)
        check_counts(col, lay, _thresholds(dup), label, label0)
    none = np.full(NP, 99, dtype=np.int32)  # no row of any column takes part
    cnt, rank, _, _ = check_select(col, lay, [0.5, 0.1], none, 5)
    assert np.all(cnt == 0) and np.all(rank == -1)


def test_select_runs_with_interleaved_non_participants():
    rng = np.random.default_rng(32)
    NP = CH + 64
    col, label, fill = rc.interleaved_runs(NP, rng)
    lay = rc.Layout(NP, fill=fill)
    cols = np.stack([col, col[::-1].copy()])
    lab = label  # column 0 sees label 5, column 1 label 6
    check_select(cols, lay, rc.PASS_PROBS, lab, 5)
    check_counts(cols, lay, [-3.0, -2.5, 0.0, 3.0, np.inf], lab, 5)
    check_select(cols, lay, rc.PASS_PROBS)
    check_counts(cols, lay, [-3.0, -2.5, 0.0, 3.0, np.inf])


@pytest.fixture(scope="module")
def many_columns():
    """C = 2048 columns of NP = 8192 + 16 rows: one block per column walks two chunks; the deciding values sit in the second"""
    rng = np.random.default_rng(33)
    Cn, NP = rc.SEL_GRID_BLOCKS, CH + 16
    nrows = NP - 3
    col = rng.standard_normal((Cn, NP))
    col[:, CH:nrows] = np.concatenate([np.linspace(-50.0, -40.0, 7), np.linspace(40.0, 50.0, 6)])[None, :] + rng.random((Cn, 1))
    col[:, nrows:] = -1e300
    return col, rc.Layout(NP, nrows=nrows)


def test_select_chunk_stride_loop(many_columns):
    col, lay = many_columns
    probs = [0.0, 0.5, 1.0]
    n, rank, value, _ = run_select(col, lay, probs)
    wn, wrank, wvalue = rc.quantiles_fast(col[:, : lay.nrows].T, probs)
    assert np.array_equal(n, wn) and np.array_equal(rank, wrank) and np.array_equal(_bits(value), _bits(wvalue))
    assert np.all(value[:, 0] < -40.0) and np.all(value[:, 2] > 40.0)  # both from the second chunk
    some = [0, 1, 1023, 2047]
    ref = ssr.quantiles(col[some][:, : lay.nrows].T, probs)
    assert np.array_equal(_bits(ref[2]), _bits(wvalue[some]))


@pytest.mark.parametrize("nthr", [1, 16])
def test_counts_chunk_stride_loop(many_columns, nthr):
    col, lay = many_columns
    thr = [45.0, -45.0, -np.inf, np.inf, 0.0, -0.0, np.nan, 41.5, -41.5, 1.0, -1.0, 49.0, -49.0, 2.0, -2.0, 0.5][:nthr]
    n, atmost = run_counts(col, lay, thr)
    v = col[:, : lay.nrows]
    with np.errstate(invalid="ignore"):
        want = np.stack([(v <= t).sum(axis=1) for t in thr], axis=1)
    assert np.all(n == lay.nrows) and np.array_equal(atmost, want)


def test_select_and_counts_refusals_and_empty():
    lay = rc.Layout(32, nrows=30)
    col = np.arange(64, dtype=np.float64).reshape(2, 32)
    run_select(col, lay, [], expect=INV)
    run_select(col, lay, [0.5] * 17, expect=INV)
    run_select(np.zeros((2, 0)), rc.Layout(0, nrows=0), [0.5], expect=INV)
    run_select(col, lay, [0.5], expect=INV, hist=False)
    run_select(col, lay, [0.5], expect=INV, state=False)
    run_counts(col, lay, [], expect=INV)
    run_counts(col, lay, [0.5] * 17, expect=INV)
    n, atmost = run_counts(np.zeros((2, 0)), rc.Layout(0, nrows=0), [0.5, 1.0])  # NP = 0: zeros, nothing launched
    assert not n.any() and not atmost.any()


# ---- launch_rows_beyond -------------------------------------------------------------------------------------------------------------
def run_beyond(col, lay, thr, above, capacity, label=None, label0=0, expect=0, **kw):
    col = np.ascontiguousarray(col, dtype=np.float64)
    a = dict(C=1, nchunks=_chunks(lay.NP), pos=True, score=True)
    a.update(kw)
    nch = _chunks(lay.NP)
    chunkoff, total = _guarded(nch, ICANARY, np.int64), np.full(1, ICANARY, dtype=np.int64)
    pos, score = _guarded(capacity, ICANARY, np.int64), _guarded(capacity, CANARY, np.float64)
    lab = None if label is None else np.ascontiguousarray(label, dtype=np.int32)
    rc_ = _hook("lcx_test_rows_beyond", BEYOND_ARGS)(ah._p(col), col.size // max(a["C"], 1), a["C"], lay.NP,
                                                    ah._p(lay.rginfo), lay.nrows, ah._p(lab), label0, float(thr), int(above), capacity,
                                                    a["nchunks"], GUARD, ah._p(chunkoff), ah._p(total), ah._p(pos) if a["pos"] else None,
                                                    ah._p(score) if a["score"] else None)
    assert rc_ == expect, rc_
    if expect != 0:
        assert total[0] == ICANARY and np.all(pos == ICANARY) and np.all(chunkoff == ICANARY)
        return None
    return int(total[0]), _mid(pos, ICANARY, "pos"), _mid(score, CANARY, "score"), _mid(chunkoff, ICANARY, "chunkoff")


def check_beyond(col, lay, thr, above, label=None, label0=0, capacities=None):
    """-> total.  Every capacity of (0, total - 1, total, total + 5), or 0 and total ("ends"): the first min(total, capacity) qualifiers in row order"""
    v = col[: lay.NP]
    ok = lay.valid & ~np.isnan(v)
    if label is not None:
        ok &= label[: lay.NP] == label0
    with np.errstate(invalid="ignore"):
        ok &= (v >= thr) if above else (v <= thr)
    want = np.flatnonzero(ok)
    per_chunk = np.add.reduceat(ok.astype(np.int64), np.arange(0, lay.NP, CH)) if lay.NP else np.zeros(0, dtype=np.int64)
    wantoff = np.concatenate([[0], np.cumsum(per_chunk)[:-1]]) if lay.NP else per_chunk
    if lay.rginfo is None and label is None:  # the shared reference, where it takes this layout
        t, _, row, sc_ = ssr.beyond(v[: lay.nrows], [lay.nrows], thr, above)
        assert t == want.size and np.array_equal(row, want) and np.array_equal(_bits(sc_), _bits(v[want]))
    if capacities == "ends":
        capacities = [0, want.size]
    for cap in capacities if capacities is not None else sorted({0, max(want.size - 1, 0), want.size, want.size + 5}):
        total, pos, score, chunkoff = run_beyond(col, lay, thr, above, cap, label, label0)
        assert total == want.size, (total, want.size)  # exact also when the output is truncated
        k = min(cap, want.size)
        assert np.array_equal(pos[:k], want[:k]) and np.array_equal(_bits(score[:k]), _bits(v[want[:k]]))
        assert np.all(pos[k:] == ICANARY) and np.all(score[k:] == CANARY)
        assert np.array_equal(chunkoff, wantoff)  # the exclusive scan of the chunks' counts
    return want.size


@pytest.mark.parametrize("NP", [16, CH + 16])
@pytest.mark.parametrize("above", [0, 1])
def test_rows_beyond(NP, above):
    rng = np.random.default_rng(40 + NP % 97 + above)
    lay = rc.Layout(NP, fill=rc.ragged_fill(NP, rng))
    col = np.concatenate([rng.standard_normal(NP), np.full(16, 1e9 if above else -1e9)])  # ld = NP + 16, the slack would qualify
    col[:NP][~lay.valid] = 1e9 if above else -1e9
    col[:NP][rng.random(NP) < 0.1] = np.nan
    col[:NP][rng.random(NP) < 0.1] = 0.7  # present values: the comparison includes equality
    col[3] = 0.7
    assert check_beyond(col, lay, 0.7, above) > 0
    assert check_beyond(col, lay, np.nan, above) == 0
    check_beyond(col, lay, -np.inf if above else np.inf, above)
    for label0 in (4, -2):
        label = (rng.integers(0, 3, NP) + label0).astype(np.int32)
        check_beyond(col, lay, 0.7, above, label, label0)
    one = rc.Layout(NP, nrows=NP - 5)
    check_beyond(col, one, 0.7, above)


@pytest.mark.parametrize("nch", [1024, 1025])
def test_rows_beyond_scan_second_round(nch):
    """more chunks than the scan block has threads: the carry between its rounds"""
    NP = nch * CH
    lay = rc.Layout(NP, nrows=NP - 9)
    col = np.zeros(NP)
    col[::4099] = 2.0
    col[(nch - 1) * CH:] = 3.0  # ... and the whole last chunk
    total = check_beyond(col, lay, 1.0, 1, capacities=None if nch == 1025 else "ends")
    assert total == np.count_nonzero(col[: NP - 9] >= 1.0) and total > CH
    if nch == 1025:
        assert check_beyond(-col, lay, -1.0, 0, capacities=[total]) == total


def test_rows_beyond_refusals():
    lay = rc.Layout(32, nrows=30)
    col = np.arange(32, dtype=np.float64)
    run_beyond(np.arange(64, dtype=np.float64), lay, 1.0, 1, 4, expect=INV, C=2)
    run_beyond(col, lay, 1.0, 1, 4, expect=INV, nchunks=2)
    run_beyond(col, lay, 1.0, 1, 4, expect=INV, nchunks=0)
    run_beyond(col, lay, 1.0, 1, 4, expect=INV, pos=False)
    run_beyond(col, lay, 1.0, 1, 4, expect=INV, score=False)
    total, pos, _, _ = run_beyond(col, lay, 1.0, 1, 0, pos=False, score=False)  # capacity 0 needs no buffer
    assert total == 29
    total, _, _, _ = run_beyond(np.zeros(0), rc.Layout(0, nrows=0), 1.0, 1, 0)
    assert total == 0
