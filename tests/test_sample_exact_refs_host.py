"""The exact references of the launcher-level sampler tests (tests/sample_ref.py) and the inputs of those tests
(tests/sample_kernel_cases.py, tests/rank_select_cases.py), held to their conditions without a GPU: the restated gamma draw
and the three families pass the project's own KS bar against scipy, next to no counter has a decision near its boundary, the
float64 reference is measured against 40-digit arithmetic on the same Philox words (E_REF), and the constants the cases
straddle are the sources'."""
import re
from pathlib import Path

import numpy as np
import pytest
from scipy import stats

import rank_select_cases as rc
import sample_kernel_cases as sc
import sample_ref as sr
import score_select_ref as ssr

CSRC = Path(__file__).resolve().parents[1] / "libcluster_amd" / "csrc"


def _cap(excluded, total, what):
    cap = 1 if total < 1000 else int(sr.EXCLUDED_SHARE * total)
    print(f"{what}: {excluded} of {total} left out (cap {cap})")
    assert excluded <= cap, what


# ---- distribution -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [0.3, 1.0, 2.5, 11.5, 250.0])
def test_gamma_draw_is_gamma(shape):
    n = 50_000
    G, attempts, margin = sr.gamma_draw(sc.SEED, 3, np.arange(n), 7, shape, row_offset=(1 << 32) - 100)
    tally = sr.Tally()
    tally.add([stats.kstest(G, stats.gamma(shape).cdf)], f"gamma_draw, shape {shape:g}, {n} counters")
    print(f"shape {shape:g}: at most {attempts.max()} attempts, smallest margin {margin.min():.3e}")
    assert attempts.max() <= 8 and attempts.min() == 1
    _cap(int((margin <= sr.NEAR).sum()), n, f"gamma decisions, shape {shape:g}")
    # another slot, block or row offset is another stream
    assert not np.array_equal(G[:100], sr.gamma_draw(sc.SEED, 3, np.arange(100), 8, shape, row_offset=(1 << 32) - 100)[0])
    assert np.array_equal(G[100:200], sr.gamma_draw(sc.SEED, 3, np.arange(100), 7, shape, row_offset=1 << 32)[0])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_families_have_their_documented_distribution(mode):
    """one component, many rows: mode 0 whitened is Student-t with 2 shape degrees of freedom, mode 1 per column, mode 2 Lomax"""
    n, D, shape = 50_000, 3, 2.5
    rng = np.random.default_rng(5)
    loc = rng.normal(size=(1, D))
    fac = np.tril(rng.normal(size=(1, D, D))) + 2 * np.eye(D) if mode == 0 else 0.5 + rng.random((1, D))
    e = sr.sample_rows(mode, sc.SEED, 1, np.arange(n), np.array([1.0]), 0, loc, fac, np.array([shape]))
    assert np.all(e.label == 0)
    tally = sr.Tally()
    if mode == 0:  # x = loc + F eps / sqrt(G): F^-1 (x - loc) sqrt(shape) has t(2 shape) coordinates
        w = np.linalg.solve(fac[0], (e.x - loc[0]).T).T * np.sqrt(shape)
        tally.add([stats.kstest(w[:, d], stats.t(2 * shape).cdf) for d in range(D)], "Gauss-Wishart rows")
        tally.add([stats.kstest((w * w).sum(axis=1) / D, stats.f(D, 2 * shape).cdf)], "Gauss-Wishart radius")
    elif mode == 1:
        w = (e.x - loc[0]) / fac[0] * np.sqrt(shape)
        tally.add([stats.kstest(w[:, d], stats.t(2 * shape).cdf) for d in range(D)], "NormGamma entries")
        assert abs(np.corrcoef(np.abs(w[:, 0]), np.abs(w[:, 1]))[0, 1]) < 0.03  # (a gamma of its own per column)
    else:
        tally.add(sr.ks_lomax(e.x, shape, fac[0]), "ExpGamma entries")
    _cap(int((~e.value_far).sum()), n, f"mode {mode}: rows with a gamma decision near its boundary")


# ---- the cases: what is left out, and the reference's own error ------------------------------------------------------------------
def _sample_cases(mode):
    return [c for c in list(sc.SAMPLE_CASES.values()) + [sc.WIDE_CASE] if c.mode == mode]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_sample_cases_leave_out_next_to_nothing(mode):
    for c in _sample_cases(mode):
        ex = [e for _, e in c.exact()]
        total = sum(e.label.size for e in ex)
        _cap(sum(int((~e.label_far).sum()) for e in ex), total, f"{c.name}: labels")
        _cap(sum(int((~(e.label_far & e.value_far)).sum()) for e in ex), total, f"{c.name}: values")
        if c.J == 3 and c.Kp > 2:  # the short sum decides somewhere, and klast is not the last component
            e = ex[-1]
            u = sr.choice_u(sc.SEED, 2, np.arange(37), 0, c.row_offset)
            assert np.any(u > c.cdf[2, -1]) and np.all(e.label[u > c.cdf[2, -1]] == c.Kp - 3)


def test_cond_cases_leave_out_next_to_nothing_and_hold_their_planted_rows():
    for c in sc.COND_CASES.values():
        ex = c.exact()
        total = sum(e.label.size for _, e in ex)
        _cap(sum(int((~e.label_far).sum()) for _, e in ex), total, f"{c.name}: labels")
        _cap(sum(int((~(e.label_far & e.value_far)).sum()) for _, e in ex), total, f"{c.name}: values")
        assert all(np.all(np.isfinite(e.x)) for _, e in ex)
        if c.planted:
            lab = np.full((c.NP, c.ndraws), -1)
            for pos, e in ex:
                lab[pos] = e.label
            assert np.all(lab[c.planted["under"]] == 2)
            assert np.sum(lab[c.planted["short"]] == c.Kp - 3) >= c.ndraws - 1  # the last component with weight
            for p in c.planted["hard"]:
                assert np.all(lab[p] == p % c.Kp)
    c = sc.COND_CASES["k17_m5_8x3_blocks"]
    assert c.NP == 272 and c.J == 2 and 5 in c.fills[0][1:-1] and 0 in c.fills[0]
    assert c.NP > sc.PC_THREADS // 64 * sc.PC_WAVE_ROWS  # two blocks of the kernel's grid
    assert {x.Kp % sc.CD_BATCH for x in sc.COND_CASES.values()} >= {0, 1, 7} and max(x.Kp for x in sc.COND_CASES.values()) > 2 * sc.CD_BATCH
    assert {x.ndraws % sc.CD_DRAWS for x in sc.COND_CASES.values()} >= {0, 1} and any(x.ndraws == sc.DRAWS_MAX for x in sc.COND_CASES.values())
    assert any(x.Db > 64 for x in sc.COND_CASES.values()) and any(x.Dae > 64 for x in sc.COND_CASES.values())


def _measure(pairs_f64, pairs_mp):
    worst = 0.0
    for (_, a), (_, b) in zip(pairs_f64, pairs_mp):
        assert np.array_equal(a.label, b.label)
        ok = np.broadcast_to((a.label_far & a.value_far)[..., None], a.x.shape)
        err = sr.scaled_error(sr.F64.lift(a.x).astype(object), b.x, b.mag)
        worst = max(worst, float(np.max(err[ok], initial=0.0)))
    return worst


def _held(key, measured):
    print(f"E_REF[{key!r}] = {sc.E_REF[key]:.3e}, measured {measured:.3e}")
    assert measured <= sc.E_REF[key] <= 2 * measured, (key, measured, sc.E_REF[key])


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reference_error_of_the_sample_cases(mode):
    pytest.importorskip("mpmath")
    mp = sr.mp_backend(40)
    _held(sc.FAMILY[mode], max(_measure(c.exact(), c.exact(mp)) for c in _sample_cases(mode)))


def test_reference_error_of_the_cond_cases():
    pytest.importorskip("mpmath")
    mp = sr.mp_backend(40)
    _held("cond", max(_measure(c.exact(), c.exact(mp)) for c in sc.COND_CASES.values()))


def test_reference_error_of_the_gamma_draw():
    pytest.importorskip("mpmath")
    mp = sr.mp_backend(40)
    worst = 0.0
    for shape in (0.3, 1.0, 2.5, 11.5, 250.0):
        a = sr.gamma_draw(sc.SEED, 0, np.arange(2000), 0, shape)[0]
        b = sr.gamma_draw(sc.SEED, 0, np.arange(2000), 0, shape, xp=mp)[0]
        worst = max(worst, float(np.max(sr.scaled_error(a.astype(object), b, abs(b)))))
    _held("gamma", worst)


def test_the_bar_is_the_issues():
    assert sr.value_bar(3, 1e-16) == 5 * 2.0 ** -53 + 8e-16 and sr.NEAR == 1e-9 and sr.EXCLUDED_SHARE == 1e-3


# ---- the constants the cases straddle are the sources' -----------------------------------------------------------------------------
def _const(text, name):
    """the value of `constexpr <integer type> name = <one integer literal>;` (decimal or hex, an optional u suffix)"""
    m = re.findall(r"constexpr\s+(?:int|uint32_t|unsigned)\s+" + name + r"\s*=\s*(0[xX][0-9a-fA-F]+|\d+)[uU]?\s*;", text)
    assert len(m) == 1, name
    return int(m[0], 0)


def test_constants_are_the_sources():
    k, rank, sel = (CSRC / "lc_kernels.h").read_text(), (CSRC / "lc_kernels_rank.hip").read_text(), (CSRC / "lc_kernels_select.hip").read_text()
    assert _const(k, "TOP_CHUNK_ROWS") == rc.TOP_CHUNK_ROWS and _const(k, "TOP_MAX_M") == rc.TOP_MAX_M
    assert _const(k, "SEL_MAX") == rc.SEL_MAX == ssr.QUANTILES_MAX and _const(k, "SEL_GRID_BLOCKS") == rc.SEL_GRID_BLOCKS
    assert _const(k, "SEL_STATE_WORDS") == rc.SEL_STATE_WORDS and "SEL_HIST_WORDS = SEL_MAX * 256" in k and rc.SEL_HIST_WORDS == rc.SEL_MAX * 256
    assert _const(rank, "TR_MERGE_WAVES") == rc.TR_MERGE_WAVES and _const(sel, "SCAN_THREADS") == rc.SCAN_THREADS
    assert "constexpr unsigned U = 4;" in rank and rc.MERGE_TRIP == rc.TR_MERGE_WAVES * 64 * 4
    assert 4 * rc.STATE_NACT_INT + 16 == 8 * rc.SEL_STATE_WORDS  # nact, a pad word and n close the state
    smp, pred, phx = (CSRC / "lc_kernels_sample.hip").read_text(), (CSRC / "lc_predict.hpp").read_text(), (CSRC / "lc_philox.hpp").read_text()
    assert _const(smp, "CD_BATCH") == sc.CD_BATCH and _const(smp, "CD_DRAWS") == sc.CD_DRAWS
    assert _const(pred, "PC_WAVE_ROWS") == sc.PC_WAVE_ROWS and _const(pred, "PC_THREADS") == sc.PC_THREADS
    assert _const(pred, "DRAWS_MAX") == sc.DRAWS_MAX and _const(phx, "RNG_GAMMA_ATTEMPTS") == sr.GAMMA_ATTEMPTS
    tags = {"CHOICE": sr.TAG_CHOICE, "NORMAL": sr.TAG_NORMAL, "GAMMA_N": sr.TAG_GAMMA_N, "GAMMA_U": sr.TAG_GAMMA_U,
            "GAMMA_B": sr.TAG_GAMMA_B, "LOMAX": sr.TAG_LOMAX}
    for name, tag in tags.items():
        assert _const(phx, "RNG_TAG_" + name) == tag, name
    header = (CSRC.parents[1] / "include" / "libcluster_hip.h").read_text()
    for tag in tags.values():
        assert re.search(rf"\*\s+0x{tag:02x}\s", header), hex(tag)


def test_rank_select_builders():
    rng = np.random.default_rng(3)
    for p in range(8):
        x = rc.pass_family(p, 16 * 24, rng)
        key = ssr.key_map(x)
        top = key >> np.uint64(64 - 8 * p) if p else np.zeros_like(key)
        assert np.unique(top).size == 1 and np.unique(key >> np.uint64(56 - 8 * p)).size == 16
        count, rank, value = ssr.quantiles(x[:, None], rc.PASS_PROBS)
        assert np.unique(ssr.key_map(value[0]) >> np.uint64(56 - 8 * p)).size == 16  # one requested rank in every group
        if p == 0:
            assert (x < 0).sum() == x.size // 2
    cols = rng.standard_normal((500, 7))
    cols[::3, 2] = 0.5
    probs = [0.0, 0.5, 1.0, 0.25]
    a, b = rc.quantiles_fast(cols, probs), ssr.quantiles(cols, probs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int64), b[2].view(np.int64))
    # the sizes at which the kernels take another path
    assert 64 * rc.TOP_CHUNK_ROWS // rc.TOP_CHUNK_ROWS * 64 == rc.MERGE_TRIP and 66 * 63 > rc.MERGE_TRIP
    assert -(-rc.SEL_GRID_BLOCKS // 2048) == 1 and (rc.TOP_CHUNK_ROWS + 16 + rc.TOP_CHUNK_ROWS - 1) // rc.TOP_CHUNK_ROWS == 2
    assert 1025 > rc.SCAN_THREADS
    lay = rc.Layout(96, fill=[16, 0, 5, 16, 1, 15])
    assert lay.valid.sum() == 53 and lay.pos[16] == 32 and lay.pos[20] == 36 and lay.pos[21] == 48
