"""The inputs of tests/test_gpu_holes_kernels.py honour the conditions that file relies on (tests/holes_kernel_cases.py), shown
without a device: on every prediction case the numpy emulation of the device's route stays within ONE TENTH of each bar against
the direct reference, so the bars of the GPU file measure the kernel and not the conditioning of the case; the rows placed
for the 64-cluster chunks have their dominant component where intended; the draws cases leave out few labels, put enough mass
into the second chunk and give every pooled sample of G its 100 values."""
import numpy as np
import pytest

import holes_kernel_cases as hc
import incomplete_draws_ref as dr
import incomplete_ref as ref
import incomplete_var_ref as vref

PREDICT = hc.SHAPES + ["edges", "gnu0", "blocks3"]


def _emulated(c, shift=0.0):
    """the device's route in numpy, block by block, with the fill value the GPU file uses (+ shift spreads per column)"""
    tab = c.tab
    fill = tab.fill(c.blocks[0][1]) + shift * (c.blocks[0][1] @ tab.sd)
    rows, logp, var = [], [], []
    for Xh, w in c.blocks:
        a, lp = ref.emulate(Xh, tab.posts, None, w, 0.0, fill)
        rows.append(a), logp.append(lp)
        if c.notes.get("table_g"):
            var.append(None)
        else:
            var.append(vref.emulate_var(Xh, tab.posts, None, w, 0.0, fill))
    return np.concatenate(rows), np.concatenate(logp), None if var[0] is None else np.concatenate(var)


@pytest.mark.parametrize("name", PREDICT)
def test_emulated_route_within_a_tenth_of_the_bars(name):
    c = hc.case(name)
    count = np.isnan(c.Xh).sum(axis=1)
    assert np.all(count <= hc.HMAX) and np.all(count < c.tab.D)
    for shift in (0.0, 3.0) if name in ("d23_k5_n70", "d3_k2_n17") else (0.0,):
        rows, logp, var = _emulated(c, shift)
        got = hc.ratios(c.ref, rows, logp, var)
        print(f"{name}, fill + {shift:g} spreads: emulated against direct, ratio over scale: " + ", ".join(f"{k} {v:.2e}" for k, v in got.items()))
        for k, v in got.items():
            assert v <= 0.1 * hc.BARS[k], (k, v)
    holed = count > 0
    assert np.all(c.ref.var[holed][np.arange(hc.HMAX)[None, :] < count[holed, None]] > 0)
    soft = np.mean(np.nanmax(c.ref.r[holed], axis=1) < 0.99)
    print(f"{name}: {holed.sum()} rows with holes, hole counts {sorted(set(count[holed]))}, share with max r < 0.99: {soft:.2f}")


def test_the_shapes_hold_what_they_are_for():
    count = lambda n: np.isnan(hc.case(n).Xh).sum(axis=1)
    assert set(count("d9_k3_n40")) == set(range(9))  # nb = 1 ... 8 at D = 9: Da down to 1
    c = count("d23_k5_n70")
    assert np.all(c[:64] > 0) and 0 < np.sum(c[64:] > 0) < 6
    for n in hc.SHAPES:
        c, N = count(n), hc.case(n).Xh.shape[0]
        assert N < 3 or (0.2 < np.mean(c == 0) < 0.45 or n == "d23_k5_n70"), n
        assert N < 3 or np.any((c[:-1] == 0) & (c[1:] > 0)), n  # complete rows between rows with holes
    e = hc.case("edges")
    c = count("edges")
    assert np.flatnonzero(c[:64]).tolist() == [0] and np.flatnonzero(c[64:128]).tolist() == [63]
    r, k = e.notes["on_mean"]
    known = ~np.isnan(e.Xh[r])
    assert c[r] > 0 and np.array_equal(e.Xh[r, known], e.tab.posts[k][2][known])
    far = e.notes["far"]
    assert c[far] > 0 and all(np.min(np.abs(e.Xh[far, known2] - p[2][known2]) / e.tab.sd[i][known2]) > 20 for i, p in enumerate(e.tab.posts)
                              for known2 in [~np.isnan(e.Xh[far])])
    assert c[134] > 0 and e.Xh.shape[0] == 135
    g = hc.case("gnu0")
    assert np.any(g.tab.gnu[2] == 0.0) and np.any(count("gnu0") == 2) and np.all(g.tab.gnu[1] > 0)


def test_table_reference_equals_direct_var_where_the_variance_exists():
    c = hc.case("d9_k3_n40")
    Xh, w = c.blocks[0]
    var, Vn = hc.direct_var_table(Xh, c.tab.posts, w, c.tab.gnu)
    assert np.all(np.abs(var - c.ref.var) <= 1e-12 * c.ref.Vn[:, None]) and np.allclose(Vn, c.ref.Vn, rtol=1e-10, atol=0)
    holed = np.isnan(Xh).any(axis=1)
    t = hc.t_reference(c.ref.mixes[0], Xh)
    from scipy.special import logsumexp
    np.testing.assert_allclose(logsumexp(t[holed], axis=1), c.ref.logp[holed], rtol=1e-12, atol=0)


def test_chunk_rows_have_their_dominant_component_where_intended():
    c = hc.case("d23_k130_n20")
    for row, k in c.notes["placed"]:
        assert np.argmax(c.ref.r[row]) == k and c.ref.r[row, k] > 0.5, (row, k)
    assert [k // 64 for _, k in c.notes["placed"]] == [0, 1, 2]
    row, k, k2 = c.notes["between"]
    r = c.ref.r[row]
    top = np.argsort(r)[-2:]
    assert set(top) == {k, k2}
    print(f"the row between two components: r = {r[top[1]]:.3f} (component {top[1]}), {r[top[0]]:.3f} (component {top[0]})")
    assert top[0] // 64 != top[1] // 64 and r[top[0]] >= 0.2


@pytest.mark.parametrize("name", sorted(hc.DRAW_CASES))
def test_draw_cases(name):
    build, nd = hc.DRAW_CASES[name]
    c = hc.case(build)
    want, far = hc.label_reference(c, hc.DRAW_SEED, nd)
    holed = np.isnan(c.Xh).any(axis=1)
    left = int((~far[holed]).sum())
    print(f"{name}: {left} of {holed.sum() * nd} labels within 1e-9 of a boundary")
    assert left <= 1e-3 * holed.sum() * nd
    assert np.all(want[~holed] == -1) and want[holed].min() >= 0
    if build == "d5_k70_n40":
        mass = c.ref.r[holed][:, 64:].sum(axis=1).mean()
        print(f"{name}: share of the responsibilities in the second chunk {mass:.3f}")
        assert mass >= 0.2 and want.max() >= 64
    if build == "d5_k1_n120":
        count = np.isnan(c.Xh).sum(axis=1)
        for nb in range(1, 5):  # (about 1e-3 of the values are left out for a small |z|: 100 stays far away)
            assert np.sum(count == nb) * nd >= 200, nb
    if build == "blocks2":
        assert len(c.blocks) == 2
