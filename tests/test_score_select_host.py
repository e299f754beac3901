"""Order and threshold queries, the parts that need no GPU: the numpy reference of the GPU tests keeps the
header's order and rank rule, the constant of the binding is the header's, and the shipped library exports the calls."""
import re

import numpy as np

import aux_hooks
import score_select_ref as ref
from libcluster_amd import capi


def test_key_map_sorts_like_numpy_and_puts_minus_zero_first():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(500), rng.standard_normal(50) * 1e300, rng.integers(-3, 4, 200) * 5e-324,
                        [np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, np.finfo(np.float64).max, np.finfo(np.float64).tiny]])
    rng.shuffle(x)
    k = ref.key_map(x)
    assert k.dtype == np.uint64
    by_key = x[np.argsort(k, kind="stable")]
    assert np.array_equal(by_key, np.sort(x))  # (== : -0.0 and +0.0 compare equal here)
    # strictly: equal keys only for equal bits, and the key order refines <
    i, j = rng.integers(0, x.size, 4000), rng.integers(0, x.size, 4000)
    assert np.all((x[i] < x[j]) <= (k[i] < k[j]))
    assert np.array_equal(k[i] == k[j], x[i].view(np.int64) == x[j].view(np.int64))
    z = np.array([0.0, -0.0, 0.0, -0.0])
    assert np.array_equal(np.signbit(z[np.argsort(ref.key_map(z), kind="stable")]), [True, True, False, False])
    assert ref.key_map(np.array([-np.inf]))[0] < ref.key_map(np.array([-1.0]))[0] < ref.key_map(np.array([-0.0]))[0]
    assert ref.key_map(np.array([0.0]))[0] < ref.key_map(np.array([5e-324]))[0] < ref.key_map(np.array([np.inf]))[0]


def test_rank_rule_is_numpys_inverted_cdf():
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 7, 16, 100, 1001):
        s = rng.standard_normal(n)
        srt = np.sort(s)
        probs = np.concatenate([rng.random(40), [0.0, 1.0, 0.5, 0.25, 1.0 / n, (n - 1.0) / n, 1e-12]])
        for p in probs:
            r = ref.rank_rule(p, n)
            assert 0 <= r < n
            assert srt[r] == np.quantile(s, p, method="inverted_cdf"), (n, p, r)
    assert ref.rank_rule(0.5, 0) == -1
    assert ref.rank_rule(0.0, 5) == 0 and ref.rank_rule(1.0, 5) == 4 and ref.rank_rule(0.4, 5) == 1 and ref.rank_rule(1e-12, 5) == 0
    count, rank, value = ref.quantiles(np.array([[3.0], [np.nan], [1.0], [2.0]]), [0.0, 0.5, 1.0])
    assert count[0] == 3 and list(rank[0]) == [0, 1, 2] and list(value[0]) == [1.0, 2.0, 3.0]


def test_quantiles_max_is_the_headers():
    m = re.findall(r"#define\s+LC_QUANTILES_MAX\s+(\d+)", capi.HEADER.read_text())
    assert len(m) == 1
    assert int(m[0]) == capi.QUANTILES_MAX == ref.QUANTILES_MAX
    assert capi.ScoreQuantiles._fields == ("count", "rank", "value")
    assert capi.ScoreCounts._fields == ("count", "atmost")
    assert capi.FlaggedRows._fields == ("total", "group", "row", "score")


def test_shipped_library_exports_the_entry_points(lib):
    names = capi.declared_symbols()
    shipped = aux_hooks.exported_symbols(aux_hooks.SHIPPED_LIB)
    for n in ("lc_ctx_score_quantiles", "lc_ctx_score_counts", "lc_ctx_rows_beyond"):
        assert n in names, f"{n} is not declared in include/libcluster_hip.h"
        assert n in shipped, f"{n} is not exported by the shipped library"
        assert hasattr(lib, n) and getattr(lib, n).argtypes is not None
