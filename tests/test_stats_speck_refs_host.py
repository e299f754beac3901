"""The premise of tests/test_gpu_stats_speck_skip.py::test_hard_rows_same_bits_with_and_without_skipping, on the CPU: for
the seeds of its problems the float64 reference itself gives the same bits for q and for q' (q with the skipped pairs
zeroed) -- a speck added to a sum of order one changes nothing.  A change of seed or generator that breaks this shows here,
not as an unexplained difference on the GPU."""
import numpy as np
import pytest

import hot_refs as hr
import test_gpu_stats_speck_skip as sk


@pytest.mark.parametrize("NP", sk.NPS)
@pytest.mark.parametrize("DP,DC,K", sk.FEAT)
def test_float64_reference_gives_the_same_bits_with_and_without_the_skipped_pairs(DP, DC, K, NP):
    X, q = sk.same_bits_problem(DP, DC, K, NP)
    qs, kept = sk.speck_rule(q)
    assert not kept.all() and not np.array_equal(q, qs), "nothing would be skipped"
    m = sk.low(DP, DC)
    assert sk.same_bits(hr.stats_ref(X, q)[:, m], hr.stats_ref(X, qs)[:, m])
