"""The premises of tests/test_gpu_stats_speck_sort.py that can be checked on the CPU.

1. For the seeds of sk.same_bits_problem the float64 reference gives the same bits for q and for q with EVERY value below
   2^-300 zeroed (the sorted pass drops more specks than the unsorted rule, at most all of them): a difference between the
   modes on the GPU is then a finding about the hardware's summation order, not about the seeds.
2. The slot rule, restated in numpy (slots: stable sort by owning quad, the rows as they come when a row keeps two quads),
   applied to the constructed responsibilities: with pure_step_q no step of any batch size mixes quads, and without sorting
   every step does; with mixed_q every batch keeps its order."""
import numpy as np
import pytest

import hot_refs as hr
import test_gpu_stats_speck_skip as sk
import test_gpu_stats_speck_sort as so


@pytest.mark.parametrize("NP", sk.NPS)
@pytest.mark.parametrize("DP,DC,K", sk.FEAT)
def test_float64_reference_gives_the_same_bits_with_every_speck_dropped(DP, DC, K, NP):
    X, q = sk.same_bits_problem(DP, DC, K, NP)
    qz = so.flushed(q)
    assert not np.array_equal(q, qz), "nothing would be dropped"
    m = sk.low(DP, DC)
    assert sk.same_bits(hr.stats_ref(X, q)[:, m], hr.stats_ref(X, qz)[:, m])


def popcounts(masks):
    return np.array([bin(int(v)).count("1") for v in masks])


def test_slot_rule_is_a_stable_sort_with_the_unowned_rows_last():
    masks = [4, 0, 1, 4, 1, 0, 2, 1]
    assert so.slots(masks, 8).tolist() == [4, 6, 0, 5, 1, 7, 3, 2]
    assert so.slots([4, 0, 3, 4], 8).tolist() == [0, 1, 2, 3], "a row with two kept quads: the batch keeps its order"


@pytest.mark.parametrize("BR", so.BATCH_ROWS)
@pytest.mark.parametrize("DP,DC,K", sk.FEAT)
def test_constructed_rows_sort_into_pure_steps(DP, DC, K, BR):
    NP = 272
    q, specks = so.pure_step_q(K, NP)
    assert np.all(popcounts(so.row_masks(q)) == 1), "every row has one owning quad"
    # unsorted, every step keeps two quads (and with them every speck: each sits in the other owner's quad)
    _, kept = sk.speck_rule(q)
    assert np.all(kept.sum(axis=0) == 2) and np.array_equal(sk.speck_rule(q)[0], q)
    # sorted, no step of any batch mixes quads, whatever the batch size and wherever the rows past the end go
    for masks in so.placed_step_masks(q, BR):
        assert np.all(popcounts(masks) <= 1), masks
    # the rows of a batch come in whole groups of eight (row chunks start at multiples of 32)
    assert BR % 8 == 0 and NP % 8 == 0


@pytest.mark.parametrize("BR", so.BATCH_ROWS)
def test_mixed_rows_keep_every_batch_in_order(BR):
    NP, K = 272, 32
    q, _ = so.mixed_q(K, NP)
    m = so.row_masks(q)
    for b0 in range(0, NP, BR):
        mb = m[b0:b0 + BR]
        assert (popcounts(mb) > 1).any() and np.array_equal(so.slots(mb, 8), np.arange(mb.size))
    assert np.array_equal(sk.speck_rule(q)[0], q), "unsorted, every speck sits in a kept pair"
