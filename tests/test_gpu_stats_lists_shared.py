"""The list kernel's shared deal (suffstat_list_kernel at DC = 64) on the shapes tests/test_gpu_stats_lists.py
leaves out: the smallest K of the feature-GEMM route, a last quad of one or two clusters, rows whose responsibility is split
between two clusters of ONE quad (all four q of a step's quad in use, nothing exact), and a second quad on every eighth row.
Every row is in a list, so nothing is left out and the dense pass (lcx_test_suffstat_speck, mode 0) alone decides: bit for
bit, S exactly symmetric, guards untouched."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import aux_hooks as ah
import test_gpu_stats_lists as tl
import test_gpu_stats_speck_skip as sk

pytestmark = pytest.mark.gpu

WIDTHS = [(64, 64)]  # the converted widths ((64, 56) keeps the consecutive deal: tests/test_gpu_stats_lists.py)


@functools.lru_cache(maxsize=None)
def smallest_feat_K(DP, DC):
    """the smallest K >= 13 that the plan sends to the feature GEMM at 272 rows"""
    K = 13
    while ah.suffstat_plan(DP, DC, 272, K, "dense")["route"] != "feat":
        K += 1
        assert K < 30
    return K


def split_q(rng, K, NP):
    """Every row has an owner with a non-dyadic responsibility r in (0.5, 1); 1 - r goes to another cluster of the owner's
    quad (where the quad has one); every eighth row keeps a value of a second quad as well.  Everything else exact zeros."""
    nq = (K + 3) // 4
    q = np.zeros((K, NP))
    own = rng.integers(0, K, size=NP)
    own[rng.permutation(NP)[:K]] = np.arange(K)  # every cluster owns a row
    r = rng.uniform(0.5, 1.0, size=NP)
    q[own, np.arange(NP)] = r
    for n in range(NP):
        c = own[n] // 4
        mates = [k for k in range(4 * c, min(4 * c + 4, K)) if k != own[n]]
        if mates:
            q[mates[rng.integers(len(mates))], n] = 1.0 - r[n]
    for n in range(0, NP, 8):
        c = (own[n] // 4 + 1 + rng.integers(nq - 1)) % nq
        q[min(4 * c + rng.integers(4), K - 1), n] = rng.uniform(0.1, 0.4)
    assert not ((q > 0.0) & (q < sk.TAU)).any()
    return q


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("K", ["smallest", 30])
@pytest.mark.parametrize("DP,DC", WIDTHS)
def test_split_rows_same_bits_as_the_dense_pass(DP, DC, K, big):
    K = smallest_feat_K(DP, DC) if K == "smallest" else K
    NP = tl.np3(DC, K) if big else 272
    plan = ah.suffstat_plan(DP, DC, NP, K, "dense")
    assert plan["route"] == "feat" and (not big or plan["nchunks"] >= 3), plan
    rng = np.random.default_rng(1000 * K + NP + DC)
    X = np.zeros((NP, DP))
    X[:, :DC] = rng.normal(size=(NP, DC))
    q = split_q(rng, K, NP)
    rc, plan, got, lens, ent, _, _ = tl.run(X, DC, q, K)  # (tl.run asserts the guards behind both buffers)
    assert rc == 0
    tl.check_lists(q, plan, lens, ent)
    kept = (q.reshape(-1, NP) != 0.0)
    nq = (K + 3) // 4
    in_quad = np.stack([kept[4 * c:4 * c + 4].any(axis=0) for c in range(nq)])
    assert in_quad.any(axis=0).all() and (in_quad.sum(axis=0) > 1).sum() >= NP // 8 - 1  # every row in a list, an eighth in two
    assert lens.sum() == in_quad.sum()
    m = sk.low(DP, DC)
    ref = sk.folded(X, DC, q, K, 0)
    assert sk.same_bits(got[:, m], ref[:, m])
    S = got[:, 1 + DP:].reshape(K, DP, DP)[:, :DC, :DC]
    assert sk.same_bits(S, np.ascontiguousarray(S.transpose(0, 2, 1)))
    assert not np.isnan(got[:, m]).any() and np.all(got[:, 0] > 0.0)
