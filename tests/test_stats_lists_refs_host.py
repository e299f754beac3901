"""tests/stats_lists_ref.py (the numpy restatement the GPU tests of the list route compare with) against a plain loop over
rows and clusters, on the CPU."""
import numpy as np

import stats_lists_ref as sl


def loop_rule(q, nchunks, chunk_rows):
    K, NP = q.shape
    nq = (K + 3) // 4
    out = [[[] for _ in range(nq)] for _ in range(nchunks)]
    for n in range(NP):
        for c in range(nq):
            keep = False
            for k in range(4 * c, min(4 * c + 4, K)):
                v = q[k, n]
                if not (v < sl.TAU):  # (a NaN compares false: kept)
                    keep = True
            if keep:
                out[n // chunk_rows][c].append(n % chunk_rows)
    return out


def test_list_rule_equals_the_loop():
    rng = np.random.default_rng(5)
    for K, NP, nchunks, rows in ((32, 272, 1, 288), (30, 200, 3, 96), (5, 96, 2, 64)):
        q = 2.0 ** -rng.uniform(0.0, 600.0, size=(K, NP))
        q[rng.random((K, NP)) < 0.3] = 0.0
        q[0, 3] = sl.TAU
        q[1, 5] = np.nextafter(sl.TAU, 0.0)
        q[K - 1, 7] = np.nan
        q[:, NP - 3:] = 0.0
        lens, lists = sl.list_rule(q, nchunks, rows)
        ref = loop_rule(q, nchunks, rows)
        assert lens.shape == (nchunks, (K + 3) // 4)
        for i in range(nchunks):
            for c in range(lens.shape[1]):
                assert list(lists[i][c]) == ref[i][c] and lens[i, c] == len(ref[i][c])
                assert all(a < b for a, b in zip(ref[i][c], ref[i][c][1:]))


def test_edges_of_the_rule():
    q = np.zeros((6, 16))
    q[0, 0] = sl.TAU                      # exactly the threshold: kept
    q[1, 1] = np.nextafter(sl.TAU, 0.0)   # the next value below: not kept
    q[2, 2] = np.nan                      # kept
    q[5, 3] = 1.0                         # the ragged last quad (clusters 4, 5)
    q[0, 4] = q[4, 4] = 0.5               # a row in two lists
    lens, lists = sl.list_rule(q, 1, 16)
    assert [list(x) for x in lists[0]] == [[0, 2, 4], [3, 4]] and lens.tolist() == [[3, 2]]
    assert sl.one_quad_share(q) == 3 / 16
