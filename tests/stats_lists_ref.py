"""The row lists of the statistics pass's list route (launch_suffstat_list_build), restated in numpy.

Quads are the clusters 4 c ... 4 c + 3 (the last one may be ragged), chunks the rows [i * chunk_rows, (i + 1) * chunk_rows).
A row is in the list of (chunk, quad) when not every value it has in the quad's clusters satisfies q < TAU: a NaN is kept,
a row of zeros (a pad row) is in no list, a soft row is in the list of every quad it keeps.  Lists hold chunk-local row
offsets in ascending order."""
from __future__ import annotations

import numpy as np

TAU = 2.0 ** -300


def kept_rows(q):
    """-> [quads x NP] bool: the row keeps a value of the quad"""
    K, NP = q.shape
    nq = -(-K // 4)
    qq = np.zeros((4 * nq, NP))
    qq[:K] = q
    with np.errstate(invalid="ignore"):
        below = (qq < TAU).reshape(nq, 4, NP)
    return ~below.all(axis=1)


def list_rule(q, nchunks, chunk_rows):
    """-> lens [nchunks x quads] and lists[chunk][quad] (int arrays of chunk-local offsets)"""
    kept = kept_rows(q)
    nq, NP = kept.shape
    lens = np.zeros((nchunks, nq), dtype=np.int64)
    lists = []
    for i in range(nchunks):
        r0, r1 = i * chunk_rows, min((i + 1) * chunk_rows, NP)
        row = [np.nonzero(kept[c, r0:r1])[0] for c in range(nq)]
        lens[i] = [len(r) for r in row]
        lists.append(row)
    return lens, lists


def one_quad_share(q):
    """share of the rows that keep exactly one quad (what the context's probe estimates from its sample)"""
    return float((kept_rows(q).sum(axis=0) == 1).mean())
