#!/usr/bin/env python3
"""How much of the feature-GEMM statistics pass multiplies nothing but specks: the numpy oracle's VBEM on
bench.py's north-star mixture, on the CPU, from smoothed labels as lc_ctx_synth leaves them (0.9 on the label, the rest
spread evenly), and after every iteration a census of the responsibilities and of the (4-row step, cluster quad) pairs
that hold a value that is not below 2^-300.

    tools/speck_census.py [--rows 40000] [--dim 64] [--clusters 32] [--seed 1004] [--iters 3]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
TAU = 2.0 ** -300


def census(q):
    """q [N x K] -> the table's columns"""
    N, K = q.shape
    top2 = np.sort(q, axis=1)[:, -2:]
    n4, k4 = N // 4 * 4, K // 4 * 4
    below = (q[:n4, :k4] < TAU).reshape(n4 // 4, 4, k4 // 4, 4)
    active = (~below.all(axis=(1, 3))).sum(axis=1)  # quads per step
    return (float((top2[:, 1] == 1.0).mean()), float((q == 0.0).mean()), float((q < TAU).mean()), float(np.median(top2[:, 0])),
            float(active.mean()), k4 // 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=40000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--clusters", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1004)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    import bench
    import lc_oracle as o

    N, D, K = a.rows, a.dim, a.clusters
    mu, L = bench.mixture(D, K, a.seed)
    rng = np.random.default_rng(a.seed)
    lab = rng.integers(0, K, N)
    X = mu[lab] + np.einsum("nij,nj->ni", L[lab], rng.normal(size=(N, D)))
    q0 = np.full((N, K), 0.1 / (K - 1))
    q0[np.arange(N), lab] = 0.9
    print(f"N = {N}, D = {D}, K = {K}, mixture seed {a.seed} (bench.mixture), labels and noise from numpy's default_rng({a.seed})")
    print("after iteration | rows with max q == 1.0 | entries == 0.0 | entries < 2^-300 | median second-largest q | active quads per 4-row step")
    for it in range(1, a.iters + 1):
        _, _, qT, _, _ = o.vbem_fixed([X], [q0], o.Dirichlet, 1.0, it)
        hard, zero, speck, second, act, nq = census(qT[0])
        print(f"{it:15d} | {100 * hard:21.1f}% | {100 * zero:13.2f}% | {100 * speck:15.2f}% | {second:23.3g} | {act:.2f} of {nq}")


if __name__ == "__main__":
    main()
