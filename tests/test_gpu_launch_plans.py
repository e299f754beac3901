"""The two launch plans (lc_kernels.h): suffstat_plan, the ONE decision on kernel, row chunks and partial records of a
Gauss-Wishart statistics pass, and estep_plan, the one on instance, grid and LDS of an E-step launch.

The plans are read through lc_test_suffstat_plan / lc_test_estep_refusal of libcluster_hip_testhooks.so (tests/aux_hooks.py);
the statistics passes run through the context API of the shipped library."""
import ctypes as C

import numpy as np
import pytest

import aux_hooks as ah
from libcluster_amd import capi

pytestmark = pytest.mark.gpu

# the active widths every padded layout has (lc_kernels.h, estep_active_width)
WIDTHS = {16: (16,), 32: (20, 24, 28, 32), 48: (36, 40, 44, 48), 64: (56, 64), 80: (72, 80), 96: (88, 96), 112: (104, 112),
          128: (120, 128), 192: (192,)}
KS = (1, 2, 3, 5, 8, 13, 16, 17, 28, 32, 33, 40, 64)
NPS = (16, 1008, 65536, 70016)  # (the last two cross the NP >= 64 * 1024 threshold of the fill searches)


def test_suffstat_plan_invariants_at_every_layout_width_cluster_count_and_mode():
    """Every (DP, active width, K, mode, NP) of the grid above: the row chunks are whole staging batches that cover NP with
    no empty chunk, KR = K + extra, the row split of a ragged last slice (extra > 0) exists only where the per-cluster
    kernel runs a dense pass (with or without a mask staged as zeros: the masked dense pass has always kept it), the quad
    and feature kernels run dense passes only, the panel route is that of DP > 128, and the name of the dense plan is what
    lc_statistics_kernel_name tells bench.py."""
    name_of = ah.hooks().lc_statistics_kernel_name
    name_of.restype, name_of.argtypes = C.c_char_p, [C.c_int, C.c_int]
    seen = set()
    for DP, widths in WIDTHS.items():
        for DC in widths:
            for K in KS:
                for mode in ah.SS_MODES:
                    for NP in NPS:
                        p = ah.suffstat_plan(DP, DC, NP, K, mode)
                        at = (DP, DC, K, mode, NP, p)
                        assert p["chunk_rows"] > 0 and p["chunk_rows"] % ah.SS_BR == 0, at
                        assert p["nchunks"] * p["chunk_rows"] >= NP > (p["nchunks"] - 1) * p["chunk_rows"], at
                        assert p["KR"] == K + p["extra"] and p["extra"] >= 0, at
                        assert 0 <= p["klast0"] <= K and (p["extra"] > 0 or p["klast0"] == K), at
                        if p["extra"] > 0:
                            assert p["route"] == "per_cluster" and mode in ("dense", "masked_dense"), at
                        if p["route"] in ("quad", "feat"):
                            assert mode == "dense", at
                        assert (p["route"] == "wide") == (DP > 128), at
                        assert p["clusters_per_block"] in (4, 8, 16), at
                        if mode == "dense":
                            assert p["name"] == name_of(DC, K).decode(), at  # (D = DC has the active width DC)
                        else:
                            assert p["name"] == "suffstat_kernel", at
                        seen.add((p["route"], mode, p["extra"] > 0))
    # the grid reaches every route, and the row split in both dense modes
    assert {r for r, _, _ in seen} == set(ah.SS_ROUTES)
    assert ("per_cluster", "dense", True) in seen and ("per_cluster", "masked_dense", True) in seen


def _active_width(D, DP):
    if DP < 32 or DP > 128:
        return DP
    g, lo = (4, DP - 12) if DP <= 48 else (8, DP - 8)
    dc = -(-D // g) * g
    return DP if dc >= DP else max(dc, lo)


def _masked_sums(X, q, mask):
    K, D = q[0].shape[1], X[0].shape[1]
    N, s, S = np.zeros(K), np.zeros((K, D)), np.zeros((K, D, D))
    for j, (x, w) in enumerate(zip(X, q)):
        w = w * mask[j][None, :]
        N += w.sum(0)
        s += w.T @ x
        S += np.stack([(x * w[:, k, None]).T @ x for k in range(K)])
    return N, s, S


@pytest.mark.parametrize("D,K,N,route", [(33, 8, 1003, "quad"), (64, 32, 1003, "feat"), (23, 5, 70001, "quad")])
def test_zero_skipping_and_masked_dense_statistics_at_quad_and_feature_eligible_shapes(D, K, N, route):
    """At a shape whose dense pass runs the quad or the feature kernel, the zero-skipping pass (with and without a mask)
    and the dense pass with a mask staged as zeros (J = 3 groups, the mask removes under 30 % of the pairs: the dense grid
    is kept) run the per-cluster kernel on the eligible kernel's chunking: N_k, s_k, S_k against numpy to
    1e-12 of the largest entry, as test_quad_statistics_kernel_at_every_instance holds the dense pass; and where the plans of
    the two modes agree in chunks and records, zero-skipping equals the masked dense pass with a full mask bit for bit."""
    rng = np.random.default_rng(N + K)
    sizes = [N // 2, N // 3, N - N // 2 - N // 3]
    X = [rng.normal(size=(n, D)) * 2.0 + rng.normal(size=(1, D)) for n in sizes]
    q = [rng.dirichlet(np.ones(K) * 0.3, n) for n in sizes]
    for w in q:
        w[w < 0.02] = 0.0  # exact zeros, whole 4-row steps of them among the rows: what the skipping variant skips
        w[: w.shape[0] // 8 * 4, K - 1] = 0.0
    mask = np.array([[(k + j) % 5 != 0 for k in range(K)] for j in range(3)], dtype=np.uint8)
    off = sum(n * int((1 - mask[j]).sum()) for j, n in enumerate(sizes)) / float(N * K)
    assert 0.0 < off < 0.3
    full = np.ones_like(mask)
    DP = -(-D // 16) * 16
    DC, NP = _active_width(D, DP), sum(-(-n // 16) * 16 for n in sizes)
    plans = {m: ah.suffstat_plan(DP, DC, NP, K, m) for m in ("dense", "masked_dense", "zero_skip")}
    assert plans["dense"]["route"] == route and plans["masked_dense"]["route"] == plans["zero_skip"]["route"] == "per_cluster"
    with capi.Context(0) as ctx:
        ctx.set_data(X)
        ctx.set_qz(q)
        got = {"masked_dense": ctx.suffstat(mask), "full_mask": ctx.suffstat(full)}
        ctx.set_skip_zero(True)
        got["zero_skip"] = ctx.suffstat()
        got["zero_skip_masked"] = ctx.suffstat(mask)
    ref = {True: _masked_sums(X, q, mask), False: _masked_sums(X, q, full)}
    for tag, (Nk, xs, xxs, Njk) in got.items():
        rN, rs, rS = ref[tag in ("masked_dense", "zero_skip_masked")]
        eN = float(np.max(np.abs(Nk - rN) / rN))
        es = float(np.max(np.abs(xs - rs)) / np.max(np.abs(rs)))
        eS = float(np.max(np.abs(xxs - rS)) / np.max(np.abs(rS)))
        print(f"D={D} K={K} N={N} {tag}: eN {eN:.2e} es {es:.2e} eS {eS:.2e}")
        assert eN < 1e-12 and es < 1e-12 and eS < 1e-12, (tag, eN, es, eS)
    a, b = plans["zero_skip"], plans["masked_dense"]
    same = all(a[key] == b[key] for key in ("route", "nchunks", "chunk_rows", "extra", "klast0", "KR", "clusters_per_block"))
    assert same  # (eligible shapes: both modes take the eligible kernel's chunking without the row split)
    for u, v in zip(got["zero_skip"][:3], got["full_mask"][:3]):
        np.testing.assert_array_equal(u, v)


def test_estep_launch_without_an_instance_is_refused_and_has_no_grid():
    """DP = 64, K = 8 takes the four-row-group instance, which exists for the active widths 56 and 64 only: a launch with
    DC = 52 is refused by launch_estep (hipErrorInvalidValue, nothing is launched) and estep_grid names no grid for it (-1);
    so are a width between two layouts and, with three row groups (raw), the same DC.  A launch the plan accepts is not
    handed on by the hook (-1)."""
    for DP, DC, K, raw in ((64, 52, 8, False), (64, 52, 8, True), (80, 60, 8, False), (40, 40, 8, False), (32, 16, 4, False)):
        rc, grid = ah.estep_refusal(DP, DC, K, nrg=1000, raw=raw)
        assert rc == ah.HIP_ERROR_INVALID_VALUE and grid == -1, (DP, DC, K, raw, rc, grid)
    assert ah.estep_refusal(64, 56, 8, nrg=1000)[0] == -1 and ah.estep_refusal(64, 0, 8, nrg=1000)[0] == -1
