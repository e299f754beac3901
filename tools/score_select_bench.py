"""Order and threshold query timings: lc_ctx_score_quantiles, lc_ctx_score_counts and lc_ctx_rows_beyond
against lc_colsums, a pass that reads the K columns of qZ exactly once (the bytes yardstick).

N = 10M, D = 64, K = 32 generated on the device (bench.mixture + lc_ctx_synth); the model comes from a few fixed-K VBEM
iterations on those rows, then lc_model_predict with qZ kept: the qZ holds real responsibilities and the context a logp per
row.  One process times, alternating, medians of --reps, wall time around each call with the stream synchronised:
  (a) colsums               lc_colsums
  (b) quantiles_logp_p1/16  lc_ctx_score_quantiles on logp, 1 and 16 probs
  (c) quantiles_qz_p3       lc_ctx_score_quantiles on the K columns of qZ, 3 probs
  (d) counts_logp_t16       lc_ctx_score_counts on logp, 16 thresholds
  (e) beyond_logp_q001/q10  lc_ctx_rows_beyond on logp at its 0.1 % and its 10 % quantile (rows downloaded)
  (f) host_route            once: lc_ctx_get_predictions + np.partition / np.flatnonzero -- what a user does without (b), (e)
and, on one column of --worst-rows rows set from the host, the radix select's worst cases (all rows equal: one bin in every
pass; two values: two bins; values that differ in their lowest 8 bits: every pass but the last is one bin) against a random
column of the same length, 16 probs each.  The floor of a select is its 8 passes times the column bytes at the rate (a)
reaches in the same run.  One JSON line.

    python tools/score_select_bench.py [--reps 7] [--rows 10000000] [--no-host-route]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/score_select_bench.py --reps 3 (a run of its own)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench  # noqa: E402
from libcluster_amd import capi  # noqa: E402
from predict_bench import _device_name  # noqa: E402
from top_rows_bench import _median_ms  # noqa: E402

PASSES = 8  # 8-bit digits of a 64-bit key
P16 = [0.001, 0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99, 0.999, 1.0]


def run(N, reps, host_route, worst_rows):
    cfg = bench.CONFIGS["northstar"]
    D, K, seed = cfg["D"], cfg["K"], cfg["seed"]
    mu, L = bench.mixture(D, K, seed)
    out = {"N": N, "D": D, "K": K, "reps": reps, "passes": PASSES}
    with capi.Context(0) as ctx:
        ctx.synth(N, D, K, mu, L, seed, 0, 0.9)
        _, _, m = ctx.vbem(capi.W_DIRICHLET, fixed_iters=3)
        m.predict_context(ctx, keep_qz=True)
        q = ctx.score_quantiles([0.001, 0.1], by="logp")
        t001, t10 = float(q.value[0, 0]), float(q.value[0, 1])
        thr16 = [float(v) for v in ctx.score_quantiles(P16, by="logp").value[0]]
        limit = int(0.11 * N) + 1024
        steps = {"colsums": ctx.colsums,
                 "quantiles_logp_p1": lambda: ctx.score_quantiles([0.001], by="logp"),
                 "quantiles_logp_p16": lambda: ctx.score_quantiles(P16, by="logp"),
                 "quantiles_qz_p3": lambda: ctx.score_quantiles([0.1, 0.5, 0.9], by="qz"),
                 "counts_logp_t16": lambda: ctx.score_counts(thr16, by="logp"),
                 "beyond_logp_q001": lambda: ctx.rows_beyond(t001, by="logp", limit=limit),
                 "beyond_logp_q10": lambda: ctx.rows_beyond(t10, by="logp", limit=limit),
                 "beyond_logp_q10_count_only": lambda: ctx.rows_beyond(t10, by="logp", limit=0)}
        ms = out["ms"] = _median_ms(steps, ctx, reps)
        rate = N * K * 8 / (ms["colsums"] * 1e-3)  # bytes / s that (a) reaches over the K columns
        out["colsums_gbps"] = round(rate / 1e9, 1)
        out["floor_ms"] = {"quantiles_logp": round(PASSES * N * 8 / rate * 1e3, 4),
                           "quantiles_qz": round(PASSES * ms["colsums"], 4),
                           "counts_logp": round(N * 8 / rate * 1e3, 4),
                           "beyond_logp_two_reads": round(2 * N * 8 / rate * 1e3, 4)}
        out["ratio_quantiles_qz_p3_over_floor"] = round(ms["quantiles_qz_p3"] / out["floor_ms"]["quantiles_qz"], 3)
        out["ratio_quantiles_logp_p16_over_floor"] = round(ms["quantiles_logp_p16"] / out["floor_ms"]["quantiles_logp"], 3)
        q16 = ctx.score_quantiles(P16, by="logp")
        c16 = ctx.score_counts(thr16, by="logp")
        f001, f10 = ctx.rows_beyond(t001, by="logp", limit=limit), ctx.rows_beyond(t10, by="logp", limit=limit)
        qq = ctx.score_quantiles([0.1, 0.5, 0.9], by="qz")
        out["flagged"] = {"q001": f001.total, "q10": f10.total}
        out["check"] = {"counts": bool(q16.count[0] == N and np.all(qq.count == N)),
                        "sorted": bool(np.all(np.diff(q16.value[0]) >= 0) and np.all(np.diff(qq.value, axis=1) >= 0)),
                        "atmost_covers_rank": bool(np.all(c16.atmost[0] >= q16.rank[0] + 1)),
                        "flagged_equals_rank": bool(f001.total == c16.atmost[0, 0] and f10.total == c16.atmost[0, 3]),
                        "flagged_in_order": bool(np.all(np.diff(f10.row) > 0) and np.all(f10.score <= t10))}
        if host_route:
            n001 = q16.rank[0, 0]
            ctx.synchronize()
            t0 = time.perf_counter()
            logp = ctx.get_predictions(0, 0, N)[2]
            t1 = time.perf_counter()
            v = np.partition(logp, n001)[n001]
            t2 = time.perf_counter()
            idx = np.flatnonzero(logp <= t10)
            t3 = time.perf_counter()
            out["host_route_ms"] = {"get_predictions": round((t1 - t0) * 1e3, 1), "partition": round((t2 - t1) * 1e3, 1),
                                    "flatnonzero": round((t3 - t2) * 1e3, 1), "quantile_total": round((t2 - t0) * 1e3, 1),
                                    "flag_total": round((t1 - t0 + t3 - t2) * 1e3, 1)}
            out["host_quantile_over_quantiles_logp_p1"] = round((t2 - t0) * 1e3 / ms["quantiles_logp_p1"], 1)
            out["host_flag_over_beyond_logp_q10"] = round((t1 - t0 + t3 - t2) * 1e3 / ms["beyond_logp_q10"], 1)
            out["check"]["host_route_same_quantile"] = bool(v == q16.value[0, 0])
            out["check"]["host_route_same_rows"] = bool(np.array_equal(idx, f10.row))
            del logp, idx
        m.close()
    if worst_rows:
        rng = np.random.default_rng(seed)
        base = np.float64(1.5).view(np.uint64)
        cols = {"all_equal": np.full(worst_rows, 0.5),
                "two_values": np.where(rng.random(worst_rows) < 0.5, 0.25, 0.75),
                "low8": (base + rng.integers(0, 256, worst_rows).astype(np.uint64)).view(np.float64),
                "random": rng.standard_normal(worst_rows)}
        with capi.Context(0) as ctx:
            ctx.set_data(np.zeros((worst_rows, 1)))
            res, ok = {}, True
            for name, col in cols.items():
                ctx.set_qz(col.reshape(-1, 1))
                res[name] = _median_ms({"q16": lambda: ctx.score_quantiles(P16, by="qz")}, ctx, reps)["q16"]
                ok = ok and bool(np.array_equal(ctx.score_quantiles(P16, by="qz").value[0],
                                                np.quantile(col, P16, method="inverted_cdf")))
            ctx.synchronize()
            t0 = time.perf_counter()
            h = ctx.get_qz([worst_rows])[0][:, 0]
            np.quantile(h, P16, method="inverted_cdf")
            host = (time.perf_counter() - t0) * 1e3
            out["worst_case"] = {"rows": worst_rows, "columns": 1, "probs": 16, "ms": res, "host_route_ms": round(host, 1),
                                 "floor_ms": round(PASSES * worst_rows * 8 / rate * 1e3, 4), "same_as_numpy": ok}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--worst-rows", type=int, default=1 << 22)
    ap.add_argument("--no-host-route", action="store_true")
    a = ap.parse_args()
    res = run(a.rows, a.reps, not a.no_host_route, a.worst_rows)
    print(json.dumps({"tool": "score_select_bench", "device": _device_name(), "results": res}))


if __name__ == "__main__":
    main()
