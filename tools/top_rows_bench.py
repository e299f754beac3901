"""Ranking timings: lc_ctx_top_rows against lc_colsums, a pass that reads exactly the same K columns.

N = 10M, D = 64, K = 32 generated on the device (bench.mixture + lc_ctx_synth); the model comes from a few fixed-K VBEM
iterations on those rows, then lc_model_predict with qZ kept: the qZ holds real responsibilities (not the two-valued ones
lc_ctx_synth starts with) and the context a logp per row.  One process times, alternating, medians of --reps, wall time
around each call with the stream synchronised:
  (a) colsums           lc_colsums
  (b) top_qz_m10/_m64   lc_ctx_top_rows over the K columns of qZ, largest, m = 10 and m = 64
  (c) bottom_logp_m64   lc_ctx_top_rows over logp, the 64 smallest
  (d) host_route        once: lc_ctx_get_qz_all + np.argpartition per column (m = 10) -- what a user does without (b)
and, on one column of --worst-rows rows set from the host, the insertion's worst case (every row beats all rows before it
in the scan of its wave, m = 64) against a random column of the same length.  One JSON line.

    python tools/top_rows_bench.py [--reps 7] [--rows 10000000] [--no-host-route]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/top_rows_bench.py --reps 3 (a run of its own)."""
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
from predict_bench import HBM_BPS, _device_name  # noqa: E402


def _median_ms(steps, ctx, reps):
    for f in steps.values():  # warm-up (allocations, code objects)
        f()
    ctx.synchronize()
    t = {k: [] for k in steps}
    for _ in range(reps):
        for k, f in steps.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            f()
            ctx.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return {k: round(float(np.median(v)), 4) for k, v in t.items()}


def run(N, reps, host_route, worst_rows):
    cfg = bench.CONFIGS["northstar"]
    D, K, seed = cfg["D"], cfg["K"], cfg["seed"]
    mu, L = bench.mixture(D, K, seed)
    out = {"N": N, "D": D, "K": K, "reps": reps}
    with capi.Context(0) as ctx:
        ctx.synth(N, D, K, mu, L, seed, 0, 0.9)
        _, _, m = ctx.vbem(capi.W_DIRICHLET, fixed_iters=3)
        m.predict_context(ctx, keep_qz=True)
        steps = {"colsums": ctx.colsums,
                 "top_qz_m10": lambda: ctx.top_rows(10),
                 "top_qz_m64": lambda: ctx.top_rows(64),
                 "bottom_logp_m64": lambda: ctx.top_rows(64, by="logp", largest=False)}
        out["ms"] = _median_ms(steps, ctx, reps)
        out["ratio_top_qz_m10_over_colsums"] = round(out["ms"]["top_qz_m10"] / out["ms"]["colsums"], 3)
        out["ratio_top_qz_m64_over_colsums"] = round(out["ms"]["top_qz_m64"] / out["ms"]["colsums"], 3)
        out["columns_hbm_floor_ms"] = round(N * K * 8 / HBM_BPS * 1e3, 4)
        top = ctx.top_rows(10)
        low = ctx.top_rows(64, by="logp", largest=False)
        out["check"] = {"counts": bool(np.all(top.count == 10) and low.count[0] == min(64, N)),
                        "sorted": bool(np.all(np.diff(top.score, axis=1) <= 0) and np.all(np.diff(low.score[0]) >= 0)),
                        "soft_responsibilities": int(np.count_nonzero((top.score > 0) & (top.score < 1)))}
        if host_route:
            ctx.synchronize()
            t0 = time.perf_counter()
            q = ctx.get_qz([N])[0]
            t1 = time.perf_counter()
            idx = np.argpartition(-q, 10, axis=0)[:10]
            t2 = time.perf_counter()
            out["host_route_ms"] = {"get_qz": round((t1 - t0) * 1e3, 1), "argpartition": round((t2 - t1) * 1e3, 1),
                                    "total": round((t2 - t0) * 1e3, 1)}
            out["host_route_over_top_qz_m10"] = round((t2 - t0) * 1e3 / out["ms"]["top_qz_m10"], 1)
            # the same rows, as sets (argpartition leaves its m unordered; ties are the device's to order)
            vals = np.sort(np.take_along_axis(q, idx, axis=0), axis=0)[::-1].T
            out["check"]["host_route_same_scores"] = bool(np.array_equal(vals, top.score))
            del q, idx
        m.close()
    if worst_rows:
        r = np.arange(worst_rows)
        e = 2 * (r % 512 // 128) + r % 2
        worst = (r // 512) * 512.0 + (7 - e) * 64 + (63 - r % 128 // 2)  # rises in the scan order of every wave
        rnd = np.random.default_rng(seed).standard_normal(worst_rows)
        with capi.Context(0) as ctx:
            ctx.set_data(np.zeros((worst_rows, 1)))
            res = {}
            for name, col in (("every_row_inserts", worst), ("random", rnd)):
                ctx.set_qz(col.reshape(-1, 1))
                res[name] = _median_ms({"top_m64": lambda: ctx.top_rows(64)}, ctx, reps)["top_m64"]
            out["worst_case"] = {"rows": worst_rows, "columns": 1, "m": 64, "ms": res}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--worst-rows", type=int, default=1 << 22)
    ap.add_argument("--no-host-route", action="store_true")
    a = ap.parse_args()
    res = run(a.rows, a.reps, not a.no_host_route, a.worst_rows)
    print(json.dumps({"tool": "top_rows_bench", "device": _device_name(), "results": res}))


if __name__ == "__main__":
    main()
