"""Timings of the leave-one-out conditionals: lc_model_predict_leave_one_out on device-resident complete rows,
with and without variance, against two yardsticks that are not the code under test:

  1. the raw E-step of the same call (the same matrix instruction on about half the tiles): the new kernel as a multiple of
     it, and as a fraction of the fp64 MFMA peak on the 2 N Kp DP^2 flops it issues;
  2. the route the library offered before: D calls of lc_model_predict_incomplete(variance) with one column NaN in every row,
     upload included (that route needs D copies of X).  Timed at --route2-rows rows (1M) on --route2-cols evenly spaced
     columns (all of them when D is not larger) and EXTRAPOLATED linearly in N and in the number of columns to the shape:
     the figure is marked as an extrapolation in the line.

For every shape: the model comes from a few fixed-K VBEM iterations on rows of the synthetic stream (bench.mixture +
lc_ctx_synth), the rows to score are synthesised on the device.  Wall time around each call with the stream synchronised
(host tables and uploads of the call included), medians over --reps; the first call of a process runs on a small context
so that no timed call loads code objects.  Kernel times come from a run of their own per shape: this tool starts itself
under `rocprofv3 --kernel-trace` (--child) and sums, per kernel, the dispatches of one call without and one with variance.
One JSON line (kept in profiles/leave_one_out_bench_line.json).

    python tools/leave_one_out_bench.py [--configs northstar,d32,wide256] [--reps 3] [--no-kernels] [--no-route2]"""
import argparse
import csv
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench  # noqa: E402
from libcluster_amd import capi  # noqa: E402
from predict_bench import _data, _device_name  # noqa: E402

KERNELS = ("holes_scan_kernel", "estep_wide_kernel", "estep_kernel", "predict_rows_kernel", "loo_rows_kernel", "loo_worst_kernel")
ROWS = {"wide256": 400_000}  # rows scored where the shape's own count does not fit beside three N x DP outputs comfortably


def _dp(D):
    return (D + 15) // 16 * 16 if D <= 128 else (D + 63) // 64 * 64


def _model(name):
    cfg = bench.CONFIGS[name]
    N, D, K, seed = ROWS.get(name, cfg["N"]), cfg["D"], cfg["K"], cfg["seed"]
    mu, L = bench.mixture(D, K, seed)
    with capi.Context(0) as tr:
        _data(tr, 400_000, D, K, mu, L, seed, cfg["N"])  # rows N .. of the stream: not the ones scored
        _, _, m = tr.vbem(capi.W_DIRICHLET, fixed_iters=3)
        m.release_data()
    warm = None
    with capi.Context(0) as ctx:
        _data(ctx, 1000, D, K, mu, L, seed, 0)
        warm = ctx.get_rows(0, 0, 1000)
    m.explain(warm, variance=True)  # (code objects, allocations)
    m.explain(warm)
    hol = warm.copy()
    hol[:, 1] = np.nan
    m.predict_incomplete(hol, variance=True)
    return m, (N, D, K, mu, L, seed)


def _timed(ctx, f):
    ctx.synchronize()
    t0 = time.perf_counter()
    f()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _wall(m, shape, reps):
    N, D, K, mu, L, seed = shape
    t, tv, tp = [], [], []
    with capi.Context(0) as ctx:
        _data(ctx, N, D, K, mu, L, seed, 0)
        for _ in range(reps):  # (in turns: the calls see the same state of the box)
            t.append(_timed(ctx, lambda: m.explain_context(ctx)))
            tv.append(_timed(ctx, lambda: m.explain_context(ctx, variance=True)))
            tp.append(_timed(ctx, lambda: m.predict_context(ctx)))
        m.explain_context(ctx, variance=True)
        n = min(N, 4096)
        got = ctx.get_leave_one_out(0, 0, n, variance=True)
        X = ctx.get_rows(0, 0, n)
        m.predict_context(ctx)
        logp = ctx.get_predictions(0, 0, n)[2]
    ok = bool(all(np.isfinite(getattr(got, f)).all() for f in ("logp", "cond_logp", "mean", "var")) and (got.var > 0).all()
              and np.array_equal(got.logp, logp) and np.array_equal(got.worst, np.argmin(got.cond_logp, axis=1)))
    return {"explain_ms": round(float(np.median(t)), 3), "explain_var_ms": round(float(np.median(tv)), 3),
            "predict_ms": round(float(np.median(tp)), 3), "explain_runs_ms": [round(x, 3) for x in t],
            "explain_var_runs_ms": [round(x, 3) for x in tv], "check_ok": ok}, X


def _route2(m, shape, rows, cols, reps):
    """D calls of predict_incomplete(variance=True), one NaN column each, uploads included: timed on `cols` columns of
    `rows` rows, extrapolated to all D columns and N rows"""
    N, D, K, mu, L, seed = shape
    n = min(rows, N)
    with capi.Context(0) as src:
        _data(src, n, D, K, mu, L, seed, 0)
        X = src.get_rows(0, 0, n)
    pick = np.unique(np.linspace(0, D - 1, min(cols, D)).astype(int))
    per = []
    with capi.Context(0) as ctx:
        for d in pick:
            Xh = X.copy()
            Xh[:, d] = np.nan
            ts = []
            for _ in range(reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.set_data(Xh)
                m.predict_incomplete_context(ctx, variance=True)
                ctx.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            per.append(float(np.median(ts)))
    per_col = float(np.median(per))
    return {"rows_timed": int(n), "columns_timed": int(pick.size), "ms_per_column_call": round(per_col, 3),
            "ms_all_columns_at_rows_timed": round(per_col * D, 1),
            "extrapolated_ms_at_N": round(per_col * D * N / n, 1),
            "extrapolated": "linear in N" + (" and in the number of columns" if pick.size < D else "")}


def _short(name):
    for k in KERNELS:
        if k in name:
            if k == "loo_rows_kernel":
                return "loo_rows_kernel<true>" if "ILb1" in name or "<true" in name else "loo_rows_kernel<false>"
            return k
    return None


def _kernel_times(name):
    """this tool under rocprofv3 --kernel-trace: the kernels of the last call without and the last call with variance"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt", "--", sys.executable,
               str(Path(__file__).resolve()), "--child", name]
        r = subprocess.run(cmd, capture_output=True, text=True)
        traces = sorted(Path(d).rglob("*kernel_trace.csv"))
        if r.returncode != 0 or not traces:
            return {"error": (r.stderr or r.stdout)[-400:]}
        rows = sorted(csv.DictReader(open(traces[-1])), key=lambda x: int(x["Start_Timestamp"]))
    print(f"leave_one_out_bench: profiled {name}", file=sys.stderr, flush=True)
    names = [_short(x["Kernel_Name"]) for x in rows]
    scans = [i for i, n in enumerate(names) if n == "holes_scan_kernel"]
    if len(scans) < 2:
        return {"error": "fewer than two holes_scan_kernel dispatches in the trace"}
    out = {}
    for key, lo, hi in (("explain", scans[-2], scans[-1]), ("explain_var", scans[-1], len(rows))):
        call = {}
        for x, n in list(zip(rows, names))[lo:hi]:
            if n is not None:
                call[n] = round(call.get(n, 0.0) + (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e6, 4)
        out[key] = call
    return out


def _child(name):
    m, (N, D, K, mu, L, seed) = _model(name)
    with capi.Context(0) as ctx:
        _data(ctx, N, D, K, mu, L, seed, 0)
        m.explain_context(ctx)
        m.explain_context(ctx, variance=True)
        ctx.synchronize()


def _rates(e, N, D, Kp):
    """the new kernel against the raw E-step of the same call and against the fp64 MFMA peak, on the flops it issues"""
    out = {}
    flops = 2.0 * N * Kp * _dp(D) ** 2
    for key in ("explain", "explain_var"):
        k = e.get("kernels_ms", {}).get(key, {})
        loo = k.get("loo_rows_kernel<true>" if key == "explain_var" else "loo_rows_kernel<false>")
        es = k.get("estep_kernel", 0.0) + k.get("estep_wide_kernel", 0.0)
        if loo and es:
            out[key] = {"loo_rows_over_raw_estep": round(loo / es, 2), "issued_gemm_tflops": round(flops / loo / 1e9, 2),
                        "share_of_fp64_mfma_peak": round(flops / loo / 1e9 / bench.FP64_PEAK_TFLOPS, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="northstar,d32,wide256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-route2", action="store_true")
    ap.add_argument("--route2-rows", type=int, default=1_000_000)
    ap.add_argument("--route2-cols", type=int, default=8)
    ap.add_argument("--child", metavar="CONFIG")
    a = ap.parse_args()
    if a.child:
        _child(a.child)
        return
    kernels = {}
    if not a.no_kernels:  # (first: the profiled runs are processes of their own, started before this one opens the device)
        kernels = {name: _kernel_times(name) for name in a.configs.split(",")}
    res = {}
    for name in a.configs.split(","):
        m, shape = _model(name)
        N, D, K = shape[:3]
        e, _ = _wall(m, shape, a.reps)
        e.update({"N": N, "D": D, "K": K, "Kp": m.dims()[1], "reps": a.reps})
        print(f"leave_one_out_bench: timed {name}", file=sys.stderr, flush=True)
        if name in kernels:
            e["kernels_ms"] = kernels[name]
            e["rates"] = _rates(e, N, D, e["Kp"])
        if not a.no_route2:
            e["route2_predict_incomplete_per_column"] = _route2(m, shape, a.route2_rows, a.route2_cols, max(1, a.reps - 1))
            e["route2_over_explain_var"] = round(e["route2_predict_incomplete_per_column"]["extrapolated_ms_at_N"] / e["explain_var_ms"], 1)
            print(f"leave_one_out_bench: route 2 of {name}", file=sys.stderr, flush=True)
        m.close()
        res[name] = e
    print(json.dumps({"tool": "leave_one_out_bench", "device": _device_name(), "results": res}))


if __name__ == "__main__":
    main()
