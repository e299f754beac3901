"""Timings of the prediction of rows with holes: lc_model_predict_incomplete on device-resident rows of
which a share holds 1 ... 8 unknown values (NaN), against lc_model_predict(keep_qz = 0) on the same rows without holes.

For every shape: the model comes from a few fixed-K VBEM iterations on rows of the synthetic stream (bench.mixture +
lc_ctx_synth), the rows to score are synthesised on the device, brought to the host once, and uploaded again per run
with NaNs in the chosen share of the rows (a call completes the rows in place, so every run needs fresh ones).  Hole rows
get 1 ... 8 holes, uniformly, in columns start + i * stride (mod D) with a random start and a stride coprime to D.
Wall time around each call with the stream synchronised (host tables and uploads of the call included); the first call of
a process runs on a small context so that no timed call loads code objects.

Kernel times come from a run of their own per (shape, share): this tool starts itself under
`rocprofv3 --kernel-trace` (--child) and sums, per kernel, the dispatches of the one timed call -- from the last
holes_scan_kernel dispatch on -- and of the lc_model_predict that follows it.  One JSON line.

    python tools/incomplete_bench.py [--configs northstar,d32] [--shares 0,1,10,100] [--reps 2] [--no-kernels]
                                     [--variance] [--draws 1,5 [--only-draws-kernels]]

--variance: per shape and share also the whole call with variance (lc_model_predict_incomplete_var), timed
in turns with the mean-only call of the same run, and its kernels from a profiled run of its own.  The variance of the
first rows with holes (up to --check-rows) is held against numpy (tests/incomplete_var_ref.py, direct_var) relative to var
itself, and the time numpy took for them -- the host route: rows on the host, one factorisation per row and cluster --
is recorded beside, per row with holes.  Such a line is kept in profiles/incomplete_var_bench_line.json.

--draws M[,M...]: per shape and share also the whole call with M draws per row
(lc_model_predict_incomplete_draws), timed in turns with the mean-only call of the same run, and its kernels -- the draws
pass holes_draws_kernel beside the predict_holes_kernel it follows -- from a profiled run of its own; the draws pass also
in ns per row with holes per draw.  Such a line is kept in profiles/incomplete_draws_bench_line.json."""
import argparse
import csv
import json
import math
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "tests"))  # (--variance: the numpy reference of the tests)
import bench  # noqa: E402
from libcluster_amd import capi  # noqa: E402
from predict_bench import _data, _device_name  # noqa: E402

KERNELS = ("holes_scan_kernel", "holes_fill_kernel", "estep_wide_kernel", "estep_kernel", "predict_holes_kernel",
           "holes_draws_kernel", "predict_rows_kernel")


def _model(name):
    cfg = bench.CONFIGS[name]
    N, D, K, seed = cfg["N"], cfg["D"], cfg["K"], cfg["seed"]
    mu, L = bench.mixture(D, K, seed)
    with capi.Context(0) as tr:
        _data(tr, 400_000, D, K, mu, L, seed, N)  # rows N .. of the stream: not the ones scored
        _, _, m = tr.vbem(capi.W_DIRICHLET, fixed_iters=3)
        m.release_data()
    with capi.Context(0) as ctx:
        _data(ctx, N, D, K, mu, L, seed, 0)
        X = ctx.get_rows(0, 0, N)
    warm = X[:1000].copy()
    warm[::3, 1] = np.nan
    m.predict_incomplete(warm)  # (code objects, allocations)
    m.predict(warm[1::3])
    return m, X, (N, D, K)


def _punch(X, share, seed):
    """a copy of X with 1 ... 8 NaNs in about share of the rows -> (rows, number of hole rows, number of holes)"""
    N, D = X.shape
    rng = np.random.default_rng(seed)
    Xh = X.copy()
    rows = np.flatnonzero(rng.random(N) < share) if share < 1.0 else np.arange(N)
    top = min(capi.HOLES_MAX, D - 1)
    nb = rng.integers(1, top + 1, rows.size)
    start = rng.integers(0, D, rows.size)
    strides = np.array([s for s in range(1, D) if math.gcd(s, D) == 1] or [1])
    stride = strides[rng.integers(0, strides.size, rows.size)]
    for i in range(top):
        sel = nb > i
        Xh[rows[sel], (start[sel] + i * stride[sel]) % D] = np.nan
    return Xh, int(rows.size), int(nb.sum())


def _timed(ctx, f):
    ctx.synchronize()
    t0 = time.perf_counter()
    f()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _check_var(m, Xh, got, check_rows):
    """var of the first rows with holes against numpy, relative to var itself, and what numpy took per such row"""
    import incomplete_var_ref as vref

    J, K, D = m.dims()
    cls = []
    for k in range(K):
        p = m.cluster(k)
        cls.append((p["nu"], p["beta"], p["mean"], p["iW"]))
    Epi, rest = capi.weights_predictive(m.kinds()[0], m.weights(0)[1])
    head = Xh[: got.rows.shape[0]]
    pick = np.flatnonzero(np.isnan(head).any(axis=1))[:check_rows]
    if not pick.size:
        return {"rows": 0}
    t0 = time.perf_counter()
    var, Vn, _, _ = vref.direct_var(head[pick], cls, (float(D), 1.0, np.zeros(D), D * np.eye(D)), Epi, rest)
    host_ms = (time.perf_counter() - t0) * 1e3
    used = var > 0
    return {"rows": int(pick.size), "max_rel_to_var": float(np.max(np.abs(got.var[pick] - var)[used] / var[used])),
            "max_rel_to_Vn": float(np.max(np.abs(got.var[pick] - var) / Vn[:, None])),
            "zeros_ok": bool(not got.var[pick][~used].any() and not got.var[~np.isnan(head).any(axis=1)].any()),
            "host_route_us_per_hole_row": round(host_ms * 1e3 / pick.size, 2)}


def _wall(m, X, share, reps, seed, variance=False, check_rows=2048, draws=()):
    Xh, nrows, nholes = _punch(X, share, seed)
    t, tp, tv, td = [], [], [], {M: [] for M in draws}
    with capi.Context(0) as ctx:
        for _ in range(reps):
            ctx.set_data(Xh)
            t.append(_timed(ctx, lambda: m.predict_incomplete_context(ctx)))
            if variance:  # (in turns: both calls see the same state of the box)
                ctx.set_data(Xh)
                tv.append(_timed(ctx, lambda: m.predict_incomplete_context(ctx, variance=True)))
            for M in draws:
                ctx.set_data(Xh)
                td[M].append(_timed(ctx, lambda: m.predict_incomplete_context(ctx, draws=M, seed=seed)))
        dgot = ctx.get_completed(0, 0, min(X.shape[0], 4096), draws=True) if draws else None
        if draws:  # (the last call of the loop drew: a mean-only call for the checks below)
            ctx.set_data(Xh)
            m.predict_incomplete_context(ctx, variance=variance)
        got = ctx.get_completed(0, 0, min(X.shape[0], 4096), variance=variance)
        ctx.set_data(X)
        for _ in range(reps):
            tp.append(_timed(ctx, lambda: m.predict_context(ctx)))
    head = Xh[: got.rows.shape[0]]
    ok = bool(np.isfinite(got.rows).all() and np.isfinite(got.logp).all()
              and np.array_equal(got.count, np.isnan(head).sum(axis=1)) and np.array_equal(got.rows[~np.isnan(head)], head[~np.isnan(head)]))
    out = {"hole_rows": nrows, "holes": nholes, "incomplete_ms": round(float(np.median(t)), 3),
           "predict_ms": round(float(np.median(tp)), 3), "check_ok": ok}
    if variance:
        out["incomplete_runs_ms"] = [round(x, 3) for x in t]
        out["incomplete_var_runs_ms"] = [round(x, 3) for x in tv]
        out["incomplete_var_ms"] = round(float(np.median(tv)), 3)
        out["var_minus_mean_ms"] = round(out["incomplete_var_ms"] - out["incomplete_ms"], 3)
        out["var_check"] = _check_var(m, Xh, got, check_rows)
    if draws:
        out["incomplete_runs_ms"] = [round(x, 3) for x in t]
        out["incomplete_draws_runs_ms"] = {str(M): [round(x, 3) for x in td[M]] for M in draws}
        out["incomplete_draws_ms"] = {str(M): round(float(np.median(td[M])), 3) for M in draws}
        out["draws_minus_mean_ms"] = {str(M): round(float(np.median(td[M])) - out["incomplete_ms"], 3) for M in draws}
        cnt = got.count[:, None, None]
        out["draws_check_ok"] = bool(np.array_equal(dgot.rows, got.rows) and np.array_equal(dgot.logp, got.logp)
                                     and np.isfinite(dgot.draws).all() and not dgot.draws[np.broadcast_to(np.arange(capi.HOLES_MAX)[None, None, :] >= cnt, dgot.draws.shape)].any()
                                     and np.array_equal(dgot.label[:, 0] >= 0, got.count > 0))
    return out


def _short(name):
    for k in KERNELS:
        if k in name:
            return k
    return None


def _kernel_times(name, share, variance=False, draws=0):
    """this tool under rocprofv3 --kernel-trace: the kernels of one timed call and of the lc_model_predict after it"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt", "--", sys.executable,
               str(Path(__file__).resolve()), "--child", name, str(share)] + (["--variance"] if variance else []) + (
                   ["--draws", str(draws)] if draws else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        traces = sorted(Path(d).rglob("*kernel_trace.csv"))
        if r.returncode != 0 or not traces:
            return {"error": (r.stderr or r.stdout)[-400:]}
        rows = sorted(csv.DictReader(open(traces[-1])), key=lambda x: int(x["Start_Timestamp"]))
    print(f"incomplete_bench: profiled {name} at {share} %{' with variance' if variance else ''}"
          f"{f' with {draws} draws' if draws else ''}", file=sys.stderr, flush=True)
    names = [_short(x["Kernel_Name"]) for x in rows]
    scans = [i for i, n in enumerate(names) if n == "holes_scan_kernel"]
    if not scans:
        return {"error": "no holes_scan_kernel dispatch in the trace"}
    call, after, seen_end = {}, {}, False
    for x, n in list(zip(rows, names))[scans[-1]:]:
        if n is None:
            continue
        ms = (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e6
        dst = after if seen_end else call
        dst[n] = round(dst.get(n, 0.0) + ms, 4)
        seen_end = seen_end or n == ("holes_draws_kernel" if draws else "predict_holes_kernel")
    return {"incomplete": call, "predict": after}


def _child(name, share, variance=False, draws=0):
    m, X, _ = _model(name)
    Xh, _, _ = _punch(X, share / 100.0, 7)
    with capi.Context(0) as ctx:
        ctx.set_data(Xh)
        m.predict_incomplete_context(ctx, variance=variance, draws=draws or None, seed=7)
        ctx.set_data(X)
        m.predict_context(ctx)
        ctx.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="northstar,d32")
    ap.add_argument("--shares", default="0,1,10,100", help="per cent of the rows that hold holes")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("CONFIG", "SHARE"))
    ap.add_argument("--variance", action="store_true", help="also the call with variance, beside the mean-only call")
    ap.add_argument("--check-rows", type=int, default=2048, help="--variance: rows with holes held against numpy")
    ap.add_argument("--draws", default="", help="draws per row, a list: also the call with draws, beside the mean-only call")
    ap.add_argument("--only-draws-kernels", action="store_true", help="--draws: profile the calls with draws only")
    a = ap.parse_args()
    draws = [int(x) for x in a.draws.split(",") if x]
    if a.child:
        _child(a.child[0], float(a.child[1]), a.variance, draws[0] if draws else 0)
        return
    res, kernels, kernels_var, kernels_draws = {}, {}, {}, {}
    if not a.no_kernels:  # (first: the profiled runs are processes of their own, started before this one opens the device)
        for name in a.configs.split(","):
            if not (draws and a.only_draws_kernels):
                kernels[name] = {s: _kernel_times(name, float(s)) for s in a.shares.split(",")}
            if a.variance and not (draws and a.only_draws_kernels):
                kernels_var[name] = {s: _kernel_times(name, float(s), True) for s in a.shares.split(",")}
            if draws:
                kernels_draws[name] = {s: {str(M): _kernel_times(name, float(s), False, M) for M in draws} for s in a.shares.split(",")}
    for name in a.configs.split(","):
        m, X, (N, D, K) = _model(name)
        out = {"N": N, "D": D, "K": K, "reps": a.reps, "shares": {}}
        for s in a.shares.split(","):
            e = _wall(m, X, float(s) / 100.0, a.reps, 7, a.variance, a.check_rows, draws)
            if e["hole_rows"]:
                e["us_per_hole_row_over_predict"] = round((e["incomplete_ms"] - e["predict_ms"]) * 1e3 / e["hole_rows"], 4)
            out["shares"][s] = e
            print(f"incomplete_bench: timed {name} at {s} %", file=sys.stderr, flush=True)
            if name in kernels:
                e["kernels_ms"] = kernels[name][s]
            if name in kernels_var:
                e["kernels_var_ms"] = kernels_var[name][s]
            if name in kernels_draws:
                e["kernels_draws_ms"] = kernels_draws[name][s]
                if e["hole_rows"]:
                    e["draws_pass_ns_per_hole_row_per_draw"] = {
                        M: round(k["incomplete"].get("holes_draws_kernel", 0.0) * 1e6 / (e["hole_rows"] * int(M)), 2)
                        for M, k in kernels_draws[name][s].items() if "incomplete" in k}
        m.close()
        del X
        res[name] = out
    print(json.dumps({"tool": "incomplete_bench", "variance": a.variance, "draws": draws, "device": _device_name(), "results": res}))


if __name__ == "__main__":
    main()
