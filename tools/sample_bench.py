"""Timings of the samplers, on device-resident data; one JSON line, also written to
profiles/sample_bench_line.json.

New rows: lc_model_sample at the north-star model (N = 10M, D = 64, K = 32) and at d32, against lc_ctx_synth of the same
shape -- the same bytes written and the same triangular product per row; the difference is the price of the gamma draw, the
inverse-CDF choice and the model's tables.  The model comes from a few fixed-K VBEM iterations on the synthetic stream.

Draws of the conditional: lc_model_predict_conditional_draws with m = 1 and 5 at 32 | 32 (north star) and 16 | 7 (d32),
alternating with lc_model_predict_conditional of the same call in one process.  draws_pass_ms is the whole call minus the
mean-only call of the same round (tables, upload, cond_draws_kernel and its synchronisation all count against it), set
against the HBM time of the bytes it writes, 8 N m Db (+ 4 N m of labels).  Wall time around each call with the stream
synchronised, medians of --reps.

    python tools/sample_bench.py [--configs northstar,d32] [--reps 5] [--out FILE]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/sample_bench.py --reps 3 (a run of its own)."""
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
from conditional_bench import _marginal_rows  # noqa: E402
from libcluster_amd import capi  # noqa: E402
from predict_bench import _data, _device_name  # noqa: E402

HBM_BPS = 6.0e12
SPLITS = {"northstar": (32, 32), "d32": (16, 7)}  # given = the first Da columns, target = the next Db
DRAWS = (1, 5)


def _median_ms(ctx, steps, reps):
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
    return {k: np.array(v) for k, v in t.items()}


def run(name, reps):
    cfg = bench.CONFIGS[name]
    N, D, K, seed = cfg["N"], cfg["D"], cfg["K"], cfg["seed"]
    Da, Db = SPLITS[name]
    given, target = list(range(Da)), list(range(Da, Da + Db))
    mu, L = bench.mixture(D, K, seed)
    out = {"N": N, "D": D, "K": K, "reps": reps}
    with capi.Context(0) as tr:
        _data(tr, 400_000, D, K, mu, L, seed, N)
        _, _, m = tr.vbem(capi.W_DIRICHLET, fixed_iters=3)
        m.release_data()
    DP = (D + 15) // 16 * 16
    with capi.Context(0) as ctx:
        t = _median_ms(ctx, {"synth": lambda: ctx.synth(N, D, K, mu, L, seed),
                             "sample": lambda: m.sample_context(ctx, [N], seed=seed)}, reps)
        rows = ctx.get_rows(0, 0, 4096)
        lab = ctx.get_sample_labels(0, 0, 4096)
    nbytes = 8.0 * N * DP + 4.0 * N
    out["sample"] = {
        "synth_ms": round(float(np.median(t["synth"])), 4), "sample_ms": round(float(np.median(t["sample"])), 4),
        "sample_over_synth": round(float(np.median(t["sample"]) / np.median(t["synth"])), 3),
        "bytes_written": nbytes, "hbm_floor_ms": round(nbytes / HBM_BPS * 1e3, 4),
        "sample_over_hbm_floor": round(float(np.median(t["sample"])) / (nbytes / HBM_BPS * 1e3), 2),
        "check": {"finite": bool(np.isfinite(rows).all()), "labels_in_range": bool(lab.min() >= 0 and lab.max() < K)}}
    with capi.Context(0) as ctx:
        _marginal_rows(ctx, N, K, mu, L, given, seed)
        steps = {"conditional": lambda: m.predict_conditional_context(ctx, given, target)}
        for nd in DRAWS:
            steps[f"draws{nd}"] = lambda nd=nd: m.predict_conditional_context(ctx, given, target, draws=nd, seed=seed)
        t = _median_ms(ctx, steps, reps)
        got = ctx.get_conditional(0, 0, 4096, Db, draws=True)
    cond = {"given": Da, "target": Db, "conditional_ms": round(float(np.median(t["conditional"])), 4)}
    for nd in DRAWS:
        extra = float(np.median(t[f"draws{nd}"] - t["conditional"]))
        nbytes = 8.0 * N * nd * Db + 4.0 * N * nd
        cond[f"m{nd}"] = {
            "call_ms": round(float(np.median(t[f"draws{nd}"])), 4), "draws_pass_ms": round(extra, 4),
            "call_over_conditional": round(float(np.median(t[f"draws{nd}"]) / np.median(t["conditional"])), 3),
            "bytes_written": nbytes, "hbm_floor_ms": round(nbytes / HBM_BPS * 1e3, 4),
            "draws_pass_over_hbm_floor": round(extra / (nbytes / HBM_BPS * 1e3), 1)}
    cond["check"] = {"finite": bool(np.isfinite(got.draws).all()), "labels_in_range": bool(got.label.min() >= 0 and got.label.max() < K)}
    out["conditional_draws"] = cond
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="northstar,d32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sample_bench_line.json"))
    a = ap.parse_args()
    res = {name: run(name, a.reps) for name in a.configs.split(",")}
    line = json.dumps({"tool": "sample_bench", "device": _device_name(), "results": res})
    print(line)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
