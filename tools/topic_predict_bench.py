"""Timings of the inference for new documents with a learned SCM model on device-resident data.

Shape (DESIGN 5.1's two-level example): --docs 20000 documents x --rows 100 rows, D = 8, drawn from 7 document classes
over 10 Gaussian segments; the model is learned on --train documents of the same stream.  One process times,
alternating,
  fused       lc_tmodel_predict(tol = -1, max_sweeps = 8): one raw E-step + topic_infer_kernel
  host_loop   the same inference driven from the host with the entry points that were there before: per sweep lc_estep
              with the per-document constant table, lc_colsums, and vbeY in numpy (8 sweeps + the last vbeZ)
and, on the overlapping set-up (3 classes over 4 segments at scale 1.5, D = 3, 30 rows a document) at the same
document count,
  converged   lc_tmodel_predict(tol = 1e-5, max_sweeps = 50): every document stops on its own
  fixed       ... against tol = -1 at the largest sweep count any document needed (what a host-driven loop would run).
Wall time around each call, the stream synchronised; medians of --reps after --warmup calls.  One JSON line (also
written to --out).

    python tools/topic_predict_bench.py [--reps 7] [--out profiles/topic_predict_bench_line.json]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/topic_predict_bench.py --reps 3 --no-host-loop
(a run of its own)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import libcluster_amd as lc  # noqa: E402
from libcluster_amd import capi  # noqa: E402

D, CLASSES, SEGMENTS = 8, 7, 10


def documents(rng, mu, mix, docs, rows):
    """`docs` documents of `rows` rows: class t ~ U, segments ~ mix[t], x = mu[z] + N(0, I)"""
    t = rng.integers(0, mix.shape[0], docs)
    cdf = np.cumsum(mix, axis=1)
    u = rng.random((docs, rows))
    z = (u[:, :, None] > cdf[t][:, None, :]).sum(axis=2).clip(0, mu.shape[0] - 1)
    X = mu[z] + rng.standard_normal((docs, rows, mu.shape[1]))
    return [X[i] for i in range(docs)]


def learn(rng, mu, mix, train, rows):
    X = documents(rng, mu, mix, train, rows)
    maxT = mix.shape[0] + 3
    q = np.abs(rng.uniform(-1, 1, (train, maxT)))
    res = lc.learnSCM([X], trunc=maxT, qY0=[q / q.sum(axis=1, keepdims=True)], return_model=True)
    m = res[-1]
    m.release_data()
    return m


def tables(m):
    """a (T,), E (T, K), whiteners A (K, D, D), means (K, D), Eloglike constants (K,) from the model's accessors"""
    d = m.dims()
    a = m.weights(0, 0)[0]
    E = np.array([m.weights(1, t)[0] for t in range(d["T"])])
    cl = [m.cluster(0, k) for k in range(d["K"])]
    A = np.array([np.sqrt(c["nu"]) * np.linalg.inv(np.linalg.cholesky(c["iW"])) for c in cl])
    mean = np.array([c["mean"] for c in cl])
    from scipy.special import digamma

    cst = np.array([0.5 * (digamma((c["nu"] + 1 - np.arange(1, D + 1)) / 2).sum() + c["logdW"]
                           - D * (1 / c["beta"] + np.log(np.pi))) for c in cl])
    return a, E, A, mean, cst


def softmax(v):
    v = v - v.max(axis=1, keepdims=True)
    e = np.exp(v)
    return e / e.sum(axis=1, keepdims=True)


def host_loop(ctx, tab, docs, sweeps):
    a, E, A, mean, cst = tab
    qY = np.repeat(softmax(a[None, :]), docs, axis=0)
    for _ in range(sweeps):
        ctx.estep(A, mean, qY @ E + cst)
        like = ctx.colsums() @ E.T
        qY = softmax(a[None, :] + like)
    ctx.estep(A, mean, qY @ E + cst)
    return qY


def timed(ctx, steps, warmup, reps):
    for _ in range(warmup):
        for f in steps.values():
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
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in t.items()}


def run(a, scale, seed, converged):
    rng = np.random.default_rng(seed)
    dim, classes, segments, rows = (3, 3, 4, 30) if converged else (D, CLASSES, SEGMENTS, a.rows)
    mu = rng.normal(0, scale, (segments, dim))
    mix = rng.dirichlet(np.full(segments, 0.4), classes)
    m = learn(rng, mu, mix, a.train, rows)
    d = m.dims()
    X = documents(rng, mu, mix, a.docs, rows)
    out = {"docs": a.docs, "rows": rows, "D": dim, "T": d["T"], "K": d["K"], "segment_scale": scale}
    with capi.Context(0) as ctx:
        ctx.set_data(X)
        if converged:
            m.predict_context(ctx, max_sweeps=50, tol=1e-5)
            sw = ctx.get_doc_predictions(0, a.docs, d["T"])[4]
            top = int(sw.max())
            out["sweeps"] = {"min": int(sw.min()), "median": float(np.median(sw)), "mean": round(float(sw.mean()), 3),
                             "max": top, "histogram": np.bincount(sw).tolist()}
            steps = {"converged": lambda: m.predict_context(ctx, max_sweeps=50, tol=1e-5),
                     "fixed": lambda: m.predict_context(ctx, max_sweeps=top, tol=-1.0)}
            out["times"] = timed(ctx, steps, a.warmup, a.reps)
        else:
            tab = tables(m)
            steps = {"fused": lambda: m.predict_context(ctx, max_sweeps=8, tol=-1.0)}
            if not a.no_host_loop:
                steps["host_loop"] = lambda: host_loop(ctx, tab, a.docs, 8)
            out["times"] = timed(ctx, steps, a.warmup, a.reps)
            m.predict_context(ctx, max_sweeps=8, tol=-1.0)
            qY = ctx.get_doc_predictions(0, a.docs, d["T"])[0]
            out["check"] = {"qY_rows_sum_to_one": bool(np.allclose(qY.sum(axis=1), 1.0, rtol=1e-12))}
            if not a.no_host_loop:
                out["check"]["max_abs_qY_fused_minus_host_loop"] = float(np.max(np.abs(qY - host_loop(ctx, tab, a.docs, 8))))
                out["speedup"] = round(out["times"]["host_loop"]["median_ms"] / out["times"]["fused"]["median_ms"], 2)
            # cost model of DESIGN 4.12.1: exponentials and bytes of the sweeps
            n = a.docs * rows * d["K"]
            out["model"] = {"exponentials": 9 * n, "tile_bytes": 8 * n, "tile_bytes_if_reread_every_pass": 9 * 8 * n}
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--train", type=int, default=400)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--no-converged", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from predict_bench import _device_name

    res = {"tool": "topic_predict_bench", "device": _device_name(), "reps": a.reps, "warmup": a.warmup,
           "fixed_sweeps": run(a, 5.0, 1, False)}
    if not a.no_converged:
        res["early_exit"] = run(a, 1.5, 2, True)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
