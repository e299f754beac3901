"""Prediction timings: lc_model_predict against the raw E-step it starts with, on device-resident data.

For every shape: the model comes from a few fixed-K VBEM iterations on other rows of the same synthetic stream
(bench.mixture + lc_ctx_synth; wide256 is drawn on the host, as bench.py does), the rows to score are generated on the
device, and one process times, alternating, (a) the raw E-step alone (lc_eloglike / lc_estep_diag raw with the model's
parameters), (b) predict without qZ, (c) predict with qZ.  Wall time around each call with the stream synchronised;
medians of --reps.  The E-step kernel of every call is also timed with the context's events, and what prediction costs
on top of its E-step is measured like for like INSIDE the same call: predict wall time minus the time of its own raw
E-step kernel (host packing, the prediction kernels and their synchronisations all count against prediction).
lc_eloglike's wall time is reported for reference only: it factorises every iW on the host on each call.  One JSON line.

    python tools/predict_bench.py [--configs northstar,d32,wide256,dgmm,bemm] [--reps 7]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/predict_bench.py --reps 3 (a run of its own)."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from libcluster_amd import capi  # noqa: E402

HBM_BPS = 6.0e12  # bytes / s (MI355X HBM3E, the figure DESIGN's rooflines use)
FAMILIES = {"GaussWish": capi.C_GAUSSWISH, "NormGamma": capi.C_NORMGAMMA, "ExpGamma": capi.C_EXPGAMMA}


def _data(ctx, N, D, K, mu, L, seed, row_offset):
    if D <= 128:
        ctx.synth(N, D, K, mu, L, seed, row_offset, 0.9)
        return
    rng = np.random.default_rng([seed, row_offset])
    z = rng.integers(0, K, N)
    X = np.empty((N, D))
    for k in range(K):
        idx = np.flatnonzero(z == k)
        X[idx] = mu[k] + rng.standard_normal((idx.size, D)) @ L[k].T
    q0 = np.full((N, K), 0.1 / (K - 1))
    q0[np.arange(N), z] = 0.9
    ctx.set_data(X)
    ctx.set_qz(q0)


def _raw_estep(ctx, m, K, D, ck):
    """the E-step pass prediction starts with: K raw columns with the model's parameters"""
    cl = [m.cluster(k) for k in range(K)]
    if ck == capi.C_GAUSSWISH:
        nu, beta, logdW = (np.array([c[f] for c in cl]) for f in ("nu", "beta", "logdW"))
        mean, iW = np.array([c["mean"] for c in cl]), np.array([c["iW"] for c in cl])
        return lambda: capi.check(capi.lib().lc_eloglike(ctx._h, K, capi.dptr(nu), capi.dptr(beta), capi.dptr(mean),
                                                         capi.dptr(iW), capi.dptr(logdW)))
    if ck == capi.C_NORMGAMMA:
        a = np.array([c["mean"] for c in cl])
        w2 = np.array([-0.5 * c["nu"] / c["L"] for c in cl])
        w1 = np.zeros((K, D))
    else:
        a, w2 = np.zeros((K, D)), np.zeros((K, D))
        w1 = np.array([-c["a"] * c["ib"] for c in cl])
    c0 = np.zeros(K)
    return lambda: ctx.estep_diag(a, w2, w1, c0, raw=True)


def run(name, reps):
    cfg = bench.CONFIGS[name]
    N, D, K, seed = cfg["N"], cfg["D"], cfg["K"], cfg["seed"]
    family = cfg.get("c", "GaussWish")
    ck = FAMILIES[family]
    mu, L = bench.mixture(D, K, seed, family)
    ntrain = 100_000 if D > 128 else 400_000
    with capi.Context(0) as tr, capi.Context(0) as ctx:
        _data(tr, ntrain, D, K, mu, L, seed, N)  # rows N .. N + ntrain of the stream: not the ones scored
        _, _, m = tr.vbem(capi.W_DIRICHLET, fixed_iters=3, ckind=ck)
        m.release_data()
        _data(ctx, N, D, K, mu, L, seed, 0)
        raw = _raw_estep(ctx, m, K, D, ck)
        steps = {"raw_estep": raw, "predict": lambda: m.predict_context(ctx),
                 "predict_qz": lambda: m.predict_context(ctx, keep_qz=True)}
        ctx.timing_enable(True)
        for f in steps.values():  # warm-up (allocations, code objects)
            f()
        ctx.synchronize()
        t = {k: [] for k in steps}
        te = {k: [] for k in steps}  # the raw E-step kernel inside each call (events on the context's stream)
        for _ in range(reps):
            for k, f in steps.items():
                ctx.synchronize()
                ctx.timing_reset()
                t0 = time.perf_counter()
                f()
                ctx.synchronize()
                t[k].append((time.perf_counter() - t0) * 1e3)
                te[k].append(ctx.timing_get()["estep_ms"])
        ctx.timing_enable(False)
        label, logZ, logp = ctx.get_predictions(0, 0, min(N, 4096))
        m.close()
    med = {k: float(np.median(v)) for k, v in t.items()}
    over = {k: float(np.median(np.array(t[k]) - np.array(te[k]))) for k in ("predict", "predict_qz")}
    # predict_rows_kernel moves N x K doubles in and label / logZ / logp out (logp of the separable families comes
    # from predict_diag_kernel, which reads X and does ~4 VALU per factor x K x D)
    bytes_rows = N * K * 8 + N * (4 + 8 + (8 if ck == capi.C_GAUSSWISH else 0))
    out = {"N": N, "D": D, "K": K, "family": family, "reps": reps,
           "raw_estep_kernel_ms": round(float(np.median(te["raw_estep"])), 4),
           "raw_estep_wall_ms": round(med["raw_estep"], 4),  # (Gauss-Wishart: host factorisation included)
           "predict_ms": round(med["predict"], 4), "predict_qz_ms": round(med["predict_qz"], 4),
           "predict_estep_kernel_ms": round(float(np.median(te["predict"])), 4),
           "predict_minus_own_estep_ms": round(over["predict"], 4),
           "predict_qz_minus_own_estep_ms": round(over["predict_qz"], 4),
           "rows_kernel_hbm_floor_ms": round(bytes_rows / HBM_BPS * 1e3, 4),
           "check": {"finite": bool(np.isfinite(logZ).all() and np.isfinite(logp).all()),
                     "jensen": bool(np.all(logZ <= logp + 1e-12 * np.maximum(1, np.abs(logp)))),
                     "labels_used": int(np.unique(label).size)}}
    if ck != capi.C_GAUSSWISH:
        out["diag_factor_updates"] = N * K * D
    return out


def _device_name(device=0):
    """the runtime's name of the device the contexts ran on (hipDeviceGetName)"""
    try:
        hip = C.CDLL("libamdhip64.so")
        buf = C.create_string_buffer(256)
        if hip.hipDeviceGetName(buf, C.c_int(256), C.c_int(device)) == 0:
            return buf.value.decode(errors="replace")
    except OSError:
        pass
    return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="northstar,d32,wide256,dgmm,bemm")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    res = {name: run(name, a.reps) for name in a.configs.split(",")}
    print(json.dumps({"tool": "predict_bench", "device": _device_name(), "results": res}))


if __name__ == "__main__":
    main()
