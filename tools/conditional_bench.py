"""Conditional prediction timings: lc_model_predict_conditional against the raw marginal E-step it starts
with, on device-resident data, and against the host route a user had before (download the rows, numpy per cluster).

For every shape: the model comes from a few fixed-K VBEM iterations on full-width rows of the synthetic stream
(bench.mixture + lc_ctx_synth; wide256 is drawn on the host, as bench.py does).  The rows to score hold the GIVEN columns
only and are synthesised from the marginal mixture: mu[:, given] and the Cholesky factor of Sigma_aa.  One process times,
alternating, (a) the raw marginal E-step alone (lc_eloglike with the marginal posteriors) and (b) the whole conditional
call; wall time around each call with the stream synchronised, medians of --reps.  The E-step kernel of every call is
timed with the context's events, so (b) minus the E-step kernel of the same call is what the conditional pass costs on top
(host tables, the upload, predict_cond_kernel and its synchronisation all count against it); the flop and byte rates
derived from that difference are therefore lower bounds of the kernel's.  At --host-rows rows the host route is timed
once: rows downloaded, then per cluster a triangular solve, the Student-t term and a GEMM in numpy.  One JSON line.

    python tools/conditional_bench.py [--configs northstar,d32,wide256] [--reps 5] [--host-rows 1000000] [--variance]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/conditional_bench.py --reps 3 --host-rows 0 (a run of its
own).

--variance adds, per shape, the whole call with the predictive variance (lc_model_predict_conditional_var)
as a third alternating step, and at --host-rows rows the host route extended by the variance in numpy, timed once.  Without
the flag the output is what it was."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import gammaln, logsumexp

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from libcluster_amd import capi  # noqa: E402
from predict_bench import _data, _device_name  # noqa: E402

FP64_MATRIX_FLOPS = 78.6e12  # the fp64 matrix roof DESIGN's rooflines use
HBM_BPS = 6.0e12
SPLITS = {"northstar": 32, "d32": 16, "wide256": 192}  # given = the first Da columns, target = the others


def _marginal_rows(ctx, N, K, mu, L, given, seed):
    """N rows of the given columns from the marginal mixture, on the device where the synthesiser takes the width"""
    Da = len(given)
    La = np.array([np.linalg.cholesky((L[k] @ L[k].T)[np.ix_(given, given)]) for k in range(K)])
    _data(ctx, N, Da, K, np.ascontiguousarray(mu[:, given]), La, seed, 0)


def _raw_marginal_estep(ctx, cl, given):
    K = len(cl)
    nu, beta = (np.array([c[f] for c in cl]) for f in ("nu", "beta"))
    mean = np.array([c["mean"][given] for c in cl])
    iW = np.array([c["iW"][np.ix_(given, given)] for c in cl])
    logdW = np.array([-np.linalg.slogdet(w)[1] for w in iW])
    return lambda: capi.check(capi.lib().lc_eloglike(ctx._h, K, capi.dptr(nu), capi.dptr(beta), capi.dptr(mean),
                                                     capi.dptr(iW), capi.dptr(logdW)))


def _host_route(Xa, cl, Epi, D, given, target, variance=False):
    """what a user did before: per cluster the marginal Student-t term and the linear expert in numpy (variance: and the
    conditional covariance's diagonal, then the mixture's variance centred on the mean)"""
    Da = len(given)
    T, M, H = [], [], []
    for k, c in enumerate(cl):
        nu, beta, m, iW = c["nu"], c["beta"], c["mean"], c["iW"]
        nup = nu + 1 - D
        Lc = np.linalg.cholesky(iW[np.ix_(given, given)])
        Y = solve_triangular(Lc, (Xa - m[given]).T, lower=True)
        d2 = nu * np.einsum("dn,dn->n", Y, Y)
        G = (gammaln((nup + Da) / 2) - gammaln(nup / 2) - 0.5 * Da * np.log(nup * np.pi)
             + 0.5 * (Da * np.log(nup * beta / (1 + beta)) - 2 * np.log(np.diag(Lc)).sum()))
        T.append(np.log(Epi[k]) + G - 0.5 * (nup + Da) * np.log1p(beta / ((1 + beta) * nu) * d2))
        Bk = solve_triangular(Lc.T, solve_triangular(Lc, iW[np.ix_(given, target)], lower=True), lower=False)
        M.append(m[target] + (Xa - m[given]) @ Bk)
        if variance:
            Sab = iW[np.ix_(given, target)]
            schur = np.diag(iW)[target] - np.einsum("ab,ab->b", Sab, Bk)
            g = (1 + beta) / (beta * (nup + Da - 2))
            H.append((g * (1 + beta / ((1 + beta) * nu) * d2), schur))
    T = np.stack(T, axis=1)
    logp = logsumexp(T, axis=1)
    mean = np.zeros_like(M[0])
    for k in range(len(cl)):
        mean += np.exp(T[:, k] - logp)[:, None] * M[k]
    if not variance:
        return mean, logp
    var = np.zeros_like(mean)
    for k in range(len(cl)):
        var += np.exp(T[:, k] - logp)[:, None] * ((M[k] - mean) ** 2 + H[k][0][:, None] * H[k][1][None, :])
    return mean, logp, var


def run(name, reps, host_rows, variance=False):
    cfg = bench.CONFIGS[name]
    N, D, K, seed = cfg["N"], cfg["D"], cfg["K"], cfg["seed"]
    Da = SPLITS[name]
    Db = D - Da
    given, target = list(range(Da)), list(range(Da, D))
    mu, L = bench.mixture(D, K, seed)
    ntrain = 100_000 if D > 128 else 400_000
    out = {"N": N, "D": D, "K": K, "given": Da, "target": Db, "reps": reps}
    with capi.Context(0) as tr:
        _data(tr, ntrain, D, K, mu, L, seed, N)
        _, _, m = tr.vbem(capi.W_DIRICHLET, fixed_iters=3)
        m.release_data()
    cl = [m.cluster(k) for k in range(K)]
    alpha = 1.0 + m.weights(0)[1]  # Dirichlet(1) prior + counts
    Epi = alpha / alpha.sum()
    with capi.Context(0) as ctx:
        _marginal_rows(ctx, N, K, mu, L, given, seed)
        steps = {"raw_estep": _raw_marginal_estep(ctx, cl, given),
                 "conditional": lambda: m.predict_conditional_context(ctx, given, target)}
        if variance:
            steps["conditional_var"] = lambda: m.predict_conditional_context(ctx, given, target, variance=True)
        ctx.timing_enable(True)
        for f in steps.values():  # warm-up (allocations, code objects)
            f()
        ctx.synchronize()
        t = {k: [] for k in steps}
        te = {k: [] for k in steps}
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
        got = ctx.get_conditional(0, 0, min(N, 4096), Db, variance)  # (of the last step: with the variance when asked for)
        ref = _host_route(ctx.get_rows(0, 0, min(N, 4096)), cl, Epi, D, given, target, variance)
    over = float(np.median(np.array(t["conditional"]) - np.array(te["conditional"])))
    estep_ms = float(np.median(te["conditional"]))
    flops = 2.0 * N * K * (Da + 1) * Db
    DPa = (Da + 15) // 16 * 16
    nbytes = 8.0 * N * (DPa + 2 * K + Db + 1)  # x, the K columns read and rewritten, mean and logp out
    estep_flops = 2.0 * N * K * Da * (Da + 1) / 2  # the triangular product of the whitener
    out.update({
        "raw_estep_kernel_ms": round(float(np.median(te["raw_estep"])), 4),
        "raw_estep_wall_ms": round(float(np.median(t["raw_estep"])), 4),  # (host factorisation included)
        "conditional_ms": round(float(np.median(t["conditional"])), 4),
        "conditional_estep_kernel_ms": round(estep_ms, 4),
        "conditional_minus_own_estep_ms": round(over, 4),
        "cond_pass_flops": flops, "cond_pass_bytes": nbytes,
        "cond_pass_tflops_lower_bound": round(flops / (over * 1e-3) / 1e12, 3),
        "cond_pass_fraction_of_fp64_matrix_roof": round(flops / (over * 1e-3) / FP64_MATRIX_FLOPS, 4),
        "cond_pass_gbytes_per_s": round(nbytes / (over * 1e-3) / 1e9, 1),
        "cond_pass_hbm_floor_ms": round(nbytes / HBM_BPS * 1e3, 4),
        "estep_tflops": round(estep_flops / (estep_ms * 1e-3) / 1e12, 3),
        "estep_fraction_of_fp64_matrix_roof": round(estep_flops / (estep_ms * 1e-3) / FP64_MATRIX_FLOPS, 4),
        "check": {"finite": bool(np.isfinite(got.mean).all() and np.isfinite(got.logp).all()),
                  "max_abs_mean_diff_vs_numpy": float(np.max(np.abs(got.mean - ref[0]))),
                  "max_rel_logp_diff_vs_numpy": float(np.max(np.abs(got.logp - ref[1]) / np.abs(ref[1])))}})
    if variance:
        tv, tc = np.array(t["conditional_var"]), np.array(t["conditional"])
        out["variance"] = {
            "conditional_var_ms": round(float(np.median(tv)), 4),
            # the same round's mean-only call subtracted: tables, upload, predict_cond_var_kernel and its synchronisation
            "var_pass_ms": round(float(np.median(tv - tc)), 4),
            "var_pass_over_cond_pass": round(float(np.median(tv - tc)) / over, 3),
            "var_pass_tflops_lower_bound": round(flops / (float(np.median(tv - tc)) * 1e-3) / 1e12, 3),
            "check": {"finite": bool(np.isfinite(got.var).all()),
                      "max_rel_var_diff_vs_numpy": float(np.max(np.abs(got.var - ref[2]) / ref[2]))}}
    if host_rows > 0:
        n1 = min(N, host_rows)
        with capi.Context(0) as c1:
            _marginal_rows(c1, n1, K, mu, L, given, seed)
            m.predict_conditional_context(c1, given, target)  # warm-up
            dev = []
            for _ in range(reps):
                c1.synchronize()
                t0 = time.perf_counter()
                m.predict_conditional_context(c1, given, target)
                c1.synchronize()
                dev.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            Xa = c1.get_rows(0, 0, n1)
            t1 = time.perf_counter()
            _host_route(Xa, cl, Epi, D, given, target)
            t2 = time.perf_counter()
            if variance:
                m.predict_conditional_context(c1, given, target, variance=True)  # warm-up
                devv = []
                for _ in range(reps):
                    c1.synchronize()
                    t3 = time.perf_counter()
                    m.predict_conditional_context(c1, given, target, variance=True)
                    c1.synchronize()
                    devv.append((time.perf_counter() - t3) * 1e3)
                t3 = time.perf_counter()
                _host_route(Xa, cl, Epi, D, given, target, variance=True)
                t4 = time.perf_counter()
        out["host_route"] = {"rows": n1, "device_call_ms": round(float(np.median(dev)), 4),
                             "download_ms": round((t1 - t0) * 1e3, 2), "numpy_ms": round((t2 - t1) * 1e3, 2),
                             "speedup": round((t2 - t0) * 1e3 / float(np.median(dev)), 1)}
        if variance:
            out["variance"]["host_route"] = {
                "rows": n1, "device_call_ms": round(float(np.median(devv)), 4), "download_ms": round((t1 - t0) * 1e3, 2),
                "numpy_ms": round((t4 - t3) * 1e3, 2),
                "speedup": round(((t1 - t0) + (t4 - t3)) * 1e3 / float(np.median(devv)), 1)}
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="northstar,d32,wide256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=1_000_000)
    ap.add_argument("--variance", action="store_true", help="also time the call with the predictive variance")
    a = ap.parse_args()
    res = {name: run(name, a.reps, a.host_rows, a.variance) for name in a.configs.split(",")}
    print(json.dumps({"tool": "conditional_bench", "device": _device_name(), "results": res}))


if __name__ == "__main__":
    main()
