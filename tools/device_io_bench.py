"""Device-resident data in, row results out: what the device route costs against a plain copy, and what it
saves end to end.

For every shape (rows drawn on the device with torch from bench.mixture's components), one process measures
  (a) Context.set_data on a row-major and on a column-major CUDA tensor (lc_ctx_set_data_device: layout, one
      pack_rows_kernel / pack_cols_kernel launch, synchronisation) against hipMemcpyAsync device-to-device of the image's byte
      count, synchronised the same way;
  (b) lc_ctx_get_qz_rows_device into a row-major tensor (unpack_qz_kernel) against the same yardstick for its bytes;
  (c) Model.predict(X, qz=True), device tensor against the numpy route on the same rows (a host copy made beforehand);
  (d) learnVDP, device tensor against the numpy route.
Wall time around each call, the device idle before and after; medians of --reps (the end-to-end pairs alternate).
One JSON line, also written to --out.

    python tools/device_io_bench.py [--configs northstar,d32] [--reps 5] [--out profiles/device_io_bench_line.json]
Kernel times: rocprofv3 --kernel-trace --stats -- python tools/device_io_bench.py --reps 2 --no-learn (a run of its own)."""
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
import libcluster_amd as lc  # noqa: E402
from libcluster_amd import capi  # noqa: E402

HIP_MEMCPY_D2D = 3  # hipMemcpyDeviceToDevice


def _hip():
    """the HIP runtime this process already runs on (the copy torch loaded): a second copy would not see the device"""
    capi.lib()
    for line in Path("/proc/self/maps").read_text().splitlines():
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            return lib
    raise RuntimeError("no HIP runtime is loaded")


def _draw(torch, N, D, K, seed):
    """N rows of bench.mixture's K components, on the device"""
    mu, L = bench.mixture(D, K, seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randint(0, K, (N,), device="cuda", generator=g)
    X = torch.empty((N, D), dtype=torch.float64, device="cuda")
    mu_t, L_t = torch.from_numpy(mu).cuda(), torch.from_numpy(L).cuda()
    step = 1 << 20
    for a in range(0, N, step):
        zz = z[a:a + step]
        eps = torch.randn((zz.numel(), D), dtype=torch.float64, device="cuda", generator=g)
        X[a:a + step] = mu_t[zz] + torch.einsum("nij,nj->ni", L_t[zz], eps)
    torch.cuda.synchronize()
    return X


def _wall(torch, f, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        del r
    return float(np.median(out))


def _memcpy_ms(torch, hip, nbytes, reps):
    """hipMemcpyAsync device-to-device of nbytes on torch's current stream, then a synchronisation"""
    src = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda").normal_()
    dst = torch.empty_like(src)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        if hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, HIP_MEMCPY_D2D, stream) != 0:
            raise RuntimeError("hipMemcpyAsync failed")

    copy()
    return _wall(torch, copy, reps)


def run(name, reps, learn):
    import torch

    cfg = bench.CONFIGS[name]
    N, D, K, seed = cfg["N"], cfg["D"], cfg["K"], cfg["seed"]
    hip = _hip()
    Xr = _draw(torch, N, D, K, seed)
    DP = D if D % 16 == 0 else (D + 15) // 16 * 16
    NP = (N + 15) // 16 * 16
    out = {"N": N, "D": D, "K": K, "reps": reps, "image_bytes": NP * DP * 8, "qz_bytes": N * K * 8}
    stream = torch.cuda.current_stream().cuda_stream
    with capi.Context(0, stream) as ctx:
        Xc = Xr.t().contiguous().t()  # column-major
        ctx.set_data(Xr)  # warm-up (the image's block, code objects)
        out["pack_rowmajor_ms"] = round(_wall(torch, lambda: ctx.set_data(Xr), reps), 4)
        out["pack_colmajor_ms"] = round(_wall(torch, lambda: ctx.set_data(Xc), reps), 4)
        del Xc
        out["memcpy_image_ms"] = round(_memcpy_ms(torch, hip, NP * DP * 8, reps), 4)
        out["data_range"] = list(ctx.data_range())
        ctx.fill_qz(K, 1.0 / K)
        ctx.get_qz_rows_device(0, 0, N)
        out["unpack_rowmajor_ms"] = round(_wall(torch, lambda: ctx.get_qz_rows_device(0, 0, N), reps), 4)
        out["memcpy_qz_ms"] = round(_memcpy_ms(torch, hip, N * K * 8, reps), 4)
    for k, ref in (("pack_rowmajor", "memcpy_image_ms"), ("pack_colmajor", "memcpy_image_ms"), ("unpack_rowmajor", "memcpy_qz_ms")):
        out[k + "_over_memcpy"] = round(out[k + "_ms"] / out[ref], 3)
    if not learn:
        return out
    Xh = Xr.cpu().numpy()  # the numpy route's starting point: rows in host memory (not timed)
    # (d) model selection end to end, the two routes alternating; the first pair warms both up
    t = {"device": [], "numpy": []}
    model = None
    for i in range(reps + 1):
        for route, X in (("device", Xr), ("numpy", Xh)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = lc.learnVDP(X, return_model=True)
            torch.cuda.synchronize()
            if i:
                t[route].append((time.perf_counter() - t0) * 1e3)
            if route == "device" and model is None:
                model, out["learn_K"], out["learn_F"] = res[-1], len(res[3]), res[0]
            else:
                out["learn_same_F"] = bool(res[0] == out["learn_F"])
                res[-1].close()
            del res
    out["learnVDP_device_ms"] = round(float(np.median(t["device"])), 3)
    out["learnVDP_numpy_ms"] = round(float(np.median(t["numpy"])), 3)
    out["learnVDP_numpy_over_device"] = round(out["learnVDP_numpy_ms"] / out["learnVDP_device_ms"], 3)
    model.release_data()
    # (c) prediction with qZ end to end
    t = {"device": [], "numpy": []}
    for i in range(reps + 1):
        for route, X in (("device", Xr), ("numpy", Xh)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p = model.predict(X, qz=True)
            torch.cuda.synchronize()
            if i:
                t[route].append((time.perf_counter() - t0) * 1e3)
            if route == "device":
                lab = p.label[:4096].cpu().numpy()
            else:
                out["predict_same_labels"] = bool(np.array_equal(lab, p.label[:4096]))
            del p
    model.close()
    out["predict_qz_device_ms"] = round(float(np.median(t["device"])), 3)
    out["predict_qz_numpy_ms"] = round(float(np.median(t["numpy"])), 3)
    out["predict_qz_numpy_over_device"] = round(out["predict_qz_numpy_ms"] / out["predict_qz_device_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="northstar,d32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-learn", action="store_true", help="the kernels against the copy only (a), (b)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "device_io_bench_line.json"))
    a = ap.parse_args()
    import torch

    res = {name: run(name, a.reps, not a.no_learn) for name in a.configs.split(",")}
    line = json.dumps({"tool": "device_io_bench", "device": torch.cuda.get_device_name(0), "results": res})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
