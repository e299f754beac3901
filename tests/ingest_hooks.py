"""ctypes prototypes and numpy-in / numpy-out wrappers for the hooks of lc_kernels_ingest.hip in libcluster_hip_testhooks.so
(libcluster_amd/csrc/lc_testhooks.hip): lcx_test_pack_rows, lcx_test_unpack_qz and lcx_test_ctx_image.  A plain helper module
of tests/test_gpu_ingest_kernels.py and tests/test_gpu_device_io.py, in the manner of tests/aux_hooks.py; no fixtures, no
pytest hooks.  (The hooks carry the lcx_ prefix of the hooks that are bound by their own test files: tests/test_host.py
holds every lc_test_* symbol to the table of tests/aux_hooks.py.)

Every wrapper returns the hook's status first (0, -1 = refused by the host-side validation, or a HIP error code)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from aux_hooks import HOOKS_LIB

RG = 16  # lck::RG: a group's rows are padded to a multiple of this

_P, _I, _L = C.c_void_p, C.c_int, C.c_longlong
PROTOTYPES = {
    "lcx_test_pack_rows": [_P, _P, _I, _P, _I, _L, _L, _L, _P, _L, _P, _P, _P],
    "lcx_test_unpack_qz": [_P, _L, _I, _L, _L, _P, _L, _L, _L, _L],
    "lcx_test_ctx_image": [_P, _P, _L, _P, _P],
}

_lib = None


def hooks():
    global _lib
    if _lib is None:
        try:  # one HIP runtime per process: bind to the copy torch bundles, as libcluster_amd.capi.lib() does
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(str(HOOKS_LIB))
        for name, args in PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = C.c_int
        _lib = lib
    return _lib


def padded_dim(D):
    """lck::padded_dim_wide: the image's row length for D columns"""
    return (D + 15) // 16 * 16 if D <= 128 else (D + 63) // 64 * 64


def image_rows(Nj):
    """padded rows of an image of groups of Nj rows"""
    return sum((int(n) + RG - 1) // RG * RG for n in Nj)


def pack_rows(bufs, Nj, D, rs, cs, guard=64):
    """launch_pack_rows over the flat float64 buffers bufs[j], in which element (n, d) of group j sits at n * rs + d * cs.
    The destination is filled with NaN first, guards included.  -> (status, image [NP, DP], the two guards, min, n_nan, raw
    range words)"""
    J = len(bufs)
    bufs = [np.ascontiguousarray(b, dtype=np.float64).reshape(-1) for b in bufs]
    DP, NP = padded_dim(D), image_rows(Nj)
    dst = np.full(NP * DP + 2 * guard, np.nan)
    ptrs = (C.c_void_p * J)(*[b.ctypes.data if b.size else None for b in bufs])
    elems = np.array([b.size for b in bufs], dtype=np.int64)
    nj = np.array(Nj, dtype=np.int64)
    rng = np.zeros(2, dtype=np.uint64)
    lo, nn = C.c_double(), C.c_longlong()
    rc = hooks().lcx_test_pack_rows(C.cast(ptrs, _P), elems.ctypes.data, J, nj.ctypes.data, D, rs, cs, guard, dst.ctypes.data,
                                    dst.size, rng.ctypes.data, C.addressof(lo), C.addressof(nn))
    return rc, dst[guard:guard + NP * DP].reshape(NP, DP), (dst[:guard], dst[guard + NP * DP:]), lo.value, nn.value, rng


def unpack_qz(col, off, n, q_elems, rs, cs, guard=64, fill=-7.0):
    """launch_unpack_qz: rows [off, off + n) of col [K, ldq] into a destination of q_elems doubles (entry (r, k) at r * rs + k *
    cs) that was filled with `fill`, guards included.  -> (status, destination [q_elems], the two guards)"""
    col = np.ascontiguousarray(col, dtype=np.float64)
    K, ldq = col.shape
    dst = np.full(q_elems + 2 * guard, fill)
    rc = hooks().lcx_test_unpack_qz(col.ctypes.data, ldq, K, off, n, dst.ctypes.data, q_elems, guard, rs, cs)
    return rc, dst[guard:guard + q_elems], (dst[:guard], dst[guard + q_elems:])


def ctx_image(ctx):
    """The whole padded image of a libcluster_amd.capi.Context -> (status, image [NP, DP]).  The context may come from the
    shipped library: both libraries are built from one lc_ctx.hpp, in which LC_TEST_HOOKS adds member functions only, so
    the object has one layout, and the hook only reads it."""
    np_, dp = C.c_longlong(), C.c_int()
    rc = hooks().lcx_test_ctx_image(ctx._h, None, 0, C.addressof(np_), C.addressof(dp))
    out = np.full((np_.value, dp.value), np.nan)
    if rc == 0 and out.size:
        rc = hooks().lcx_test_ctx_image(ctx._h, out.ctypes.data, out.size, None, None)
    return rc, out
