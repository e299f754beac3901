"""ctypes prototypes and numpy-in / numpy-out wrappers for the lc_test_* entry points of libcluster_hip_testhooks.so
(libcluster_amd/csrc/lc_testhooks.hip): one launcher of lc_kernels_aux.hip, lc_kernels_predict.hip or lc_kernels_topic.hip per
call, on host arrays, and the two launch plans (tests/test_gpu_launch_plans.py).  A plain helper module of
tests/test_gpu_aux_kernels.py and tests/test_gpu_predict_kernels.py (and of the symbol test in tests/test_host.py); no
fixtures, no pytest hooks.  The launchers of lc_kernels_diag.hip (tests/test_gpu_diag_kernels.py) are at the end.

Every wrapper returns the hook's status first (0, -1 = refused by the host-side validation, or a HIP error code); arrays
the caller passes as destinations are uploaded as they are and overwritten with what the device left in them."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
HOOKS_LIB = ROOT / "libcluster_amd" / "lib" / "libcluster_hip_testhooks.so"
SHIPPED_LIB = ROOT / "libcluster_amd" / "lib" / "libcluster_hip.so"

# (the constants below restate csrc/lc_kernels.h, lc_device.hpp and lc_kernels_aux.hip; tests/test_host.py compares them
# with the sources, so a changed constant cannot silently move the boundaries the cases straddle)
QHASH_NONE = -(1 << 63)
QHASH_SEED = 0x243F6A8885A308D3
REDUCE_TMP_ELEMS = 512
SEL_ROWS = 1024
GCS_SLICES = 64
BOUND_MAX_COLS, BOUND_MAX_K = 8, 72
# (lc_kernels_predict.hip, lc_predict.hpp, lc_kernels_topic.hip, lc_kernels.h: tests/test_gpu_predict_kernels.py)
PR_COLS = 8
PC_CHUNK, PC_PANEL, PC_WAVE_ROWS, PC_THREADS = 32, 32, 64, 256
PRED_RENORM = 4
TI_KR = 16
TOPIC_E_LDS = 128
TOPIC_LDS_BYTES = 40 * 1024
HIP_ERROR_INVALID_VALUE = 1
# (lc_kernels.h: the statistics plan, tests/test_gpu_launch_plans.py)
SS_BR = 32
SS_ROUTES = ("per_cluster", "feat", "quad", "wide")            # SuffstatRoute, in the order of the enum
SS_MODES = ("dense", "masked_dense", "zero_skip", "work_list")  # SuffstatMode
# (lc_kernels.h, lc_kernels_fused.hip, lc_kernels_estep.hip: the hot path, tests/test_gpu_hot_kernels.py)
FUSED_ROWS, FUSED_KMAX, FUSED_CT_CAP = 256, 16, 1024
FUSED_YSHARE = 410  # per mille of a CU's tiles for its second block when the grid is two blocks per CU (launch_fused)
ES_LQ_LDS_CAP = 80 * 1024
WIDE_R, WIDE_WAVES, WIDE_CHUNK = 2, 4, 256 * 16 + 64


def estep_cfg_r(DP):
    return 4 if DP <= 48 else 3 if DP <= 96 else 2


def estep_cfg_waves(DP):
    return 4 if DP <= 96 else 8
_M64 = (1 << 64) - 1

_P, _I, _L, _D = C.c_void_p, C.c_int, C.c_longlong, C.c_double
PROTOTYPES = {
    "lc_test_rank_order_sum": [_P, _I, _L, _P],
    "lc_test_exp_nonpos": [_P, _L, _P],
    "lc_test_rcp_pos": [_P, _L, _P],
    "lc_test_log1p_nonneg": [_P, _L, _P],
    "lc_test_reduce_partials": [_P, _I, _L, _P, _I],
    "lc_test_reduce_records": [_P, _I, _L, _I, _P, _P, _P],
    "lc_test_group_colsum": [_P, _L, _I, _P, _I, _P, _I, _L],
    "lc_test_fill_qz": [_P, _L, _I, _I, _P, _L, _L, _D],
    "lc_test_select_rows": [_P, _L, _D, _P, _I, _P, _P, _L, _P, _P],
    "lc_test_gather_rows": [_P, _L, _I, _P, _L, _P, _P, _I, _P, _L],
    "lc_test_gather_rows_plain": [_P, _L, _I, _P, _L, _P, _L],
    "lc_test_gather_cols": [_P, _L, _L, _I, _P, _L, _P, _P, _I, _P, _L],
    "lc_test_gather_rowmajor": [_P, _L, _L, _I, _P, _L, _P, _P, _I, _P, _L],
    "lc_test_gather_rowmajor_cols": [_P, _L, _L, _P, _I, _P, _L, _P, _P, _I, _P, _L],
    "lc_test_scatter_cols": [_P, _L, _I, _P, _L, _P, _L],
    "lc_test_split_init": [_P, _I, _I, _L, _P, _L, _I, _P, _P, _L, _I, _P],
    "lc_test_aug_from_sub": [_P, _L, _L, _I, _I, _P, _L, _P, _P, _I, _P, _L, _P],
    "lc_test_transpose_qz": [_P, _L, _I, _L, _P, _L],
    "lc_test_softmax_cached": [_P, _I, _L, _P, _I, _L, _P, _P, _I, _I, _P, _L, _L, _P, _I, _L, _P, _L, _P, _P, _L, _P, _P, _I,
                               _P, _P, _P],
    "lc_test_qhash_verify": [_P, _L, _I, _L, _P, _P],
    "lc_test_qz_resync": [_P, _P, _L, _I, _I, _L, _P, _P],
    "lc_test_bound_select": [_I, _I, _L, _P, _P, _P, _P, _P, _P, _P, _D, _P, _P, _P],
    "lc_test_predict_rows": [_P, _I, _L, _I, _I, _L, _P, _L, _I, _P, _P, _P, _P, _I, _P, _P, _P],
    "lc_test_predict_diag": [_I, _P, _I, _L, _P, _L, _I, _I, _P, _P, _P, _P, _P, _P],
    "lc_test_predict_cond": [_P, _I, _I, _I, _I, _I, _I, _P, _L, _L, _P, _L, _I, _P, _P, _P, _P, _P, _P, _P],
    "lc_test_topic_plan": [_I, _I, _I, _P, _I, _P, _P],
    "lc_test_topic_infer": [_P, _L, _L, _I, _I, _I, _P, _P, _P, _P, _I, _D, _I, _I, _L, _P, _P, _P, _P, _P],
    "lc_test_suffstat_plan": [_I, _I, _L, _I, _I, _P, _P],
    "lc_test_estep_refusal": [_I, _I, _I, _I, _I, _L, _P],
    "lc_test_estep_plan": [_I, _I, _I, _I, _I, _L, _P],
    "lc_test_estep": [_P, _I, _I, _L, _P, _P, _I, _P, _L, _I, _I, _I, _P, _I, _L, _P, _L, _P, _L],
    "lc_test_fold_extra": [_P, _L, _L, _I, _I, _I],
    "lc_test_suffstat": [_P, _I, _I, _L, _P, _I, _L, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _L, _I, _P, _L, _P],
    "lc_test_fused_plan": [_I, _L, _I, _P],
    "lc_test_fused": [_P, _I, _L, _P, _P, _I, _P, _L, _I, _I, _I, _P, _I, _L, _P, _L, _P],
    "lc_test_estep_diag_plan": [_I, _I, _I, _L, _I, _I, _I, _I, _I, _P, _P],
    "lc_test_estep_diag": [_P, _I, _L, _P, _I, _P, _I, _P, _L, _I, _I, _P, _L, _P, _P, _P, _I, _L, _P, _L, _P, _L, _P, _P, _P],
    "lc_test_suffstat_diag_plan": [_I, _I, _I, _P, _P],
    "lc_test_suffstat_diag": [_P, _I, _L, _P, _I, _L, _P, _P, _I, _I, _L, _I, _P, _L, _I, _P, _L, _P],
    "lc_test_diag_pack": [_I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _L, _P],
    "lc_test_diag_weights": [_I, _I, _I],
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


def exported_symbols(path) -> set:
    """Names in the dynamic symbol table of a shared library (nm -D --defined-only)."""
    import subprocess

    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def _a(x, dtype):
    """A C-contiguous array of exactly this dtype (None stays None)."""
    return None if x is None else np.ascontiguousarray(x, dtype=dtype)


def _p(a):
    return None if a is None else a.ctypes.data


def _io(a, dtype):
    """Destination arrays are written in place: they must already be what the hook expects."""
    if a is None:
        return None
    assert isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.flags.writeable, (a.dtype, dtype)
    return a


f64, i64, i32, u8, u64 = np.float64, np.int64, np.int32, np.uint8, np.uint64


# ---- fingerprints (lc_device.hpp: qhash_step / qhash_finish), 64-bit wrap-around -------------------------------------------
def qhash(row) -> int:
    """Fingerprint of one row of responsibilities, as a signed 64-bit integer."""
    acc = QHASH_SEED
    bits = np.ascontiguousarray(row, dtype=f64).view(u64)
    for j, b in enumerate(bits.tolist()):
        if b == 0:
            continue
        t = ((acc ^ ((b + 0xD6E8FEB86659FD93 * (j + 1)) & _M64)) * 0x9E3779B97F4A7C15) & _M64
        acc = t ^ (t >> 32)
    h = acc - (1 << 64) if acc >= (1 << 63) else acc
    return 1 if h == QHASH_NONE else h


def qhash_rows(q_colmajor, rows=None) -> np.ndarray:
    """qhash of the rows of a column-major [K x ld] table (all of its ld rows, or the listed ones)."""
    q = np.asarray(q_colmajor)
    rows = range(q.shape[1]) if rows is None else rows
    return np.array([qhash(q[:, r]) for r in rows], dtype=i64)


# ---- layouts -------------------------------------------------------------------------------------------------------------
def padded_offsets(counts) -> np.ndarray:
    """Group offsets with every group padded to a multiple of 16 rows (Context::build_layout)."""
    c = (np.asarray(counts, dtype=i64) + 15) // 16 * 16
    return np.concatenate([[0], np.cumsum(c)]).astype(i64)


def rginfo_of(counts) -> np.ndarray:
    """(group << 5) | nvalid per 16-row group of the padded layout."""
    out = []
    for j, n in enumerate(np.asarray(counts).tolist()):
        full, rest = divmod(n, 16)
        out += [(j << 5) | 16] * full + ([(j << 5) | rest] if rest else [])
    return np.array(out, dtype=i32)


def valid_rows(counts) -> np.ndarray:
    """Boolean mask over the padded rows: True on a group's real rows."""
    goff = padded_offsets(counts)
    m = np.zeros(int(goff[-1]), dtype=bool)
    for j, n in enumerate(np.asarray(counts).tolist()):
        m[goff[j]:goff[j] + n] = True
    return m


def group_of_rows(counts) -> np.ndarray:
    goff = padded_offsets(counts)
    g = np.zeros(int(goff[-1]), dtype=i64)
    for j in range(len(counts)):
        g[goff[j]:goff[j + 1]] = j
    return g


# ---- wrappers ------------------------------------------------------------------------------------------------------------
def exp_nonpos(x):
    x = _a(x, f64)
    out = np.empty_like(x)
    return hooks().lc_test_exp_nonpos(_p(x), x.size, _p(out)), out


def rcp_pos(x):
    x = _a(x, f64)
    out = np.empty_like(x)
    return hooks().lc_test_rcp_pos(_p(x), x.size, _p(out)), out


def log1p_nonneg(x):
    x = _a(x, f64)
    out = np.empty_like(x)
    return hooks().lc_test_log1p_nonneg(_p(x), x.size, _p(out)), out


def reduce_partials(partial, use_tmp=False, sentinel=np.nan):
    p = _a(partial, f64)
    nparts, n = p.shape
    out = np.full(n, sentinel)
    return hooks().lc_test_reduce_partials(_p(p), nparts, n, _p(out), int(use_tmp)), out


def reduce_records(partial, kptr, krec, sentinel=np.nan):
    p, kptr, krec = _a(partial, f64), _a(kptr, i32), _a(krec, i32)
    nrec, n = p.shape
    K = kptr.size - 1
    out = np.full((K, n), sentinel)
    return hooks().lc_test_reduce_records(_p(p), nrec, n, K, _p(kptr), _p(krec), _p(out)), out


def group_colsum(qZ, goff, use_tmp=False, rows=0, sentinel=np.nan):
    q, goff = _a(qZ, f64), _a(goff, i64)
    K, ldq = q.shape
    J = goff.size - 1
    out = np.full((J, K), sentinel)
    return hooks().lc_test_group_colsum(_p(q), ldq, K, _p(goff), J, _p(out), int(use_tmp), rows), out


def fill_qz(qZ, K, nrg, value, rginfo=None, nrows=0):
    q = _io(qZ, f64)
    rg = _a(rginfo, i32)
    return hooks().lc_test_fill_qz(_p(q), q.shape[1], K, q.shape[0], _p(rg), nrows, nrg, value)


def select_rows(qcol, thresh, goff, sentinel=-7):
    """-> status, M, idx [NP] (entries >= M keep the sentinel), starts [J + 1], per-block counts"""
    q, goff = _a(qcol, f64), _a(goff, i64)
    NP, J = q.size, goff.size - 1
    counts = np.full((NP + SEL_ROWS - 1) // SEL_ROWS, sentinel, dtype=i32)
    idx = np.full(NP, sentinel, dtype=i64)
    starts = np.full(J + 1, sentinel, dtype=i64)
    M = C.c_longlong(sentinel)
    rc = hooks().lc_test_select_rows(_p(q), NP, thresh, _p(goff), J, _p(counts), _p(idx), NP, _p(starts), C.addressof(M))
    return rc, M.value, idx, starts, counts


def gather_rows(X, idx, starts, goff_sub, Xdst):
    X, idx, starts, goff_sub, Xdst = _a(X, f64), _a(idx, i64), _a(starts, i64), _a(goff_sub, i64), _io(Xdst, f64)
    return hooks().lc_test_gather_rows(_p(X), X.shape[0], X.shape[1], _p(idx), idx.size, _p(starts), _p(goff_sub), starts.size - 1,
                                       _p(Xdst), Xdst.shape[0])


def gather_rows_plain(X, idx, Xdst):
    X, idx, Xdst = _a(X, f64), _a(idx, i64), _io(Xdst, f64)
    return hooks().lc_test_gather_rows_plain(_p(X), X.shape[0], X.shape[1], _p(idx), idx.size, _p(Xdst), Xdst.shape[0])


def gather_cols(src, nsrc, idx, starts, goff_sub, dst):
    """src column-major [K x lds], rows < nsrc; dst column-major [K x ldd]"""
    src, idx, starts, goff_sub, dst = _a(src, f64), _a(idx, i64), _a(starts, i64), _a(goff_sub, i64), _io(dst, f64)
    return hooks().lc_test_gather_cols(_p(src), src.shape[1], nsrc, src.shape[0], _p(idx), idx.size, _p(starts), _p(goff_sub),
                                       starts.size - 1, _p(dst), dst.shape[1])


def gather_rowmajor(src, K, idx, starts, goff_sub, dst):
    """src row-major [nsrc x lds], its first K columns; dst column-major [K x ldd]"""
    src, idx, starts, goff_sub, dst = _a(src, f64), _a(idx, i64), _a(starts, i64), _a(goff_sub, i64), _io(dst, f64)
    return hooks().lc_test_gather_rowmajor(_p(src), src.shape[1], src.shape[0], K, _p(idx), idx.size, _p(starts), _p(goff_sub),
                                           starts.size - 1, _p(dst), dst.shape[1])


def gather_rowmajor_cols(src, cols, idx, starts, goff_sub, dst):
    src, cols, idx, starts, goff_sub, dst = (_a(src, f64), _a(cols, i32), _a(idx, i64), _a(starts, i64), _a(goff_sub, i64),
                                             _io(dst, f64))
    return hooks().lc_test_gather_rowmajor_cols(_p(src), src.shape[1], src.shape[0], _p(cols), cols.size, _p(idx), idx.size,
                                                _p(starts), _p(goff_sub), starts.size - 1, _p(dst), dst.shape[1])


def scatter_cols(src, idx, dest):
    """src [ncol x lds]; dest [ncol x ndst] in place: dest[t, idx[p]] = src[t, p]"""
    src, idx, dest = _a(src, f64), _a(idx, i64), _io(dest, f64)
    return hooks().lc_test_scatter_cols(_p(src), src.shape[1], src.shape[0], _p(dest), dest.shape[1], _p(idx), idx.size)


def split_init(X, D, mv, q, mode, rginfo=None, nrows=0, ngroups=1, thr=None, NP=None):
    X, mv, q, rg, thr = _a(X, f64), _a(mv, f64), _io(q, f64), _a(rginfo, i32), _a(thr, f64)
    NP = X.shape[0] if NP is None else NP
    assert mv.size == 2 * X.shape[1] and q.shape[0] == 2 and (thr is None or thr.size == ngroups)
    return hooks().lc_test_split_init(_p(X), X.shape[1], D, NP, _p(rg), nrows, ngroups, _p(mv), _p(q), q.shape[1], mode, _p(thr))


def aug_from_sub(q, NP, k, idx, starts, goff_sub, qsub1, qhash_arr=None):
    """q [(K + 1) x ldq] in place"""
    q, idx, starts, goff_sub, qsub1, qh = (_io(q, f64), _a(idx, i64), _a(starts, i64), _a(goff_sub, i64), _a(qsub1, f64),
                                           _io(qhash_arr, i64))
    assert qh is None or qh.size == NP
    return hooks().lc_test_aug_from_sub(_p(q), q.shape[1], NP, k, q.shape[0] - 1, _p(idx), idx.size, _p(starts), _p(goff_sub),
                                        starts.size - 1, _p(qsub1), qsub1.size, _p(qh))


def transpose_qz(qZ, NP, qT):
    q, qT = _a(qZ, f64), _io(qT, f64)
    return hooks().lc_test_transpose_qz(_p(q), q.shape[1], q.shape[0], NP, _p(qT), qT.size)


def softmax_cached(dcache, ctab, K, NP, qZ, fz_part, fresh=None, colmap=None, rginfo=None, nrows=0, ll_part=None, dq=None,
                   amax=None, qhash_arr=None, qhash_in=0, rmax=None, ramax=None, colmask=None):
    """dcache [Kc x ldc], fresh [nfresh x ldf], ctab [J x K]; qZ [Kq x ldq], fz_part [nblk], ll_part [nblk x K], dq [NP x ldd],
    amax / qhash / rmax / ramax [NP], colmask [2]: all destinations in place."""
    dc, ct, fr, cm, rg = _a(dcache, f64), _a(ctab, f64), _a(fresh, f64), _a(colmap, i32), _a(rginfo, i32)
    assert ct.ndim == 2 and ct.shape[1] == K and (cm is None or cm.size == K)
    q, fz, ll, dq, amax = _io(qZ, f64), _io(fz_part, f64), _io(ll_part, f64), _io(dq, f64), _io(amax, f64)
    qh, rmax, ramax, cmk = _io(qhash_arr, i64), _io(rmax, f64), _io(ramax, i32), _io(colmask, u64)
    assert ll is None or ll.shape == (fz.size, K)
    for v in (amax, qh, rmax, ramax):
        assert v is None or v.size == NP
    assert dq is None or dq.shape[0] == NP
    assert cmk is None or cmk.size == 2
    return hooks().lc_test_softmax_cached(_p(dc), dc.shape[0], dc.shape[1], _p(fr), 0 if fr is None else fr.shape[0],
                                          0 if fr is None else fr.shape[1], _p(cm), _p(ct), ct.shape[0], K, _p(rg), nrows, NP,
                                          _p(q), q.shape[0], q.shape[1], _p(fz), fz.size, _p(ll), _p(dq),
                                          0 if dq is None else dq.shape[1], _p(amax), _p(qh), qhash_in, _p(rmax), _p(ramax), _p(cmk))


def qhash_verify(qZ, K, NP, qhash_arr):
    """-> status, number of rows whose stored fingerprint does not describe them"""
    q, qh = _a(qZ, f64), _a(qhash_arr, i64)
    bad = C.c_ulonglong(0)
    rc = hooks().lc_test_qhash_verify(_p(q), q.shape[1], K, NP, _p(qh), C.addressof(bad))
    return rc, bad.value


def qz_resync(dst, src, K, NP, dhash, shash):
    dst, src, dhash, shash = _io(dst, f64), _a(src, f64), _io(dhash, i64), _a(shash, i64)
    assert src.shape[1] == dst.shape[1] and src.shape[0] == K
    return hooks().lc_test_qz_resync(_p(dst), _p(src), dst.shape[1], K, dst.shape[0], NP, _p(dhash), _p(shash))


def bound_select(K, ref, dest, sigma, bnorm, cnew, rmax, ramax, T, usable, dcj, need):
    """ref / dest [ncol x NP] (dest, need in place); usable, dcj [K]"""
    ref, dest, need = _a(ref, f64), _io(dest, f64), _io(need, f64)
    sigma, bnorm, cnew, rmax, ramax = _a(sigma, f64), _a(bnorm, f64), _a(cnew, f64), _a(rmax, f64), _a(ramax, i32)
    usable, dcj = _a(usable, u8), _a(dcj, f64)
    ncol, NP = ref.shape
    assert dest.shape == ref.shape and sigma.size == bnorm.size == cnew.size == ncol and usable.size == dcj.size == K
    assert rmax.size == ramax.size == need.size == NP
    return hooks().lc_test_bound_select(ncol, K, NP, _p(ref), _p(dest), _p(sigma), _p(bnorm), _p(cnew), _p(rmax), _p(ramax), T,
                                        _p(usable), _p(dcj), _p(need))


# ---- prediction and document inference -----------------------------------------------------------------------------------
def _rows(rginfo, nrows, nrg, tab):
    """-> rginfo array or None, nrows, J of a prediction launch whose per-group table is `tab` [J x *]"""
    rg = _a(rginfo, i32)
    assert tab.ndim == 2 and (rg is None or rg.size == nrg) and (rg is not None or tab.shape[0] == 1)
    return rg, int(nrows), tab.shape[0]


def predict_rows(col, K, Kp, nrg, ctab, ptab, pscale, pexp, keep_q, label, logZ, logp, rginfo=None, nrows=0):
    """col [ncols x ldq] in place; ctab [J x K]; ptab [J x Kp], pscale / pexp [Kp] (None when Kp = 0); label (int32), logZ,
    logp [nrg * 16] in place"""
    col, label, logZ, logp = _io(col, f64), _io(label, i32), _io(logZ, f64), _io(logp, f64)
    ct, pt, ps, pe = _a(ctab, f64), _a(ptab, f64), _a(pscale, f64), _a(pexp, f64)
    rg, nrows, J = _rows(rginfo, nrows, nrg, ct)
    assert ct.shape == (J, K) and label.size == logZ.size == logp.size == nrg * 16
    assert Kp == 0 or (pt.shape == (J, Kp) and ps.size == pe.size == Kp)
    return hooks().lc_test_predict_rows(_p(col), col.shape[0], col.shape[1], K, Kp, nrg, _p(rg), nrows, J, _p(ct), _p(pt), _p(ps),
                                        _p(pe), int(keep_q), _p(label), _p(logZ), _p(logp))


def predict_diag(mode, X, a, w, ptab, pexp, logp, flag, rginfo=None, nrows=0):
    """X [nrg * 16 x DP]; a / w [Kp x DP]; ptab [J x Kp]; logp [nrg * 16] and flag (int32 [1]) in place"""
    X, a, w, pt, pe, logp, flag = _a(X, f64), _a(a, f64), _a(w, f64), _a(ptab, f64), _a(pexp, f64), _io(logp, f64), _io(flag, i32)
    NP, DP = X.shape
    Kp = pe.size
    rg, nrows, J = _rows(rginfo, nrows, NP // 16, pt)
    assert NP % 16 == 0 and a.shape == w.shape == (Kp, DP) and pt.shape == (J, Kp) and logp.size == NP and flag.size == 1
    return hooks().lc_test_predict_diag(mode, _p(X), DP, NP // 16, _p(rg), nrows, J, Kp, _p(a), _p(w), _p(pt), _p(pe), _p(logp),
                                        _p(flag))


def predict_cond(X, Da, Dae, Db, Dbp, col, ttab, pscale, pexp, mext, T, mean, logp, rginfo=None, nrows=0, check_shapes=True, Kp=None):
    """X [nrg * 16 x DP]; col [Kp x ldq], mean [nrg * 16 x Db], logp [nrg * 16] in place; ttab [J x Kp]; mext [Kp x Dae];
    T [Kp x Dae x Dbp].  check_shapes=False: the widths (and Kp, when given) go to the hook as they are (the launcher's refusals)."""
    X, col, mean, logp = _a(X, f64), _io(col, f64), _io(mean, f64), _io(logp, f64)
    tt, ps, pe, mext, T = _a(ttab, f64), _a(pscale, f64), _a(pexp, f64), _a(mext, f64), _a(T, f64)
    NP, DP = X.shape
    Kp = ps.size if Kp is None else Kp
    rg, nrows, J = _rows(rginfo, nrows, NP // 16, tt)
    if check_shapes:
        assert NP % 16 == 0 and col.shape[0] == Kp and tt.shape == (J, Kp) and pe.size == Kp and mext.shape == (Kp, Dae)
        assert T.shape == (Kp, Dae, Dbp) and mean.shape == (NP, Db) and logp.size == NP
    return hooks().lc_test_predict_cond(_p(X), DP, Da, Dae, Db, Dbp, Kp, _p(col), col.shape[1], NP // 16, _p(rg), nrows, J, _p(tt),
                                        _p(ps), _p(pe), _p(mext), _p(T), _p(mean), _p(logp))


def topic_plan(K, T, threads, nrows):
    """-> bytes of dynamic LDS (0: does not fit, -1: refused), tile_cap, e_lds"""
    nr = _a(nrows, i64)
    cap, el = C.c_longlong(-7), C.c_int(-7)
    rc = hooks().lc_test_topic_plan(K, T, threads, _p(nr), nr.size, C.addressof(cap), C.addressof(el))
    return rc, cap.value, el.value


def topic_infer(col, NP, K, T, goff, nrows, a, E, max_sweeps, tol, keep_q, threads, label, logZ, qY, F, dint, lds_request=0,
                check_shapes=True):
    """col [K x ldq] in place (its shape is not looked at when check_shapes is False: the launcher's refusals); goff / nrows
    [docs]; a [docs x T]; E [T x K]; label (int32) / logZ [NP], qY [docs x T], F / dint (int32) [docs x 2] in place"""
    col, label, logZ, qY, F, dint = _io(col, f64), _io(label, i32), _io(logZ, f64), _io(qY, f64), _io(F, f64), _io(dint, i32)
    goff, nrows, a, E = _a(goff, i64), _a(nrows, i64), _a(a, f64), _a(E, f64)
    docs = goff.size
    if check_shapes:
        assert col.shape[0] == K and nrows.size == docs and a.shape == (docs, T) and E.shape == (T, K)
        assert label.size == logZ.size == NP and qY.shape == (docs, T) and F.shape == (docs, 2) and dint.shape == (docs, 2)
    return hooks().lc_test_topic_infer(_p(col), col.shape[1], NP, K, T, docs, _p(goff), _p(nrows), _p(a), _p(E), max_sweeps, tol,
                                       int(keep_q), threads, lds_request, _p(label), _p(logZ), _p(qY), _p(F), _p(dint))


def suffstat_plan(DP, DC, NP, K, mode):
    """suffstat_plan(DP, DC, NP, K, mode) as a dict: route and mode by name (SS_ROUTES, SS_MODES), nchunks, chunk_rows, extra,
    klast0, KR, clusters_per_block, name"""
    out = np.full(7, -7, dtype=i64)
    name = C.create_string_buffer(32)
    rc = hooks().lc_test_suffstat_plan(DP, DC, NP, K, SS_MODES.index(mode), _p(out), C.addressof(name))
    assert rc == 0, rc
    keys = ("route", "nchunks", "chunk_rows", "extra", "klast0", "KR", "clusters_per_block")
    d = dict(zip(keys, (int(v) for v in out)), name=name.value.decode(), mode=mode)
    d["route"] = SS_ROUTES[d["route"]]
    return d


def estep_refusal(DP, DC, K, nrg, raw=False, sparse=False):
    """-> launch_estep's return value for a launch without buffers that estep_plan refuses (-1: the plan accepts it, nothing
    was handed on) and estep_grid of that launch"""
    grid = C.c_longlong(-7)
    rc = hooks().lc_test_estep_refusal(DP, DC, K, int(raw), int(sparse), nrg, C.addressof(grid))
    return rc, grid.value


# ---- the hot path: E-step, statistics pass, fused pass (tests/test_gpu_hot_kernels.py) ----------------------------------------
def estep_plan(DP, DC, K, nrg, raw=False, sparse=False):
    """estep_plan of a launch as a dict: ok, rows_per_block, grid, four_groups, DC, lq_lds, lds_bytes, pstride"""
    out = np.full(8, -7, dtype=i64)
    rc = hooks().lc_test_estep_plan(DP, DC, K, int(raw), int(sparse), nrg, _p(out))
    assert rc == 0, rc
    return dict(zip(("ok", "rows_per_block", "grid", "four_groups", "DC", "lq_lds", "lds_bytes", "pstride"), (int(v) for v in out)))


def estep(X, DC, params, ctab, K, qZ, fz_part, ll_part=None, rginfo=None, nrows=0, raw=False, sparse=False):
    """X [nrg * 16 x DP]; params [K x pstride]; ctab [J x K]; qZ [Kbuf x ldq], fz_part, ll_part (or None) in place"""
    X, pr, ct, rg = _a(X, f64), _a(params, f64), _a(ctab, f64), _a(rginfo, i32)
    q, fz, ll = _io(qZ, f64), _io(fz_part, f64), _io(ll_part, f64)
    NP, DP = X.shape
    assert NP % 16 == 0 and ct.ndim == 2 and ct.shape[1] == K and pr.ndim == 2 and pr.shape[0] == K
    assert rg is None or rg.size == NP // 16
    return hooks().lc_test_estep(_p(X), DP, DC, NP // 16, _p(pr), _p(ct), ct.shape[0], _p(rg), int(nrows), K, int(raw), int(sparse),
                                 _p(q), q.shape[0], q.shape[1], _p(fz), fz.size, _p(ll), 0 if ll is None else ll.size)


def fold_extra(rec, SS, K, klast0, extra):
    """rec (flat, in place): launch_fold_extra alone"""
    rec = _io(rec, f64)
    return hooks().lc_test_fold_extra(_p(rec), rec.size, SS, K, klast0, extra)


def suffstat(X, DC, qZ, K, mode, partial, rginfo=None, smask=None, items=None, klist=None, nrec=0, skip_listed=False,
             folded=None):
    """One statistics pass.  X [NP x DP]; qZ [K x ldq]; partial (flat) and folded (flat, or None: no fold) in place; items: a
    list of (r0, r1, kofs, kcnt, rec0) for mode "work_list".  -> status, the plan as suffstat_plan() returns it (without name)"""
    X, q, rg, sm = _a(X, f64), _a(qZ, f64), _a(rginfo, i32), _a(smask, u8)
    part, fo = _io(partial, f64), _io(folded, f64)
    NP, DP = X.shape
    assert q.shape[0] == K and (sm is None or (sm.ndim == 2 and sm.shape[1] == K)) and (rg is None or rg.size == NP // 16)
    it = [None] * 5
    kl = _a(klist, i32)
    if items is not None:
        cols = list(zip(*items))
        it = [_a(cols[0], i64), _a(cols[1], i64), _a(cols[2], i32), _a(cols[3], i32), _a(cols[4], i64)]
    out = np.full(7, -7, dtype=i64)
    rc = hooks().lc_test_suffstat(_p(X), DP, DC, NP, _p(q), K, q.shape[1], SS_MODES.index(mode), _p(rg), _p(sm),
                                  0 if sm is None else sm.shape[0], 0 if items is None else len(items), _p(it[0]), _p(it[1]),
                                  _p(it[2]), _p(it[3]), _p(it[4]), _p(kl), 0 if kl is None else kl.size, int(nrec),
                                  int(skip_listed), _p(part), part.size, int(fo is not None), _p(fo), 0 if fo is None else fo.size,
                                  _p(out))
    keys = ("route", "nchunks", "chunk_rows", "extra", "klast0", "KR", "clusters_per_block")
    d = dict(zip(keys, (int(v) for v in out)), mode=mode)
    d["route"] = SS_ROUTES[d["route"]] if 0 <= d["route"] < 4 else None
    return rc, d


def fused_plan(nrg, K, DP=16):
    """-> dict: eligible, grid (fused_plan), cus, record (fused_record)"""
    out = np.full(4, -7, dtype=i64)
    rc = hooks().lc_test_fused_plan(DP, nrg, K, _p(out))
    assert rc == 0, rc
    return dict(zip(("eligible", "grid", "cus", "record"), (int(v) for v in out)))


def fused(X, D, params, ctab, K, qZ, partial, want_ll=False, grid=0, rginfo=None, nrows=0):
    """X [nrg * 16 x 16]; qZ [Kbuf x ldq] and partial (flat) in place -> status, blocks launched"""
    X, pr, ct, rg = _a(X, f64), _a(params, f64), _a(ctab, f64), _a(rginfo, i32)
    q, part = _io(qZ, f64), _io(partial, f64)
    NP, DP = X.shape
    assert DP == 16 and NP % 16 == 0 and ct.ndim == 2 and ct.shape[1] == K and pr.shape[0] == K
    assert rg is None or rg.size == NP // 16
    g = C.c_int(-7)
    rc = hooks().lc_test_fused(_p(X), D, NP // 16, _p(pr), _p(ct), ct.shape[0], _p(rg), int(nrows), K, int(want_ll), grid, _p(q),
                               q.shape[0], q.shape[1], _p(part), part.size, C.addressof(g))
    return rc, g.value


# ---- the separable families: lc_kernels_diag.hip (tests/test_gpu_diag_kernels.py, tests/test_diag_refs_host.py) ------------------
DIAG_SINK, DIAG_SINK_GUARD = 256, 64
EDI_NAMES = ("none", "generic", "plain", "tabled", "one_group")  # DiagEstepInstance, in the order of the enum
_EDP_KEYS = ("ok", "mfma", "mode", "grid", "lds_bytes", "wide", "KT", "REG", "NT", "QUAD", "R", "KTM", "instance", "nslots", "per_cu",
             "block_cap")
_SDP_KEYS = ("ok", "nslice", "rsplit", "second", "nblocks", "width", "last_width", "BR", "BR_last", "nstage", "nstage_last", "deep",
             "deep_last", "lds_bytes")


def _edp(out, name):
    d = dict(zip(_EDP_KEYS, (int(v) for v in out)), name=name.value.decode())
    d["instance"] = EDI_NAMES[d["instance"]] if 0 <= d["instance"] < len(EDI_NAMES) else None
    return d


def estep_diag_plan(DP, K, mode, nrg, mfma, raw=False, want_ll=False, grouped=False, ngroups=1):
    """estep_diag_plan of a launch described by numbers alone, as a dict (instance by name).  The matrix-pipe plan needs a device."""
    out = np.full(16, -7, dtype=i64)
    name = C.create_string_buffer(32)
    rc = hooks().lc_test_estep_diag_plan(DP, K, mode, nrg, int(mfma), int(raw), int(want_ll), int(grouped), ngroups, _p(out),
                                         C.addressof(name))
    assert rc == 0, rc
    return _edp(out, name)


def estep_diag(X, params, mode, ctab, K, qZ, fz_part, ll_part=None, rginfo=None, nrows=0, raw=False, wt=None, mu=None, constk=None,
               sink=None):
    """One launch_estep_diag.  X [nrg * 16 x DP]; params [3][K][DP]; ctab [J x K]; qZ [Kbuf x ldq], fz_part, ll_part (or None), sink
    ([DIAG_SINK + DIAG_SINK_GUARD], with wt) in place; wt None: the difference-form kernels.  -> status, the plan"""
    X, pr, ct, rg = _a(X, f64), _a(params, f64), _a(ctab, f64), _a(rginfo, i32)
    wt, mu, ck = _a(wt, f64), _a(mu, f64), _a(constk, f64)
    q, fz, ll, sk = _io(qZ, f64), _io(fz_part, f64), _io(ll_part, f64), _io(sink, f64)
    NP, DP = X.shape
    assert NP % 16 == 0 and ct.ndim == 2 and ct.shape[1] == K and pr.shape == (3, K, DP)
    assert rg is None or rg.size == NP // 16
    assert mu is None or mu.size == DP
    assert ck is None or ck.size >= K
    assert sk is None or sk.size == DIAG_SINK + DIAG_SINK_GUARD
    out = np.full(16, -7, dtype=i64)
    name = C.create_string_buffer(32)
    rc = hooks().lc_test_estep_diag(_p(X), DP, NP // 16, _p(pr), mode, _p(ct), ct.shape[0], _p(rg), int(nrows), K, int(raw), _p(wt),
                                    0 if wt is None else wt.size, _p(mu), _p(ck), _p(q), q.shape[0], q.shape[1], _p(fz), fz.size,
                                    _p(ll), 0 if ll is None else ll.size, _p(sk), _p(out), C.addressof(name))
    return rc, _edp(out, name)


def suffstat_diag_plan(DP, K, second):
    out = np.full(14, -7, dtype=i64)
    name = C.create_string_buffer(32)
    rc = hooks().lc_test_suffstat_diag_plan(DP, K, int(second), _p(out), C.addressof(name))
    assert rc == 0, rc
    return dict(zip(_SDP_KEYS, (int(v) for v in out)), name=name.value.decode())


def suffstat_diag(X, qZ, K, nchunks, chunk_rows, second, partial, rginfo=None, smask=None, folded=None, NP=None):
    """One launch_suffstat_diag.  X [NP x DP]; qZ [K x ldq]; partial (flat) and folded (flat, or None: no fold) in place.
    -> status, the plan (without name)"""
    X, q, rg, sm = _a(X, f64), _a(qZ, f64), _a(rginfo, i32), _a(smask, u8)
    part, fo = _io(partial, f64), _io(folded, f64)
    NP = X.shape[0] if NP is None else NP
    DP = X.shape[1]
    assert q.shape[0] == K and (sm is None or (sm.ndim == 2 and sm.shape[1] == K)) and (rg is None or rg.size == NP // 16)
    out = np.full(14, -7, dtype=i64)
    rc = hooks().lc_test_suffstat_diag(_p(X), DP, NP, _p(q), K, q.shape[1], _p(rg), _p(sm), 0 if sm is None else sm.shape[0],
                                       nchunks, chunk_rows, int(second), _p(part), part.size, int(fo is not None), _p(fo),
                                       0 if fo is None else fo.size, _p(out))
    return rc, dict(zip(_SDP_KEYS, (int(v) for v in out)))


def diag_weights(DP, K, mode):
    """estep_diag_mfma_weights (no device)"""
    return hooks().lc_test_diag_weights(DP, K, mode)


def diag_pack(a, w2, w1, DP, mode):
    """the host packer of Context::estep_diag (no device): a / w2 / w1 [K x D] -> status, mu [DP], constk [K], wt, cond"""
    a, w2, w1 = _a(a, f64), _a(w2, f64), _a(w1, f64)
    K, D = a.shape
    nw = max(diag_weights(DP, K, mode), 0)
    mu, ck, wt = np.full(DP, np.nan), np.full(K + 1, np.nan), np.full(nw, np.nan)
    cond = C.c_double(np.nan)
    rc = hooks().lc_test_diag_pack(D, DP, K, mode, _p(a), _p(w2), _p(w1), _p(mu), _p(ck), _p(wt), nw, C.addressof(cond))
    return rc, mu, ck[:K], wt, cond.value
