"""ctypes binding of include/libcluster_hip.h (plumbing only: every function
here forwards to the C-ABI; there is no Python or CPU implementation of the
data path).  Loading fails loudly if the shared library has not been built."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np

PKG = Path(__file__).resolve().parent
LIB_PATH = PKG / "lib" / "libcluster_hip.so"
if __import__("os").environ.get("LC_LIB_PATH"):  # kernel experiments (tools/variants.py): another build of the library
    LIB_PATH = Path(__import__("os").environ["LC_LIB_PATH"])
HEADER = PKG.parent / "include" / "libcluster_hip.h"

LC_OK, LC_EINVAL, LC_ERUNTIME, LC_EHIP, LC_EDOMAIN = range(5)
W_DIRICHLET, W_STICKBREAK, W_GDIRICHLET = 0, 1, 2
ALGO_VDP, ALGO_BGMM, ALGO_GMC, ALGO_SGMC, ALGO_DGMM, ALGO_BEMM, ALGO_DGMC, ALGO_EGMC = range(8)
C_GAUSSWISH, C_NORMGAMMA, C_EXPGAMMA = 0, 1, 2
RANK_QZ, RANK_LOGZ, RANK_LOGP = 0, 1, 2  # LC_RANK_*: what lc_ctx_top_rows ranks

c_double_p = C.POINTER(C.c_double)
c_int64_p = C.POINTER(C.c_int64)
c_int_p = C.POINTER(C.c_int)
c_ubyte_p = C.POINTER(C.c_ubyte)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
COMM_ID_BYTES = 128


class Prediction(NamedTuple):
    """Per-row outputs of Model.predict (lc_model_predict): label (int32), logZ, logp, qZ ((N, K) or None)."""
    label: np.ndarray
    logZ: np.ndarray
    logp: np.ndarray
    qZ: np.ndarray | None


class Conditional(NamedTuple):
    """Per-row outputs of Model.predict_conditional (lc_model_predict_conditional): mean (N, ntarget) =
    E[x_target | x_given, training data], logp (N,) = log p(x_given | training data).  var is None: a call with
    variance=True returns a ConditionalVar, which holds it."""
    mean: np.ndarray
    logp: np.ndarray

    @property
    def var(self):
        return None


class ConditionalVar(NamedTuple):
    """Conditional with the predictive variance (lc_model_predict_conditional_var): var (N, ntarget) = the diagonal of the
    mixture's predictive covariance of the target columns, in their order."""
    mean: np.ndarray
    logp: np.ndarray
    var: np.ndarray


class ConditionalDraws(NamedTuple):
    """Conditional with draws (lc_model_predict_conditional_draws): draws (N, m, ntarget) = m draws per row of the target
    columns from p(x_target | x_given, training data), label (N, m) int32 = the component of every draw (K = the prior
    component).  mean and logp are those of the call without draws, bit for bit."""
    mean: np.ndarray
    logp: np.ndarray
    draws: np.ndarray
    label: np.ndarray

    @property
    def var(self):
        return None


class Sample(NamedTuple):
    """New rows from a model (Model.sample, lc_model_sample): rows (n, D), label (n,) int32 = the component every row was
    drawn from (K = the prior component of StickBreak weights)."""
    rows: np.ndarray
    label: np.ndarray


DRAWS_MAX = 64  # LC_DRAWS_MAX: the draws one row of a conditional prediction may have


class Completion(NamedTuple):
    """Per-row outputs of Model.predict_incomplete (lc_model_predict_incomplete): rows (N, D) = the rows with every NaN
    replaced by E[x_unknown | x_known, training data], logp (N,) = log p(x_known | training data), count (N,) int32 = the
    NaNs the row had, cols (N, HOLES_MAX) int32 = their columns, ascending, -1 beyond count."""
    rows: np.ndarray
    logp: np.ndarray
    count: np.ndarray
    cols: np.ndarray

    @property
    def var(self):
        return None


class CompletionVar(NamedTuple):
    """Completion with the predictive variance of the filled values (lc_model_predict_incomplete_var): var (N, HOLES_MAX),
    slot i belongs to cols[:, i]; 0 beyond count and in rows without holes."""
    rows: np.ndarray
    logp: np.ndarray
    count: np.ndarray
    cols: np.ndarray
    var: np.ndarray


class CompletionDraws(NamedTuple):
    """Completion with draws of the filled values (lc_model_predict_incomplete_draws): draws (N, m, HOLES_MAX) = m draws per
    row of its unknown values from p(x_unknown | x_known, training data), slot i belongs to cols[:, i], 0 beyond count and
    in rows without holes; label (N, m) int32 = the component of every draw (K = the prior component), -1 in rows without
    holes.  rows holds the MEAN-completed rows; rows, logp, count and cols are those of the call without draws, bit for bit."""
    rows: np.ndarray
    logp: np.ndarray
    count: np.ndarray
    cols: np.ndarray
    draws: np.ndarray
    label: np.ndarray

    @property
    def var(self):
        return None


HOLES_MAX = 8  # LC_HOLES_MAX: the NaNs one row may hold


class LeaveOneOut(NamedTuple):
    """Per-row outputs of Model.explain (lc_model_predict_leave_one_out): logp (N,) = log p(x | training data), the bits of
    Model.predict's; cond_logp (N, D) = log p(x_d | x_-d, training data); mean (N, D) = E[x_d | x_-d]; worst (N,) int32 =
    the column with the smallest cond_logp (the lowest on ties)."""
    logp: np.ndarray
    cond_logp: np.ndarray
    mean: np.ndarray
    worst: np.ndarray

    @property
    def var(self):
        return None


class LeaveOneOutVar(NamedTuple):
    """LeaveOneOut with var (N, D) = Var[x_d | x_-d]: (x - mean) / sqrt(var) is a z-score per cell."""
    logp: np.ndarray
    cond_logp: np.ndarray
    mean: np.ndarray
    var: np.ndarray
    worst: np.ndarray


class TopRows(NamedTuple):
    """The m best rows of each of C columns (lc_ctx_top_rows, lc_model_exemplars), best first: count (C,) int32, group
    (C, m) int32 (block of the context / of X), row (C, m) int64 (row of that block), score (C, m); the entries past
    count[c] are -1, -1, NaN."""
    count: np.ndarray
    group: np.ndarray
    row: np.ndarray
    score: np.ndarray


QUANTILES_MAX = 16  # LC_QUANTILES_MAX: the probs / thresholds of one order or threshold query


class ScoreQuantiles(NamedTuple):
    """Order statistics of each of C device columns (lc_ctx_score_quantiles): count (C,) int64 = the participating rows
    (valid, score not NaN), rank (C, nprobs) int64 = min(n - 1, max(0, ceil(p n) - 1)) (numpy's "inverted_cdf"), value
    (C, nprobs) = the score of that rank, bit for bit one of the column's; NaN / -1 where count is 0."""
    count: np.ndarray
    rank: np.ndarray
    value: np.ndarray


class ScoreCounts(NamedTuple):
    """lc_ctx_score_counts: count (C,) int64 as ScoreQuantiles, atmost (C, nthr) int64 = the participating scores <= the
    threshold."""
    count: np.ndarray
    atmost: np.ndarray


class FlaggedRows(NamedTuple):
    """The rows of one column beyond a threshold, in context order (lc_ctx_rows_beyond): total = how many there are;
    group int32 (block of the context / of X), row int64 (row of that block), score: the first min(total, limit)."""
    total: int
    group: np.ndarray
    row: np.ndarray
    score: np.ndarray


class TopicPrediction(NamedTuple):
    """Outputs of TopicModel.predict (lc_tmodel_predict).  Per document: qY (docs, T), label_t (int32), Fyz, Fz, sweeps
    (int32); per document lists of per-row arrays: label (int32), logZ, qZ ((N_i, K) each, or None)."""
    qY: np.ndarray
    label_t: np.ndarray
    Fyz: np.ndarray
    Fz: np.ndarray
    sweeps: np.ndarray
    label: list
    logZ: list
    qZ: Optional[list]


def comm_unique_id() -> bytes:
    """ncclGetUniqueId: rank 0 calls it and ships the bytes to the other ranks."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(lib().lc_comm_unique_id(buf))
    return buf.raw


def rccl_available() -> bool:
    return bool(lib().lc_comm_rccl_available())


class HipError(RuntimeError):
    """HIP runtime failure (including: no GPU -- there is no CPU fallback)."""


class DomainError(ArithmeticError):
    pass


_lib = None


def declared_symbols() -> list[str]:
    """Every function the public header declares (used by the symbol test)."""
    txt = HEADER.read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", txt)
    return sorted(set(n for n in names if n != "lc_allreduce_fn"))


def _load_checked() -> C.CDLL:
    """dlopen the library and compare the source hash compiled into it (lc_source_hash) with the tree it sits in: a
    stale binary (sources edited after the last build; the .so is git-ignored and travels prebuilt) is rebuilt when
    hipcc is there and refused otherwise.  LC_ALLOW_STALE_LIB=1 skips the check, and so does LC_LIB_PATH (a user-supplied
    library is loaded as it is)."""
    import os

    from . import build as _build

    def load():
        L = C.CDLL(str(LIB_PATH))
        try:
            L.lc_source_hash.restype = C.c_char_p
            return L, L.lc_source_hash().decode()
        except AttributeError:  # a binary from before the guard existed
            return L, "missing"

    L, have = load()
    # LC_LIB_PATH names another build of the library (kernel experiments): it is the caller's, never compared with this
    # tree and never rebuilt into or over
    if os.environ.get("LC_ALLOW_STALE_LIB") or os.environ.get("LC_LIB_PATH"):
        return L
    want = _build.source_hash()
    if have == want:
        return L
    # dlopen caches by path: a rebuilt file must be loaded under a new name, so rebuild BEFORE anything else binds to
    # the stale handle, then load a private copy of the fresh file
    try:
        _build.build()
    except Exception as e:  # noqa: BLE001
        raise ImportError(f"{LIB_PATH} is stale (built from sources {have}, tree is {want}) and rebuilding failed: {e}. "
                          "Run `python -m libcluster_amd.build`.") from e
    import shutil
    import tempfile

    tmp = Path(tempfile.mkdtemp(prefix="lc_fresh_")) / LIB_PATH.name
    shutil.copy2(LIB_PATH, tmp)
    L2 = C.CDLL(str(tmp))
    L2.lc_source_hash.restype = C.c_char_p
    if L2.lc_source_hash().decode() != want:
        raise ImportError(f"{LIB_PATH} is stale and the rebuild did not pick up the current sources")
    import sys

    print(f"libcluster_amd: rebuilt a stale {LIB_PATH.name} (was {have}, now {want})", file=sys.stderr)
    return L2


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m libcluster_amd.build` "
            "(hipcc, --offload-arch=gfx950).  There is no Python/CPU fallback for the E-step."
        )
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64, and
    # a process that initialises both that copy and the system ROCm copy loses the GPU in the second
    # one ("no ROCm-capable device").  Loading torch first makes the C-ABI library bind to the runtime
    # torch uses (same SONAME), which is also what lets torch streams and RCCL see our buffers.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = _load_checked()
    L.lc_last_error.restype = C.c_char_p
    L.lc_comm_unique_id.argtypes = [C.c_void_p]
    L.lc_ctx_comm_init_rccl.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.lc_ctx_comm_init_host.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int]
    L.lc_ctx_comm_free.argtypes = [C.c_void_p]
    L.lc_ctx_comm_info.argtypes = [C.c_void_p, c_int_p, c_int_p, C.POINTER(C.c_char_p)]
    L.lc_ctx_allreduce.argtypes = [C.c_void_p, c_double_p, C.c_int]
    for f in ("lc_const_converge", "lc_const_fengydel", "lc_const_zerocutoff"):
        getattr(L, f).restype = C.c_double
    L.lc_digamma.restype = C.c_double
    L.lc_digamma.argtypes = [C.c_double]
    L.lc_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    L.lc_ctx_destroy.argtypes = [C.c_void_p]
    L.lc_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.lc_ctx_synchronize.argtypes = [C.c_void_p]
    L.lc_ctx_dims.argtypes = [C.c_void_p, c_int_p, c_int_p, c_int64_p, c_int_p]
    L.lc_ctx_set_data.argtypes = [C.c_void_p, C.c_int, C.POINTER(c_double_p), c_int64_p, C.c_int, C.c_int64, C.c_int64]
    L.lc_ctx_synth.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, c_double_p, c_double_p, C.c_uint64,
                               C.c_int64, C.c_double]
    L.lc_ctx_synth_groups.argtypes = [C.c_void_p, C.c_int, c_int64_p, C.c_int, C.c_int, c_double_p, c_double_p,
                                      c_double_p, C.c_uint64, c_int64_p, C.c_double]
    L.lc_ctx_set_sharding.argtypes = [C.c_void_p, C.c_int]
    L.lc_ctx_set_skip_zero.argtypes = [C.c_void_p, C.c_int]
    L.lc_ctx_set_speck_skip.argtypes = [C.c_void_p, C.c_int]
    L.lc_ctx_speck_passes.argtypes = [C.c_void_p, c_int64_p, c_int64_p]
    L.lc_ctx_speck_list_passes.argtypes = [C.c_void_p, c_int64_p]
    L.lc_ctx_set_estep_masks.argtypes = [C.c_void_p, C.c_int]
    L.lc_ctx_speck_mask_passes.argtypes = [C.c_void_p, c_int64_p]
    L.lc_ctx_get_rows.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p]
    L.lc_ctx_set_qz.argtypes = [C.c_void_p, C.c_int, c_double_p, C.c_int, C.c_int64, C.c_int64]
    L.lc_ctx_get_qz.argtypes = [C.c_void_p, C.c_int, c_double_p, C.c_int64, C.c_int64]
    L.lc_ctx_get_qz_rows.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p, C.c_int64, C.c_int64]
    L.lc_ctx_fill_qz.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.lc_estep.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.lc_estep_posterior.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                     c_double_p, c_ubyte_p, c_double_p, c_double_p]
    L.lc_eloglike.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.lc_mahaldist.argtypes = [C.c_void_p, c_double_p, c_double_p, c_double_p]
    L.lc_suffstat.argtypes = [C.c_void_p, c_ubyte_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.lc_suffstat_diag.argtypes = [C.c_void_p, c_ubyte_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.lc_estep_diag.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, C.c_int,
                                c_double_p, c_double_p]
    L.lc_colsums.argtypes = [C.c_void_p, c_double_p]
    L.lc_ctx_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p]
    L.lc_ctx_timing_enable.argtypes = [C.c_void_p, C.c_int]
    L.lc_ctx_timing_reset.argtypes = [C.c_void_p]
    L.lc_ctx_timing_get.argtypes = [C.c_void_p, c_double_p, c_int64_p, c_double_p, c_int64_p]
    L.lc_vbem.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                          C.c_int, C.c_int, C.c_int, C.c_uint, c_double_p, c_int_p, c_double_p, C.c_int]
    L.lc_learn.argtypes = [C.c_int, C.c_int, C.POINTER(c_double_p), c_int64_p, C.c_int, C.c_int64, C.c_int64,
                           C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int,
                           C.POINTER(C.c_void_p), c_double_p]
    L.lc_learn_w.argtypes = [C.c_int, C.c_int, C.POINTER(c_double_p), c_int64_p, C.c_int, C.c_int64, C.c_int64,
                             C.c_double, c_double_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int,
                             C.POINTER(C.c_void_p), c_double_p]
    L.lc_cluster.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                             C.c_uint, C.POINTER(C.c_void_p), c_double_p]
    L.lc_prune.argtypes = [C.c_void_p, C.c_void_p, C.c_int, c_int_p]
    L.lc_model_free.argtypes = [C.c_void_p]
    L.lc_model_dims.argtypes = [C.c_void_p, c_int_p, c_int_p, c_int_p]
    L.lc_model_rounds.argtypes = [C.c_void_p, c_int_p]
    L.lc_model_round.argtypes = [C.c_void_p, C.c_int, c_int_p, c_int_p, c_double_p, C.c_int]
    L.lc_model_get_qz.argtypes = [C.c_void_p, C.c_int, c_double_p, C.c_int64, C.c_int64]
    L.lc_model_weights.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p]
    L.lc_model_cluster.argtypes = [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                   c_double_p, c_double_p]
    L.lc_model_kinds.argtypes = [C.c_void_p, c_int_p, c_int_p]
    L.lc_model_fenergy.argtypes = [C.c_void_p, c_double_p, c_double_p]
    L.lc_weights_update.argtypes = [C.c_int, C.c_double, c_double_p, C.c_int, c_double_p, c_double_p]
    L.lc_gw_mstep.argtypes = [C.c_double, C.c_int, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p,
                              c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.lc_learn_topic.argtypes = [C.c_int, c_int_p, C.POINTER(c_double_p), c_int64_p, C.c_int, C.c_int64, C.c_int64,
                                 C.POINTER(c_double_p), C.c_int, C.POINTER(c_double_p), C.c_double, C.c_double,
                                 C.c_uint, C.c_int, C.c_int, C.c_uint, C.c_int, C.POINTER(C.c_void_p), c_double_p]
    L.lc_learn_topic_dist.argtypes = [C.c_int, c_int_p, C.POINTER(c_double_p), c_int64_p, C.c_int, C.c_int64, C.c_int64,
                                      C.POINTER(c_double_p), C.c_int, C.POINTER(c_double_p), C.c_double, C.c_double,
                                      C.c_uint, C.c_int, C.c_int, C.c_uint, C.c_int, C.c_void_p, ALLREDUCE_FN,
                                      C.c_void_p, C.POINTER(C.c_void_p), c_double_p]
    L.lc_tmodel_free.argtypes = [C.c_void_p]
    L.lc_tmodel_dims.argtypes = [C.c_void_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p]
    L.lc_tmodel_get_qy.argtypes = [C.c_void_p, C.c_int, c_double_p]
    L.lc_tmodel_get_qz.argtypes = [C.c_void_p, C.c_int, c_double_p, C.c_int64, C.c_int64]
    L.lc_tmodel_get_qz_all.argtypes = [C.c_void_p, c_double_p]
    L.lc_model_get_qz_all.argtypes = [C.c_void_p, c_double_p]
    L.lc_ctx_get_qz_all.argtypes = [C.c_void_p, c_double_p]
    L.lc_tmodel_weights.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p]
    L.lc_tmodel_cluster.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p,
                                    c_double_p, c_double_p, c_double_p, c_double_p]
    L.lc_tmodel_rounds.argtypes = [C.c_void_p, c_int_p]
    L.lc_tmodel_round.argtypes = [C.c_void_p, C.c_int, c_int_p, c_int_p, c_int_p, c_double_p, C.c_int]
    L.lc_tmodel_predict.argtypes = [C.c_void_p, C.c_void_p, c_int_p, c_double_p, C.c_int, C.c_double, C.c_int]
    L.lc_ctx_get_doc_predictions.argtypes = [C.c_void_p, C.c_int, C.c_int, c_double_p, C.POINTER(C.c_int32), c_double_p,
                                             c_double_p, C.POINTER(C.c_int32)]
    L.lc_tmodel_release_data.argtypes = [C.c_void_p]
    L.lc_ng_mstep.argtypes = [C.c_double, C.c_int, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p,
                              c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.lc_eg_mstep.argtypes = [C.c_double, C.c_int, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p,
                              c_double_p, c_double_p]
    c_int32_p = C.POINTER(C.c_int32)
    L.lc_model_predict.argtypes = [C.c_void_p, C.c_void_p, c_int_p, C.c_int]
    L.lc_ctx_get_predictions.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_int32_p, c_double_p, c_double_p]
    L.lc_model_release_data.argtypes = [C.c_void_p]
    L.lc_weights_predictive.argtypes = [C.c_int, C.c_double, c_double_p, C.c_int, c_double_p, c_double_p]
    L.lc_ctx_top_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, c_int32_p, c_int64_p,
                                  c_double_p]
    L.lc_model_exemplars.argtypes = [C.c_void_p, C.c_void_p, c_int_p, C.c_int, c_int32_p, c_int32_p, c_int64_p, c_double_p]
    L.lc_ctx_score_quantiles.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p, C.c_int, c_int64_p, c_int64_p,
                                         c_double_p]
    L.lc_ctx_score_counts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p, C.c_int, c_int64_p, c_int64_p]
    L.lc_ctx_rows_beyond.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int64,
                                     c_int64_p, c_int32_p, c_int64_p, c_double_p]
    L.lc_model_predict_conditional.argtypes = [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, c_int_p, C.c_int]
    L.lc_ctx_get_conditional.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p, C.c_int64, c_double_p]
    L.lc_model_predict_conditional_var.argtypes = [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, c_int_p, C.c_int]
    L.lc_ctx_get_conditional_var.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p, C.c_int64]
    L.lc_gw_conditional_var.argtypes = [C.c_int, C.c_double, C.c_double, c_double_p, c_int_p, C.c_int, c_int_p, C.c_int,
                                        c_double_p, c_double_p]
    L.lc_gw_conditional.argtypes = [C.c_int, C.c_double, C.c_double, c_double_p, c_double_p, c_int_p, C.c_int, c_int_p,
                                    C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                    c_double_p]
    L.lc_model_predict_incomplete.argtypes = [C.c_void_p, C.c_void_p, c_int_p]
    L.lc_ctx_get_completed.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p, C.c_int64, c_double_p,
                                       c_int32_p, c_int32_p]
    L.lc_gw_precision.argtypes = [C.c_int, C.c_double, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p,
                                  c_double_p, c_double_p]
    L.lc_model_predict_incomplete_var.argtypes = [C.c_void_p, C.c_void_p, c_int_p]
    L.lc_ctx_get_completed_var.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p, C.c_int64]
    L.lc_gw_precision_var.argtypes = [C.c_int, C.c_double, C.c_double, c_double_p]
    L.lc_model_predict_incomplete_draws.argtypes = [C.c_void_p, C.c_void_p, c_int_p, C.c_int, C.c_uint64]
    L.lc_ctx_get_completed_draws.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p, c_int32_p]
    L.lc_ctx_completed_draws.argtypes = [C.c_void_p, c_int_p]
    L.lc_model_predict_leave_one_out.argtypes = [C.c_void_p, C.c_void_p, c_int_p, C.c_int]
    L.lc_ctx_get_leave_one_out.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p, c_double_p, c_double_p,
                                           c_double_p, C.c_int64, c_int32_p]
    L.lc_model_predict_conditional_draws.argtypes = [C.c_void_p, C.c_void_p, c_int_p, c_int_p, C.c_int, c_int_p, C.c_int,
                                                     C.c_int, C.c_uint64]
    L.lc_ctx_get_conditional_draws.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_double_p, c_int32_p]
    L.lc_ctx_conditional_draws.argtypes = [C.c_void_p, c_int_p, c_int_p]
    L.lc_model_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_int, c_int64_p, c_int_p, C.c_uint64, C.c_int64]
    L.lc_ctx_get_sample_labels.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, c_int32_p]
    L.lc_gw_conditional_cov.argtypes = [C.c_int, C.c_double, C.c_double, c_double_p, c_int_p, C.c_int, c_int_p, C.c_int,
                                        c_double_p, c_double_p]
    # device-resident data in, row results out: device addresses travel as plain integers
    L.lc_ctx_set_data_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), c_int64_p, C.c_int, C.c_int64, C.c_int64]
    L.lc_ctx_data_range.argtypes = [C.c_void_p, c_double_p, c_int64_p]
    L.lc_learn_ctx.argtypes = [C.c_int, C.c_void_p, C.c_double, c_double_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint,
                               C.POINTER(C.c_void_p), c_double_p]
    L.lc_ctx_get_qz_rows_device.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64]
    L.lc_ctx_get_predictions_device.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def check(rc: int) -> None:
    """Map lc_status to the exception classes the reference throws."""
    if rc == LC_OK:
        return
    msg = lib().lc_last_error().decode("utf-8", "replace")
    if rc == LC_EINVAL:
        raise ValueError(msg)  # std::invalid_argument
    if rc == LC_EHIP:
        raise HipError(msg)
    if rc == LC_EDOMAIN:
        raise DomainError(msg)  # std::domain_error
    raise RuntimeError(msg)  # std::runtime_error


def dptr(a):
    if a is None:
        return None
    assert a.dtype == np.float64
    return a.ctypes.data_as(c_double_p)


def _strides(a: np.ndarray):
    assert a.ndim == 2 and a.dtype == np.float64
    return a.strides[0] // 8, a.strides[1] // 8


def is_device_tensor(x) -> bool:
    """True for a torch tensor that lives on a GPU.  torch is only imported once an object of a torch type shows up: numpy
    callers never load it through this module (a CPU tensor is host data and goes through np.asarray as ever)."""
    if not type(x).__module__.startswith("torch"):
        return False
    import torch

    return isinstance(x, torch.Tensor) and bool(x.is_cuda)


def device_blocks(X):
    """How the data entry points read X: None for host data (numpy arrays, CPU tensors, lists of them), or the
    list of blocks when X is a 2-D CUDA torch.float64 tensor or a list of them on one device.  TypeError for another dtype
    (nothing is converted silently), ValueError for a list that mixes host and device blocks, a block that is not 2-D,
    blocks of different widths or on different devices.  Nothing is launched or copied here."""
    Xs = list(X) if isinstance(X, (list, tuple)) else [X]
    on_device = [is_device_tensor(x) for x in Xs]
    if not any(on_device):
        return None
    if not all(on_device):
        raise ValueError("X mixes host arrays and device tensors: move every block to one side first")
    import torch

    for x in Xs:
        if x.dtype != torch.float64:
            raise TypeError(f"device tensors must be float64, not {x.dtype}: convert with X.double() (nothing is converted "
                            "silently)")
        if x.ndim != 2:
            raise ValueError(f"a device tensor of observations must be 2-D (N, D), not {x.ndim}-D")
    if any(x.shape[1] != Xs[0].shape[1] for x in Xs):
        raise ValueError("X dimensions are inconsistent between groups!")
    if any(x.device != Xs[0].device for x in Xs):
        raise ValueError("the blocks of X live on different devices")
    return Xs


def _torch_stream(tdev) -> int:
    import torch

    return int(torch.cuda.current_stream(tdev).cuda_stream)


def _top_rows_call(call, C_, m):
    """the output arrays of lc_ctx_top_rows / lc_model_exemplars for C_ columns of m entries -> TopRows"""
    shape = (max(C_, 0), max(min(m, 64), 0))  # (out-of-range arguments are the library's to refuse: nothing is written)
    count = np.zeros(shape[0], dtype=np.int32)
    group, row = np.full(shape, -1, dtype=np.int32), np.full(shape, -1, dtype=np.int64)
    score = np.full(shape, np.nan)
    c_int32_p = C.POINTER(C.c_int32)
    check(call(count.ctypes.data_as(c_int32_p), group.ctypes.data_as(c_int32_p), row.ctypes.data_as(c_int64_p), dptr(score)))
    return TopRows(count, group, row, score)


class Context:
    """lc_ctx: device-resident observations + qZ (one per data set / rank)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._h = C.c_void_p()
        self._cb = None
        self._device, self._stream = int(device), int(stream or 0)
        check(lib().lc_ctx_create(device, C.c_void_p(stream or 0), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lc_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- data ---------------------------------------------------------------
    def set_data(self, X):
        """X: (N, D) array or list of (N_j, D) arrays, any strides (no copy).  Also a 2-D CUDA torch.float64 tensor or a list
        of them on this context's device, any strides (device_blocks for what is refused): one kernel packs them into the
        context's own image, so the tensors may be overwritten or freed afterwards and are not kept alive."""
        blocks = device_blocks(X)
        if blocks is not None:
            return self._set_data_device(blocks)
        Xs = [X] if isinstance(X, np.ndarray) else list(X)
        Xs = [np.asarray(x, dtype=np.float64) for x in Xs]
        D = Xs[0].shape[1]
        for x in Xs:
            if x.ndim != 2 or x.shape[1] != D:
                raise ValueError("X dimensions are inconsistent between groups!")
        st = {_strides(x) for x in Xs}
        if len(st) == 1 and all(x.shape[0] > 1 for x in Xs) and min(next(iter(st))) > 0:
            rs, cs = next(iter(st))  # e.g. all column-major (Eigen default) or all row-major: no copy
        else:
            Xs = [np.ascontiguousarray(x) for x in Xs]
            rs, cs = D, 1
        J = len(Xs)
        ptrs = (c_double_p * J)(*[dptr(x) for x in Xs])
        Nj = (C.c_int64 * J)(*[x.shape[0] for x in Xs])
        check(lib().lc_ctx_set_data(self._h, J, ptrs, Nj, D, rs, cs))
        self._X = Xs  # keep alive

    def _after_torch(self, tdev):
        """Order the context's stream behind torch's current stream of tdev: nothing to do when they are one stream (the
        wrappers that create the context see to that), a host wait for torch's stream otherwise."""
        if _torch_stream(tdev) != self._stream:
            import torch

            torch.cuda.current_stream(tdev).synchronize()

    def _set_data_device(self, Xs):
        tdev = Xs[0].device
        if tdev.index != self._device:
            raise ValueError(f"X lives on device {tdev.index}, the context on device {self._device}")
        st = {(x.stride(0), x.stride(1)) for x in Xs}
        if len(st) == 1 and all(x.shape[0] > 1 for x in Xs) and min(next(iter(st))) > 0:
            rs, cs = next(iter(st))  # e.g. all row-major, all column-major (a .t() view), a slice of a wider tensor: no copy
        else:  # a zero stride (expand), single rows, or blocks laid out differently: contiguous copies on the device
            Xs = [x.contiguous() for x in Xs]
            rs, cs = Xs[0].shape[1], 1
        J, D = len(Xs), Xs[0].shape[1]
        ptrs = (C.c_void_p * J)(*[x.data_ptr() if x.shape[0] else None for x in Xs])
        Nj = (C.c_int64 * J)(*[x.shape[0] for x in Xs])
        self._after_torch(tdev)
        check(lib().lc_ctx_set_data_device(self._h, J, ptrs, Nj, D, rs, cs))  # (synchronises the context's stream)
        self._X = None

    def data_range(self):
        """(min, n_nan) of the observations (lc_ctx_data_range): the smallest entry that is a number (+inf: none) and the
        count of NaN entries."""
        lo, nn = C.c_double(), C.c_int64()
        check(lib().lc_ctx_data_range(self._h, C.byref(lo), C.byref(nn)))
        return lo.value, nn.value

    def get_qz_rows_device(self, j, row0, n, tdev=None):
        """Rows [row0, row0 + n) of group j of qZ as a row-major (n, K) torch.float64 tensor on the context's device,
        filled on the context's stream (lc_ctx_get_qz_rows_device): synchronize() before another stream reads it."""
        import torch

        tdev = torch.device("cuda", self._device) if tdev is None else tdev
        K = self.dims()[3]
        q = torch.empty((n, K), dtype=torch.float64, device=tdev)
        if n and K:
            self._after_torch(tdev)
            check(lib().lc_ctx_get_qz_rows_device(self._h, j, row0, n, q.data_ptr(), K, 1))
        return q

    def get_predictions_device(self, j, row0, n, logp=True, tdev=None):
        """get_predictions as torch tensors on the context's device (label int32, logZ, logp), copied on the context's
        stream (lc_ctx_get_predictions_device): synchronize() before another stream reads them."""
        import torch

        tdev = torch.device("cuda", self._device) if tdev is None else tdev
        label = torch.empty(n, dtype=torch.int32, device=tdev)
        logZ = torch.empty(n, dtype=torch.float64, device=tdev)
        lp = torch.empty(n, dtype=torch.float64, device=tdev) if logp else None
        if n:
            self._after_torch(tdev)
            check(lib().lc_ctx_get_predictions_device(self._h, j, row0, n, label.data_ptr(), logZ.data_ptr(),
                                                      lp.data_ptr() if logp else None))
        return label, logZ, lp

    def synth(self, N, D, K, mu, L, seed, row_offset=0, hard=0.9):
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        L = np.ascontiguousarray(L, dtype=np.float64)
        assert mu.shape == (K, D) and L.shape == (K, D, D)
        check(lib().lc_ctx_synth(self._h, N, D, K, dptr(mu), dptr(L), seed, row_offset, hard))

    def synth_groups(self, Nj, D, K, mu, L, seed, mix=None, group_ids=None, hard=0.9):
        """J groups of Nj rows; mix: (J, K) mixing proportions per group (None = uniform)."""
        Nj = np.ascontiguousarray(Nj, dtype=np.int64)
        J = Nj.size
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        L = np.ascontiguousarray(L, dtype=np.float64)
        cdf = None
        if mix is not None:
            cdf = np.ascontiguousarray(np.cumsum(np.asarray(mix, dtype=np.float64), axis=1))
            assert cdf.shape == (J, K)
        gid = None if group_ids is None else np.ascontiguousarray(group_ids, dtype=np.int64)
        check(lib().lc_ctx_synth_groups(self._h, J, Nj.ctypes.data_as(c_int64_p), D, K, dptr(mu), dptr(L), dptr(cdf),
                                        seed, None if gid is None else gid.ctypes.data_as(c_int64_p), hard))

    def set_skip_zero(self, on: bool = True):
        """Exact: leave out (4-row step, cluster) pairs with all-zero responsibilities in the statistics pass."""
        check(lib().lc_ctx_set_skip_zero(self._h, int(on)))

    def set_speck_skip(self, on: bool = True):
        """Feature-GEMM statistics pass: leave out (4-row step, cluster quad) pairs whose responsibilities are all below
        2^-300 (the default); False multiplies every speck as the dense kernel always did."""
        check(lib().lc_ctx_set_speck_skip(self._h, int(on)))

    def speck_passes(self):
        """-> (statistics passes that ran the speck-skipping kernel, passes its probe sent to the dense one)"""
        a, b = C.c_int64(), C.c_int64()
        check(lib().lc_ctx_speck_passes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def speck_list_passes(self):
        """-> how many of the skipping passes summed per-quad row lists (the list route)"""
        a = C.c_int64()
        check(lib().lc_ctx_speck_list_passes(self._h, C.byref(a)))
        return a.value

    def set_estep_masks(self, on: bool = True):
        """E-steps whose statistics pass could take the list route write one "kept" bit per (row, cluster quad) next to
        the responsibilities (the default); the pass that follows builds its lists from them.  False: every pass probes
        and builds from qZ.  Same results bit for bit."""
        check(lib().lc_ctx_set_estep_masks(self._h, int(on)))

    def speck_mask_passes(self):
        """-> how many list passes were built from the kept bits of the E-step that wrote qZ"""
        a = C.c_int64()
        check(lib().lc_ctx_speck_mask_passes(self._h, C.byref(a)))
        return a.value

    def set_sharding(self, whole_groups: bool):
        check(lib().lc_ctx_set_sharding(self._h, int(whole_groups)))

    def dims(self):
        J, D, K, N = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        check(lib().lc_ctx_dims(self._h, C.byref(J), C.byref(D), C.byref(N), C.byref(K)))
        return J.value, D.value, N.value, K.value

    def get_rows(self, j, row0, n):
        _, D, _, _ = self.dims()
        out = np.empty((n, D))
        check(lib().lc_ctx_get_rows(self._h, j, row0, n, dptr(out)))
        return out

    def set_qz(self, qZ):
        qs = [qZ] if isinstance(qZ, np.ndarray) else list(qZ)
        K = qs[0].shape[1]
        for j, q in enumerate(qs):
            q = np.asarray(q, dtype=np.float64)
            if q.shape[1] != K:
                raise ValueError("qZ groups must have the same number of columns")
            if q.shape[0] == 0:
                q = np.zeros((1, K))[:0]
                check(lib().lc_ctx_set_qz(self._h, j, dptr(np.zeros(1)), K, K, 1))
                continue
            rs, cs = _strides(q)
            check(lib().lc_ctx_set_qz(self._h, j, dptr(q), K, rs, cs))

    def get_qz(self, rows_per_group):
        """qZ of every group (one device-to-host transfer) -> list of (N_j, K) arrays."""
        _, _, _, K = self.dims()
        rows = [int(n) for n in rows_per_group]
        allq = np.zeros((sum(rows), K))
        if allq.size:
            check(lib().lc_ctx_get_qz_all(self._h, dptr(allq)))
        return [allq[o - n:o] for n, o in zip(rows, np.cumsum(rows))]

    def get_qz_colmajor(self, rows_per_group):
        """The same through the column-major bulk getter (what Eigen callers use): list of Fortran-ordered (N_j, K)."""
        _, _, _, K = self.dims()
        out = [np.zeros((int(n), K), order="F") for n in rows_per_group]
        ptrs = (c_double_p * len(out))(*[dptr(a) if a.size else None for a in out])
        if sum(a.size for a in out):
            fn = lib().lc_ctx_get_qz_all_colmajor
            fn.argtypes = [C.c_void_p, C.POINTER(c_double_p)]
            check(fn(self._h, ptrs))
        return out

    def get_qz_rows(self, j, row0, n):
        _, _, _, K = self.dims()
        q = np.empty((n, K))
        if n:
            check(lib().lc_ctx_get_qz_rows(self._h, j, row0, n, dptr(q), K, 1))
        return q

    def fill_qz(self, K, value=1.0):
        check(lib().lc_ctx_fill_qz(self._h, K, value))

    # -- hot path -------------------------------------------------------------
    def estep_posterior(self, nu, beta, m, iW, logdW, Elogpi, active=None, want_ll=True):
        K = len(nu)
        nu, beta, m, iW, logdW, Elogpi = (np.ascontiguousarray(a, dtype=np.float64)
                                          for a in (nu, beta, m, iW, logdW, Elogpi))
        Fz = C.c_double()
        ll = np.zeros(K) if want_ll else None
        act = None
        if active is not None:
            active = np.ascontiguousarray(active, dtype=np.uint8)
            act = active.ctypes.data_as(c_ubyte_p)
        check(lib().lc_estep_posterior(self._h, K, dptr(nu), dptr(beta), dptr(m), dptr(iW), dptr(logdW),
                                       dptr(Elogpi), act, C.byref(Fz), dptr(ll)))
        return Fz.value, ll

    def eloglike(self, nu, beta, m, iW, logdW, rows_per_group):
        """K x GaussWish::Eloglike for every group -> list of (N_j, K) arrays."""
        K = len(nu)
        nu, beta, m, iW, logdW = (np.ascontiguousarray(a, dtype=np.float64) for a in (nu, beta, m, iW, logdW))
        check(lib().lc_eloglike(self._h, K, dptr(nu), dptr(beta), dptr(m), dptr(iW), dptr(logdW)))
        return self.get_qz(rows_per_group)

    def estep(self, A, m, c):
        A, m, c = (np.ascontiguousarray(a, dtype=np.float64) for a in (A, m, c))
        K = A.shape[0]
        Fz = C.c_double()
        ll = np.zeros(K)
        check(lib().lc_estep(self._h, K, dptr(A), dptr(m), dptr(c), C.byref(Fz), dptr(ll)))
        return Fz.value, ll

    def mahaldist(self, mu, A):
        """probutils::mahaldist for every resident row -> (N_total,) array."""
        J, D, N, _ = self.dims()
        mu, A = (np.ascontiguousarray(v, dtype=np.float64) for v in (mu, A))
        out = np.zeros(N)
        check(lib().lc_mahaldist(self._h, dptr(mu), dptr(A), dptr(out)))
        return out

    def suffstat(self, smask=None):
        J, D, _, K = self.dims()
        Nk, xs, xxs, Njk = np.zeros(K), np.zeros((K, D)), np.zeros((K, D, D)), np.zeros((J, K))
        sm = None
        if smask is not None:
            smask = np.ascontiguousarray(smask, dtype=np.uint8)
            sm = smask.ctypes.data_as(c_ubyte_p)
        check(lib().lc_suffstat(self._h, sm, dptr(Nk), dptr(xs), dptr(xxs), dptr(Njk)))
        return Nk, xs, xxs, Njk

    def suffstat_diag(self, smask=None, second=True):
        """NormGamma / ExpGamma statistics: N_k, sum q x, sum q x.^2 (None when second=False), N_jk."""
        J, D, _, K = self.dims()
        Nk, xs, Njk = np.zeros(K), np.zeros((K, D)), np.zeros((J, K))
        xxs = np.zeros((K, D)) if second else None
        sm = None
        if smask is not None:
            smask = np.ascontiguousarray(smask, dtype=np.uint8)
            sm = smask.ctypes.data_as(c_ubyte_p)
        check(lib().lc_suffstat_diag(self._h, sm, dptr(Nk), dptr(xs), dptr(xxs), dptr(Njk)))
        return Nk, xs, xxs, Njk

    def estep_diag(self, a, w2, w1, c, raw=False):
        a, w2, w1, c = (np.ascontiguousarray(v, dtype=np.float64) for v in (a, w2, w1, c))
        K = a.shape[0]
        Fz = C.c_double()
        ll = np.zeros(K)
        check(lib().lc_estep_diag(self._h, K, dptr(a), dptr(w2), dptr(w1), dptr(c), int(raw), C.byref(Fz), dptr(ll)))
        return Fz.value, ll

    def colsums(self):
        J, _, _, K = self.dims()
        out = np.zeros((J, K))
        check(lib().lc_colsums(self._h, dptr(out)))
        return out

    def set_allreduce(self, fn):
        """fn(device_ptr:int, count:int, stream:int) -> None; sums in place across ranks."""
        if fn is None:
            self._cb = None
            check(lib().lc_ctx_set_allreduce(self._h, C.cast(None, ALLREDUCE_FN), None))
            return

        def tramp(user, buf, count, stream):
            try:
                fn(buf or 0, count, stream or 0)
                return 0
            except Exception as e:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        self._cb = ALLREDUCE_FN(tramp)
        check(lib().lc_ctx_set_allreduce(self._h, self._cb, None))

    # -- native collectives (lc_comm.cpp) ---------------------------------------
    def comm_init_rccl(self, unique_id: bytes, rank: int, world: int):
        """ncclCommInitRank on this context's device with the id rank 0 got from comm_unique_id()."""
        assert len(unique_id) == COMM_ID_BYTES
        buf = C.create_string_buffer(unique_id, COMM_ID_BYTES)
        check(lib().lc_ctx_comm_init_rccl(self._h, buf, rank, world))

    def comm_init_host(self, name: str, rank: int, world: int):
        """Host-staged communicator over the shared-memory object /lc_comm_<name> (any placement of ranks)."""
        check(lib().lc_ctx_comm_init_host(self._h, name.encode(), rank, world))

    def comm_free(self):
        check(lib().lc_ctx_comm_free(self._h))

    def comm_info(self):
        r, w, k = C.c_int(), C.c_int(), C.c_char_p()
        check(lib().lc_ctx_comm_info(self._h, C.byref(r), C.byref(w), C.byref(k)))
        return {"rank": r.value, "world": w.value, "kind": (k.value or b"none").decode()}

    def allreduce(self, values):
        """Sum a small host vector over the ranks (through the context's communicator / hook)."""
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        check(lib().lc_ctx_allreduce(self._h, dptr(v), v.size))
        return v

    def timing_enable(self, on=True):
        check(lib().lc_ctx_timing_enable(self._h, int(on)))

    def timing_reset(self):
        check(lib().lc_ctx_timing_reset(self._h))

    def timing_get(self):
        a, b = C.c_double(), C.c_double()
        na, nb = C.c_int64(), C.c_int64()
        check(lib().lc_ctx_timing_get(self._h, C.byref(a), C.byref(na), C.byref(b), C.byref(nb)))
        f, nf = C.c_double(), C.c_int64()
        fn = lib().lc_ctx_timing_get_fused
        fn.argtypes = [C.c_void_p, c_double_p, c_int64_p]
        check(fn(self._h, C.byref(f), C.byref(nf)))
        return {"estep_ms": a.value, "estep_calls": na.value, "suffstat_ms": b.value, "suffstat_calls": nb.value,
                "fused_ms": f.value, "fused_calls": nf.value}

    TIMING_FIELDS = ("estep_ms", "estep_calls", "suffstat_ms", "suffstat_calls", "fused_ms", "fused_calls",
                     "allreduce_ms", "allreduce_calls", "host_stats_ms", "host_mstep_ms", "host_estep_ms",
                     "host_fenergy_ms", "host_iters", "estep_diag_mfma_calls")

    def timing_get_all(self):
        """Kernel, collective and host-phase times since the last reset (lc_ctx_timing_get_all)."""
        out = (C.c_double * len(self.TIMING_FIELDS))()
        fn = lib().lc_ctx_timing_get_all
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        check(fn(self._h, out, len(self.TIMING_FIELDS)))
        return {k: (int(v) if k.endswith(("_calls", "_iters")) else float(v)) for k, v in zip(self.TIMING_FIELDS, out)}

    def get_predictions(self, j, row0, n, logp=True):
        """Rows [row0, row0+n) of block j of the last Model.predict_context on this context -> (label int32, logZ,
        logp) arrays (logp None when logp=False)."""
        label, logZ = np.zeros(n, dtype=np.int32), np.zeros(n)
        lp = np.zeros(n) if logp else None
        if n:
            check(lib().lc_ctx_get_predictions(self._h, j, row0, n, label.ctypes.data_as(C.POINTER(C.c_int32)),
                                               dptr(logZ), dptr(lp)))
        return label, logZ, lp

    def get_conditional(self, j, row0, n, ntarget, variance=False, draws=False):
        """Rows [row0, row0+n) of block j of the last Model.predict_conditional_context on this context ->
        Conditional(mean (n, ntarget), logp (n,)); ntarget is the number of target columns of that call.  variance:
        ConditionalVar, with var (n, ntarget) (lc_ctx_get_conditional_var; ValueError when that call was made without
        variance=True).  draws: True, or the number of draws per row of that call -> ConditionalDraws, with draws
        (n, m, ntarget) and label (n, m) (lc_ctx_get_conditional_draws; ValueError when that call was made without
        draws)."""
        if variance and draws:
            raise ValueError("a conditional prediction holds its variance or draws, not both")
        mean, logp = np.zeros((n, ntarget)), np.zeros(n)
        check(lib().lc_ctx_get_conditional(self._h, j, row0, n, dptr(mean), ntarget, dptr(logp)))
        if draws:
            m, nt = self.conditional_draws()  # (the library's own counts size the buffers)
            if m < 1:
                raise ValueError("the context holds no draws of a conditional prediction (lc_model_predict_conditional_draws)")
            if draws is not True and int(draws) != m:
                raise ValueError(f"the context's conditional prediction has {m} draws per row, not {int(draws)}")
            if nt != ntarget:
                raise ValueError(f"the context's conditional prediction has {nt} target columns, not {ntarget}")
            dr, lab = np.zeros((n, m, ntarget)), np.zeros((n, m), dtype=np.int32)
            check(lib().lc_ctx_get_conditional_draws(self._h, j, row0, n, dptr(dr), lab.ctypes.data_as(C.POINTER(C.c_int32))))
            return ConditionalDraws(mean, logp, dr, lab)
        if not variance:
            return Conditional(mean, logp)
        var = np.zeros((n, ntarget))
        check(lib().lc_ctx_get_conditional_var(self._h, j, row0, n, dptr(var), ntarget))
        return ConditionalVar(mean, logp, var)

    def conditional_draws(self):
        """(ndraws, ntarget) of the draws the context holds (lc_ctx_conditional_draws); (0, 0): none."""
        nd, nt = C.c_int(), C.c_int()
        check(lib().lc_ctx_conditional_draws(self._h, C.byref(nd), C.byref(nt)))
        return nd.value, nt.value

    def get_sample_labels(self, j, row0, n):
        """The components of rows [row0, row0+n) of block j of a context filled by Model.sample_context -> (n,) int32, K =
        the prior component (lc_ctx_get_sample_labels; ValueError when the rows come from anywhere else)."""
        lab = np.zeros(n, dtype=np.int32)
        check(lib().lc_ctx_get_sample_labels(self._h, j, row0, n, lab.ctypes.data_as(C.POINTER(C.c_int32))))
        return lab

    def completed_draws(self):
        """The draws per row of the completed rows the context holds (lc_ctx_completed_draws); 0: none."""
        nd = C.c_int()
        check(lib().lc_ctx_completed_draws(self._h, C.byref(nd)))
        return nd.value

    def get_completed(self, j, row0, n, variance=False, draws=False):
        """Rows [row0, row0+n) of block j after the last Model.predict_incomplete_context on this context ->
        Completion(rows (n, D), logp (n,), count (n,), cols (n, HOLES_MAX)).  variance: CompletionVar, with var
        (n, HOLES_MAX) (lc_ctx_get_completed_var; ValueError when that call was made without variance=True).  draws: True,
        or the number of draws per row of that call -> CompletionDraws, with draws (n, m, HOLES_MAX) and label (n, m)
        (lc_ctx_get_completed_draws; ValueError when that call was made without draws)."""
        if variance and draws:
            raise ValueError("a completion holds its variance or draws, not both")
        D = self.dims()[1]
        rows, logp = np.zeros((n, D)), np.zeros(n)
        count, cols = np.zeros(n, dtype=np.int32), np.full((n, HOLES_MAX), -1, dtype=np.int32)
        c_int32_p = C.POINTER(C.c_int32)
        check(lib().lc_ctx_get_completed(self._h, j, row0, n, dptr(rows), D, dptr(logp), count.ctypes.data_as(c_int32_p),
                                         cols.ctypes.data_as(c_int32_p)))
        if draws:
            m = self.completed_draws()  # (the library's own count sizes the buffers)
            if m < 1:
                raise ValueError("the context holds no draws of completed rows (lc_model_predict_incomplete_draws)")
            if draws is not True and int(draws) != m:
                raise ValueError(f"the context's completed rows have {m} draws per row, not {int(draws)}")
            dr, lab = np.zeros((n, m, HOLES_MAX)), np.zeros((n, m), dtype=np.int32)
            check(lib().lc_ctx_get_completed_draws(self._h, j, row0, n, dptr(dr), lab.ctypes.data_as(c_int32_p)))
            return CompletionDraws(rows, logp, count, cols, dr, lab)
        if not variance:
            return Completion(rows, logp, count, cols)
        var = np.zeros((n, HOLES_MAX))
        check(lib().lc_ctx_get_completed_var(self._h, j, row0, n, dptr(var), HOLES_MAX))
        return CompletionVar(rows, logp, count, cols, var)

    def get_leave_one_out(self, j, row0, n, variance=False):
        """Rows [row0, row0+n) of block j after the last Model.explain_context on this context -> LeaveOneOut(logp (n,),
        cond_logp (n, D), mean (n, D), worst (n,)) (lc_ctx_get_leave_one_out).  variance: LeaveOneOutVar, with var (n, D)
        (ValueError when that call was made without variance=True)."""
        D = self.dims()[1]
        logp, cond, mean = np.zeros(n), np.zeros((n, D)), np.zeros((n, D))
        var = np.zeros((n, D)) if variance else None
        worst = np.zeros(n, dtype=np.int32)
        check(lib().lc_ctx_get_leave_one_out(self._h, j, row0, n, dptr(logp), dptr(cond), dptr(mean),
                                             dptr(var) if variance else None, D, worst.ctypes.data_as(C.POINTER(C.c_int32))))
        return LeaveOneOutVar(logp, cond, mean, var, worst) if variance else LeaveOneOut(logp, cond, mean, worst)

    def top_rows(self, m, by="qz", largest=True, ncols=None, by_label=False):
        """TopRows of the m best rows (1 ... 64) of each column, ranked on the device (lc_ctx_top_rows): by="qz" the first
        ncols columns of qZ (None: all), by="logz" / "logp" the per-row outputs of the last prediction on this context
        (one column).  Ties go to the earlier row; NaN scores and pad rows are never selected.  by_label: column c only
        sees the rows the last prediction labelled c."""
        what = {"qz": RANK_QZ, "logz": RANK_LOGZ, "logp": RANK_LOGP}.get(by)
        if what is None:
            raise ValueError("by must be 'qz', 'logz' or 'logp'")
        if what != RANK_QZ:
            ncols = 1
        elif ncols is None:
            ncols = self.dims()[3]
        return _top_rows_call(lambda *out: lib().lc_ctx_top_rows(self._h, what, int(ncols), int(m), int(bool(largest)),
                                                                 int(bool(by_label)), *out), int(ncols), int(m))

    def _score_columns(self, by, ncols):
        what = {"qz": RANK_QZ, "logz": RANK_LOGZ, "logp": RANK_LOGP}.get(by)
        if what is None:
            raise ValueError("by must be 'qz', 'logz' or 'logp'")
        if what != RANK_QZ:
            ncols = 1
        elif ncols is None:
            ncols = self.dims()[3]
        return what, int(ncols)

    def score_quantiles(self, probs, by="logp", ncols=None, by_label=False):
        """ScoreQuantiles of each column at the probabilities probs (1 ... QUANTILES_MAX values in [0, 1], any order),
        selected on the device (lc_ctx_score_quantiles): the columns, by_label and the rows that take part as top_rows;
        the quantile is numpy's method="inverted_cdf" in the order -inf < ... < -0.0 < +0.0 < ... < +inf."""
        what, ncols = self._score_columns(by, ncols)
        p = np.ascontiguousarray(np.atleast_1d(probs), dtype=np.float64).reshape(-1)
        shape = (max(ncols, 0), min(p.size, QUANTILES_MAX))  # (out-of-range arguments are the library's to refuse)
        count = np.zeros(shape[0], dtype=np.int64)
        rank, value = np.full(shape, -1, dtype=np.int64), np.full(shape, np.nan)
        check(lib().lc_ctx_score_quantiles(self._h, what, ncols, int(bool(by_label)), dptr(p), p.size,
                                           count.ctypes.data_as(c_int64_p), rank.ctypes.data_as(c_int64_p), dptr(value)))
        return ScoreQuantiles(count, rank, value)

    def score_counts(self, thresholds, by="logp", ncols=None, by_label=False):
        """ScoreCounts of each column at 1 ... QUANTILES_MAX thresholds (+-inf allowed), counted on the device
        (lc_ctx_score_counts): how many participating scores are <= each threshold."""
        what, ncols = self._score_columns(by, ncols)
        t = np.ascontiguousarray(np.atleast_1d(thresholds), dtype=np.float64).reshape(-1)
        shape = (max(ncols, 0), min(t.size, QUANTILES_MAX))
        count, atmost = np.zeros(shape[0], dtype=np.int64), np.zeros(shape, dtype=np.int64)
        check(lib().lc_ctx_score_counts(self._h, what, ncols, int(bool(by_label)), dptr(t), t.size,
                                        count.ctypes.data_as(c_int64_p), atmost.ctypes.data_as(c_int64_p)))
        return ScoreCounts(count, atmost)

    def rows_beyond(self, threshold, by="logp", col=0, above=False, by_label=False, limit=1 << 20, ncols=None):
        """FlaggedRows of ONE column: every participating row with score <= threshold (above: >=), in context order,
        compacted on the device (lc_ctx_rows_beyond).  total counts them all; at most limit of them are returned."""
        what, ncols = self._score_columns(by, ncols)
        cap = max(int(limit), 0)
        group, row, score = np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.int64), np.empty(cap)
        total = C.c_int64(0)
        check(lib().lc_ctx_rows_beyond(self._h, what, ncols, int(col), int(bool(by_label)), float(threshold), int(bool(above)),
                                       int(limit), C.byref(total), group.ctypes.data_as(C.POINTER(C.c_int32)),
                                       row.ctypes.data_as(c_int64_p), dptr(score)))
        n = min(total.value, cap)
        return FlaggedRows(total.value, group[:n].copy(), row[:n].copy(), score[:n].copy())

    def get_doc_predictions(self, doc0, n, T):
        """Documents [doc0, doc0+n) of the last TopicModel.predict_context on this context -> (qY (n, T), label_t int32,
        Fyz, Fz, sweeps int32)."""
        qY, lt, sw = np.zeros((n, T)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        Fyz, Fz = np.zeros(n), np.zeros(n)
        check(lib().lc_ctx_get_doc_predictions(self._h, doc0, n, dptr(qY), lt.ctypes.data_as(C.POINTER(C.c_int32)),
                                               dptr(Fyz), dptr(Fz), sw.ctypes.data_as(C.POINTER(C.c_int32))))
        return qY, lt, Fyz, Fz, sw

    def synchronize(self):
        check(lib().lc_ctx_synchronize(self._h))

    def vbem(self, wkind, wprior=1.0, clusterprior=1.0, maxit=-1, sparse=False, fixed_iters=-1, verbose=False,
             nthreads=1, model=None, ntrace=4096, ckind=C_GAUSSWISH):
        mh = model._h if model is not None else C.c_void_p()
        F, nit = C.c_double(), C.c_int()
        tr = np.zeros(ntrace)
        check(lib().lc_vbem(self._h, C.byref(mh), wkind, ckind, wprior, clusterprior, maxit, int(sparse), fixed_iters,
                            int(verbose), nthreads, C.byref(F), C.byref(nit), dptr(tr), ntrace))
        if model is None:
            model = Model(mh, ctx=self)
        return F.value, tr[: nit.value].copy(), model


    def prune(self, model, verbose=False):
        """prune_clusters (cluster.cpp:505-552) on `model` and this context's qZ -> number of clusters removed."""
        n = C.c_int()
        check(lib().lc_prune(self._h, model._h, int(verbose), C.byref(n)))
        return n.value

    def cluster(self, wkind, wprior=1.0, clusterprior=1.0, maxclusters=-1, sparse=False, verbose=False, nthreads=1,
                ckind=C_GAUSSWISH):
        """cluster() (model selection) on the data resident in this context -> (F, Model)."""
        mh, F = C.c_void_p(), C.c_double()
        check(lib().lc_cluster(self._h, wkind, ckind, wprior, clusterprior, maxclusters, int(sparse), int(verbose),
                               nthreads, C.byref(mh), C.byref(F)))
        return F.value, Model(mh, ctx=self)


class Model:
    """lc_model: weights + clusters (+ access to the context's qZ)."""

    def __init__(self, handle, ctx=None):
        self._h = handle
        self._ctx = ctx  # keep a borrowed context alive
        self._torch_device = None  # learn() on device tensors: where qZ is handed out (qz_all_device), and the context is ours

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lc_model_free(self._h)
            self._h = C.c_void_p()
            if getattr(self, "_torch_device", None) is not None and self._ctx is not None:
                self._ctx.close()  # (the context learn() made for the tensors: nobody else holds it)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dims(self):
        J, K, D = C.c_int(), C.c_int(), C.c_int()
        check(lib().lc_model_dims(self._h, C.byref(J), C.byref(K), C.byref(D)))
        return J.value, K.value, D.value

    def rounds(self):
        n = C.c_int()
        check(lib().lc_model_rounds(self._h, C.byref(n)))
        out = []
        for r in range(n.value):
            K, ni = C.c_int(), C.c_int()
            check(lib().lc_model_round(self._h, r, C.byref(K), C.byref(ni), None, 0))
            F = np.zeros(ni.value)
            check(lib().lc_model_round(self._h, r, None, None, dptr(F), ni.value))
            out.append((K.value, F.tolist()))
        return out

    def qz_all(self, rows):
        """All groups with one transfer -> list of (N_j, K) views."""
        _, K, _ = self.dims()
        allq = np.zeros((int(sum(rows)), K))
        if allq.size:
            check(lib().lc_model_get_qz_all(self._h, dptr(allq)))
        return [allq[o - n:o] for n, o in zip(rows, np.cumsum(rows))]

    def qz_all_device(self, rows):
        """A model learned from device tensors: every group's qZ as a row-major (N_j, K) torch.float64 tensor on the
        tensors' device, written there by the device (no host staging)."""
        out = [self._ctx.get_qz_rows_device(j, 0, n, self._torch_device) for j, n in enumerate(rows)]
        self._ctx.synchronize()  # (any stream may read them)
        return out

    def qz(self, j, n):
        _, K, _ = self.dims()
        q = np.empty((n, K))
        if n:
            check(lib().lc_model_get_qz(self._h, j, dptr(q), K, 1))
        return q

    def weights(self, j):
        _, K, _ = self.dims()
        e, n = np.zeros(K), np.zeros(K)
        check(lib().lc_model_weights(self._h, j, dptr(e), dptr(n)))
        return e, n

    def kinds(self):
        w, c = C.c_int(), C.c_int()
        check(lib().lc_model_kinds(self._h, C.byref(w), C.byref(c)))
        return w.value, c.value

    def cluster(self, k):
        """Posterior of cluster k.  GaussWish: mean, cov (D x D), nu, beta, iW, logdW.  NormGamma: mean, cov (D,
        = L*nu as the reference's getcov), nu, beta, L, logL.  ExpGamma: rate (= a*ib), a, ib, logb."""
        _, _, D = self.dims()
        ck = self.kinds()[1]
        N, nu, beta, logdW = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        if ck == C_GAUSSWISH:
            mean, cov, iW = np.zeros(D), np.zeros((D, D)), np.zeros((D, D))
        else:
            mean, cov, iW = np.zeros(D), (np.zeros(D) if ck == C_NORMGAMMA else None), np.zeros(D)
        check(lib().lc_model_cluster(self._h, k, C.byref(N), dptr(mean), dptr(cov), C.byref(nu), C.byref(beta),
                                     dptr(iW), C.byref(logdW)))
        if ck == C_GAUSSWISH:
            return {"N": N.value, "mean": mean, "cov": cov, "nu": nu.value, "beta": beta.value, "iW": iW,
                    "logdW": logdW.value}
        if ck == C_NORMGAMMA:
            return {"N": N.value, "mean": mean, "cov": cov, "nu": nu.value, "beta": beta.value, "L": iW,
                    "logL": logdW.value}
        return {"N": N.value, "rate": mean, "a": nu.value, "ib": iW, "logb": logdW.value}

    def fenergy(self):
        J, K, _ = self.dims()
        Fw, Fc = np.zeros(J), np.zeros(K)
        check(lib().lc_model_fenergy(self._h, dptr(Fw), dptr(Fc)))
        return Fw, Fc

    # -- prediction ----------------------------------------------------------------------------------
    def predict_context(self, ctx, groups=None, keep_qz=False):
        """Score the observations resident in ctx (lc_model_predict): block b with the weights of learned group
        groups[b] (None: 0).  Nothing is downloaded: read the rows with ctx.get_predictions / ctx.get_qz."""
        g = None
        if groups is not None:
            garr = np.ascontiguousarray(groups, dtype=np.int32)
            if garr.shape != (ctx.dims()[0],):
                raise ValueError("groups needs one learned group index per block of the context")
            g = garr.ctypes.data_as(C.POINTER(C.c_int))
        check(lib().lc_model_predict(self._h, ctx._h, g, int(keep_qz)))

    def predict(self, X, groups=None, qz=False, device=None):
        """Prediction(label, logZ, logp, qZ) for the host rows X ((N, D) array), or a list of them for a list of
        blocks (block b scored with learned group groups[b], default 0).  qZ is None unless qz=True.
        X may also be a 2-D CUDA torch.float64 tensor or a list of them (device_blocks): the rows are read where they are,
        on torch's current stream of their device, and label (int32), logZ, logp and qZ come back as torch tensors on that
        device, ready for any stream."""
        blocks = isinstance(X, (list, tuple))
        Xd = device_blocks(X)
        if Xd is not None:
            tdev = Xd[0].device
            if device is not None and device != tdev.index:
                raise ValueError(f"device={device}, but X lives on device {tdev.index}")
            with Context(tdev.index, _torch_stream(tdev)) as ctx:
                ctx.set_data(Xd)
                self.predict_context(ctx, groups, keep_qz=qz)
                out = [Prediction(*ctx.get_predictions_device(j, 0, x.shape[0], tdev=tdev),
                                  ctx.get_qz_rows_device(j, 0, x.shape[0], tdev) if qz else None) for j, x in enumerate(Xd)]
                ctx.synchronize()
            return out if blocks else out[0]
        device = 0 if device is None else device
        Xs = list(X) if blocks else [X]
        Xs = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, self.dims()[2])) for x in Xs]
        with Context(device) as ctx:
            ctx.set_data(Xs)
            self.predict_context(ctx, groups, keep_qz=qz)
            rows = [x.shape[0] for x in Xs]
            qs = ctx.get_qz(rows) if qz else [None] * len(Xs)
            out = [Prediction(*ctx.get_predictions(j, 0, n), None if q is None else q.copy())
                   for j, (n, q) in enumerate(zip(rows, qs))]
        return out if blocks else out[0]

    # -- conditional prediction ------------------------------------------------------------------------
    def _targets(self, given, target):
        if target is not None:
            return [int(t) for t in target]
        gs = set(int(g) for g in given)
        return [c for c in range(self.dims()[2]) if c not in gs]

    def predict_conditional_context(self, ctx, given, target=None, groups=None, variance=False, draws=None, seed=0):
        """E[x_target | x_given] and log p(x_given) of the rows resident in ctx, whose column i is model column
        given[i] (lc_model_predict_conditional).  target None: every model column that is not given, ascending.
        variance: also the predictive variance of every target column (lc_model_predict_conditional_var; DomainError
        where it does not exist: a component with weight and nu + 1 - D + len(given) <= 2).
        draws = m (1 ... DRAWS_MAX): also m draws per row of the target columns from p(x_target | x_given, training data)
        (lc_model_predict_conditional_draws; a draw depends on seed, block, row, its index and the row's values only).
        Nothing is downloaded: read the rows with ctx.get_conditional.  Returns the number of target columns."""
        if draws is not None and variance:
            raise ValueError("draws and variance are separate calls: ask for one of them")
        g = None
        if groups is not None:
            garr = np.ascontiguousarray(groups, dtype=np.int32)
            if garr.shape != (ctx.dims()[0],):
                raise ValueError("groups needs one learned group index per block of the context")
            g = garr.ctypes.data_as(c_int_p)
        gv = np.ascontiguousarray(given, dtype=np.int32).reshape(-1)
        tv = None if target is None else np.ascontiguousarray(target, dtype=np.int32).reshape(-1)
        args = (self._h, ctx._h, g, gv.ctypes.data_as(c_int_p), gv.size,
                None if tv is None else tv.ctypes.data_as(c_int_p), 0 if tv is None else tv.size)
        if draws is not None:
            m = int(draws)
            if m < 1 or m > DRAWS_MAX:
                raise ValueError(f"draws must be in 1 ... {DRAWS_MAX}")
            check(lib().lc_model_predict_conditional_draws(*args, m, int(seed)))
        else:
            call = lib().lc_model_predict_conditional_var if variance else lib().lc_model_predict_conditional
            check(call(*args))
        return len(self._targets(gv, tv))

    def predict_conditional(self, Xa, given, target=None, groups=None, device=0, variance=False, draws=None, seed=0):
        """Conditional(mean, logp) for the host rows Xa ((N, len(given)) array: the known columns, in the order of
        given), or a list of them for a list of blocks (block b mixed with learned group groups[b], default 0).
        variance: ConditionalVar(mean, logp, var) with the predictive variance of every target column.
        draws = m: ConditionalDraws(mean, logp, draws (N, m, ntarget), label (N, m)): m draws per row from
        p(x_target | x_given, training data), the same bits for the same seed."""
        if draws is not None and variance:
            raise ValueError("draws and variance are separate calls: ask for one of them")
        blocks = isinstance(Xa, (list, tuple))
        Xs = list(Xa) if blocks else [Xa]
        Da = len(given)
        Xs = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, max(Da, 1))) for x in Xs]
        with Context(device) as ctx:
            ctx.set_data(Xs)
            nt = self.predict_conditional_context(ctx, given, target, groups, variance, draws, seed)
            out = [ctx.get_conditional(j, 0, x.shape[0], nt, variance, draws if draws is not None else False)
                   for j, x in enumerate(Xs)]
        return out if blocks else out[0]

    def impute(self, X, missing=None, groups=None, device=0, return_var=False, draws=None, seed=0):
        """A copy of the full-width rows X ((N, D) array or a list of blocks) with the columns `missing` replaced by
        their conditional mean given the other columns (predict_conditional).  What X holds in the missing columns is
        not looked at (NaN is fine).
        missing None: the NaNs of X say what is missing, every row with its own set (predict_incomplete, up to HOLES_MAX
        per row): the filled copy, or with draws = m the list of m completed copies, copy i with draw i in every hole;
        return_var is not offered there (predict_incomplete(variance=True) gives the variance by slot).
        return_var: (filled, var) with var (N, len(missing)) the predictive variance of the values filled in, in the
        order of `missing` (lists of each for a list of blocks).
        draws = m: multiple imputation -- a list of m completed copies, copy i filled with draw i of every row from
        p(x_missing | x_known, training data) (a list per block for a list of blocks)."""
        if draws is not None and return_var:
            raise ValueError("draws and return_var are separate calls: ask for one of them")
        blocks = isinstance(X, (list, tuple))
        if missing is None:
            if return_var:
                raise ValueError("return_var needs the columns `missing`: predict_incomplete(variance=True) gives the "
                                 "variance of the values filled into NaNs")
            res = self.predict_incomplete(list(X) if blocks else [X], groups, device, draws=draws, seed=seed)
            if draws is None:
                out = [r.rows for r in res]
            else:
                out = []
                for r in res:
                    copies = []
                    ri, si = np.nonzero(r.cols >= 0)
                    for i in range(int(draws)):
                        c = r.rows.copy()
                        c[ri, r.cols[ri, si]] = r.draws[ri, i, si]
                        copies.append(c)
                    out.append(copies)
            return out if blocks else out[0]
        D = self.dims()[2]
        Xs = [np.array(np.asarray(x, dtype=np.float64).reshape(-1, D)) for x in (X if blocks else [X])]
        miss = [int(c) for c in missing]
        given = [c for c in range(D) if c not in set(miss)]
        if draws is not None:
            res = self.predict_conditional([x[:, given] for x in Xs], given, miss, groups, device, draws=draws, seed=seed)
            out = []
            for x, r in zip(Xs, res):
                copies = []
                for i in range(int(draws)):
                    c = x.copy()
                    c[:, miss] = r.draws[:, i, :]
                    copies.append(c)
                out.append(copies)
            return out if blocks else out[0]
        res = self.predict_conditional([x[:, given] for x in Xs], given, miss, groups, device, variance=return_var)
        for x, r in zip(Xs, res):
            x[:, miss] = r.mean
        if not return_var:
            return Xs if blocks else Xs[0]
        var = [r.var for r in res]
        return (Xs, var) if blocks else (Xs[0], var[0])

    # -- new rows --------------------------------------------------------------------------------------
    def sample_context(self, ctx, counts, groups=None, seed=0, row_offset=0):
        """Fill ctx with len(counts) blocks of counts[b] new rows, each a draw from the density predict() scores as logp:
        block b with the weights of learned group groups[b] (None: 0) (lc_model_sample).  Whatever ctx held is replaced;
        read the rows with ctx.get_rows, their components with ctx.get_sample_labels, or score them with any predict
        call.  Rows [a, b) of a call with row_offset 0 are the rows of a call for b - a rows with row_offset = a."""
        Nj = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
        g = None
        if groups is not None:
            garr = np.ascontiguousarray(groups, dtype=np.int32)
            if garr.shape != (Nj.size,):
                raise ValueError("groups needs one learned group index per block")
            g = garr.ctypes.data_as(c_int_p)
        check(lib().lc_model_sample(self._h, ctx._h, Nj.size, Nj.ctypes.data_as(c_int64_p), g, int(seed), int(row_offset)))

    def sample(self, n, seed=0, groups=None, device=0):
        """Sample(rows (n, D), label (n,)): n new rows from the model (group 0, or groups), and the component each came
        from.  A list of counts gives a list of Samples, block b drawn with learned group groups[b]."""
        blocks = isinstance(n, (list, tuple, np.ndarray))
        counts = [int(c) for c in n] if blocks else [int(n)]
        if groups is not None and not blocks:
            groups = [int(np.asarray(groups).reshape(-1)[0])]
        D = self.dims()[2]
        with Context(device) as ctx:
            self.sample_context(ctx, counts, groups, seed)
            out = []
            for j, c in enumerate(counts):
                rows = np.zeros((c, D))
                if c:
                    check(lib().lc_ctx_get_rows(ctx._h, j, 0, c, dptr(rows)))
                out.append(Sample(rows, ctx.get_sample_labels(j, 0, c)))
        return out if blocks else out[0]

    # -- rows with holes -------------------------------------------------------------------------------
    def predict_incomplete_context(self, ctx, groups=None, variance=False, draws=None, seed=0):
        """Complete the full-width rows resident in ctx in place: every NaN (up to HOLES_MAX per row, every row its own
        set) becomes E[x_unknown | x_known, training data] (lc_model_predict_incomplete).  Nothing is downloaded: read
        the rows with ctx.get_completed.  A second call on the same context finds no NaN any more.
        variance: also the predictive variance of every filled value (lc_model_predict_incomplete_var; DomainError, with
        the NaNs left in place, where it does not exist); read it with ctx.get_completed(..., variance=True).
        draws = m (1 ... DRAWS_MAX): also m draws per row of its unknown values from p(x_unknown | x_known, training
        data) (lc_model_predict_incomplete_draws; a draw depends on seed, block, row, its index and the row's values only;
        no moment has to exist); read them with ctx.get_completed(..., draws=m).  The context's rows hold the means."""
        if draws is not None and variance:
            raise ValueError("draws and variance are separate calls: ask for one of them")
        g = None
        if groups is not None:
            garr = np.ascontiguousarray(groups, dtype=np.int32)
            if garr.shape != (ctx.dims()[0],):
                raise ValueError("groups needs one learned group index per block of the context")
            g = garr.ctypes.data_as(c_int_p)
        if draws is not None:
            m = int(draws)
            if m < 1 or m > DRAWS_MAX:
                raise ValueError(f"draws must be in 1 ... {DRAWS_MAX}")
            check(lib().lc_model_predict_incomplete_draws(self._h, ctx._h, g, m, int(seed)))
            return
        fn = lib().lc_model_predict_incomplete_var if variance else lib().lc_model_predict_incomplete
        check(fn(self._h, ctx._h, g))

    def predict_incomplete(self, X, groups=None, device=0, variance=False, draws=None, seed=0):
        """Completion(rows, logp, count, cols) for the host rows X ((N, D) array, NaN = unknown), or a list of them for a
        list of blocks (block b mixed with learned group groups[b], default 0).  rows is a filled copy: X keeps its NaNs.
        variance: CompletionVar, with var (N, HOLES_MAX) the predictive variance of the filled values.
        draws = m: CompletionDraws(rows, logp, count, cols, draws (N, m, HOLES_MAX), label (N, m)): m draws per row of its
        unknown values, the same bits for the same seed; rows holds the means."""
        if draws is not None and variance:
            raise ValueError("draws and variance are separate calls: ask for one of them")
        blocks = isinstance(X, (list, tuple))
        Xs = self._blocks(X)
        if not Xs:
            return []
        with Context(device) as ctx:
            ctx.set_data(Xs)
            self.predict_incomplete_context(ctx, groups, variance, draws, seed)
            out = [ctx.get_completed(j, 0, x.shape[0], variance, draws if draws is not None else False)
                   for j, x in enumerate(Xs)]
        return out if blocks else out[0]

    # -- leave-one-out conditionals -------------------------------------------------------------------
    def explain_context(self, ctx, groups=None, variance=False):
        """Score every column of the complete full-width rows resident in ctx given the row's other columns
        (lc_model_predict_leave_one_out).  Nothing is downloaded and the rows keep every bit: read the results with
        ctx.get_leave_one_out.  ValueError for a row that holds a NaN (predict_incomplete takes those).  variance: also
        Var[x_d | x_-d] (DomainError where a component with weight has nu <= 2)."""
        g = None
        if groups is not None:
            garr = np.ascontiguousarray(groups, dtype=np.int32)
            if garr.shape != (ctx.dims()[0],):
                raise ValueError("groups needs one learned group index per block of the context")
            g = garr.ctypes.data_as(c_int_p)
        check(lib().lc_model_predict_leave_one_out(self._h, ctx._h, g, 1 if variance else 0))

    def explain(self, X, groups=None, device=0, variance=False):
        """LeaveOneOut(logp, cond_logp, mean, worst) for the complete host rows X ((N, D) array), or a list of them for a
        list of blocks (block b mixed with learned group groups[b], default 0): which value of a row disagrees with the
        row's other values.  variance: LeaveOneOutVar, with var (N, D)."""
        blocks = isinstance(X, (list, tuple))
        Xs = self._blocks(X)
        if not Xs:
            return []
        with Context(device) as ctx:
            ctx.set_data(Xs)
            self.explain_context(ctx, groups, variance)
            out = [ctx.get_leave_one_out(j, 0, x.shape[0], variance) for j, x in enumerate(Xs)]
        return out if blocks else out[0]

    # -- ranking -------------------------------------------------------------------------------------
    def _blocks(self, X):
        blocks = isinstance(X, (list, tuple))
        Xs = list(X) if blocks else [X]
        return [np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, self.dims()[2])) for x in Xs]

    def exemplars_context(self, ctx, m=10, groups=None):
        """TopRows with one column per cluster: the m rows of ctx labelled k with the largest Eloglike_k(x) (for
        Gauss-Wishart clusters: the smallest expected Mahalanobis distance), score = Eloglike_k(x)
        (lc_model_exemplars).  Runs predict_context(ctx, groups) first: the context's prediction is replaced."""
        g = None
        if groups is not None:
            garr = np.ascontiguousarray(groups, dtype=np.int32)
            if garr.shape != (ctx.dims()[0],):
                raise ValueError("groups needs one learned group index per block of the context")
            g = garr.ctypes.data_as(C.POINTER(C.c_int))
        return _top_rows_call(lambda *out: lib().lc_model_exemplars(self._h, ctx._h, g, int(m), *out), self.dims()[1], int(m))

    def exemplars(self, X, m=10, groups=None, device=0):
        """exemplars_context for the host rows X ((N, D) array or a list of blocks, as predict takes): group is the
        block index, row the row of that block."""
        with Context(device) as ctx:
            ctx.set_data(self._blocks(X))
            return self.exemplars_context(ctx, m, groups)

    def outliers(self, X, m=10, groups=None, device=0):
        """TopRows (one column) of the m rows of X the model finds least likely: the smallest logp of predict."""
        with Context(device) as ctx:
            ctx.set_data(self._blocks(X))
            self.predict_context(ctx, groups)
            return ctx.top_rows(m, by="logp", largest=False)

    def logp_quantiles(self, X, probs, groups=None, device=0):
        """ScoreQuantiles (one column) of the logp of predict over all rows of X, selected on the device."""
        with Context(device) as ctx:
            ctx.set_data(self._blocks(X))
            self.predict_context(ctx, groups)
            return ctx.score_quantiles(probs, by="logp")

    def flag(self, X, threshold, groups=None, device=0, limit=1 << 20):
        """FlaggedRows of the rows of X with logp <= threshold, in the order of X: the detector next to logp_quantiles."""
        with Context(device) as ctx:
            ctx.set_data(self._blocks(X))
            self.predict_context(ctx, groups)
            return ctx.rows_beyond(threshold, by="logp", limit=limit)

    def release_data(self):
        """Free the training observations and qZ; the parameters (and predict) stay."""
        check(lib().lc_model_release_data(self._h))


def _learn_device(algo, Xd, wprior, clusterprior, maxclusters, sparse, verbose, nthreads, device, wprior_j):
    """learn() for device tensors: a context on the tensors' device and torch's current stream of it takes
    the rows where they are, lc_learn_ctx learns on it.  The model keeps the context (its qZ: Model.qz_all_device)."""
    tdev = Xd[0].device
    if device is not None and device != tdev.index:
        raise ValueError(f"device={device}, but X lives on device {tdev.index}")
    J = len(Xd)
    wj = None
    if wprior_j is not None:
        wj = np.ascontiguousarray(wprior_j, dtype=np.float64)
        if wj.shape != (J,):
            raise ValueError("wprior_j needs one value per group")
    ctx = Context(tdev.index, _torch_stream(tdev))
    try:
        ctx.set_data(Xd)
        mh, F = C.c_void_p(), C.c_double()
        check(lib().lc_learn_ctx(algo, ctx._h, wprior, dptr(wj), clusterprior, maxclusters, int(sparse), int(verbose),
                                 nthreads, C.byref(mh), C.byref(F)))
    except BaseException:
        ctx.close()
        raise
    m = Model(mh, ctx=ctx)
    m._torch_device = tdev
    return F.value, m, [x.shape[0] for x in Xd]


def learn(algo, X, wprior=1.0, clusterprior=1.0, maxclusters=-1, sparse=False, verbose=False, nthreads=1, device=None,
          wprior_j=None):
    """wprior_j: one weight prior per group (the priors the caller's weight objects carry into the multi-group
    learners: learnSGMC's Dirichlet alphas); None = defaults.  device: None = GPU 0 for host data, the tensors' own
    device for CUDA torch.float64 tensors (device_blocks), which are read where they are."""
    Xd = device_blocks(X)
    if Xd is not None:
        return _learn_device(algo, Xd, wprior, clusterprior, maxclusters, sparse, verbose, nthreads, device, wprior_j)
    device = 0 if device is None else device
    Xs = [X] if isinstance(X, np.ndarray) else list(X)
    Xs = [np.ascontiguousarray(x, dtype=np.float64) for x in Xs]
    J, D = len(Xs), Xs[0].shape[1]
    ptrs = (c_double_p * J)(*[dptr(x) for x in Xs])
    Nj = (C.c_int64 * J)(*[x.shape[0] for x in Xs])
    mh, F = C.c_void_p(), C.c_double()
    wj = None
    if wprior_j is not None:
        wj = np.ascontiguousarray(wprior_j, dtype=np.float64)
        if wj.shape != (J,):
            raise ValueError("wprior_j needs one value per group")
    check(lib().lc_learn_w(algo, J, ptrs, Nj, D, D, 1, wprior, dptr(wj), clusterprior, maxclusters, int(sparse),
                           int(verbose), nthreads, device, C.byref(mh), C.byref(F)))
    return F.value, Model(mh), [x.shape[0] for x in Xs]


def trim_cache():
    """Return every cached device / page-locked block to the driver."""
    check(lib().lc_trim_cache())


def weights_predictive(wkind, Nk, wprior=1.0):
    """E[pi_k] of the weights updated with Nk, and the mass beyond the truncation (StickBreak; 0 otherwise)."""
    Nk = np.ascontiguousarray(Nk, dtype=np.float64)
    e, r = np.zeros(Nk.size), C.c_double()
    check(lib().lc_weights_predictive(wkind, wprior, dptr(Nk), Nk.size, dptr(e), C.byref(r)))
    return e, r.value


def weights_update(wkind, Nk, wprior=1.0):
    Nk = np.ascontiguousarray(Nk, dtype=np.float64)
    e, f = np.zeros(Nk.size), C.c_double()
    check(lib().lc_weights_update(wkind, wprior, dptr(Nk), Nk.size, dptr(e), C.byref(f)))
    return e, f.value


def gw_mstep(clustwidth, Ns, xs, xxs):
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    xxs = np.ascontiguousarray(xxs, dtype=np.float64)
    D = xs.size
    nu, beta, logdW, fe, cst = (C.c_double() for _ in range(5))
    m, iW, A = np.zeros(D), np.zeros((D, D)), np.zeros((D, D))
    check(lib().lc_gw_mstep(clustwidth, D, Ns, dptr(xs), dptr(xxs), C.byref(nu), C.byref(beta), dptr(m), dptr(iW),
                            C.byref(logdW), C.byref(fe), dptr(A), C.byref(cst)))
    return {"nu": nu.value, "beta": beta.value, "m": m, "iW": iW, "logdW": logdW.value, "fenergy": fe.value,
            "A": A, "eloglike_const": cst.value}


def gw_conditional(nu, beta, m, iW, given, target=None):
    """The per-cluster tables of the conditional prediction (lc_gw_conditional) from one Gauss-Wishart posterior:
    A (whitener of the given columns), ma, B (= iW_ba iW_aa^-1), mb, G, s, e and the target list."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    iW = np.ascontiguousarray(iW, dtype=np.float64)
    D = m.size
    gv = np.ascontiguousarray(given, dtype=np.int32).reshape(-1)
    tv = None if target is None else np.ascontiguousarray(target, dtype=np.int32).reshape(-1)
    tg = [int(t) for t in tv] if tv is not None else [c for c in range(D) if c not in set(int(g) for g in gv)]
    Da, Db = gv.size, len(tg)
    A, ma, B, mb = np.zeros((Da, Da)), np.zeros(Da), np.zeros((Db, Da)), np.zeros(Db)
    G, s, e = (C.c_double() for _ in range(3))
    check(lib().lc_gw_conditional(D, nu, beta, dptr(m), dptr(iW), gv.ctypes.data_as(c_int_p), Da,
                                  None if tv is None else tv.ctypes.data_as(c_int_p), 0 if tv is None else tv.size,
                                  dptr(A), dptr(ma), dptr(B), dptr(mb), C.byref(G), C.byref(s), C.byref(e)))
    return {"A": A, "ma": ma, "B": B, "mb": mb, "G": G.value, "s": s.value, "e": e.value, "target": tg}


def gw_conditional_var(nu, beta, iW, given, target=None):
    """The tables of the conditional variance (lc_gw_conditional_var) from one Gauss-Wishart posterior -> (S, g): S the
    diagonal of iW_bb - iW_ba iW_aa^-1 iW_ab in the order of target (None: the columns not given, ascending), g =
    (1 + beta) / (beta (nu + 1 - D + len(given) - 2)).  DomainError where the variance does not exist."""
    iW = np.ascontiguousarray(iW, dtype=np.float64)
    D = iW.shape[0]
    gv = np.ascontiguousarray(given, dtype=np.int32).reshape(-1)
    tv = None if target is None else np.ascontiguousarray(target, dtype=np.int32).reshape(-1)
    Db = tv.size if tv is not None else len([c for c in range(D) if c not in set(int(g) for g in gv)])
    S, g = np.zeros(Db), C.c_double()
    check(lib().lc_gw_conditional_var(D, nu, beta, dptr(iW), gv.ctypes.data_as(c_int_p), gv.size,
                                      None if tv is None else tv.ctypes.data_as(c_int_p), 0 if tv is None else tv.size,
                                      dptr(S), C.byref(g)))
    return S, g.value


def gw_conditional_cov(nu, beta, iW, given, target=None):
    """The scale matrix of the conditional Student-t behind the draws (lc_gw_conditional_cov) from one Gauss-Wishart
    posterior -> (S, L): S = iW_bb - iW_ba iW_aa^-1 iW_ab (ntarget x ntarget, in the order of target; None: the columns
    not given, ascending) and L its lower Cholesky factor.  DomainError when S is not numerically positive definite."""
    iW = np.ascontiguousarray(iW, dtype=np.float64)
    D = iW.shape[0]
    gv = np.ascontiguousarray(given, dtype=np.int32).reshape(-1)
    tv = None if target is None else np.ascontiguousarray(target, dtype=np.int32).reshape(-1)
    Db = tv.size if tv is not None else len([c for c in range(D) if c not in set(int(g) for g in gv)])
    S, L = np.zeros((Db, Db)), np.zeros((Db, Db))
    check(lib().lc_gw_conditional_cov(D, nu, beta, dptr(iW), gv.ctypes.data_as(c_int_p), gv.size,
                                      None if tv is None else tv.ctypes.data_as(c_int_p), 0 if tv is None else tv.size,
                                      dptr(S), dptr(L)))
    return S, L


def gw_precision(nu, beta, m, iW):
    """The host table of the prediction of rows with holes (lc_gw_precision) from one Gauss-Wishart posterior:
    P (D, D) = nu iW^-1, G and e (HOLES_MAX + 1 values: one per hole count), s."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    iW = np.ascontiguousarray(iW, dtype=np.float64)
    D = m.size
    P, G, e, s = np.zeros((D, D)), np.zeros(HOLES_MAX + 1), np.zeros(HOLES_MAX + 1), C.c_double()
    check(lib().lc_gw_precision(D, nu, beta, dptr(m), dptr(iW), dptr(P), dptr(G), C.byref(s), dptr(e)))
    return {"P": P, "G": G, "s": s.value, "e": e}


def gw_precision_var(nu, beta, D):
    """The table of the variance of filled values (lc_gw_precision_var): g (HOLES_MAX + 1 values, one per hole count) =
    (1 + beta) / (beta (nu - 1 - nb)); NaN where nb >= D or the variance does not exist."""
    g = np.zeros(HOLES_MAX + 1)
    check(lib().lc_gw_precision_var(D, nu, beta, dptr(g)))
    return g


def ng_mstep(clustwidth, Ns, xs, xxs):
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    xxs = np.ascontiguousarray(xxs, dtype=np.float64)
    D = xs.size
    nu, beta, logL, fe, cst = (C.c_double() for _ in range(5))
    m, L = np.zeros(D), np.zeros(D)
    check(lib().lc_ng_mstep(clustwidth, D, Ns, dptr(xs), dptr(xxs), C.byref(nu), C.byref(beta), dptr(m), dptr(L),
                            C.byref(logL), C.byref(fe), C.byref(cst)))
    return {"nu": nu.value, "beta": beta.value, "m": m, "L": L, "logL": logL.value, "fenergy": fe.value,
            "eloglike_const": cst.value}


def eg_mstep(obsmag, Ns, xs):
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    D = xs.size
    a, logb, fe, cst = (C.c_double() for _ in range(4))
    ib = np.zeros(D)
    check(lib().lc_eg_mstep(obsmag, D, Ns, dptr(xs), C.byref(a), dptr(ib), C.byref(logb), C.byref(fe), C.byref(cst)))
    return {"a": a.value, "ib": ib, "logb": logb.value, "fenergy": fe.value, "eloglike_const": cst.value}


class TopicModel:
    """lc_tmodel: the result of learnSCM / learnMCM."""

    def __init__(self, handle, Ij, Nji):
        self._h = handle
        self.Ij = list(Ij)
        self.Nji = list(Nji)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lc_tmodel_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def dims(self):
        v = [C.c_int() for _ in range(6)]
        check(lib().lc_tmodel_dims(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("J", "Itot", "T", "K", "D", "Dt"), (x.value for x in v)))

    def qY(self):
        d = self.dims()
        out = []
        for j, I in enumerate(self.Ij):
            q = np.zeros((I, d["T"]))
            check(lib().lc_tmodel_get_qy(self._h, j, dptr(q)))
            out.append(q)
        return out

    def qZ(self):
        K = self.dims()["K"]
        allq = np.zeros((int(sum(self.Nji)), K))
        if allq.size:
            check(lib().lc_tmodel_get_qz_all(self._h, dptr(allq)))  # one transfer, then views per document
        out, doc, o = [], 0, 0
        for I in self.Ij:
            g = []
            for _ in range(I):
                g.append(allq[o:o + self.Nji[doc]])
                o += self.Nji[doc]
                doc += 1
            out.append(g)
        return out

    def weights(self, level, idx):
        d = self.dims()
        n = d["T"] if level == 0 else d["K"]
        e, nk = np.zeros(n), np.zeros(n)
        check(lib().lc_tmodel_weights(self._h, level, idx, dptr(e), dptr(nk)))
        return e, nk

    def cluster(self, level, idx):
        d = self.dims()
        D = d["D"] if level == 0 else d["Dt"]
        N, nu, beta, logdW, fe = (C.c_double() for _ in range(5))
        mean, cov, iW = np.zeros(D), np.zeros((D, D)), np.zeros((D, D))
        check(lib().lc_tmodel_cluster(self._h, level, idx, C.byref(N), dptr(mean), dptr(cov), C.byref(nu),
                                      C.byref(beta), dptr(iW), C.byref(logdW), C.byref(fe)))
        return {"N": N.value, "mean": mean, "cov": cov, "nu": nu.value, "beta": beta.value, "iW": iW,
                "logdW": logdW.value, "fenergy": fe.value}

    def rounds(self):
        n = C.c_int()
        check(lib().lc_tmodel_rounds(self._h, C.byref(n)))
        out = []
        for r in range(n.value):
            T, K, ni = C.c_int(), C.c_int(), C.c_int()
            check(lib().lc_tmodel_round(self._h, r, C.byref(T), C.byref(K), C.byref(ni), None, 0))
            F = np.zeros(ni.value)
            check(lib().lc_tmodel_round(self._h, r, None, None, None, dptr(F), ni.value))
            out.append((T.value, K.value, F.tolist()))
        return out

    # -- inference for new documents ---------------------------------------------------------------
    def predict_context(self, ctx, W=None, groups=None, max_sweeps=50, tol=None, keep_qz=False):
        """Infer the documents resident in ctx (lc_tmodel_predict; one block per document): document i with the weights
        of learned group groups[i] (None: 0) and, for an MCM model, its observation W[i].  tol: None = CONVERGE, < 0 =
        exactly max_sweeps sweeps.  Nothing is downloaded: read the results with ctx.get_doc_predictions /
        ctx.get_predictions / ctx.get_qz."""
        docs = ctx.dims()[0]
        g = w = None
        if groups is not None:
            garr = np.ascontiguousarray(groups, dtype=np.int32)
            if garr.shape != (docs,):
                raise ValueError("groups needs one learned group index per document of the context")
            g = garr.ctypes.data_as(C.POINTER(C.c_int))
        if W is not None:
            warr = np.ascontiguousarray(W, dtype=np.float64)
            if warr.ndim != 2 or warr.shape != (docs, self.dims()["Dt"]):
                raise ValueError("W and X need to have the same number of 'docs'!")
            w = dptr(warr)
        tol = float(lib().lc_const_converge()) if tol is None else float(tol)
        check(lib().lc_tmodel_predict(self._h, ctx._h, g, w, int(max_sweeps), tol, int(keep_qz)))

    def predict(self, X, W=None, groups=None, max_sweeps=50, tol=None, qz=False, device=0):
        """TopicPrediction for the documents X, a list of (N_i, D) arrays (W: (docs, Dt) for an MCM model)."""
        d = self.dims()
        Xs = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, d["D"])) for x in X]
        with Context(device) as ctx:
            ctx.set_data(Xs)
            self.predict_context(ctx, W, groups, max_sweeps, tol, keep_qz=qz)
            rows = [x.shape[0] for x in Xs]
            qY, lt, Fyz, Fz, sw = ctx.get_doc_predictions(0, len(Xs), d["T"])
            per = [ctx.get_predictions(i, 0, n, logp=False) for i, n in enumerate(rows)]
            qs = [q.copy() for q in ctx.get_qz(rows)] if qz else None
        return TopicPrediction(qY, lt, Fyz, Fz, sw, [p[0] for p in per], [p[1] for p in per], qs)

    def release_data(self):
        """Free the training documents, qY and qZ; the parameters (and predict) stay."""
        check(lib().lc_tmodel_release_data(self._h))


def learn_topic(X, W=None, qY0=None, prior_t=1.0, prior_k=1.0, maxT=100, maxK=-1, verbose=False, nthreads=1,
                device=0, allreduce=None, stream=None):
    """lc_learn_topic: X is a list (groups) of lists (documents) of (N_ji, D) arrays; W (MCM) a list of (I_j, Dt)
    arrays; qY0 an optional list of (I_j, maxT) initial assignments.  Returns (F, TopicModel).
    allreduce (one process per GPU, whole groups per rank): fn(device_ptr, count, stream) summing in place across
    ranks, e.g. libcluster_amd.dist.make_device_hook(device); stream: the HIP stream to work on."""
    Xs = [[np.ascontiguousarray(x, dtype=np.float64) for x in Xj] for Xj in X]
    J = len(Xs)
    docs = [x for Xj in Xs for x in Xj]
    if not docs:
        raise ValueError("need at least one document")
    D = docs[0].shape[1]
    for x in docs:
        if x.ndim != 2 or x.shape[1] != D:
            raise ValueError("X dimensions are inconsistent between documents!")
    Ij = (C.c_int * J)(*[len(Xj) for Xj in Xs])
    ptrs = (c_double_p * len(docs))(*[dptr(x) for x in docs])
    Nji = (C.c_int64 * len(docs))(*[x.shape[0] for x in docs])
    Wp, Dt, Ws = None, 0, None
    if W is not None:
        Ws = [np.ascontiguousarray(w, dtype=np.float64) for w in W]
        if len(Ws) != J:  # mcluster.cpp:548-549
            raise ValueError("W and X need to have the same number of groups!")
        for j in range(J):
            if Ws[j].shape[0] != len(Xs[j]):  # mcluster.cpp:553-555
                raise ValueError("W and X need to have the same number of 'docs'!")
        Dt = Ws[0].shape[1]
        Wp = (c_double_p * J)(*[dptr(w) for w in Ws])
    Qp, Qs = None, None
    if qY0 is not None:
        Qs = [np.ascontiguousarray(q, dtype=np.float64) for q in qY0]
        for j in range(J):
            if Qs[j].shape != (len(Xs[j]), maxT):
                raise ValueError("qY0[j] must be (I_j, maxT)")
        Qp = (c_double_p * J)(*[dptr(q) for q in Qs])
    mh, F = C.c_void_p(), C.c_double()
    cb = C.cast(None, ALLREDUCE_FN)
    if allreduce is not None:
        def tramp(user, buf, count, strm):
            try:
                allreduce(buf or 0, count, strm or 0)
                return 0
            except Exception:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        cb = ALLREDUCE_FN(tramp)
    check(lib().lc_learn_topic_dist(J, Ij, ptrs, Nji, D, D, 1, Wp, Dt, Qp, prior_t, prior_k, maxT, maxK, int(verbose),
                                    nthreads, device, C.c_void_p(stream) if stream else None, cb, None, C.byref(mh),
                                    C.byref(F)))
    return F.value, TopicModel(mh, [len(Xj) for Xj in Xs], [x.shape[0] for x in docs])
