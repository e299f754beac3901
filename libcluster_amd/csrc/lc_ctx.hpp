// Device context: owns the device-resident copy of one data set (all groups,
// padded), the responsibility matrix qZ and every workspace of the hot path,
// and drives the kernels of lc_kernels_*.hip.  One context per learn*() call
// (and one per split sub-problem); contexts are independent.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "lc_comm.hpp"
#include "lc_kernels.h"

namespace lck {
struct PredictCondLaunch;  // (lc_predict.hpp)
}

namespace lcc {

struct HipFailure : std::runtime_error {
  explicit HipFailure(const std::string& s) : std::runtime_error(s) {}
};
// a failing HIP call throws HipFailure with the call's text and place (every translation unit of the context)
#define LC_HIP(expr)                                                                                          \
  do {                                                                                                        \
    hipError_t e_ = (expr);                                                                                   \
    if (e_ != hipSuccess)                                                                                     \
      throw ::lcc::HipFailure(std::string("HIP error: ") + hipGetErrorString(e_) + " in " #expr " (" __FILE__ \
                              ":" + std::to_string(__LINE__) + ")");                                          \
  } while (0)
// hipMalloc said no (after the block cache was trimmed): optional accelerations catch this one and take their ordinary path
struct AllocFailure : HipFailure {
  explicit AllocFailure(const std::string& s) : HipFailure(s) {}
};
// Context::estep_cache: the device has no room for the distance cache at this width (nothing was changed; the caller
// runs the ordinary E-step instead)
struct CacheNoRoom : std::runtime_error {
  explicit CacheNoRoom(const std::string& s) : std::runtime_error(s) {}
};

// all-reduce hook: sum `count` doubles in place across ranks (device buffer),
// enqueued on / ordered with `stream`.  Returns 0 on success.
typedef int (*allreduce_fn)(void* user, void* device_buf, int64_t count, void* stream);

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  int device = -1;  // the GPU the block lives on (tagged when it is taken, so it returns to the right cache bin)
  ~DevBuf() { release(); }
  void release();  // back to the block cache (lc_ctx.cpp), not to the driver
  // grow (contents NOT preserved)
  void reserve(size_t n);
};

// page-locked host staging buffer (grow-only): asynchronous copies to / from it do not bounce through the
// driver's own pinned pool, which is what a pageable std::vector costs on every small per-iteration transfer
struct PinnedBuf {
  double* p = nullptr;
  size_t cap = 0, n = 0;
  ~PinnedBuf();
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  void resize(size_t count);  // contents NOT preserved when it grows
  void assign(size_t count, double v) {
    resize(count);
    for (size_t i = 0; i < count; ++i) p[i] = v;
  }
  double* data() { return p; }
  const double* data() const { return p; }
  size_t size() const { return n; }
  double& operator[](size_t i) { return p[i]; }
  const double& operator[](size_t i) const { return p[i]; }
  double* begin() { return p; }
  double* end() { return p + n; }
};

// an ordered set of (padded, global) row indices of one context, kept on the device
struct RowSelection {
  DevBuf<int64_t> idx;          // [M] ascending
  DevBuf<int64_t> starts_d;     // [J+1] first position of every group inside idx
  std::vector<int64_t> starts;  // host copy
  int64_t M = 0;
};

// return every cached device / page-locked block to the driver
void trim_cache();
// while one of these lives on the calling thread, a device allocation may be served by a cached block up to 16 times
// the request (2 otherwise): for the short-lived buffers of sub-problems
struct RelaxedFit {
  RelaxedFit();
  ~RelaxedFit();
  RelaxedFit(const RelaxedFit&) = delete;
  RelaxedFit& operator=(const RelaxedFit&) = delete;
};
// Cached blocks are handed back only to the host thread that released them (one thread = one stream = ordered re-use).
// A thread that is about to end calls this AFTER synchronising its stream: its blocks become available to everybody.
void cache_release_thread();

struct KernelTimes {
  double estep_ms = 0, suffstat_ms = 0, fused_ms = 0;  // fused: E-step + statistics in one launch (small observations)
  int64_t estep_calls = 0, suffstat_calls = 0, fused_calls = 0;
  int64_t estep_diag_mfma_calls = 0;  // separable families: E-step launches that took estep_diag_mfma_kernel (of estep_calls)
  // the exchange step (events around the collective on the context's stream: the sum itself plus the wait for the
  // slowest rank to arrive) and the host's wall time per phase of a VBEM iteration (vbem): what a multi-GPU run
  // needs to tell a slow collective from a slow M-step from a straggling rank
  double allreduce_ms = 0;
  int64_t allreduce_calls = 0;
  double host_stats_ms = 0, host_mstep_ms = 0, host_estep_ms = 0, host_fenergy_ms = 0;
  int64_t host_iters = 0;
};

class Context {
 public:
  Context(int device, hipStream_t stream);
  ~Context();
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;

  // ---- data ---------------------------------------------------------------
  // Host groups -> device (row-major, padded).  Element (n,d) of group j is at
  // Xj[j][n*row_stride + d*col_stride].
  void set_data(int J, const double* const* Xj, const int64_t* Nj, int D, int64_t row_stride, int64_t col_stride);
  // Device groups -> the same image: Xj is a HOST array of J DEVICE pointers, strides >= 1.  Every pointer of a
  // group with rows is checked (require_device_memory) before the layout changes or anything is launched; one launch packs
  // all groups on the context's stream, which is synchronised before the call returns.  The image is a copy.
  void set_data_device(int J, const double* const* Xj_dev, const int64_t* Nj, int D, int64_t row_stride, int64_t col_stride);
  // The minimum over the valid entries that are numbers (+inf: none) and how many are NaN: what the pack of set_data_device
  // left behind, or -- after anything else filled or changed the observations -- one reduction pass over the image.
  void data_range(double* min, int64_t* n_nan);
  // throws std::invalid_argument unless p is plain (not managed, not host) device memory of this context's device
  void require_device_memory(const void* p, const std::string& what) const;
  // Single-group synthetic mixture generated on the device (+ initial qZ, K columns)
  void synth(int64_t N, int D, int K, const double* mu, const double* L, uint64_t seed, int64_t row_offset,
             double hard);
  // J groups; cdf: J x K cumulative mixing proportions (host) or null; group_ids: J global ids (Philox
  // counters: a group looks the same on whichever rank generates it) or null = 0..J-1
  void synth_groups(int J, const int64_t* Nj, int D, int K, const double* mu, const double* L, const double* cdf,
                    uint64_t seed, const int64_t* group_ids, int64_t row_offset, double hard);
  // rows [row0, row0+n) of group j -> row-major n x D host buffer
  void get_rows(int j, int64_t row0, int64_t n, double* out) const;
#ifdef LC_TEST_HOOKS
  // tests (libcluster_hip_testhooks.so only): the whole padded image, pad rows and pad columns included -> [NP x DP] host buffer
  void test_image(double* out) const;
#endif

  int J() const { return J_; }
  int D() const { return D_; }
  int DP() const { return DP_; }
  int K() const { return qz_[cur_].K; }
  int64_t N(int j) const { return Nj_[j]; }
  int64_t Ntotal() const { return Ntot_; }
  int64_t NP() const { return NP_; }
  int device() const { return device_; }
  hipStream_t stream() const { return stream_; }
  void set_stream(hipStream_t s) { stream_ = s; }
  void synchronize() const;
  void set_allreduce(allreduce_fn f, void* user) {
    ar_fn_ = f;
    ar_user_ = user;
  }
  // native collective (RCCL or host-staged, lc_comm.hpp); takes precedence over the hook
  void set_comm(std::shared_ptr<lcm::Comm> c) { comm_ = std::move(c); }
  const std::shared_ptr<lcm::Comm>& comm() const { return comm_; }
  bool distributed() const { return ar_fn_ != nullptr || comm_ != nullptr; }
  // sum of one host value over all ranks (identity without a hook); via the device hook
  double allreduce_value(double v);
  void allreduce_values(double* v, int n);
  // Sharding of a distributed run: false (default) = every rank holds rows of the SAME groups (BGMM/VDP
  // row blocks): counts are summed; true = every rank holds WHOLE, different groups (GMC): the per-group
  // counts stay local, only cluster statistics and scalars are summed.
  void set_group_sharded(bool on) { group_sharded_ = on; }
  // statistics pass: skip (4-row step, cluster) pairs whose responsibilities are all exactly 0.0 (bit-identical
  // results; pays off once qZ is mostly hard).  Always on in sparse mode.
  void set_skip_zero(bool on) { skip_zero_ = on; }
  // dense statistics passes on the feature-GEMM route: leave out (4-row step, cluster quad) pairs whose responsibilities
  // are all below 2^-300 (lck::SPECK_TAU) -- in the passes whose qZ a probe finds hard enough
  // (lck::launch_speck_probe; soft passes and passes of fewer than SPECK_PROBE_MIN_ROWS rows run the dense instance).  On by
  // default; the other routes keep every speck either way.
  void set_speck_skip(bool on) { speck_skip_ = on; }
  // statistics passes of this context that ran the skipping instance / that the probe sent to the dense one
  int64_t speck_passes_skipping() const { return speck_skipping_; }
  int64_t speck_passes_dense() const { return speck_dense_; }
  // ... and how many of the skipping ones took the list route (per-quad row lists, lck::launch_suffstat_lists)
  int64_t speck_passes_lists() const { return speck_lists_; }
  // E-steps whose statistics pass could take the list route leave kept-quad masks of the responsibilities they store
  // (lck::EstepLaunch::qmask) and the selector's counts with them: that pass then needs neither the probe's round trip nor
  // a third reading of qZ for its lists.  On by default; off: every pass probes and builds from qZ.  Same results either way.
  void set_estep_masks(bool on) { estep_masks_ = on; }
  // ... and how many list passes were built from such masks
  int64_t speck_passes_masks() const { return speck_masks_; }
  bool group_sharded() const { return group_sharded_ && distributed(); }
  // a context for a sub-problem of this one: same device, stream and all-reduce hook
  void inherit_comm(const Context& parent) {
    ar_fn_ = parent.ar_fn_;
    ar_user_ = parent.ar_user_;
    comm_ = parent.comm_;
    group_sharded_ = parent.group_sharded_;
    skip_zero_ = parent.skip_zero_;
    speck_skip_ = parent.speck_skip_;
    estep_masks_ = parent.estep_masks_;
  }

  // ---- qZ -----------------------------------------------------------------
  void qz_fill(int K, double value);  // K columns = value on valid rows
  void qz_set(int j, const double* q, int K, int64_t row_stride, int64_t col_stride);
  void qz_get(int j, double* q, int64_t row_stride, int64_t col_stride) const;
  void qz_get_all(double* out) const;  // [Ntotal x K] row-major, groups concatenated
  // out[j] = [N_j x K] column-major (Eigen's default layout); ld[j] (optional) = column stride of out[j] when the
  // group's rows are a block of a taller matrix (row-sharded learners), default N_j
  void qz_get_all_colmajor(double* const* out, const int64_t* ld = nullptr) const;
  void qz_get_rows(int j, int64_t row0, int64_t n, double* q, int64_t row_stride, int64_t col_stride) const;
  // ... into DEVICE memory q_dev[r * row_stride + k * col_stride] (strides >= 1), enqueued on the context's stream: no
  // synchronisation (synchronize())
  void qz_get_rows_device(int j, int64_t row0, int64_t n, double* q_dev, int64_t row_stride, int64_t col_stride) const;
  void qz_get_column(int j, int k, double* out) const;  // N(j) doubles
  void qz_keep_columns(const std::vector<int>& keep);    // prune_clusters
  void qz_clone_to_alt();                                // alt <- copy of current (capacity K+1)
  void qz_swap_alt();                                    // current <-> alt
  // ---- split search on the device (partobs / splitobs / auglabels) ----------
  // rows with qZ[.,k] > thresh, in order (partobs' index part, comutils.cpp:56-72)
  void select_rows(int k, double thresh, RowSelection& sel);
  void select_rows_col(const double* col, double thresh, RowSelection& sel);  // ... of any device column of NP values
  // this context := the selected rows of src, group structure kept (partobs' copy part)
  void set_data_gather(const Context& src, const RowSelection& sel);
  // qZ := the selected rows of column `col` of src's current qZ (one column; this context holds src's selected rows)
  void qz_gather_column(const Context& src, const RowSelection& sel, int col);
  // qZ := [s, 1-s], s = ((x-m).v >= 0)   (splitobs + cluster.cpp:446-449); m, v: D host doubles
  void qz_init_split(const double* m, const double* v);
  // ExpGamma::splitobs (distributions.cpp:575-581): s = (x.v > mean over the group's rows of x.v)
  void qz_init_split_mean(const double* v);
  // auglabels (comutils.cpp:75-104) on the current buffer (K -> K+1 columns): selected rows whose
  // refined second responsibility in `sub` exceeds 0.5 move their column-k mass to the new column
  void qz_split_from(const Context& sub, const RowSelection& sel, int k);

  // ---- hot path -------------------------------------------------------------
  // A: K x D x D row-major lower-triangular whiteners, m: K x D, c: J x K.
  // Writes new responsibilities into qZ (K columns).  Fz = -sum logZ; LLk[k] =
  // sum_n q_nk (log q~_nk - c_jk)  (the data term of cluster.cpp:409-410).
  // raw = true stops after log q~ (c_jk - 0.5 d^2) has been written to qZ: GaussWish::Eloglike.
  // target (raw mode only): write the K columns of c_jk - 0.5 d^2 there (leading dimension NP) instead of into qZ
  void estep(int K, const double* A, const double* m, const double* c, double* Fz, double* LLk, bool raw = false,
             double* target = nullptr);
  // Model selection (cluster.cpp:564-629): the distances -0.5 d^2_k(x_n) of the clusters, kept on the device
  // [K x NP], every column tagged on the host with the whitener and mean it was computed from.  An E-step through the
  // cache recomputes the columns whose tag differs IN ANY BIT from the cluster it is asked about (raw estep_kernel),
  // then adds the constants c_jk and normalises over all K columns (softmax_cached_kernel): the same outputs as
  // estep().  Between two iterations of a converging model, and between the candidates of a split round, most
  // clusters' posteriors are bit for bit the same, so most columns are re-used.  Returns the number of recomputed
  // columns; *stale = how many of them had a valid (but different) tag.
  // delta_tol >= 0: also leave every row's largest |q_new - q_old| (against the responsibilities being overwritten,
  // when the buffer held K columns) and, for the rows where it exceeds delta_tol, q_new - q_old, on the device for
  // delta_suffstat(); rows that come out bit for bit as they were are not even written.
  bool dcache_eligible(int K) const;  // a property of the shape (identical on every rank)
  int estep_cache(int K, const double* A, const double* m, const double* c, double* Fz, double* LLk, double delta_tol,
                  int* stale = nullptr);
  // a split candidate works on the cache in place: from journal_begin() on, a column is copied aside before it is
  // first overwritten; rollback() puts columns, tags and width back, journal_end() keeps the new state
  void dcache_journal_begin();
  void dcache_rollback();
  void dcache_journal_end();
  void dcache_invalidate();
  void dcache_release();  // ... and give the memory back
  // The CHANGE of the statistics caused by the last estep_cache(delta_tol = tau): sum over the rows whose
  // responsibilities moved by more than tau in some column of (q_new - q_old) x the usual terms -- the statistics are linear in q, so
  // adding it to the statistics of q_old gives those of q_new up to tau * sum_n |x_n x_n^T| (rows that moved by <= tau
  // are left out).  The rows are compacted in order and gathered into a sub-context (as partobs does), so the cost is
  // proportional to the rows that moved.  Returns false, having computed nothing, when more than max_frac of all rows
  // (summed over ranks) moved -- the caller then runs the ordinary pass.
  bool delta_suffstat(int K1, double max_frac, double* dNk, double* dxs, double* dxxs, double* dNjk);
  int delta_pending() const { return dq_K_; }  // width of the move the last estep_cache(delta_tol >= 0) left (0: none)
  int64_t delta_rows() const { return delta_rows_; }  // rows the last delta_suffstat() found moved (this rank)
  // Small observations (D <= 16, K <= 16, Gauss-Wishart, dense): the E-step AND the statistics of the responsibilities it
  // produces, in one pass (lc_kernels_fused.hip).  Same outputs as estep() followed by suffstat(nullptr, ...).
  // Returns false, having done nothing, when the shape has no fused path.
  bool estep_suffstat_fused(int K, const double* A, const double* m, const double* c, double* Fz, double* LLk,
                            double* Nk, double* xs, double* xxs, double* Njk);
  // Sufficient statistics of the current qZ.  smask: J x K (1 = accumulate) or null.
  // Nk[K], xs[K*D], xxs[K*D*D] (row-major, symmetric), Njk[J*K].
  void suffstat(const unsigned char* smask, double* Nk, double* xs, double* xxs, double* Njk);
  void colsums(double* Njk);  // J x K column sums of the current qZ
  // Diagonal / exponential families: log q~[n,k] = c_jk + sum_d (w2_kd (x_nd - a_kd)^2 + w1_kd x_nd);
  // a, w2, w1: K x D host arrays.  Same outputs as estep().
  void estep_diag(int K, const double* a, const double* w2, const double* w1, const double* c, double* Fz,
                  double* LLk, bool raw = false);
  // N_k, x_s = sum q x [K*D], xx_s = sum q x^2 [K*D] (elementwise), Njk[J*K]
  void suffstat_diag(const unsigned char* smask, double* Nk, double* xs, double* xxs, double* Njk);

  // ---- prediction (lc_predict.cpp) -------------------------------------------------------------------
  // After a raw E-step with zero constants left at least max(K, Kp) columns in qZ: per row the label, logZ and (Kp > 0,
  // Gauss-Wishart) logp into the context's per-row outputs (lck::PredictRowsLaunch for the tables: c, pc J x K / J x Kp
  // row-major, ps, pe Kp).  keep_q: the K columns become the responsibilities.  qZ is left K columns wide.
  void predict_rows(int K, int Kp, const double* c, const double* pc, const double* ps, const double* pe, bool keep_q);
  // Separable families: logp per row (lck::PredictDiagLaunch; mode 0 NormGamma, 1 ExpGamma; a, w: Kp x D host arrays,
  // pc: J x Kp, pe: Kp).  Returns false, when mode 1 met a negative observation.
  bool predict_diag(int mode, int Kp, const double* a, const double* w, const double* pc, const double* pe);
  // rows [row0, row0+n) of group j of the last prediction (any output may be null)
  void get_predictions(int j, int64_t row0, int64_t n, int32_t* label, double* logZ, double* logp) const;
  // ... into DEVICE arrays, enqueued on the context's stream: no synchronisation (synchronize())
  void get_predictions_device(int j, int64_t row0, int64_t n, int32_t* label_dev, double* logZ_dev, double* logp_dev) const;
  // no prediction is readable until the next one completes (a prediction that fails leaves none behind)
  void predict_clear() {
    pred_vb_ = pred_logp_ = false;
    pred_docs_T_ = 0;
    pred_cond_ = 0;
    pred_cond_var_ = false;
    pred_holes_ = false;
    pred_holes_var_ = false;
    pred_holes_draws_ = 0;
    pred_cond_draws_ = 0;
    pred_loo_ = false;
    pred_loo_var_ = false;
  }
  // Conditional prediction: after a raw E-step with zero constants over the context's (given) columns left
  // Kp columns in qZ, per row E[x_target | x_given] (Db columns) and log p(x_given) into the context's conditional outputs
  // (lck::PredictCondLaunch for the tables: tt J x Kp, ps, pe Kp, ma Kp x D, B Kp x Db x D, mb Kp x Db, host arrays).
  // qZ is left holding the Kp per-cluster log terms.
  void predict_cond(int Kp, int Db, const double* tt, const double* ps, const double* pe, const double* ma,
                    const double* B, const double* mb);
  // rows [row0, row0+n) of group j of the last conditional prediction (either output may be null)
  void get_conditional(int j, int64_t row0, int64_t n, double* mean, int64_t row_stride, double* logp) const;
  int conditional_width() const { return pred_cond_; }  // target columns of the conditional prediction held (0: none)
  // Predictive variance, right after predict_cond with the same Kp and Db, on the columns, logp and mean it
  // left: per row the diagonal of the mixture's covariance of the target columns (lck::PredictCondVarLaunch for the tables:
  // S Kp x Db, g Kp, host arrays).
  void predict_cond_var(int Kp, int Db, const double* S, const double* g);
  // rows [row0, row0+n) of group j of that variance (var may be null); throws when the prediction held has none
  void get_conditional_var(int j, int64_t row0, int64_t n, double* var, int64_t row_stride) const;
  // Draws of the conditional, right after predict_cond with the same Kp and Db, on the columns and logp it left:
  // ndraws draws of the target columns per row and their components (lck::PredictCondDrawsLaunch; L Kp x Db x Db lower
  // Cholesky factors of the Schur complements, row-major, cq Kp, host arrays).
  void predict_cond_draws(int Kp, int Db, int ndraws, uint64_t seed, const double* L, const double* cq);
  // rows [row0, row0+n) of group j of those draws: draws [n x ndraws x Db], label [n x ndraws] (either may be null)
  void get_conditional_draws(int j, int64_t row0, int64_t n, double* draws, int32_t* label) const;
  int conditional_draws() const { return pred_cond_draws_; }  // draws per row of the conditional prediction held (0: none)
  // New rows from a model: J blocks of Nj rows at width D replace whatever the context held, as set_data
  // does (lck::SampleLaunch for mode and tables: cdf J x Kp, klast J, loc Kp x D, fac Kp x D x D or Kp x D, shape Kp, host
  // arrays).  The component of every row stays on the device (get_sample_labels).
  void sample(int mode, int J, const int64_t* Nj, int D, int Kp, const double* cdf, const int* klast, const double* loc,
              const double* fac, const double* shape, uint64_t seed, int64_t row_offset);
  // components of rows [row0, row0+n) of group j; throws when the context's rows do not come from sample()
  void get_sample_labels(int j, int64_t row0, int64_t n, int32_t* label) const;
  // Rows with holes (a NaN in X is an unknown value).  holes_scan: one read of X leaves the per-row hole
  // records on the device and returns the number of rows with holes, the largest count and the first row (in block, row
  // order) that has more than lck::HOLES_MAX holes or no known column (*bad_block = -1: none), with its count.
  // holes_fill: fill[c] (D host values) into the recorded positions.  predict_holes: after a raw E-step with zero constants
  // over the filled rows left Kp columns in qZ, the completed rows into X in place and log p(x_known) per row
  // (lck::PredictHolesLaunch for the tables: tt J x NH x Kp, ps Kp, pe NH x Kp, mean Kp x D, P Kp x D x D host arrays,
  // NH = lck::HOLES_MAX + 1).  qZ is left holding the raw columns.  gnu (NH x Kp host values g_k(nb) nu_k):
  // also the predictive variance of every filled value (lck::PredictHolesVarLaunch), in a buffer that only such a call
  // reserves; null: what the call did before, and no variance is readable afterwards.  ndraws > 0 (cqnu Kp
  // host values, not together with gnu): also ndraws draws of every unknown value with their components
  // (lck::HolesDrawsLaunch), in buffers that only such a call reserves; qZ then holds t_k for the rows with holes.
  void holes_scan(int64_t* holed_rows, int* max_count, int* bad_block, int64_t* bad_row, int* bad_count);
  void holes_fill(const double* fill);
  // after holes_scan: the first row (in block, row order) with at least one hole (*block = -1: none)
  void first_holed_row(int* block, int64_t* row) const;
  void predict_holes(int Kp, const double* tt, const double* ps, const double* pe, const double* mean, const double* P,
                     const double* gnu = nullptr, const double* cqnu = nullptr, int ndraws = 0, uint64_t seed = 0);
  // rows [row0, row0+n) of group j after the last predict_holes (any output may be null): the completed rows (row_stride
  // >= D doubles apart), logp, count and cols [n x lck::HOLES_MAX] (ascending, -1 beyond count)
  void get_completed(int j, int64_t row0, int64_t n, double* rows, int64_t row_stride, double* logp, int32_t* count,
                     int32_t* cols) const;
  // ... and their variances [n x lck::HOLES_MAX] (row_stride >= lck::HOLES_MAX doubles apart; slot i belongs to cols[i], 0
  // beyond count; var may be null): throws when the last predict_holes had no gnu
  void get_completed_var(int j, int64_t row0, int64_t n, double* var, int64_t row_stride) const;
  // ... and their draws [n x ndraws x lck::HOLES_MAX] (slot i belongs to cols[i], 0 beyond count) with the component of
  // every draw [n x ndraws] (-1 in a row without holes); either may be null: throws when the last predict_holes drew none
  void get_completed_draws(int j, int64_t row0, int64_t n, double* draws, int32_t* label) const;
  int completed_draws() const { return pred_holes_ ? pred_holes_draws_ : 0; }  // draws per row held (0: none)
  // Leave-one-out conditionals, after holes_scan found no hole and a raw E-step with zero constants over the
  // complete rows left Kp columns in qZ: log p(x) per row (predict_rows_kernel over the nb = 0 tables pc J x Kp, ps Kp, pe0
  // Kp), then per row and column the conditional log density, mean and -- gnu1 not null -- variance (lck::LooRowsLaunch for
  // the tables: tt1 J x Kp, pe1 Kp, gnu1 Kp, mean Kp x D, P Kp x D x D host arrays; log(P_dd) / 2 and 1 / P_dd are formed
  // here), then the worst column per row.  qZ is left holding the raw columns; X is only read.
  void predict_loo(int Kp, const double* pc, const double* ps, const double* pe0, const double* tt1, const double* pe1,
                   const double* gnu1, const double* mean, const double* P);
  // rows [row0, row0+n) of group j of the last predict_loo (any output may be null): logp and worst [n]; cond, mean and var
  // [n x D], row_stride >= D doubles apart; throws for var when the last predict_loo had no gnu1
  void get_leave_one_out(int j, int64_t row0, int64_t n, double* logp, double* cond, double* mean, double* var,
                         int64_t row_stride, int32_t* worst) const;
  // ---- ranking ----------------------------------------------------------------------------------------------
  // The m best rows of each column (lck::TopRowsLaunch for the order): what = 0 the first ncols columns of qZ, 1 / 2 the
  // logZ / logp of the last prediction (one column; ncols is not looked at).  by_label: column c only sees the rows the
  // last prediction labelled c.  count[C]; group, row, score [C x m], best first, -1 / -1 / NaN past count[c].
  void top_rows(int what, int ncols, int m, bool largest, bool by_label, int32_t* count, int32_t* group, int64_t* row,
                double* score);
  // Order and threshold queries over the same columns (lck::ScoreSelectLaunch, ScoreCountsLaunch,
  // RowsBeyondLaunch; the outputs are those of lc_ctx_score_quantiles, lc_ctx_score_counts, lc_ctx_rows_beyond).  None of
  // them changes the prediction, the qZ or the observations.
  void score_quantiles(int what, int ncols, bool by_label, const double* probs, int nprobs, int64_t* count, int64_t* rank,
                       double* value);
  void score_counts(int what, int ncols, bool by_label, const double* thr, int nthr, int64_t* count, int64_t* atmost);
  void rows_beyond(int what, int ncols, int col, bool by_label, double thr, bool above, int64_t capacity, int64_t* total,
                   int32_t* group, int64_t* row, double* score);
  // Two-level models (lc_topic_predict.cpp): after a raw E-step left L_nk = Eloglike_k(x_n) in K columns of
  // qZ, every group of the context is one document: its qY, label_t, Fyz, Fz and sweep count into the context's
  // per-document outputs, label / logZ per row as above (lck::TopicInferLaunch; a: J x T, E: T x K host arrays).
  void topic_infer(int K, int T, const double* a, const double* E, int max_sweeps, double tol, bool keep_q);
  // documents [doc0, doc0+n) of the last topic_infer (any output may be null; qY: n x T row-major)
  void get_doc_predictions(int doc0, int n, double* qY, int32_t* label_t, double* Fyz, double* Fz, int32_t* sweeps) const;

  // Host work to run while the NEXT normalising E-step is on the device: the E-step calls it once, after its last
  // launch and before it waits for the stream (vbem hands over the free-energy terms that depend on the posteriors
  // only).  A hook that is still pending when the E-step returns was not called; the owner runs it itself.
  void set_overlap(std::function<void()> f) { overlap_ = std::move(f); }
  bool overlap_pending() const { return (bool)overlap_; }
  void run_overlap() {
    if (!overlap_) return;
    std::function<void()> f = std::move(overlap_);
    overlap_ = nullptr;
    f();
  }

  // ---- timing ---------------------------------------------------------------
  void timing_enable(bool on) {
    timing_ = on;
    if (on) timing_prepare(1024);  // (two events per timed launch: created here, outside anybody's timed region)
  }
  bool timing_enabled() const { return timing_; }
  void timing_host_phases(double stats_ms, double mstep_ms, double estep_ms, double fenergy_ms) {  // one VBEM iteration
    times_.host_stats_ms += stats_ms;
    times_.host_mstep_ms += mstep_ms;
    times_.host_estep_ms += estep_ms;
    times_.host_fenergy_ms += fenergy_ms;
    times_.host_iters += 1;
  }
  KernelTimes timing_get();  // resolves pending events (synchronises the stream)
  void timing_prepare(int events);  // events created ahead of a timed region (they are recycled afterwards)
  void timing_reset();

 private:
  struct QZ {
    DevBuf<double> buf;
    int cap = 0;  // columns allocated
    int K = 0;    // columns in use
    // cluster(): a 64-bit fingerprint per row of what the buffer holds (softmax_cached_kernel keeps it, and skips the
    // old values of the rows it leaves unchanged).  Every other writer of the buffer goes through ensure_qz(), which
    // clears hash_ok; qz_clone_to_alt copies it, qz_split_from marks the rows it rewrites.
    DevBuf<int64_t> hash;
    bool hash_ok = false;
    // Kept-quad masks of what the buffer holds (lck::EstepLaunch::qmask, [quads of mask_K x NP / 16]), written by the E-step
    // that wrote the buffer, with the two counts of the selector's sample taken from them (lck::launch_speck_probe_masks;
    // they arrive under that E-step's own synchronisation).  mask_ok: they describe the buffer as it is.
    // EVERY other writer clears it: ensure_qz() does, and so does each writer that does not come through there
    // (qz_written()).  qz_clone_to_alt clears the copy's flag; qz_swap_alt needs nothing, the masks belong to the slot.
    DevBuf<unsigned short> qmask;
    bool mask_ok = false;
    int mask_K = 0;
    int64_t mask_nrg = 0;  // the shape they were written for
    int mask_counts[2] = {0, 0};
    int64_t mask_pairs = 0, mask_rows = 0;
  };
  // a writer of q's buffer that does not come through ensure_qz(): the masks no longer describe it
  void qz_written(QZ& q);
#ifdef LC_TEST_HOOKS
  void verify_qmask(const QZ& q);
#endif
  void ensure_qz(QZ& q, int K, bool preserve);
  void build_layout(int J, const int64_t* Nj, int D);
  void allreduce(double* dbuf, int64_t count);
  // pack the E-step parameter stream (tiles of A_k in consumption order, -b_k; then the J x K table c) into hpack_
  void pack_estep_params(int K, const double* A, const double* m, const double* c);
  // ... packs and uploads them, and returns the launch of the Gauss-Wishart E-step over the `rows` (padded) rows of X, of
  // which the first `nrows` are valid when the context has one group; out: K columns, leading dimension `rows`.  The
  // partial buffers are sized for lck::estep_grid() of the launch (llpart_ only with want_ll).
  lck::EstepLaunch gw_estep_launch(int K, const double* A, const double* m, const double* c, const double* X, int64_t rows,
                                   int64_t nrows, double* out, bool raw, bool want_ll);
  // The frame the passes share.  timed: run `launch` between two events of the pool when timing is on
  // (a launch that throws leaves no pair behind).
  enum class Timed { Estep, Suffstat, Fused, Allreduce };  // the heading of KernelTimes a launch is counted under
  template <class F>
  void timed(Timed kind, F&& launch);
  // F_z and LL_k of a normalising pass: fold the `grid` rows of fzpart_ / llpart_ (0: this rank holds no rows), sum over
  // ranks, and leave [F_z | LL_k] in hred_ once the stream has been synchronised; read_sums() hands them out after that
  void enqueue_sums(int64_t grid, int K, bool want_ll);
  void read_sums(int K, double* Fz, double* LLk) const;
  // N_jk comes from a column-sum pass of its own: several groups, whole groups per rank, or a mask that removes clusters
  bool own_counts(bool masked) const { return J_ > 1 || group_sharded() || masked; }
  void use_device() const;         // hipSetDevice(device_): every method that allocates, launches or copies starts here
  void require_gw_width() const;  // throws for DP > 128 (full-covariance kernels)
  int build_sparse_worklist(const unsigned char* smask, int K, const lck::SuffstatPlan& plan, lck::SuffstatLaunch& a);

  int device_;
  hipStream_t stream_;
  allreduce_fn ar_fn_ = nullptr;
  void* ar_user_ = nullptr;
  std::shared_ptr<lcm::Comm> comm_;
  bool group_sharded_ = false;
  bool skip_zero_ = false;
  bool speck_skip_ = true;
  int64_t speck_skipping_ = 0, speck_dense_ = 0, speck_lists_ = 0;
  DevBuf<int> speck_active_;
  bool estep_masks_ = true;
  int mask_route_K_ = -1, mask_route_DC_ = -1;  // the shape Context::estep last asked the statistics plan's route for, and the answer
  int64_t mask_route_NP_ = -1;
  bool mask_route_feat_ = false;
  int64_t speck_masks_ = 0;
  PinnedBuf hprobe_;  // the two counts of a probe enqueued behind an E-step (8 bytes), read after its synchronisation
  DevBuf<unsigned char> sslists_;  // the row lists of a list pass (lck::ss_list_layout: about 2 bytes per row and cluster quad)

  int J_ = 0, D_ = 0, DP_ = 0;
  int DC_ = 0;  // active width of the Gauss-Wishart E-step / feature-GEMM statistics (lck::estep_active_width): DP_ - 8 or DP_
  std::vector<int64_t> Nj_, goff_;  // goff_: padded row offsets, size J+1
  int64_t Ntot_ = 0, NP_ = 0;
  DevBuf<double> X_;
  DevBuf<int> rginfo_;      // only when J > 1
  DevBuf<int64_t> goff_d_;  // J+1
  // set_data_device / data_range: [range 2 | source pointers J | rows J] of the last pack launch; range_ok_: range_min_ and
  // range_nan_ describe the observations as they are (cleared by whatever replaces or rewrites them)
  DevBuf<int64_t> ingest_tab_;
  bool range_ok_ = false;
  double range_min_ = 0.0;
  int64_t range_nan_ = 0;
  lck::PackRowsLaunch pack_launch(const std::vector<int64_t>& tab, int64_t rs, int64_t cs, double* image);
  void read_range();
  DevBuf<unsigned char> ssitems_;  // sparse statistics: work items, and [klist | kptr | krec]
  DevBuf<int> ssints_;
  const int* sskptr_ = nullptr;
  const int* sskrec_ = nullptr;
  QZ qz_[2];
  // distance cache: slab of dc_cap_ column SLOTS [dc_cap_ x NP]; cluster k's column of -0.5 d^2 lives in slot dc_slot_[k]
  // (k < dc_K_), host tags say for which posterior it was computed; scratch for recomputed columns that find no run of
  // free slots.  Round 5: a column that changes under the journal (a split candidate's trial) is written into a FREE
  // slot and the map is switched -- the old slot is what a rollback returns to, a commit frees it: no column is ever
  // copied (round 4: 2 456 device-to-device copies of 80 MB per model selection at N = 10M, 66 ms).
  DevBuf<double> dc_slab_, dfresh_;
  int dc_cap_ = 0, dc_K_ = 0;
  int dc_room_K_ = 0;  // widest K for which all ranks found room
  std::vector<int> dc_slot_;            // [dc_K_] slot of cluster k's column
  std::vector<unsigned char> dc_used_;  // [dc_cap_] slot in use (by the map or by the journal)
  std::vector<std::vector<double>> dc_tagA_, dc_tagm_;
  struct SavedColumn {
    int col = -1;
    int slot = -1;  // where the column's journaled content stays
    uint64_t ver = 0;
    std::vector<double> A, m;
  };
  // which rows a recomputed column matters for (lck::BoundSelectLaunch): every sweep leaves each row's largest log q~ and
  // its cluster; valid for cluster j while column j is the version it was then (dc_ver_)
  std::vector<uint64_t> dc_ver_;  // [dc_K_] version of cluster k's column (bumped on every recomputation)
  uint64_t dc_vernext_ = 0;
  DevBuf<double> rm_max_, bs_need_, bs_x_, bs_out_;
  DevBuf<int> rm_arg_;
  bool rm_valid_ = false;
  int rm_K_ = 0;
  std::vector<uint64_t> rm_ver_;
  std::vector<double> rm_c_;
  int64_t clone_resyncs_ = 0, clone_fulls_ = 0;  // split trials whose working copy was re-synchronised row by row / copied whole (trace)
  int64_t bound_rows_ = 0, bound_passes_ = 0;  // rows recomputed / passes taken by the bounded recomputation (trace)
  bool bound_static_ok() const;  // the bounded recomputation's shape preconditions (one group, one rank, enough rows)
  bool recompute_bounded(int K, const std::vector<int>& changed, const std::vector<int>& oldslot,
                         const std::vector<std::vector<double>>& oldA, const std::vector<std::vector<double>>& oldm,
                         const std::vector<int>& dest, const double* A, const double* m, const double* c, bool delta);
  int dc_find_run(int n) const;  // first run of n free slots (-1: none)
  std::vector<std::unique_ptr<SavedColumn>> dc_saved_;
  bool dc_journal_ = false;
  int dc_jK0_ = 0;
  DevBuf<double> sink_;  // estep_diag_mfma_kernel's store sink
  DevBuf<double> dq_, amax_;  // estep_cache(delta_tol): q_new - q_old [K x NP] (moved rows), per-row max |.|
  DevBuf<int64_t> dq_maskd_;  // [2] device: columns with any non-zero difference (CachedNormLaunch::colmask)
  DevBuf<int> dq_colsd_;
  uint64_t dq_mask_[2] = {0, 0};
  bool dq_mask_ok_ = false;
  double dq_tol_ = 0.0;
  int dq_K_ = 0;
  int64_t dq_ld_ = 0;  // row stride of dq_ (row-major: a moved row's differences are contiguous)
  int64_t delta_rows_ = 0;
  int cur_ = 0;

  DevBuf<double> params_, ctab_, fzpart_, llpart_, red_, redtmp_, sspart_, ssout_, ssext_;
  // sspart_ holds zeros in every Gauss-Wishart record entry of the columns past the active width (suffstat()): true once
  // it has been cleared and until it is re-allocated or lent to another record layout
  bool sspart_clean_ = false;
  void sspart_reserve(size_t n) {
    if (n > sspart_.cap) {
      sspart_.reserve(n);
      sspart_clean_ = false;
    }
  }
  DevBuf<unsigned char> smask_;
  DevBuf<int> selcnt_;
  DevBuf<int64_t> seloff_;
  DevBuf<double> mv_;
  // per-row outputs of the last prediction ([NP] each; valid until the observations change) and its small tables
  DevBuf<int> plabel_, pflag_;
  DevBuf<double> plogz_, plogp_, ptab_;
  bool pred_vb_ = false, pred_logp_ = false;
  // ... of the last conditional prediction: mean [NP x pred_cond_] and log p(x_given) [NP]; pred_cond_ = 0: none
  DevBuf<double> pcmean_, pclogp_;
  int pred_cond_ = 0;
  // ... and, when pred_cond_var_, its variance [NP x pred_cond_] with the tables of that pass [g Kp | S Kp x Dbp]
  DevBuf<double> pcvar_, pvtab_;
  bool pred_cond_var_ = false;
  lck::PredictCondLaunch predict_cond_args(int Kp, int Db) const;  // over the tables predict_cond left in ptab_
  // ... and, when pred_cond_draws_ > 0, that many draws per row [NP x pred_cond_draws_ x pred_cond_] with their components
  // [NP x pred_cond_draws_] and the tables of that pass [cq Kp | Lt Kp x Dbp x Dbp]
  DevBuf<double> pcdraws_, pdtab_;
  DevBuf<int> pcdlabel_;
  int pred_cond_draws_ = 0;
  // the components of the rows when they come from sample() ([NP]; sampled_ is cleared by whatever replaces the rows)
  DevBuf<int> slabel_;
  bool sampled_ = false;
  // ... of the last prediction of rows with holes: count [NP], cols [NP x HOLES_MAX], log p(x_known) [NP], the scan's
  // three integers; pred_holes_: X holds the completed rows of such a prediction
  DevBuf<int> hcount_, hcols_;
  DevBuf<double> hlogp_;
  DevBuf<int64_t> hscan_;
  bool pred_holes_ = false;
  // ... and, when pred_holes_var_, the variance of the filled values [NP x HOLES_MAX]
  DevBuf<double> hvar_;
  bool pred_holes_var_ = false;
  // ... and, when pred_holes_draws_ > 0, that many draws of the filled values [NP x pred_holes_draws_ x HOLES_MAX] with
  // their components [NP x pred_holes_draws_]
  DevBuf<double> hdraws_;
  DevBuf<int> hdlabel_;
  int pred_holes_draws_ = 0;
  // ... of the last leave-one-out prediction: log p(x) [NP], cond and mean [NP x DP], the worst column and its value [NP]
  // and, when pred_loo_var_, the variance [NP x DP]
  DevBuf<double> llogp_, lcond_, lmean_, lvar_, lworstv_;
  DevBuf<int> lworst_;
  bool pred_loo_ = false;
  bool pred_loo_var_ = false;
  // top_rows: the first stage's partial lists and the result [C x m scores | C x m positions]; the order and threshold
  // queries keep their integer scratch and results in toppos_ and the flagged rows' scores in topkey_
  DevBuf<double> topkey_, topout_;
  DevBuf<int64_t> toppos_;
  // the columns `what` names, after the argument checks top_rows and the order and threshold queries share
  struct RankColumns {
    const double* col = nullptr;
    int C = 1;
  };
  RankColumns rank_columns(int what, int ncols, bool by_label) const;
  lck::ScoreColumns score_columns(const RankColumns& rc, bool by_label, const char* who) const;  // NP_ > 0
  // per-document outputs of the last topic_infer ([J x T], [J x 2], [J x 2]); pred_docs_T_ = its T (0: none)
  DevBuf<double> tqy_, tf_;
  DevBuf<int> tint_;
  DevBuf<int64_t> tnrows_;
  int pred_docs_T_ = 0;
  PinnedBuf hpack_, hred_, hss_, hmask_;
  std::function<void()> overlap_;

  bool timing_ = false;
  struct EvPair {
    hipEvent_t a, b;
    Timed kind;
  };
  std::vector<EvPair> pending_;
  std::vector<hipEvent_t> evpool_;  // recycled timing events
  hipEvent_t timing_event();
  KernelTimes times_;
};

}  // namespace lcc
