/* libcluster_hip.h -- C ABI of the MI355X (gfx950) implementation of
 * libcluster's variational E-step / sufficient-statistic hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Every entry point names the reference (dsteinberg/libcluster) interface it
 * replaces.  All functions return an lc_status; on failure lc_last_error()
 * (thread-local) holds the message.  The C++ facade (include/libcluster.h,
 * include/distributions.h) re-throws the reference's exception classes:
 *   LC_EINVAL  -> std::invalid_argument   LC_ERUNTIME -> std::runtime_error
 *   LC_EDOMAIN -> std::domain_error       LC_EHIP     -> std::runtime_error
 *
 * There is NO CPU fallback: without a HIP device every data-path call fails
 * with LC_EHIP.  Host-only entry points (lc_mstep_*, lc_weights_*, lc_digamma)
 * work anywhere.
 *
 * Matrices are described as (pointer, row_stride, col_stride) in elements, so
 * both Eigen storage orders (column-major default, row-major when the
 * reference is built with -DEIGEN_DEFAULT_TO_ROW_MAJOR, CMakeLists.txt:59-61)
 * are accepted without a copy on the caller's side.
 *
 * Random numbers (lc_ctx_synth, lc_model_sample, lc_model_predict_conditional_draws, lc_model_predict_incomplete_draws;
 * DESIGN 4.16, 4.16.1): Philox-4x32-10.  The key
 * is the 64-bit seed (k0 = low word, k1 = high word).  (c0, c1) are the low and high word of
 *   g = (block << 40) + row_offset + row inside its block      (row_offset = 0 for conditional and incomplete draws)
 * c3 = tag | (sub << 8); o[0..3] are the output words, u01(a, b) = ((a << 32 | b) >> 11 + 0.5) / 2^53, and a Box-Muller
 * pair is sqrt(-2 log u01(o[0], o[1])) (cos, sin)(2 pi u01(o[2], o[3])).
 *   tag   c2            sub        stream
 *   0x01  pair p        0          lc_ctx_synth: the normals of columns 2p, 2p + 1
 *   0x02  0             0          lc_ctx_synth: the label
 *   0x10  draw i        0          component choice: u = u01(o[0], o[1]); the first k, in the order 0 ... K-1 then the prior
 *                                  component, whose running sum of weights exceeds u (the sum short: the last with weight)
 *   0x11  draw i        pair p     the normals z[2p], z[2p + 1] of the draw (cos, sin)
 *   0x12  draw or slot  attempt t  gamma draw (Marsaglia-Tsang): the normal of attempt t (the cos value)
 *   0x13  draw or slot  attempt t  gamma draw: the uniform u01(o[0], o[1]) of attempt t
 *   0x14  draw or slot  0          gamma draw of a shape < 1: the U of Gamma(shape + 1) U^(1 / shape)
 *   0x15  pair p        0          ExpGamma: the Lomax uniforms of columns 2p (o[0], o[1]) and 2p + 1 (o[2], o[3])
 * lc_model_sample draws one row per counter: i = 0, and the slot of a gamma draw is 0 (Gauss-Wishart: one per row) or the
 * column (NormGamma: one per entry).  lc_model_predict_conditional_draws: i = the draw, one gamma draw per draw.
 * lc_model_predict_incomplete_draws uses the same streams: i = the draw, one gamma draw per draw, and pair p holds the
 * normals of the holes in slots 2p, 2p + 1 of the row's cols (only the first ceil(count / 2) pairs are generated).  For equal
 * seeds the choice uniform of (block, row, draw) is the one lc_model_predict_conditional_draws uses.
 */
#ifndef LIBCLUSTER_HIP_H
#define LIBCLUSTER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { LC_OK = 0, LC_EINVAL = 1, LC_ERUNTIME = 2, LC_EHIP = 3, LC_EDOMAIN = 4 } lc_status;

/* weight distribution kinds: include/distributions.h:163 (Dirichlet), :103 (StickBreak), :147 (GDirichlet) */
typedef enum { LC_W_DIRICHLET = 0, LC_W_STICKBREAK = 1, LC_W_GDIRICHLET = 2 } lc_weight_kind;
/* learners: include/libcluster.h:177 (learnVDP), :218 (learnBGMM), :356 (learnGMC), :409 (learnSGMC) */
typedef enum {
  LC_ALGO_VDP = 0,  /* learnVDP   cluster.cpp:636  StickBreak + GaussWish */
  LC_ALGO_BGMM = 1, /* learnBGMM  cluster.cpp:667  Dirichlet  + GaussWish */
  LC_ALGO_GMC = 2,  /* learnGMC   cluster.cpp:763  GDirichlet + GaussWish */
  LC_ALGO_SGMC = 3, /* learnSGMC  cluster.cpp:787  Dirichlet  + GaussWish */
  LC_ALGO_DGMM = 4, /* learnDGMM  cluster.cpp:697  Dirichlet  + NormGamma */
  LC_ALGO_BEMM = 5, /* learnBEMM  cluster.cpp:730  Dirichlet  + ExpGamma  */
  LC_ALGO_DGMC = 6, /* learnDGMC  cluster.cpp:811  GDirichlet + NormGamma */
  LC_ALGO_EGMC = 7  /* learnEGMC  cluster.cpp:842  GDirichlet + ExpGamma  */
} lc_algo;
/* cluster parameter distributions (distributions.h:264, 334, 406) */
typedef enum { LC_C_GAUSSWISH = 0, LC_C_NORMGAMMA = 1, LC_C_EXPGAMMA = 2 } lc_ckind;

typedef struct lc_ctx lc_ctx;     /* device-resident data set + qZ + workspaces */
typedef struct lc_model lc_model; /* weights + clusters (+ the context that holds qZ) */
typedef struct lc_tmodel lc_tmodel; /* two-level (SCM / MCM) model: qY, qZ, weights_j, weights_t, clusters(_t) */

const char* lc_last_error(void);
int lc_version(void);
/* Name of the device kernel a dense Gauss-Wishart statistics pass (updateSS, src/cluster.cpp:53-82) runs for D columns
 * and K clusters: "suffstat_kernel" (per-cluster form), "suffstat_feat_kernel" (feature GEMM) or "suffstat_quad_kernel"
 * (3 <= K <= 16 at D = 17 ... 64: four clusters in the four blocks of one matrix instruction) -- what a profiler will list;
 * bench.py prices that kernel. */
const char* lc_statistics_kernel_name(int D, int K);
/* hash of the sources this binary was built from (libcluster_amd/build.py::source_hash); the Python loader compares it
 * with the tree it sits in and rebuilds or refuses a stale binary */
const char* lc_source_hash(void);
/* number of visible HIP devices (0 on a host without a GPU; never fails) */
int lc_device_count(void);

/* ---- constants: include/libcluster.h:122-127, include/distributions.h:39-43 */
double lc_const_converge(void);   /* CONVERGE   = (double)1e-5f */
double lc_const_fengydel(void);   /* FENGYDEL   = CONVERGE/10   */
double lc_const_zerocutoff(void); /* ZEROCUTOFF = (double)0.1f  */
int lc_const_splititer(void);     /* SPLITITER  = 15            */

/* ======================================================================== *
 * Device context.  `stream` is a hipStream_t (NULL = the null stream).
 * ======================================================================== */
int lc_ctx_create(int device, void* stream, lc_ctx** out);
int lc_ctx_destroy(lc_ctx* ctx);
int lc_ctx_set_stream(lc_ctx* ctx, void* stream);
int lc_ctx_synchronize(lc_ctx* ctx);
int lc_ctx_dims(lc_ctx* ctx, int* J, int* D, int64_t* Ntotal, int* K);

/* Upload J groups of observations (the `const vMatrixXd& X` of
 * cluster.cpp:564-566; learnVDP/learnBGMM pass J = 1, cluster.cpp:651/682).
 * Element (n,d) of group j is Xj[j][n*row_stride + d*col_stride].
 * Any D for the diagonal / exponential families; the Gauss-Wishart entry points return LC_EINVAL beyond D = 1024. */
int lc_ctx_set_data(lc_ctx* ctx, int J, const double* const* Xj, const int64_t* Nj, int D, int64_t row_stride,
                    int64_t col_stride);
/* The same for observations that already live in device memory: Xj_dev is a HOST array of J DEVICE
 * pointers to float64 data, the strides (in doubles) are positive; row-major (col_stride = 1) and column-major
 * (row_stride = 1) sources are read coalesced, any other strides are gathered.  One kernel launch packs all groups on the
 * context's stream, which is synchronised before the call returns.  The context holds a COPY: the sources may be
 * overwritten or freed afterwards.  Work that produced the sources must be ordered before the context's stream (the same
 * stream, or the caller synchronises).
 * LC_EINVAL, before anything is launched and with the context unchanged: a pointer of a group with rows that is NULL,
 * host memory, managed memory or memory of another device than the context's (the message names the group), a
 * non-positive stride, J < 1, D < 1, a negative group size. */
int lc_ctx_set_data_device(lc_ctx* ctx, int J, const double* const* Xj_dev, const int64_t* Nj, int D, int64_t row_stride,
                           int64_t col_stride);
/* The smallest observation that is a number (+inf when there is none) and how many observations are NaN (unknown values,
 * lc_model_predict_incomplete).  After lc_ctx_set_data_device these are what its pass over the data left behind; after
 * anything else filled or changed the observations, one reduction pass over them.  The same bits on every call.  Either
 * pointer may be NULL. */
int lc_ctx_data_range(lc_ctx* ctx, double* min, int64_t* n_nan);
/* Synthetic K-component full-covariance Gaussian mixture generated on the
 * device (bench workload): x = mu_z + L_z eps, z uniform,
 * Philox-4x32-10 keyed by `seed`, counter = row_offset + row.  Also writes the
 * initial qZ (true label = `hard`, rest (1-hard)/(K-1)).  mu: K x D, L: K x D x D
 * row-major lower Cholesky factors (host pointers). */
int lc_ctx_synth(lc_ctx* ctx, int64_t N, int D, int K, const double* mu, const double* L, uint64_t seed,
                 int64_t row_offset, double hard);
/* Grouped variant (GMC workload): J groups of Nj rows; cdf = J x K cumulative mixing proportions of
 * each group (NULL: uniform labels); group_ids = J global group ids used as Philox counters, so a group is
 * identical on whichever rank generates it (NULL: 0..J-1). */
int lc_ctx_synth_groups(lc_ctx* ctx, int J, const int64_t* Nj, int D, int K, const double* mu, const double* L,
                        const double* cdf, uint64_t seed, const int64_t* group_ids, double hard);
/* rows [row0,row0+n) of group j -> row-major n x D host buffer */
int lc_ctx_get_rows(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* out);

/* qZ (the `vMatrixXd& qZ` of cluster.cpp:179): host <-> device, any strides. */
int lc_ctx_set_qz(lc_ctx* ctx, int j, const double* q, int K, int64_t row_stride, int64_t col_stride);
int lc_ctx_get_qz(lc_ctx* ctx, int j, double* q, int64_t row_stride, int64_t col_stride);
/* rows [row0,row0+n) of group j only (qZ[j].block(row0,0,n,K)) */
int lc_ctx_get_qz_rows(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* q, int64_t row_stride, int64_t col_stride);
/* ... into DEVICE memory of the context's device: q_dev[r*row_stride + k*col_stride], positive strides (row-major
 * destinations go through an LDS tile, column-major ones are K contiguous copies).  Enqueued on the context's stream and
 * NOT synchronised (lc_ctx_synchronize).  LC_EINVAL as lc_ctx_get_qz_rows, and for a q_dev that is not plain device
 * memory of that device or a non-positive stride, before anything is launched. */
int lc_ctx_get_qz_rows_device(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* q_dev, int64_t row_stride,
                              int64_t col_stride);
/* every group at once: q is [sum_j N_j x K] row-major, the groups' rows concatenated (one transfer) */
int lc_ctx_get_qz_all(lc_ctx* ctx, double* q);
/* every group at once, q[j] = the N_j x K matrix of group j in column-major order (Eigen's default: the `vMatrixXd& qZ`
 * of cluster.cpp:179 as the caller holds it); no transpose on either side */
int lc_ctx_get_qz_all_colmajor(lc_ctx* ctx, double* const* q);
int lc_ctx_fill_qz(lc_ctx* ctx, int K, double value); /* qZ[j].setOnes(N,1): cluster.cpp:583-585 */

/* ---- the hot path ------------------------------------------------------ */
/* vbexpectation (cluster.cpp:91-138) for ALL groups, from the posterior
 * hyper-parameters the reference keeps inside GaussWish (distributions.h:
 * 325-330) and the weights' Elogweight() (distributions.h:113/173):
 *   nu[K], beta[K], m[K*D], iW[K*D*D] row-major, logdW[K], Elogpi[J*K],
 *   active[J*K] (sparse mask: 0 => column zeroed, cluster.cpp:109-112/134-135)
 *   or NULL.  Overwrites the context's qZ with the new responsibilities.
 * Fz  <- -sum_n logZ_n  (cluster.cpp:137, summed over groups as in :221-223)
 * LLk <- K values sum_n q_nk * Eloglike_k(x_n) (data term of cluster.cpp:409-410) or NULL. */
int lc_estep_posterior(lc_ctx* ctx, int K, const double* nu, const double* beta, const double* m, const double* iW,
                       const double* logdW, const double* Elogpi, const unsigned char* active, double* Fz,
                       double* LLk);
/* Same kernel, kernel-level parameters: A[K*D*D] row-major lower-triangular
 * with nu*maha_k(x) = ||A_k (x - m_k)||^2, m[K*D], c[J*K] = Elogpi_jk +
 * 0.5*(sum psi + logdW - D/beta - D ln pi).  LLk here excludes the constant:
 * LLk = sum_n q_nk (log q~_nk - c_jk). */
int lc_estep(lc_ctx* ctx, int K, const double* A, const double* m, const double* c, double* Fz, double* LLk);
/* K x GaussWish::Eloglike(X) (distributions.cpp:356-370) for ALL groups: column k of the
 * context's qZ receives the expected log-likelihood of every observation under cluster k
 * (no weights, no normalisation); fetch it with lc_ctx_get_qz. */
int lc_eloglike(lc_ctx* ctx, int K, const double* nu, const double* beta, const double* m, const double* iW,
                const double* logdW);
/* probutils::mahaldist (probutils.cpp:113-138) on the context's observations: dist[n] = (x_n - mu) A^-1 (x_n - mu)^T
 * for every row of every group (concatenated); A is D x D row-major, symmetric positive definite, else LC_EINVAL
 * "Matrix A is not positive definite".  Overwrites the context's qZ (one scratch column). */
int lc_mahaldist(lc_ctx* ctx, const double* mu, const double* A, double* dist);
/* updateSS (cluster.cpp:53-82) + K x GaussWish::addobs (distributions.cpp:301-313)
 * for ALL groups on the current qZ: Nk[K], xs[K*D], xxs[K*D*D] (row-major),
 * Njk[J*K] (the returned `Njk` of every group).  smask[J*K]: sparse updates,
 * 0 => group j contributes nothing to cluster k (cluster.cpp:67-79); NULL = dense.
 * Any output pointer may be NULL. */
int lc_suffstat(lc_ctx* ctx, const unsigned char* smask, double* Nk, double* xs, double* xxs, double* Njk);
/* The diagonal / exponential families (NormGamma, ExpGamma: distributions.cpp:418-590).
 * updateSS + K x NormGamma::addobs / ExpGamma::addobs (distributions.cpp:426-438, 533-542) for ALL groups:
 * Nk[K], xs[K*D] = sum_n q_nk x_n, xxs[K*D] = sum_n q_nk x_n.^2 (NULL for ExpGamma), Njk[J*K]. */
int lc_suffstat_diag(lc_ctx* ctx, const unsigned char* smask, double* Nk, double* xs, double* xxs, double* Njk);
/* vbexpectation with clusters whose Eloglike is separable over dimensions:
 *   log q~_nk = c_jk + sum_d [ w2_kd (x_nd - a_kd)^2 + w1_kd x_nd ]         a, w2, w1: K*D each, c: J*K
 * NormGamma::Eloglike (distributions.cpp:483-492): a = m, w2 = -nu/(2L), w1 = 0,
 *   c = Elogpi + 0.5*(D*(psi(nu) - ln 2pi - 1/beta) - logL).
 * ExpGamma::Eloglike (distributions.cpp:568-572): a = 0, w2 = 0, w1 = -a*ib, c = Elogpi + D*psi(a) - logb.
 * raw != 0: no weights/normalisation, column k of qZ receives log q~ (the Eloglike columns).
 * Fz / LLk as lc_estep. */
int lc_estep_diag(lc_ctx* ctx, int K, const double* a, const double* w2, const double* w1, const double* c, int raw,
                  double* Fz, double* LLk);
/* qZ[j].colwise().sum() for every group (cluster.cpp:62, 546) */
int lc_colsums(lc_ctx* ctx, double* Njk);

/* ---- multi-GPU: rows are sharded one context per rank; the two per-iteration
 * reductions (packed suff-stats, [Fz; LLk]) call this hook on a device buffer.
 * fn must sum `count` doubles in place across ranks, ordered after work already
 * enqueued on `stream`; return 0 on success. */
typedef int (*lc_allreduce_fn)(void* user, void* device_buf, int64_t count, void* stream);
int lc_ctx_set_allreduce(lc_ctx* ctx, lc_allreduce_fn fn, void* user);
/* Native collectives (libcluster_amd/csrc/lc_comm.cpp) -- nothing in the reference corresponds: its loop over groups
 * (cluster.cpp:207-223) is single-process OpenMP; this is that loop distributed.  A context with a communicator sums
 * its packed statistics and [Fz; LL_k] over the ranks on its own stream; the communicator takes precedence over a hook.
 *   RCCL: rank 0 calls lc_comm_unique_id and ships the LC_COMM_ID_BYTES to the other ranks (any channel); every rank
 *         then calls lc_ctx_comm_init_rccl (ncclCommInitRank on the context's device; one rank per GPU;
 *         ncclAllReduce(ncclDouble, ncclSum) over xGMI).  librccl is bound on first use.
 *   host: staged through the POSIX shared-memory object "/lc_comm_<name>", summed in rank order by every rank -- any
 *         placement of the ranks of one node, including several ranks on one GPU (which RCCL refuses). */
#define LC_COMM_ID_BYTES 128
int lc_comm_rccl_available(void); /* 1 when librccl could be loaded */
int lc_comm_unique_id(void* id /* LC_COMM_ID_BYTES */);
int lc_ctx_comm_init_rccl(lc_ctx* ctx, const void* id, int rank, int world);
int lc_ctx_comm_init_host(lc_ctx* ctx, const char* name, int rank, int world);
int lc_ctx_comm_free(lc_ctx* ctx);
/* kind: "rccl" | "host-shm" | "host-local" | "hook" | "none" (static string) */
int lc_ctx_comm_info(lc_ctx* ctx, int* rank, int* world, const char** kind);
/* sum n host doubles over the ranks of the context's communicator / hook (identity without one) */
int lc_ctx_allreduce(lc_ctx* ctx, double* values, int n);
/* How a distributed run is sharded.  0 (default): every rank holds rows of the SAME groups (BGMM / VDP row
 * blocks; also GMC with every group split by rows) -- statistics and per-group counts are summed.
 * 1: every rank holds WHOLE, different groups (GMC) -- cluster statistics, Fz, LL_k and the
 * weights' free energy are summed, the per-group counts N_jk and the group weights stay local. */
int lc_ctx_set_sharding(lc_ctx* ctx, int whole_groups);
/* Statistics pass: skip every (4-row step, cluster) pair whose responsibilities are all exactly 0.0.  Their
 * contribution is exactly zero, so results are bit-identical; it pays off once qZ is mostly hard (late EM
 * iterations on separated data).  Off by default (the dense kernel has no test in its inner loop); always on in the
 * reference's `sparse` mode, whose point is to leave massless (group, cluster) pairs out (cluster.cpp:67-79). */
int lc_ctx_set_skip_zero(lc_ctx* ctx, int on);

/* Statistics pass, feature-GEMM kernel (dense passes at 32 <= D <= 128 and more than 12 clusters): leave out every
 * (4-row step, cluster quad) pair whose sixteen responsibilities are all below 2^-300.  Once the posteriors have
 * sharpened that is most of the pass.  A statistic loses at most N * 2^-300 * max |x_u x_w| in absolute terms; NaN
 * responsibilities are kept.  A probe of qZ in front of every such pass (a fixed, strided sample of 4-row steps: a
 * deterministic function of qZ) sends the pass to the dense kernel when fewer than a quarter of the pairs could be skipped,
 * and passes of fewer than 4096 rows are always dense.  Where the probe finds at most half of the pairs kept and D < 128,
 * the skipping kernel sorts the rows of every staged batch (32 or 48 rows) by the cluster quad that owns them before it
 * forms the 4-row steps, when every row of the batch has at most one such quad; the bound above holds either way.  On by default; 0 restores the pass that multiplies every speck.
 * The other statistics kernels are not affected.  Sub-problems of the split search inherit the setting. */
int lc_ctx_set_speck_skip(lc_ctx* ctx, int on);
/* How many statistics passes of this context ran the skipping kernel, and how many the probe sent to the dense one
 * (either pointer may be NULL). */
int lc_ctx_speck_passes(lc_ctx* ctx, int64_t* skipping, int64_t* dense);
/* How many of the skipping passes took the list route: at D <= 64 (a padded width of 64 columns), where the probe finds
 * that at least 58 of every 64 sampled rows keep values of exactly one cluster quad, the pass first writes, per row
 * chunk and quad, the list of the rows that keep a value of that quad, and then sums every list on its own.  At
 * 57 <= D <= 64 a listed row is summed into a cluster of the quad only where that cluster's own responsibility is not
 * below 2^-300 (one wave per cluster).  Same records, same bound; lc_ctx_set_speck_skip(ctx, 0) turns it off with the rest. */
int lc_ctx_speck_list_passes(lc_ctx* ctx, int64_t* lists);
/* A Gauss-Wishart E-step at 49 <= D <= 64 (a padded width of 64 columns) whose statistics pass could take the list route
 * (the feature-GEMM kernel owns it: more than 16 clusters there) writes, next to the responsibilities,
 * one bit per (row, cluster quad): "the row keeps a value of the quad", taken on the value it stores.  The pass that
 * follows then takes the probe's counts and builds its lists from those bits instead of reading qZ again.  Any other
 * writer of qZ withdraws the bits, and the pass probes and builds from qZ as before.  Same results bit for bit.  On by
 * default; sub-problems of the split search inherit the setting. */
int lc_ctx_set_estep_masks(lc_ctx* ctx, int on);
/* How many list passes of this context were built from such bits. */
int lc_ctx_speck_mask_passes(lc_ctx* ctx, int64_t* masks);

/* Device and page-locked blocks released by contexts are cached for re-use (the split search builds a context per
 * attempt); this returns all of them to the driver. */
int lc_trim_cache(void);

/* ---- kernel timing (hipEvents on the context's stream) ------------------ */
int lc_ctx_timing_enable(lc_ctx* ctx, int on);
int lc_ctx_timing_reset(lc_ctx* ctx);
int lc_ctx_timing_get(lc_ctx* ctx, double* estep_ms, int64_t* estep_calls, double* suffstat_ms,
                      int64_t* suffstat_calls);
/* launches of the fused pass (small observations, D <= 16: vbexpectation + the next iteration's updateSS in one kernel) */
int lc_ctx_timing_get_fused(lc_ctx* ctx, double* fused_ms, int64_t* fused_calls);
/* Everything the context timed since the last reset, for the per-rank report of a multi-GPU run (the loop over groups
 * of src/cluster.cpp:207-223, one rank per GPU): out[0..LC_TIMING_FIELDS-1] =
 *   0 estep_ms  1 estep_calls  2 suffstat_ms  3 suffstat_calls  4 fused_ms  5 fused_calls
 *   6 allreduce_ms  7 allreduce_calls   (events around the exchange step: the sum + the wait for the slowest rank)
 *   8 host_stats_ms  9 host_mstep_ms  10 host_estep_ms  11 host_fenergy_ms  12 host_iters
 *     (host wall time per phase of the VBEM iterations: statistics pass + weights update, cluster M-step + parameter
 *      packing, E-step, free energy)
 *   13 estep_diag_mfma_calls  (separable families: how many of the estep_calls took estep_diag_mfma_kernel, the
 *      matrix-pipe form of NormGamma / ExpGamma::Eloglike, distributions.cpp:483-492, 568-581; the rest ran estep_diag_kernel) */
#define LC_TIMING_FIELDS 14
int lc_ctx_timing_get_all(lc_ctx* ctx, double* out, int n);

/* ======================================================================== *
 * Variational Bayes EM on a context (vbem, cluster.cpp:177-239).
 * The model is created on first use (*model == NULL) with `wkind` weights of
 * prior `wprior` and `ckind` clusters (lc_ckind) of prior `clusterprior`.
 * fixed_iters >= 0 runs exactly that many iterations without the convergence
 * and free-energy-increase tests (bench / parity harness: the reference has no
 * public fixed-K entry point).  Ftrace (may be NULL) gets
 * up to ntrace values of F, one per iteration; *niter the iterations run.
 * ======================================================================== */
int lc_vbem(lc_ctx* ctx, lc_model** model, int wkind, int ckind, double wprior, double clusterprior, int maxit,
            int sparse, int fixed_iters, int verbose, unsigned nthreads, double* F, int* niter, double* Ftrace,
            int ntrace);

/* prune_clusters (cluster.cpp:505-552) on a model lc_vbem produced and its context: clusters whose getN() is below
 * ZEROCUTOFF leave the model and their columns leave qZ; every group's weights are then updated with the remaining
 * columns' sums (not renormalised, cluster.cpp:546).  *removed (may be NULL) = how many went.  cluster() calls this
 * between vbem and the split search (cluster.cpp:606). */
int lc_prune(lc_ctx* ctx, lc_model* model, int verbose, int* removed);

/* learnVDP / learnBGMM / learnDGMM / learnBEMM / learnGMC / learnSGMC / learnDGMC / learnEGMC
 * (cluster.cpp:636-873; lc_algo): uploads X,
 * runs the model-selection loop, returns the model (which owns its context so
 * qZ can be fetched).  wprior: StickBreak concentration / Dirichlet alpha the
 * caller's `weights` argument carried (1.0 = default-constructed); ignored
 * for the multi-group learners (default-constructed GDirichlet / Dirichlet per group, cluster.cpp:192).
 * BEMM / EGMC: LC_EINVAL "X has to be in the range [0, inf)!" on a negative observation (cluster.cpp:742, 862). */
/* Environment (the frozen learn*() signatures have no room for it): LIBCLUSTER_GPUS = N | "all" shards the
 * observations over N GPUs of this node inside this one call -- row blocks for the single-matrix learners, whole
 * groups for the GMC family -- one host thread and one context per GPU, RCCL all-reduce of the statistics; results
 * (F, rounds, qZ, weights, clusters) are returned exactly as from one GPU.  `device` is then ignored (GPUs 0..N-1).
 * LIBCLUSTER_COMM = "host" (host-staged sum in rank order, any placement) | "rccl-gather" (ncclAllGather + the same
 * rank-order additions on every GPU: results independent of RCCL's ring order); default ncclAllReduce. */
int lc_learn(int algo, int J, const double* const* Xj, const int64_t* Nj, int D, int64_t row_stride,
             int64_t col_stride, double wprior, double clusterprior, int maxclusters, int sparse, int verbose,
             unsigned nthreads, int device, lc_model** out, double* F);

/* The same with the prior of EVERY group's weight distribution (wprior_j[J], NULL = defaults): what the caller's
 * `std::vector<Dirichlet>& weights` carries into learnSGMC (vbem's weights.resize(J, W()) keeps existing elements,
 * cluster.cpp:192).  GDirichlet has no parameter (ignored there); single-matrix learners use `wprior`. */
int lc_learn_w(int algo, int J, const double* const* Xj, const int64_t* Nj, int D, int64_t row_stride,
               int64_t col_stride, double wprior, const double* wprior_j, double clusterprior, int maxclusters,
               int sparse, int verbose, unsigned nthreads, int device, lc_model** out, double* F);
/* lc_learn_w on observations that already live in ctx (lc_ctx_set_data_device, lc_ctx_set_data, lc_ctx_synth): the same
 * algorithms, priors, messages and results as the one-device path of lc_learn_w on the same rows.  The data lives on one
 * device: LIBCLUSTER_GPUS is not consulted.  The ExpGamma learners take "X has to be in the range [0, inf)!" from
 * lc_ctx_data_range's minimum, before anything is printed or learned.  The returned model borrows ctx, as lc_cluster's. */
int lc_learn_ctx(int algo, lc_ctx* ctx, double wprior, const double* wprior_j, double clusterprior, int maxclusters,
                 int sparse, int verbose, unsigned nthreads, lc_model** out, double* F);

/* The same model-selection loop (cluster(), cluster.cpp:564-629) on observations that already live in
 * a context (lc_ctx_set_data or lc_ctx_synth): nothing but the M-step statistics crosses PCIe, the
 * split search (partobs / splitobs / auglabels, cluster.cpp:438-470) runs on the device too.
 * wkind / wprior as in lc_vbem (GDirichlet and per-group Dirichlet ignore wprior for new groups).
 * The returned model borrows ctx (keep it alive while reading qZ through the model). */
int lc_cluster(lc_ctx* ctx, int wkind, int ckind, double wprior, double clusterprior, int maxclusters, int sparse,
               int verbose, unsigned nthreads, lc_model** out, double* F);

/* ---- model accessors ----------------------------------------------------- */
int lc_model_free(lc_model* m);
int lc_model_dims(lc_model* m, int* J, int* K, int* D);
int lc_model_rounds(lc_model* m, int* nrounds);                       /* vbem rounds of cluster() */
int lc_model_round(lc_model* m, int r, int* K, int* niter, double* F, int nF); /* F trace of round r */
int lc_model_get_qz(lc_model* m, int j, double* q, int64_t row_stride, int64_t col_stride);
int lc_model_get_qz_all(lc_model* m, double* q); /* all groups, [sum_j N_j x K] row-major */
int lc_model_get_qz_all_colmajor(lc_model* m, double* const* q); /* q[j]: N_j x K column-major (see lc_ctx_...) */
/* WeightDist::Elogweight() / getNk() of group j (K values each; may be NULL) */
int lc_model_weights(lc_model* m, int j, double* Elogweight, double* Nk);
int lc_model_kinds(lc_model* m, int* wkind, int* ckind);
/* Cluster k (any pointer may be NULL).
 * GaussWish: getN(), getmean() [D], getcov() [D*D row-major], posterior nu, beta, iW [D*D], logdW.
 * NormGamma: getN(), getmean() [D], cov [D] = getcov() = L*nu (distributions.h:375), nu, beta, iW [D] = L,
 *            logdW = logL.
 * ExpGamma:  getN(), mean [D] = getrate() = a*ib (distributions.h:433), cov must be NULL, nu = a, beta = 0,
 *            iW [D] = ib, logdW = logb. */
int lc_model_cluster(lc_model* m, int k, double* N, double* mean, double* cov, double* nu, double* beta, double* iW,
                     double* logdW);
int lc_model_fenergy(lc_model* m, double* Fw /*[J]*/, double* Fc /*[K]*/);

/* ---- prediction on new observations (nothing in the reference corresponds: its users call
 * clusters[k].Eloglike(Xnew), distributions.cpp:356-370 / 483-492 / 568-572, and do vbexpectation's log-sum-exp,
 * cluster.cpp:91-138, themselves).  The new rows live in ctx (lc_ctx_set_data / lc_ctx_synth); block b of ctx is scored
 * with the weights of learned group groups[b] (NULL: group 0).  Per row:
 *   qZ    (keep_qz != 0: the context's qZ, K columns) vbexpectation with the model's final posteriors and Elogweight()
 *         of the group; sparse models use the same Kful rule, getNk() >= ZEROCUTOFF (cluster.cpp:107-112)
 *   logZ  log sum_{k in Kful} exp(E[log pi_jk] + Eloglike_k(x)): the row's term of Fxz = -sum logZ (cluster.cpp:121-137)
 *   label argmax_k of E[log pi_jk] + Eloglike_k(x) (the largest responsibility), lowest k on ties
 *   logp  log p(x | training data) = log(sum_k E[pi_jk] P_k(x) + E[pi_rest] P_0(x)), P_k the posterior predictive of
 *         cluster k (multivariate Student-t / product of Student-t / product of Lomax), P_0 that of the cluster prior
 *         (StickBreak only: the mass beyond the truncation)
 * Works for models of lc_learn / lc_learn_w (sharded ones included), lc_vbem and lc_cluster, on the device of ctx.
 * LC_EINVAL: D mismatch ("Mismatched dims. of cluster params and obs.!"), a group index outside [0, J), a negative
 * observation for ExpGamma clusters ("X has to be in the range [0, inf)!", cluster.cpp:742), a freed model.
 * Without keep_qz the context's qZ holds intermediate values afterwards. */
int lc_model_predict(lc_model* m, lc_ctx* ctx, const int* groups /* [J of ctx] or NULL */, int keep_qz);
/* rows [row0, row0+n) of block j of the last prediction on ctx (like lc_ctx_get_qz_rows); any output may be NULL */
int lc_ctx_get_predictions(lc_ctx* ctx, int j, int64_t row0, int64_t n, int32_t* label, double* logZ, double* logp);
/* ... into DEVICE arrays of the context's device (any may be NULL): device-to-device copies enqueued on the context's
 * stream and NOT synchronised (lc_ctx_synchronize).  LC_EINVAL as lc_ctx_get_predictions, and for an output that is not
 * plain device memory of that device, before anything is enqueued. */
int lc_ctx_get_predictions_device(lc_ctx* ctx, int j, int64_t row0, int64_t n, int32_t* label_dev, double* logZ_dev,
                                  double* logp_dev);
/* ---- conditional prediction (nothing in the reference corresponds): some columns of a new row are known,
 * the others are wanted.  Gauss-Wishart models only.  ctx holds the KNOWN columns only: its width is ngiven and its column
 * i is model column given[i]; target lists the wanted model columns (NULL: every column that is not given, ascending;
 * ntarget is not looked at then).  Block b of ctx is mixed with the weights of learned group groups[b] (NULL: group 0).
 * With a = given, b = target, cluster k's posterior (nu, beta, m, iW) and nu' = nu + 1 - D (D the model's full width):
 *   P_k,a(x_a)  Student-t, nu' degrees of freedom, location m_a, scale (1 + beta) / (beta nu') iW_aa: the marginal of the
 *               posterior predictive lc_model_predict mixes
 *   M_k(x_a)  = m_b + iW_ba iW_aa^-1 (x_a - m_a): the cluster's linear expert (the conditional mean of that Student-t)
 *   logp      = log(sum_k E[pi_jk] P_k,a(x_a) + E[pi_rest] P_0,a(x_a)), the prior component as in lc_model_predict
 *   mean      = sum_k r_k M_k(x_a), r_k = E[pi_jk] P_k,a(x_a) / exp(logp): E[x_b | x_a, training data]
 * All K clusters take part, also for sparse models (as in logp of lc_model_predict).  Works for the same models as
 * lc_model_predict.  Replaces any prediction ctx held (lc_ctx_get_predictions reports none afterwards); a call that
 * fails leaves none.  The context's qZ holds intermediate values afterwards.
 * LC_EINVAL: clusters that are not Gauss-Wishart, ngiven < 1, no target column, an index outside [0, D), an index
 * twice in a list, a column in both lists, a context whose width is not ngiven, a group index outside [0, J), a freed
 * model. */
int lc_model_predict_conditional(lc_model* m, lc_ctx* ctx, const int* groups /* [J of ctx] or NULL */, const int* given,
                                 int ngiven, const int* target /* or NULL */, int ntarget);
/* rows [row0, row0+n) of block j of the last conditional prediction on ctx: mean is n x ntarget with row_stride doubles
 * between rows (>= ntarget), logp n values; either may be NULL.  LC_EINVAL: no conditional prediction on ctx, a row
 * range out of bounds. */
int lc_ctx_get_conditional(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* mean, int64_t row_stride, double* logp);
/* ---- predictive variance of the conditional prediction (nothing in the reference corresponds).  Everything
 * lc_model_predict_conditional does, and per row the diagonal of the mixture's predictive covariance of the target columns.
 * The conditional of cluster k's predictive Student-t has nu' + ngiven degrees of freedom, location M_k(x_a) and, with
 * d^2 = nu (x_a - m_a)^T iW_aa^-1 (x_a - m_a) and s = beta / ((1 + beta) nu), the covariance
 *   Cov_k(x_a) = g_k (1 + s d^2) S_k,  S_k = iW_bb - iW_ba iW_aa^-1 iW_ab,  g_k = (1 + beta) / (beta (nu' + ngiven - 2))
 *   var_t     = sum_k r_k (Cov_k(x_a)_tt + (M_k,t - mean_t)^2): within the experts plus between them, centred on mean
 * in the order of target; the prior component of StickBreak weights takes part as in mean.  mean and logp are those of
 * lc_model_predict_conditional, bit for bit.  LC_EINVAL: the cases of lc_model_predict_conditional.  LC_EDOMAIN, before
 * anything runs on the device: a component with positive weight has nu' + ngiven <= 2, so that its covariance does not
 * exist (every StickBreak model with ngiven = 1: the prior component has nu' = 1); the message names the component, no
 * prediction is left on ctx, and lc_model_predict_conditional still works.  A learned cluster that ended up empty has a
 * huge but finite variance, which is returned as it is. */
int lc_model_predict_conditional_var(lc_model* m, lc_ctx* ctx, const int* groups /* [J of ctx] or NULL */, const int* given,
                                     int ngiven, const int* target /* or NULL */, int ntarget);
/* rows [row0, row0+n) of block j of the variance of the last lc_model_predict_conditional_var on ctx: var is n x ntarget
 * with row_stride doubles between rows (>= ntarget); it may be NULL (the checks only).  mean and logp of the same call:
 * lc_ctx_get_conditional.  LC_EINVAL: no conditional prediction on ctx, one without variance
 * (lc_model_predict_conditional), a row range out of bounds, row_stride < ntarget. */
int lc_ctx_get_conditional_var(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* var, int64_t row_stride);
/* ---- draws of the conditional (nothing in the reference corresponds).  Everything lc_model_predict_conditional
 * does, mean and logp bit for bit, and per row ndraws draws of the target columns from p(x_b | x_a, training data): draw i
 * chooses component k with the responsibilities r_k (the prior component takes part as in mean) and draws cluster k's
 * conditional Student-t with eta = nu' + ngiven degrees of freedom,
 *   x_b = M_k(x_a) + sqrt(c_k (1 + s d^2)) L_k z sqrt(eta / chi^2_eta),  c_k = (1 + beta) / (beta eta),  L_k = chol(S_k)
 * with S_k, s and d^2 as in lc_model_predict_conditional_var.  m completed copies of a table, each from one draw per row, are
 * a multiple imputation.  A draw depends on (seed, block, row, i) and the row's values only: not on the number of rows, on
 * ndraws or on other rows; the same call gives the same bits.  Random numbers: the table at the top of this header.
 * LC_EINVAL: the cases of lc_model_predict_conditional, ndraws outside [1, LC_DRAWS_MAX].  LC_EDOMAIN, before anything runs
 * on the device: an S_k that is not numerically positive definite.  No moment has to exist. */
#define LC_DRAWS_MAX 64
int lc_model_predict_conditional_draws(lc_model* m, lc_ctx* ctx, const int* groups /* [J of ctx] or NULL */, const int* given,
                                       int ngiven, const int* target /* or NULL */, int ntarget, int ndraws, uint64_t seed);
/* rows [row0, row0+n) of block j of the draws of the last lc_model_predict_conditional_draws on ctx: draws is n x ndraws x
 * ntarget, label n x ndraws (the component of every draw; K = the prior component); either may be NULL.  mean and logp of
 * the same call: lc_ctx_get_conditional.  LC_EINVAL: no such prediction on ctx, a row range out of bounds. */
int lc_ctx_get_conditional_draws(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* draws, int32_t* label);
/* the shape of those draws: ndraws and ntarget of the last lc_model_predict_conditional_draws on ctx, both 0 when ctx holds
 * no such prediction (never an error for that): what a caller sizes the buffers of lc_ctx_get_conditional_draws with.
 * Either pointer may be NULL. */
int lc_ctx_conditional_draws(lc_ctx* ctx, int* ndraws, int* ntarget);
/* ---- new rows from a learned model (nothing in the reference corresponds).  Fills ctx with J blocks of Nj[b]
 * rows at the model's width D: afterwards ctx is as after lc_ctx_set_data with those rows (lc_ctx_get_rows and every
 * lc_model_predict* call work on it; the data, qZ and predictions it held are gone).  Every row is one draw from the density
 * whose logarithm lc_model_predict returns as logp: the component is chosen with E[pi_jk] of learned group groups[b] (NULL:
 * group 0), the prior component with E[pi_rest] (StickBreak); all K clusters take part, also for sparse models.  Then
 *   Gauss-Wishart  x = m + sqrt((1 + beta) / (beta nu')) chol(iW) z sqrt(nu' / chi^2_nu'),  nu' = nu + 1 - D
 *   NormGamma      per column a Student-t with 2 nu degrees of freedom, location m_d, scale^2 (1 + beta) L_d / (beta nu)
 *   ExpGamma       per column a Lomax with shape a and scale 1 / ib_d, by inverse CDF (every value >= 0)
 * No moment has to exist.  Rows [a, b) of a call with row_offset = 0 are the rows of a call for b - a rows with row_offset =
 * a, bit for bit, and block b's rows do not depend on J.  LC_EINVAL: a freed model, no clusters, J < 1, a negative Nj, a
 * group index outside [0, J of the model), Gauss-Wishart with D > 1024; ctx is untouched then. */
int lc_model_sample(lc_model* m, lc_ctx* ctx, int J, const int64_t* Nj, const int* groups /* [J] or NULL: group 0 */,
                    uint64_t seed, int64_t row_offset);
/* the components of rows [row0, row0+n) of block j of a context filled by lc_model_sample (K = the prior component).
 * LC_EINVAL: the context's rows do not come from lc_model_sample, a row range out of bounds. */
int lc_ctx_get_sample_labels(lc_ctx* ctx, int j, int64_t row0, int64_t n, int32_t* label);
/* ---- rows whose unknown columns differ from row to row (nothing in the reference corresponds).  Gauss-Wishart
 * models only.  ctx holds the rows at the model's FULL width D; a NaN marks an unknown value ("hole"), +-inf is data.  A row
 * may have up to LC_HOLES_MAX holes and needs at least one known column; every row has its own set.  Block b of ctx is mixed
 * with the weights of learned group groups[b] (NULL: group 0).  With a = the known columns of a row, b = its holes, nb = |b|
 * and P_k,a, M_k as in lc_model_predict_conditional above, after the call
 *   the context's observations hold the completed rows: every NaN is replaced by E[x_b | x_a, training data] =
 *     sum_k r_k M_k(x_a); every other value keeps its bits (lc_ctx_get_rows and lc_ctx_get_completed return them)
 *   logp = log p(x_a | training data) per row and the per-row hole records (count, columns) are on the device.  A row
 *     without holes has the logp of lc_model_predict.
 * All K clusters take part, also for sparse models.  Works for the same models as lc_model_predict.  Replaces any prediction
 * ctx held (lc_ctx_get_predictions and lc_ctx_get_conditional report none afterwards); a call that fails leaves none, and
 * leaves the observations untouched, NaNs included.  The context's qZ holds intermediate values afterwards.  A second call
 * on the same context finds no NaN any more: it scores the completed rows as fully observed (every count 0).
 * An empty context is LC_OK.  LC_EINVAL: clusters that are not Gauss-Wishart, D mismatch ("Mismatched dims. of cluster
 * params and obs.!"), a group index outside [0, J), a freed model, and a row with more than LC_HOLES_MAX NaNs or without a
 * known column -- the message names block, row and count of the first such row in (block, row) order; for a pattern shared
 * by all rows, of any size, there is lc_model_predict_conditional. */
#define LC_HOLES_MAX 8
int lc_model_predict_incomplete(lc_model* m, lc_ctx* ctx, const int* groups /* [J of ctx] or NULL */);
/* rows [row0, row0+n) of block j after the last lc_model_predict_incomplete on ctx: rows is n x D (the completed rows) with
 * row_stride doubles between rows (>= D), logp n values, count n values (the holes the row had), cols n x LC_HOLES_MAX (their
 * columns, ascending, -1 beyond count).  Any output may be NULL.  LC_EINVAL: no such prediction on ctx, a row range out of
 * bounds, row_stride < D. */
int lc_ctx_get_completed(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* rows, int64_t row_stride, double* logp,
                         int32_t* count, int32_t* cols);
/* ---- predictive variance of the filled values (nothing in the reference corresponds).  Everything
 * lc_model_predict_incomplete does, and per row the diagonal of the mixture's predictive covariance of its holes.  With
 * a, b, nb as above, Da = D - nb, H = (P_k)_bb, d_a^2 the distance of the known columns and s = beta / ((1 + beta) nu), the
 * conditional of cluster k's predictive Student-t has nu' + Da degrees of freedom, location M_k(x_a) and the covariance
 *   Cov_k(x_a) = g_k(nb) (1 + s d_a^2) S_k,  S_k = iW_bb - iW_ba iW_aa^-1 iW_ab = nu H^-1,  g_k(nb) = (1 + beta) / (beta (nu - 1 - nb))
 *   var_i     = sum_k r_k (Cov_k(x_a)_ii + (M_k,i - mean_i)^2): within the experts plus between them, centred on mean
 * for hole i of the row, in the order of cols (ascending); the prior component of StickBreak weights takes part as in the
 * completed rows.  Completed rows, logp, count and cols are those of lc_model_predict_incomplete, bit for bit.
 * LC_EINVAL: the cases of lc_model_predict_incomplete.  LC_EDOMAIN, after the scan and before anything is written to the
 * observations: a component with positive weight in some block has nu - 1 - cmax <= 0, where cmax is the largest hole
 * count of the WHOLE context -- conservative (the row with cmax holes may give that component next to no weight, and may
 * sit in another block) and strict, as in lc_model_predict_conditional_var.  In practice: a row with a single known
 * column scored against the prior component of StickBreak weights (nu = D) or a cluster that ended up empty.  The
 * message names the component and the count; the NaNs stay, no prediction is left on ctx, and
 * lc_model_predict_incomplete on the same context still works.  A context without holes never fails this check. */
int lc_model_predict_incomplete_var(lc_model* m, lc_ctx* ctx, const int* groups /* [J of ctx] or NULL */);
/* rows [row0, row0+n) of block j of the variance of the last lc_model_predict_incomplete_var on ctx: var is n x LC_HOLES_MAX
 * with row_stride doubles between rows (>= LC_HOLES_MAX); slot i belongs to cols[i] of lc_ctx_get_completed, the slots
 * i >= count are exactly 0.0, and so is every slot of a row without holes.  var may be NULL (the checks only).  LC_EINVAL:
 * no incomplete prediction on ctx, one without variance (lc_model_predict_incomplete), a row range out of bounds,
 * row_stride < LC_HOLES_MAX. */
int lc_ctx_get_completed_var(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* var, int64_t row_stride);
/* ---- draws of the unknown values of rows with holes (nothing in the reference corresponds).  Everything
 * lc_model_predict_incomplete does (the context's rows hold the MEAN-completed rows afterwards), and per row ndraws draws of
 * its holes from the mixture of the clusters' conditional Student-t densities: multiple imputation for rows that each miss
 * their own columns.  With the notation above, L L^T = H = (P_k)_bb and e_k(nb) = (nu' + Da) / 2, draw i of a row
 *   chooses k by inverse CDF over r_k = exp(t_k - logp) (0 ... K-1, then the prior component),
 *   draws G ~ Gamma(e_k(nb)) and the normals z of its holes, and is
 *   x_b = M_k + sqrt((1 + beta_k) nu_k / (2 beta_k) (1 + s_k d_a^2) / G) v,   L^T v = z
 * (sqrt(nu) L^-T is a factor of S_k = nu H^-1: the Student-t of 2 e_k(nb) degrees of freedom, location M_k and scale matrix
 * (1 + beta) / (beta (nu' + Da)) (1 + s d_a^2) S_k).  No moment has to exist: the prior component draws too, and there is no
 * LC_EDOMAIN case.  The random numbers are in the table at the top of this file: a draw is a function of (seed, block, row,
 * draw, the row's values) and of nothing else -- not of ndraws, the number of rows or the row's neighbours.  Completed rows,
 * logp, count and cols are those of lc_model_predict_incomplete, bit for bit.
 * LC_EINVAL: the cases of lc_model_predict_incomplete (raised before anything is written, the NaNs stay), ndraws outside
 * [1, LC_DRAWS_MAX].  A context without any hole is valid. */
int lc_model_predict_incomplete_draws(lc_model* m, lc_ctx* ctx, const int* groups /* [J of ctx] or NULL */, int ndraws,
                                      uint64_t seed);
/* rows [row0, row0+n) of block j of the draws of the last lc_model_predict_incomplete_draws on ctx: draws is n x ndraws x
 * LC_HOLES_MAX, contiguous; slot i belongs to cols[i] of lc_ctx_get_completed, the slots i >= count are exactly 0.0, and so is
 * every slot of a row without holes.  label is n x ndraws: the component of every draw (K = the prior component), -1 for
 * every draw of a row without holes (nothing is drawn for it).  Either output may be NULL.  LC_EINVAL: no such prediction on
 * ctx (none, or one without draws), a row range out of bounds. */
int lc_ctx_get_completed_draws(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* draws, int32_t* label);
/* ndraws of the last lc_model_predict_incomplete_draws on ctx, 0 when ctx holds no such prediction (never an error for that) */
int lc_ctx_completed_draws(lc_ctx* ctx, int* ndraws);
/* ---- leave-one-out conditionals (nothing in the reference corresponds): which value of a row is the odd one.
 * Gauss-Wishart models only.  ctx holds COMPLETE rows at the model's full width D >= 2.  Block b of ctx is mixed with the
 * weights of learned group groups[b] (NULL: group 0).  For every row and every column d, with b = {d} the single unknown
 * column in the notation of lc_model_predict_incomplete above, y = x - m_k, P_k = nu_k iW_k^-1, v = P_k y, s_k, G_k(1), e_k(1)
 * as in lc_gw_precision and g_k(1) as in lc_gw_precision_var:
 *   d_a^2    = max(d^2 - v_d^2 / P_k,dd, 0),  t_k,d = log E[pi_jk] + G_k(1) - log(P_k,dd) / 2 - e_k(1) log1p(s_k d_a^2)
 *   rest_d   = LSE_k t_k,d = log p(x_-d),     r_k,d = exp(t_k,d - rest_d),  M_k,d = x_d - v_d / P_k,dd
 *   cond[d]  = logp - rest_d = log p(x_d | x_-d, training data)     (logp: lc_model_predict's, bit for bit)
 *   mean[d]  = x_d + sum_k r_k,d (M_k,d - x_d) = E[x_d | x_-d]
 *   var[d]   = sum_k r_k,d (g_k(1) nu_k (1 + s_k d_a^2) / P_k,dd + (M_k,d - x_d)^2) - (mean[d] - x_d)^2     (variance != 0)
 *   worst    = the column with the smallest cond (the lowest column on ties; a NaN is never chosen)
 * The sum of cond over d is the pseudo-log-likelihood of the row; (x_d - mean[d]) / sqrt(var[d]) a z-score per cell.  All K
 * clusters take part, also for sparse models, and the prior component of StickBreak weights.  The observations keep every
 * bit.  Replaces any prediction ctx held (lc_ctx_get_predictions, lc_ctx_get_conditional and lc_ctx_get_completed report
 * none afterwards, and the ranking and threshold queries refuse it as they refuse an incomplete prediction); a call that
 * fails leaves none.  The context's qZ holds intermediate values afterwards.  The same bits on every call and wherever a row
 * sits in its block.
 * An empty context is LC_OK.  LC_EINVAL: clusters that are not Gauss-Wishart, D mismatch ("Mismatched dims. of cluster
 * params and obs.!"), D = 1 (no known column is left), a group index outside [0, J), a freed model, and a row that holds a
 * NaN -- the message names block and row of the first such row in (block, row) order, nothing has been written then, and
 * rows with unknown values go to lc_model_predict_incomplete.  LC_EDOMAIN (variance != 0 only), before any output: a
 * component with positive weight in some block has nu - 2 <= 0 (the prior component of StickBreak weights at D = 2, or a
 * cluster that ended up empty there); the message names the component, and the call without variance still works. */
int lc_model_predict_leave_one_out(lc_model* m, lc_ctx* ctx, const int* groups /* [J of ctx] or NULL */, int variance);
/* rows [row0, row0+n) of block j after the last lc_model_predict_leave_one_out on ctx: logp and worst are n values, cond,
 * mean and var n x D with row_stride doubles between rows (>= D).  Any output may be NULL.  LC_EINVAL: no such prediction on
 * ctx, var asked of a call made without variance, a row range out of bounds, row_stride < D with cond, mean or var given. */
int lc_ctx_get_leave_one_out(lc_ctx* ctx, int j, int64_t row0, int64_t n, double* logp, double* cond, double* mean,
                             double* var, int64_t row_stride, int32_t* worst);
/* ---- ranking on the device (nothing in the reference corresponds): the m best rows of each of C device-resident
 * columns, 1 <= m <= 64, without bringing the columns to the host.  Entry a is better than entry b when its score is larger
 * (largest != 0; smaller otherwise), or the scores compare equal (+0.0 and -0.0 do) and a comes first in the context (lower
 * block, then lower row): a total order, so the answer is unique.  A NaN score is never selected.
 *   LC_RANK_QZ:   C = ncols, the first ncols columns of the context's qZ, whatever they hold (1 <= ncols <= K of lc_ctx_dims);
 *                 by_label != 0: column c only sees the rows the last prediction on ctx labelled c
 *   LC_RANK_LOGZ, LC_RANK_LOGP: C = 1, the per-row logZ / logp of the last prediction on ctx (ncols is not looked at)
 * count[C]; group[C*m] (block of ctx), row[C*m] (row within its block), score[C*m]: best first; entries past count[c] are
 * -1, -1, NaN.  Outliers: lc_model_predict, then lc_ctx_top_rows(ctx, LC_RANK_LOGP, 1, m, 0, 0, ...).
 * LC_EINVAL: m outside 1 ... 64, ncols outside 1 ... K, by_label / LC_RANK_LOGZ / LC_RANK_LOGP without a prediction on ctx
 * (LC_RANK_LOGP: one with a log density), by_label together with LC_RANK_LOGZ / LC_RANK_LOGP, a context without data. */
enum { LC_RANK_QZ = 0, LC_RANK_LOGZ = 1, LC_RANK_LOGP = 2 };
int lc_ctx_top_rows(lc_ctx* ctx, int what, int ncols, int m, int largest, int by_label, int32_t* count, int32_t* group, int64_t* row, double* score);
/* ---- order and threshold queries over the same columns: quantiles, counts at thresholds and the rows beyond a
 * threshold, without bringing the columns to the host.  All three take their columns as lc_ctx_top_rows does: `what` is
 * LC_RANK_QZ with ncols, or LC_RANK_LOGZ, or LC_RANK_LOGP (C = 1, ncols is not looked at); by_label != 0: column c only sees the
 * rows the last prediction on ctx labelled c.  Only valid rows take part (never a pad row, in contexts of one and of several
 * blocks alike), and never a row whose score is NaN: n_c below is the number of participating rows of column c.  LC_EINVAL in
 * the cases lc_ctx_top_rows names for these arguments, with the same messages.  A context whose blocks are all empty answers
 * with counts of 0 and LC_OK.  None of the calls changes the prediction, the qZ or the observations of ctx.  A context inside a
 * communicator answers for ITS OWN rows only: nothing here is reduced across ranks. */
#define LC_QUANTILES_MAX 16
/* value[c*nprobs + i] = the order statistic of rank r_i of column c's n_c participating scores, bit for bit one of
 * them; rank[c*nprobs + i] = r_i; count[c] = n_c.  Order: the IEEE total order restricted to non-NaN values
 * (-inf < ... < -0.0 < +0.0 < ... < +inf), so the answer is unique down to the sign of zero.
 * r_i = min(n_c - 1, max(0, (int64)ceil(probs[i] * (double)n_c) - 1))  (numpy's method="inverted_cdf").
 * n_c = 0: value NaN, rank -1.  probs need not be sorted and may repeat.
 * LC_EINVAL additionally: nprobs outside 1 ... LC_QUANTILES_MAX, a prob outside [0, 1] or NaN. */
int lc_ctx_score_quantiles(lc_ctx* ctx, int what, int ncols, int by_label, const double* probs, int nprobs,
                           int64_t* count, int64_t* rank, double* value);
/* atmost[c*nthr + i] = the number of participating scores s of column c with s <= thr[i] (IEEE comparison:
 * -0.0 <= +0.0 holds both ways); count[c] = n_c.  thr may hold +-inf; a NaN threshold is LC_EINVAL;
 * nthr in 1 ... LC_QUANTILES_MAX. */
int lc_ctx_score_counts(lc_ctx* ctx, int what, int ncols, int by_label, const double* thr, int nthr,
                        int64_t* count, int64_t* atmost);
/* every participating row of ONE column (col; 0 for LOGZ / LOGP) with score <= thr (above == 0) or >= thr (above != 0),
 * in context order (block, then row) -- not by score.  *total = how many there are; the first min(total, capacity) of
 * them are written to group / row / score (any may be NULL, capacity may be 0: the count only).  by_label: only rows
 * labelled col.  LC_EINVAL additionally: col outside [0, ncols), capacity < 0, a NaN threshold. */
int lc_ctx_rows_beyond(lc_ctx* ctx, int what, int ncols, int col, int by_label, double thr, int above, int64_t capacity,
                       int64_t* total, int32_t* group, int64_t* row, double* score);
/* Exemplars: lc_model_predict(m, ctx, groups, 0), then per cluster k the mtop rows labelled k (by that prediction) with the
 * largest Eloglike_k(x) -- for Gauss-Wishart clusters the smallest expected Mahalanobis distance; the responsibility is no
 * use here: in a separated mixture most rows of a cluster have q = 1.0 exactly.  C = K; score = Eloglike_k(x_n), the raw
 * data term ranked on the device plus the cluster's constant, added on the host to K*mtop values.  Same side effects on
 * ctx as lc_model_predict(..., 0): its prediction is replaced and its qZ holds intermediate values afterwards (the raw
 * data terms, K columns).  LC_EINVAL as lc_model_predict and lc_ctx_top_rows. */
int lc_model_exemplars(lc_model* m, lc_ctx* ctx, const int* groups, int mtop, int32_t* count, int32_t* group, int64_t* row, double* score);
/* free the training observations and qZ (and shards) of a model; its parameters stay, so lc_model_predict still works
 * while the qZ accessors return LC_EINVAL.  A borrowed context (lc_vbem, lc_cluster) is left to its owner. */
int lc_model_release_data(lc_model* m);
/* expected weights of WeightDist::update(Nk) (distributions.cpp:124-168, 186-196, 242-256): Epi[K] = E[pi_k],
 * *Erest (may be NULL) = E[pi_rest], the mass beyond the truncation.  Dirichlet: alpha_k / sum(alpha), rest 0.
 * StickBreak: E[v_k] prod_{i before k} E[1 - v_i], E[v] = a1 / (a1 + a2), "before" in ordvec order (:139-165), rest
 * prod_i E[1 - v_i].  GDirichlet: the last stick of ordvec has v = 1 (:184-194), rest 0. */
int lc_weights_predictive(int wkind, double wprior, const double* Nk, int K, double* Epi, double* Erest);

/* ======================================================================== *
 * Two-level models: learnSCM (libcluster.h:583-596, scluster.cpp:578-605) and
 * learnMCM (libcluster.h:661-676, mcluster.cpp:613-642).
 * X[j][i]: J groups with Ij[j] "documents" each; Xji holds the sum(Ij) document
 * matrices group-major, document d is Nji[d] x D with the given strides.  Every
 * document is one group of an internal context, so vbeZ (scluster.cpp:93-124 /
 * mcluster.cpp:100-135) is the E-step kernel and the bottom-level M-step is the
 * suff-stat kernel; qY and W (document level, small) stay on the host.
 * Wj: NULL selects the SCM (GDirichlet / Dirichlet(prior_t) / GaussWish(prior_k));
 *     else J pointers to (Ij[j] x Dt) row-major document observations: the MCM
 *     (GDirichlet / Dirichlet() / GaussWish(prior_t, Dt) / GaussWish(prior_k, D)).
 * qY0: NULL = the reference's random start, |U(-1,1)| rows normalised, drawn with
 *     std::rand() (Eigen's Random(), scluster.cpp:519-521); else J pointers to
 *     (Ij[j] x maxT) row-major initial assignments (additive: reproducible runs).
 * Errors: LC_EINVAL for nthreads < 1, and for the SCM maxT > number of documents
 * ("maxT must be less than the number of documents ofX!", scluster.cpp:531-533);
 * LC_ERUNTIME "Free energy increase!" (scluster.cpp:248-249).
 * ======================================================================== */
int lc_learn_topic(int J, const int* Ij, const double* const* Xji, const int64_t* Nji, int D, int64_t row_stride,
                   int64_t col_stride, const double* const* Wj, int Dt, const double* const* qY0, double prior_t,
                   double prior_k, unsigned maxT, int maxK, int verbose, unsigned nthreads, int device,
                   lc_tmodel** out, double* F);
/* The same on one process per GPU: every rank passes WHOLE groups (with all their documents); fn (see
 * lc_ctx_set_allreduce) sums the cluster statistics, N_tk, the document-level Gaussian statistics, Fyz / Fz and the
 * decision counts of the split search, so all ranks take the same decisions.  qY0 (if given) holds this rank's
 * documents.  stream: the HIP stream the context works on (the hook's collectives must be ordered with it). */
int lc_learn_topic_dist(int J, const int* Ij, const double* const* Xji, const int64_t* Nji, int D, int64_t row_stride,
                        int64_t col_stride, const double* const* Wj, int Dt, const double* const* qY0, double prior_t,
                        double prior_k, unsigned maxT, int maxK, int verbose, unsigned nthreads, int device,
                        void* stream, lc_allreduce_fn fn, void* user, lc_tmodel** out, double* F);
int lc_tmodel_free(lc_tmodel* m);
int lc_tmodel_dims(lc_tmodel* m, int* J, int* Itot, int* T, int* K, int* D, int* Dt);
int lc_tmodel_get_qy(lc_tmodel* m, int j, double* qY /* Ij[j] x T row-major */);
int lc_tmodel_get_qz(lc_tmodel* m, int doc, double* q, int64_t row_stride, int64_t col_stride); /* Nji[doc] x K */
int lc_tmodel_get_qz_all(lc_tmodel* m, double* q); /* all documents, [sum N_ji x K] row-major */
int lc_tmodel_get_qz_all_colmajor(lc_tmodel* m, double* const* q); /* q[doc]: N_ji x K column-major, documents in (j, i) order */
/* level 0: weights_j[idx] (T values each); level 1: weights_t[idx] (K values each) */
int lc_tmodel_weights(lc_tmodel* m, int level, int idx, double* Elogweight, double* Nk);
/* level 0: bottom-level clusters[idx] (D); level 1: top-level clusters_t[idx] (Dt, MCM only) */
int lc_tmodel_cluster(lc_tmodel* m, int level, int idx, double* N, double* mean, double* cov, double* nu, double* beta,
                      double* iW, double* logdW, double* fenergy);
int lc_tmodel_rounds(lc_tmodel* m, int* nrounds);
int lc_tmodel_round(lc_tmodel* m, int r, int* T, int* K, int* niter, double* F, int nF);

/* ---- inference for new documents with a learned SCM / MCM model (nothing in the reference corresponds: its users would
 * iterate vbeY / vbeZ, scluster.cpp:50-124 / mcluster.cpp:49-135, by hand with the posteriors held fixed).  Every block
 * of ctx is one document; nothing learned is updated.  With a_t = E[log pi_gt] (+ Eloglike_t(w_i), MCM),
 * E_tk = E[log pi_tk] and L_nk = Eloglike_k(x_n):
 *   qY^0 = softmax_t(a_t); sweep r = 1, 2, ...: c_k = sum_t qY^{r-1}_t E_tk, q_nk = softmax_k(c_k + L_nk),
 *   N_k = sum_n q_nk; like_t = sum_k N_k E_tk, qY^r = softmax_t(a_t + like_t); delta_r = max_t |qY^r_t - qY^{r-1}_t|.
 * A document stops after sweep R, the first with delta_R <= tol, or R = max_sweeps (tol < 0: always max_sweeps; a
 * document without rows has delta_1 = 0).  One last vbeZ with qY^R gives qZ (keep_qz != 0: the context's qZ), and per row
 * logZ and label (argmax_k of c_k + L_nk, lowest k on ties), read with lc_ctx_get_predictions (logp: LC_EINVAL, there
 * is no density).  Per document: qY^R, label_t (argmax, lowest t on ties), Fyz = sum_t qY^R_t like_t - logZ_y of sweep
 * R, Fz = -sum_n logZ_n of the last vbeZ, and R.  The sweeps of a document run on the device without host round trips.
 * LC_EINVAL: D mismatch ("Mismatched dims. of cluster params and obs.!"), W given for an SCM model or missing for an
 * MCM model, a group index outside [0, J), max_sweeps < 1, a freed model, and a model whose per-document vectors
 * (4 T + 6 K doubles and a few) do not fit the kernel's 40 KB of LDS: K of about 800 and above ("the model is too
 * large for the inference kernel"). */
/* groups[doc]: learned group of every document of ctx (NULL: group 0); W: docs x Dt row-major (MCM; must be NULL for SCM) */
int lc_tmodel_predict(lc_tmodel* m, lc_ctx* ctx, const int* groups, const double* W, int max_sweeps, double tol, int keep_qz);
/* documents [doc0, doc0+n) of the last lc_tmodel_predict on ctx; any output may be NULL; qY is n x T row-major */
int lc_ctx_get_doc_predictions(lc_ctx* ctx, int doc0, int n, double* qY, int32_t* label_t, double* Fyz, double* Fz, int32_t* sweeps);
/* free the training documents and qZ; the parameters stay (as lc_model_release_data): lc_tmodel_predict still works
 * while the qY / qZ accessors return LC_EINVAL */
int lc_tmodel_release_data(lc_tmodel* m);

/* ======================================================================== *
 * Host-only pieces of the path (no GPU needed; used by the C++ facade classes
 * and by tests of the host arithmetic).
 * ======================================================================== */
double lc_digamma(double x); /* boost::math::digamma in the reference (probutils.cpp:213) */
/* WeightDist::update(Nk) + Elogweight() + fenergy(): distributions.cpp:124-168, 186-196, 242-266 */
int lc_weights_update(int wkind, double wprior, const double* Nk, int K, double* Elogweight, double* fenergy);
/* GaussWish: clearobs + addobs-sums + update (distributions.cpp:316-337) from
 * reduced statistics; outputs the posterior, the free energy (:388-399), the
 * E-step whitener A (D*D) and Eloglike constant.  Any output may be NULL. */
int lc_gw_mstep(double clustwidth, int D, double Ns, const double* xs, const double* xxs, double* nu, double* beta,
                double* m, double* iW, double* logdW, double* fenergy, double* A, double* eloglike_const);
/* The per-cluster tables of lc_model_predict_conditional from one Gauss-Wishart posterior (nu, beta, m [D], iW [D x D])
 * and a split into given / target columns (checked as there; target NULL: the columns not given, ntarget not looked at):
 *   A [ngiven x ngiven] row-major, lower-triangular: ||A (x_a - m_a)||^2 = nu (x_a - m_a)^T iW_aa^-1 (x_a - m_a)
 *   ma [ngiven], mb [ntarget]; B [ntarget x ngiven] row-major = iW_ba iW_aa^-1 (Cholesky factor of iW_aa and two
 *   triangular solves)
 *   log P_a(x_a) = G - e log1p(s ||A (x_a - m_a)||^2), s = beta / ((1 + beta) nu), e = (nu + 1 - D + ngiven) / 2
 * Any output may be NULL.  LC_EINVAL: the index cases above, nu <= D - 1, beta <= 0, iW_aa not positive definite. */
int lc_gw_conditional(int D, double nu, double beta, const double* m, const double* iW, const int* given, int ngiven,
                      const int* target, int ntarget, double* A, double* ma, double* B, double* mb, double* G, double* s,
                      double* e);
/* The tables of lc_model_predict_conditional_var from the same posterior and split (checked as in lc_gw_conditional):
 *   S [ntarget] = the diagonal of iW_bb - iW_ba iW_aa^-1 iW_ab, in the order of target (one triangular solve per target
 *   with the Cholesky factor of iW_aa; no inverse is formed),  g = (1 + beta) / (beta (nu + 1 - D + ngiven - 2))
 * so that cluster k's conditional covariance has the diagonal g (1 + s ||A (x_a - m_a)||^2) S.  Either output may be NULL.
 * LC_EINVAL: the cases of lc_gw_conditional.  LC_EDOMAIN: nu + 1 - D + ngiven <= 2 (the covariance does not exist). */
int lc_gw_conditional_var(int D, double nu, double beta, const double* iW, const int* given, int ngiven, const int* target,
                          int ntarget, double* S, double* g);
/* The scale matrix of the conditional Student-t of lc_model_predict_conditional_draws from the same posterior and split
 * (checked as in lc_gw_conditional): S [ntarget x ntarget] = iW_bb - iW_ba iW_aa^-1 iW_ab, formed as iW_bb - Y^T Y with
 * Y = L_aa^-1 iW_ab on the Cholesky factor of iW_aa that lc_gw_conditional uses (no inverse), and L its lower Cholesky factor
 * (row-major, the upper part zero).  Either may be NULL.  LC_EDOMAIN: S is not numerically positive definite (checked
 * whichever output is asked for). */
int lc_gw_conditional_cov(int D, double nu, double beta, const double* iW, const int* given, int ngiven, const int* target,
                          int ntarget, double* S, double* L);
/* The host table of lc_model_predict_incomplete from one Gauss-Wishart posterior (nu, beta, m [D], iW [D x D]); with
 * nu' = nu + 1 - D and, for nb = 0 ... LC_HOLES_MAX holes, Da = D - nb known columns:
 *   P [D x D] row-major = nu iW^-1 (symmetric; the square A^T A of the E-step whitener of lc_gw_mstep)
 *   e[nb] = (nu' + Da) / 2,  s = beta / ((1 + beta) nu)
 *   G[nb] = lgamma(e[nb]) - lgamma(nu'/2) - (Da/2) log(nu' pi) + (Da log(nu' beta / (1 + beta)) - log|iW| + nb log nu) / 2
 *           (NaN where nb > D)
 * so that log P_a(x_a) = G[nb] - log|P_bb| / 2 - e[nb] log1p(s d_a^2) for the holes b of a row, d_a^2 = d^2 - u^T P_bb^-1 u,
 * u = (P (x - m))_b and d^2 = (x - m)^T P (x - m) with any finite values in the holes of x.  G and e have LC_HOLES_MAX + 1
 * entries.  Any output may be NULL.  LC_EINVAL: nu <= D - 1, beta <= 0, iW not positive definite. */
int lc_gw_precision(int D, double nu, double beta, const double* m, const double* iW, double* P, double* G, double* s,
                    double* e);
/* The table of lc_model_predict_incomplete_var from the same posterior: for nb = 0 ... LC_HOLES_MAX holes
 *   g[nb] = (1 + beta) / (beta (nu' + Da - 2)) = (1 + beta) / (beta (nu - 1 - nb))
 * so that the conditional covariance of the holes b is g[nb] (1 + s d_a^2) nu (P_bb)^-1; NaN where nb >= D (no known
 * column) or nu - 1 - nb <= 0 (the covariance does not exist).  g[0] is the g of lc_gw_conditional_var with every column
 * given.  g has LC_HOLES_MAX + 1 entries.  LC_EINVAL: D < 1, nu <= D - 1, beta <= 0, g NULL. */
int lc_gw_precision_var(int D, double nu, double beta, double* g);
/* NormGamma: addobs sums -> update() (distributions.cpp:441-464), fenergy (:508-517), Eloglike constant (:486-488).
 * xs, xxs: D values each (sum q x, sum q x.^2). */
int lc_ng_mstep(double clustwidth, int D, double Ns, const double* xs, const double* xxs, double* nu, double* beta,
                double* m, double* L, double* logL, double* fenergy, double* eloglike_const);
/* ExpGamma: addobs sums -> update() (distributions.cpp:545-552), fenergy (:584-589), Eloglike constant (:570). */
int lc_eg_mstep(double obsmag, int D, double Ns, const double* xs, double* a, double* ib, double* logb,
                double* fenergy, double* eloglike_const);

#ifdef __cplusplus
}
#endif
#endif /* LIBCLUSTER_HIP_H */
