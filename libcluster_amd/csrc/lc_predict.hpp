// Prediction with a learned mixture: VB responsibilities, per-row log normaliser, label and posterior
// predictive log density of observations that were not in the training set.  Nothing in the reference corresponds: its
// users call clusters[k].Eloglike(Xnew) per cluster (distributions.cpp:356-370, 483-492, 568-572) and do the
// log-sum-exp of vbexpectation (cluster.cpp:91-138) themselves.
//
// Launch structs of lc_kernels_predict.hip (device pointers, enqueue only) and the host side of the pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace lck {

// predict_rows_kernel: one thread per padded row.  Reads the columns a raw E-step with zero constants left (column k at
// col[k * ldq + row]: -d^2/2 for Gauss-Wishart, the data term of Eloglike for the separable families) ONCE and writes
//   label[row] = first k of max (c_jk + col_k),  logZ[row] = log sum_k exp(c_jk + col_k)
// and, when Kp > 0 (Gauss-Wishart), logp[row] = log sum_{k < Kp} exp(p_jk - e_k log1p(-2 s_k col_k)).  keep_q: the K
// columns are rewritten in place as q = exp(c_jk + col_k - logZ).
struct PredictRowsLaunch {
  const double* col = nullptr;  // [>= max(K, Kp) columns x ldq]
  double* qcol = nullptr;       // == col (written when keep_q)
  int64_t ldq = 0;
  int K = 0;                    // VB columns
  int Kp = 0;                   // predictive columns (0: logp is not written here)
  int64_t nrg = 0;              // row groups (NP / 16)
  const int* rginfo = nullptr;  // [nrg] or nullptr (single group; nvalid from nrows)
  int64_t nrows = 0;
  const double* ctab = nullptr;  // [J x K] E[log pi_jk] + Eloglike constant_k (-inf: outside Kful)
  const double* ptab = nullptr;  // [J x Kp] log E[pi_jk] + log-density constant_k
  const double* pscale = nullptr;  // [Kp] s_k
  const double* pexp = nullptr;    // [Kp] e_k
  int keep_q = 0;
  int* label = nullptr;  // [NP]
  double* logZ = nullptr;
  double* logp = nullptr;
};
hipError_t launch_predict_rows(const PredictRowsLaunch& a, hipStream_t stream);

// predict_diag_kernel<MODE>: logp of the separable families, one thread per padded row, the clusters wave-uniform.
//   MODE 0 (NormGamma): log P_k = p_jk - e_k log prod_d (1 + w_kd (x_d - a_kd)^2)
//   MODE 1 (ExpGamma):  log P_k = p_jk - e_k log prod_d (1 + w_kd x_d)
// The products are renormalised with frexp every PRED_RENORM factors (one log per row and cluster, no overflow while
// every factor stays below 2^255).  flag (MODE 1): set to 1 when a valid observation is negative.
constexpr int PRED_RENORM = 4;
struct PredictDiagLaunch {
  int mode = 0;
  const double* X = nullptr;  // [NP x DP]
  int DP = 0;
  int64_t nrg = 0;
  const int* rginfo = nullptr;
  int64_t nrows = 0;
  int Kp = 0;
  const double* a = nullptr;  // [Kp x DP] (pad columns 0)
  const double* w = nullptr;  // [Kp x DP] (pad columns 0: a factor of exactly 1)
  const double* ptab = nullptr;  // [J x Kp]
  const double* pexp = nullptr;  // [Kp]
  double* logp = nullptr;        // [NP]
  int* flag = nullptr;
};
hipError_t launch_predict_diag(const PredictDiagLaunch& a, hipStream_t stream);

// predict_cond_kernel: the conditional mean of the target columns given the context's columns under a
// Gauss-Wishart mixture.  A raw E-step over the given columns left -d_k^2 / 2 in column k; per valid row
//   t_k = ttab_jk - e_k log1p(s_k d_k^2),  logp = LSE_k t_k,  r_k = exp(t_k - logp)
//   mean[row, :] = sum_k r_k (m_b,k + B_k (x_a - m_a,k))
// The sum over k and over the given columns is one GEMM on the fp64 matrix pipe (v_mfma_f64_4x4x4_4b): its left operand
// r_k [x_a - m_a,k, 1] is formed in registers, its right operand is the table T.  The kernel overwrites the Kp columns with
// t_k (each lane reads back only what it wrote itself).  One wave owns 64 rows: no atomics, the same bits on every call.
constexpr int PC_THREADS = 256;   // four waves, each on its own 64 rows
constexpr int PC_WAVE_ROWS = 64;  // four row groups of 16: one MFMA block per quad of rows
constexpr int PC_CHUNK = 32;      // given columns (ones column included) whose x stays in registers: 8 MFMA k-steps
constexpr int PC_PANEL = 32;      // target columns whose accumulators are resident: 8 quads
struct PredictCondLaunch {
  const double* X = nullptr;  // [NP x DP] the given columns (pad columns zero)
  int DP = 0;
  int Da = 0;   // given columns
  int Dae = 0;  // Da + 1 (the ones column) rounded up to a multiple of 4
  int Db = 0;   // target columns
  int Dbp = 0;  // Db rounded up to a multiple of 4
  int Kp = 0;
  double* col = nullptr;  // [Kp columns x ldq] raw E-step in, t_k out
  int64_t ldq = 0;
  int64_t nrg = 0;
  const int* rginfo = nullptr;
  int64_t nrows = 0;
  const double* ttab = nullptr;    // [J x Kp] log E[pi_jk] + G_k
  const double* pscale = nullptr;  // [Kp] s_k
  const double* pexp = nullptr;    // [Kp] e_k
  const double* mext = nullptr;    // [Kp x Dae] m_a,k, then zeros (the ones column is centred on 0)
  const double* T = nullptr;       // [Kp x Dae x Dbp] T[k][c][t] = B_k[t][c] (c < Da), m_b,k[t] (c = Da), 0 beyond
  double* mean = nullptr;          // [NP x Db]
  double* logp = nullptr;          // [NP]
};
hipError_t launch_predict_cond(const PredictCondLaunch& a, hipStream_t stream);

// predict_cond_var_kernel: the predictive variance of the target columns, the diagonal of the mixture's
// covariance centred on the mean predict_cond_kernel left.  It runs after that kernel on the same launch arguments and
// reads what it wrote: t_k in the Kp columns, logp and mean.  Per valid row, with r_k = exp(t_k - logp),
//   h_k = g_k (1 + s_k d_k^2) = g_k exp((ttab_jk - t_k) / e_k)        (the raw column is gone: t_k holds the same d_k^2)
//   var[row, t] = sum_k r_k ((M_k,t - mean_t)^2 + h_k S_k,t),  M_k = [x_a - m_a,k, 1] T_k
// M_k is a tile on the matrix pipe from zeroed accumulators per cluster (the operand is NOT scaled by r_k: the tile gets
// squared), the update one group of VALU instructions after the cluster's MFMAs.  One wave owns 64 rows: no atomics, the
// same bits on every call.  PCV_PANEL target columns are resident per pass (accumulators, mean and tile).
#ifndef LC_PCV_PANEL
#define LC_PCV_PANEL 16
#endif
constexpr int PCV_PANEL = LC_PCV_PANEL;
static_assert(PCV_PANEL == 16 || PCV_PANEL == 32, "a panel is 4 or 8 quads of target columns");
struct PredictCondVarLaunch {
  PredictCondLaunch c;        // as launched before (col, mean and logp are read here)
  const double* S = nullptr;  // [Kp x Dbp] diagonal of iW_bb - iW_ba iW_aa^-1 iW_ab, pads zero
  const double* g = nullptr;  // [Kp] (1 + beta) / (beta (nu' + Da - 2)); 0 for a component without weight
  double* var = nullptr;      // [NP x Db]
};
hipError_t launch_predict_cond_var(const PredictCondVarLaunch& a, hipStream_t stream);

// ---- rows whose unknown columns differ from row to row (lc_kernels_holes.hip) ---------------------------------
// A NaN in X marks an unknown value ("hole"); a row may hold up to HOLES_MAX of them (LC_HOLES_MAX of the C header).
constexpr int HOLES_MAX = 8;
// holes_scan_kernel: the one read of X that finds the holes.  Per valid row: count[row] = its number of NaNs (all of
// them, also beyond HOLES_MAX) and cols[row][0 .. HOLES_MAX) = the first HOLES_MAX of their columns, ascending, -1 beyond
// the count.  Pad rows and pad columns are not read.  out (cleared to {0, 0, ~0} by the launcher) receives, through integer
// atomics only (the same values on every run):
//   out[0] rows with at least one hole   out[1] the largest count   out[2] the smallest padded row position whose count
//   exceeds HOLES_MAX or leaves no known column (count >= D)
struct HolesScanLaunch {
  const double* X = nullptr;  // [NP x DP]
  int DP = 0;
  int D = 0;
  int64_t nrg = 0;
  const int* rginfo = nullptr;
  int64_t nrows = 0;
  int* count = nullptr;  // [NP]
  int* cols = nullptr;   // [NP x HOLES_MAX]
  unsigned long long* out = nullptr;  // [3]
};
hipError_t launch_holes_scan(const HolesScanLaunch& a, hipStream_t stream);

// holes_fill_kernel: X[row][cols[row][i]] = fill[cols[row][i]] for i < count[row] -- the recorded positions only
struct HolesFillLaunch {
  double* X = nullptr;
  int DP = 0;
  int64_t nrg = 0;
  const int* rginfo = nullptr;
  int64_t nrows = 0;
  const int* count = nullptr;
  const int* cols = nullptr;
  const double* fill = nullptr;  // [D]
};
hipError_t launch_holes_fill(const HolesFillLaunch& a, hipStream_t stream);

// predict_holes_kernel: after a raw E-step over the FILLED rows left -d_full^2 / 2 in column k, with b the holes of a row,
// nb their number, y = x_filled - m_k and P_k = nu_k iW_k^-1:
//   u = (P_k y)_b, H = (P_k)_bb = L L^T,  d_a^2 = max(d_full^2 - u^T H^-1 u, 0),  M_k = x_filled,b - H^-1 u
//   t_k = ttab[j][nb][k] - log prod_i L_ii - pexp[nb][k] log1p(s_k d_a^2),  logp = LSE_k t_k,  x_b <- sum_k r_k M_k
// A row without holes (nb = 0) takes predict_rows_kernel's loop, one lane per row; a row with holes is worked on by its
// whole wave.  No atomics, no scratch: the same bits on every call.  The hole positions of X are overwritten in place.
constexpr int PH_THREADS = 256;
struct PredictHolesLaunch {
  double* X = nullptr;  // [NP x DP], holes filled
  int DP = 0;
  int Kp = 0;
  const double* col = nullptr;  // [Kp columns x ldq] raw E-step
  int64_t ldq = 0;
  int64_t nrg = 0;
  const int* rginfo = nullptr;
  int64_t nrows = 0;
  const int* count = nullptr;
  const int* cols = nullptr;
  const double* ttab = nullptr;    // [J x (HOLES_MAX + 1) x Kp] log E[pi_jk] + G_k(nb)
  const double* pscale = nullptr;  // [Kp] s_k
  const double* pexp = nullptr;    // [(HOLES_MAX + 1) x Kp] e_k(nb)
  const double* mean = nullptr;    // [Kp x DP] m_k, pad columns zero
  const double* P = nullptr;       // [Kp x DP x DP] P_k, pad rows and columns zero
  double* logp = nullptr;          // [NP]
};
hipError_t launch_predict_holes(const PredictHolesLaunch& a, hipStream_t stream);

// predict_holes_var_kernel: everything predict_holes_kernel does, with the same bits in X and logp, and per
// row the predictive variance of every filled value.  With w = H^-1 u and S_k = nu_k H^-1 the Schur complement of iW_k:
//   Cov_k,ii = gnu[nb][k] (1 + s_k d_a^2) (H^-1)_ii,  (H^-1)_ii = ||L^-1 e_i||^2 (one forward solve per hole)
//   var_i    = sum_k r_k (Cov_k,ii + w_k,i^2) - (sum_k r_k w_k,i)^2   (M_k,i - fill_i = -w_k,i: centred on the mean)
// var[row][i] belongs to cols[row][i]; the slots i >= count and all eight slots of a row without holes are 0.  Every valid
// row's eight slots are written.  One more running sum per lane (the fold of u leaves hole i's sum in the lanes that
// own it), no atomics, a fixed tree: the same bits on every call and wherever the row sits in its block.
struct PredictHolesVarLaunch {
  PredictHolesLaunch h;         // as launched without variance
  const double* gnu = nullptr;  // [(HOLES_MAX + 1) x Kp] g_k(nb) nu_k; 0 where the variance does not exist
  double* var = nullptr;        // [NP x HOLES_MAX]
};
hipError_t launch_predict_holes_var(const PredictHolesVarLaunch& a, hipStream_t stream);

// ---- draws (lc_kernels_sample.hip; random numbers: lc_philox.hpp) ------------------------------------------------
constexpr int DRAWS_MAX = 64;  // draws per row of a conditional prediction (LC_DRAWS_MAX of the C header): one lane each
// sample_gw_kernel / sample_diag_kernel: new rows from a learned model, synth_kernel's shape (16 rows per 256-thread block,
// one block of the context per row group).  Row g = (block id << 40) + row_offset + row inside its block chooses component
// z by inverse CDF (first k with cdf[k] > u, else klast) and becomes
//   mode 0 (Gauss-Wishart): loc_z + fac_z eps / sqrt(G),  G ~ Gamma(shape_z) per row, fac_z lower triangular (normals in LDS)
//   mode 1 (NormGamma):     loc_zd + fac_zd eps_d / sqrt(G_d),  G_d ~ Gamma(shape_z) per entry
//   mode 2 (ExpGamma):      fac_zd expm1(-log(u_d) / shape_z)   (Lomax by inverse CDF)
// Pad rows and pad columns are written as zeros, the label of a pad row as -1.
struct SampleLaunch {
  int mode = 0;
  int DP = 0, D = 0, Kp = 0;
  double* X = nullptr;   // [NP x DP]
  int* label = nullptr;  // [NP]
  int64_t nrows = 0;     // valid rows (single block)
  int64_t NP = 0;
  int64_t row_offset = 0;
  uint64_t seed = 0;
  const int* rginfo = nullptr;     // [NP / 16] or nullptr (single block)
  const int64_t* goff = nullptr;   // [J + 1] padded block offsets, or nullptr
  const double* cdf = nullptr;     // [J x Kp] running sums of the weights of the block's learned group
  const int* klast = nullptr;      // [J] last component with positive weight
  const double* loc = nullptr;     // [Kp x D]
  const double* fac = nullptr;     // [Kp x D x D] (mode 0) or [Kp x D]
  const double* shape = nullptr;   // [Kp]
};
hipError_t launch_sample(const SampleLaunch& a, hipStream_t stream);

// cond_draws_kernel: after predict_cond_kernel, on the same launch arguments and what it left (t_k in the Kp columns,
// logp).  Per valid row and draw i < ndraws: component k by inverse CDF over r_k = exp(t_k - logp), then
//   x_b = M_k(x_a) + sqrt(cq_k (1 + s_k d_k^2) / G) L_k z,  G ~ Gamma(e_k),  M_k = [x_a - m_a,k, 1] T_k
// (cq_k = (1 + beta) / (2 beta): the Student-t with 2 e_k = nu' + Da degrees of freedom).  A wave owns its 64 rows: lane =
// row in the choice and the gamma draw (four draws of every row at a time), then the rows one after the other with lane t =
// target column t in the products; M_k is formed once for consecutive draws of a row that chose the same component.  No
// atomics, no LDS, no barrier: the same bits on every call.
struct PredictCondDrawsLaunch {
  PredictCondLaunch c;              // as launched before (col and logp are read here)
  const int64_t* goff = nullptr;    // [J + 1] padded block offsets, or nullptr (single block)
  const double* Lt = nullptr;       // [Kp x Dbp x Dbp] Lt[k][j][t] = chol(S_k)[t][j] (j <= t), zero elsewhere
  const double* cq = nullptr;       // [Kp]
  int ndraws = 0;
  uint64_t seed = 0;
  double* draws = nullptr;  // [NP x ndraws x Db]
  int* label = nullptr;     // [NP x ndraws]
};
hipError_t launch_predict_cond_draws(const PredictCondDrawsLaunch& a, hipStream_t stream);

// Draws for rows with holes (lc_kernels_holes.hip).  launch_predict_holes_keep: predict_holes_kernel with
// the same bits in X and logp, which also leaves t_k of every row WITH holes in tcol[k * ldq + row] (the raw column of that
// row and cluster, read by the one lane that then overwrites it; the rows without holes keep their raw columns).
struct PredictHolesKeepLaunch {
  PredictHolesLaunch h;    // as launched without draws
  double* tcol = nullptr;  // == h.col
};
hipError_t launch_predict_holes_keep(const PredictHolesKeepLaunch& a, hipStream_t stream);
// holes_draws_kernel: after that launch, on its arguments and what it left (t_k, logp, the mean-completed X).  Per row with
// holes and draw i < ndraws: component k by inverse CDF over r_k = exp(t_k - logp) (the choice uniform of (block, row, draw)
// is cond_draws_kernel's), G ~ Gamma(e_k(nb)), z the normals of the holes (pair p -> slots 2p, 2p + 1 of cols), then with
// H = (P_k)_bb = L L^T, M_k = x_b - H^-1 (P_k (x - m_k))_b (the same for any value in the holes) and
// h_k = exp((ttab[j][nb][k] - log prod_i L_ii - t_k) / e_k(nb)):
//   x_b = M_k + sqrt(cqnu_k h_k / G) v,  L^T v = z
// A wave works on its rows with holes one after the other: lane i = draw i in the choice, the gamma draw and the normals,
// then per DISTINCT chosen component the lanes own columns for u (predict_holes_kernel's reads and fold) and every lane
// runs the factorisation and the solves, with its own z in the last.  draws [row][i][slot] belongs to cols[row][slot];
// label [row][i] = k.  Only rows with holes are written, slots < count: the launcher's caller clears draws to 0 and label
// to -1 first.  No atomics, no LDS, no barrier: the same bits on every call, whatever ndraws and wherever the row sits.
struct HolesDrawsLaunch {
  PredictHolesLaunch h;            // as launched before (col holds t_k for the rows with holes)
  const int64_t* goff = nullptr;   // [J + 1] padded block offsets, or nullptr (single block)
  const double* cqnu = nullptr;    // [Kp] (1 + beta_k) nu_k / (2 beta_k)
  int ndraws = 0;
  uint64_t seed = 0;
  double* draws = nullptr;  // [NP x ndraws x HOLES_MAX]
  int* label = nullptr;     // [NP x ndraws]
};
hipError_t launch_holes_draws(const HolesDrawsLaunch& a, hipStream_t stream);

// ---- leave-one-out conditionals (lc_kernels_loo.hip) ----------------------------------------------------------------
// loo_rows_kernel<VAR>: after a raw E-step over COMPLETE rows left -d^2 / 2 in column k and predict_rows_kernel left logp, per
// valid row and column d < D, with y = x - m_k, v = P_k y (one GEMM per cluster on the matrix pipe, the full contraction):
//   d_a^2 = max(d^2 - v_d^2 / P_k,dd, 0),  t_k,d = ttab[j][k] - hlogp[k][d] - pexp[k] log1p(s_k d_a^2),  delta_k,d = -v_d / P_k,dd
//   rest_d = LSE_k t_k,d,  r_k,d = exp(t_k,d - rest_d),  cond[row][d] = logp[row] - rest_d
//   cmean[row][d] = x_d + sum_k r_k,d delta_k,d
//   var[row][d] = sum_k r_k,d (gnu[k] (1 + s_k d_a^2) / P_k,dd + delta_k,d^2) - (cmean[row][d] - x_d)^2          (VAR: var != null)
// A wave owns LOO_WAVE_ROWS rows and a panel of LOO_PANEL output columns (grid y: the panels) and folds the clusters in
// ascending order into a running (max, sum e, sum e delta, sum e (Cov + delta^2)) per element.  No atomics, no scratch, the
// order of every sum fixed: the same bits on every call and wherever a row sits.  Pad rows and pad columns are not written.
constexpr int LOO_THREADS = 256;    // four waves, each on its own rows
constexpr int LOO_WAVE_ROWS = 32;   // two row groups of 16
constexpr int LOO_PANEL = 16;       // output columns whose running state is resident: 4 quads
struct LooRowsLaunch {
  const double* X = nullptr;  // [NP x DP] complete rows
  int DP = 0;
  int D = 0;
  int Kp = 0;
  const double* col = nullptr;  // [Kp columns x ldq] raw E-step
  int64_t ldq = 0;
  int64_t nrg = 0;
  const int* rginfo = nullptr;
  int64_t nrows = 0;
  const double* ttab = nullptr;    // [J x Kp] log E[pi_jk] + G_k(1)
  const double* pscale = nullptr;  // [Kp] s_k
  const double* pexp = nullptr;    // [Kp] e_k(1)
  const double* gnu = nullptr;     // [Kp] g_k(1) nu_k; 0 for a component without weight whose variance does not exist (VAR)
  const double* mean = nullptr;    // [Kp x DP] m_k, pad columns zero
  const double* P = nullptr;       // [Kp x DP x DP] P_k, pad rows and columns zero
  const double* hlogp = nullptr;   // [Kp x DP] log(P_k,dd) / 2, pad columns zero
  const double* ipd = nullptr;     // [Kp x DP] 1 / P_k,dd, pad columns zero (no division on the device)
  const double* logp = nullptr;    // [NP] log p(x), predict_rows_kernel's
  double* cond = nullptr;          // [NP x DP]
  double* cmean = nullptr;         // [NP x DP]
  double* var = nullptr;           // [NP x DP] or null
};
hipError_t launch_loo_rows(const LooRowsLaunch& a, hipStream_t stream);

// loo_worst_kernel: per valid row worst[row] = the column d < D with the smallest cond[row][d] (the lowest column on ties; a
// NaN is never chosen; -1 when every entry is NaN) and value[row] = that entry (NaN with -1).  16 / 32 / 64 lanes read one row,
// as in holes_scan_kernel.
struct LooWorstLaunch {
  const double* cond = nullptr;  // [NP x DP]
  int DP = 0;
  int D = 0;
  int64_t nrg = 0;
  const int* rginfo = nullptr;
  int64_t nrows = 0;
  int* worst = nullptr;     // [NP]
  double* value = nullptr;  // [NP]
};
hipError_t launch_loo_worst(const LooWorstLaunch& a, hipStream_t stream);

}  // namespace lck

namespace lch {
struct WeightState;
}
namespace lcc {
class Context;
}
namespace lce {
struct Model;
}

namespace lcp {
// The two column lists of a conditional prediction, checked: every index in [0, D), no index twice, none in both lists,
// at least one of each.  target == nullptr: every column that is not given, ascending.  Returns the target list; throws
// std::invalid_argument naming the case.
std::vector<int> conditional_split(int D, const int* given, int ngiven, const int* target, int ntarget);
// Per-cluster tables of the conditional prediction from a Gauss-Wishart posterior (nu, beta, m [D], iW
// [D x D]) and a checked split (a = given, b = target):
//   A [Da x Da] lower-triangular, row-major: ||A (x_a - m_a)||^2 = nu (x_a - m_a)^T iW_aa^-1 (x_a - m_a)
//   B [Db x Da] = iW_ba iW_aa^-1 (two triangular solves with the Cholesky factor of iW_aa), ma [Da], mb [Db]
//   log P_a(x_a) = G - e log1p(s d^2): the Student-t marginal with nu + 1 - D degrees of freedom
// Any output may be null.
void gw_conditional(int D, double nu, double beta, const double* m, const double* iW, const std::vector<int>& given,
                    const std::vector<int>& target, double* A, double* ma, double* B, double* mb, double* G, double* s,
                    double* e);
// The tables of the conditional variance from the same posterior and split: the conditional of the
// cluster's predictive Student-t has nu' + Da degrees of freedom and the covariance g (1 + s d^2) (iW_bb - iW_ba iW_aa^-1 iW_ab);
//   S [Db] = the diagonal of that Schur complement: iW_tt - ||L^-1 iW_a,t||^2 with the Cholesky factor L of iW_aa that
//            gw_conditional uses (one triangular solve per target, no inverse)
//   g = (1 + beta) / (beta (nu' + Da - 2))
// Either output may be null.  Throws std::domain_error for nu' + Da <= 2 (the covariance does not exist), and
// std::invalid_argument as gw_conditional does.
void gw_conditional_var(int D, double nu, double beta, const double* iW, const std::vector<int>& given,
                        const std::vector<int>& target, double* S, double* g);
// E[x_target | x_given, training data] and log p(x_given | training data) of the rows in ctx (its columns are the given
// columns, in the order of `given`): into the context's conditional outputs (Context::get_conditional).  Gauss-Wishart
// models only; all K clusters take part (and the prior component of StickBreak weights), as in predict()'s logp.
// want_var: also the diagonal of the mixture's predictive covariance of the target columns (Context::get_conditional_var).
// Throws std::domain_error, before anything is launched, when a component with weight has nu' + Da <= 2.
// ndraws > 0: also that many draws of the target columns per row, each from the mixture of the clusters'
// conditional Student-t densities (Context::get_conditional_draws); mean and logp are the bits of the call without.  Throws
// std::domain_error, before anything is launched, when a cluster's Schur complement is not numerically positive definite.
void predict_conditional(lcc::Context& ctx, const lce::Model& model, const int* groups, const int* given, int ngiven,
                         const int* target, int ntarget, bool want_var = false, int ndraws = 0, uint64_t seed = 0);
// The full conditional scale matrix of that Student-t from the same posterior and split, on the Cholesky factor of iW_aa
// that gw_conditional uses: with Y = L_aa^-1 iW_ab, S [Db x Db] = iW_bb - Y^T Y (no inverse) and L [Db x Db] its lower
// Cholesky factor (the upper part zero).  Either output may be null.  Throws std::domain_error when S is not numerically
// positive definite (whichever output is wanted), and std::invalid_argument as gw_conditional does.
void gw_conditional_cov(int D, double nu, double beta, const double* iW, const std::vector<int>& given,
                        const std::vector<int>& target, double* S, double* L);
// New rows from the model's posterior predictive: J blocks of Nj rows at the model's width into ctx, block b
// with the weights of learned group groups[b] (null: 0); every row is a draw from the density whose logarithm predict()
// returns as logp (all K clusters and, with StickBreak weights, the prior component).  The component of every row stays on
// the device (Context::get_sample_labels; K = the prior component).  Throws std::invalid_argument, with ctx untouched.
void sample(lcc::Context& ctx, const lce::Model& model, int J, const int64_t* Nj, const int* groups, uint64_t seed,
            int64_t row_offset);
// The host table of one Gauss-Wishart posterior for rows with holes, NH = lck::HOLES_MAX + 1:
//   P [D x D] = nu iW^-1 = A^T A with the whitener A (symmetric)
//   G [NH]: G[nb] = lgam(e[nb]) - lgam(nu'/2) - (Da/2) log(nu' pi) + (Da log(nu' beta / (1 + beta)) - log|iW| + nb log nu) / 2
//           with Da = D - nb, nu' = nu + 1 - D (NaN where Da < 0); the device adds -log|P_bb| / 2
//   s = beta / ((1 + beta) nu),  e [NH]: e[nb] = (nu' + Da) / 2
// Any output may be null.  Throws std::invalid_argument for nu <= D - 1, beta <= 0, iW not positive definite.
void gw_precision(int D, double nu, double beta, const double* iW, double* P, double* G, double* s, double* e);
// Completes the rows in ctx (the model's full width; NaN = unknown) in place and leaves log p(x_known | training data)
// per row and the hole records in the context (Context::get_completed).  Gauss-Wishart models only; all K clusters take
// part (and the prior component of StickBreak weights).  Throws std::invalid_argument, with the observations untouched,
// for a row with more than lck::HOLES_MAX holes or without a known column.
// want_var: also the predictive variance of every filled value (Context::get_completed_var).  Throws
// std::domain_error, after the scan and before anything is written to the observations, when a component with weight in
// some block has nu - 1 - cmax <= 0 with cmax the largest hole count of the WHOLE context (conservative and strict).
// ndraws > 0 (not together with want_var): also that many draws of every unknown value per row, each from
// the mixture of the clusters' conditional Student-t densities (Context::get_completed_draws); the completed rows, logp and
// the hole records are the bits of the call without.  No moment has to exist: no std::domain_error.
void predict_incomplete(lcc::Context& ctx, const lce::Model& model, const int* groups, bool want_var = false, int ndraws = 0,
                        uint64_t seed = 0);
// The table of that variance: g[nb] = (1 + beta) / (beta (nu' + Da - 2)) = (1 + beta) / (beta (nu - 1 - nb)) for nb = 0 ...
// lck::HOLES_MAX holes, so that cluster k's conditional covariance is g[nb] (1 + s d_a^2) nu (P_bb)^-1; NaN where nb >= D or
// nu - 1 - nb <= 0.  Throws std::invalid_argument for nu <= D - 1, beta <= 0.
void gw_precision_var(int D, double nu, double beta, double* g);
// Leave-one-out conditionals of the COMPLETE rows in ctx (the model's full width): per row n and column d
// log p(x_d | x_-d, training data), E[x_d | x_-d] and, with want_var, Var[x_d | x_-d]; log p(x) per row (the bits of
// predict()'s logp) and the column with the smallest conditional log density (Context::get_leave_one_out).  Gauss-Wishart
// models only; all K clusters take part (and the prior component of StickBreak weights).  The observations keep every bit.
// Throws std::invalid_argument, with nothing written, for a row that holds a NaN (naming block and row), D = 1, and the
// argument cases of predict_incomplete; std::domain_error, before any output, when want_var meets a component with weight
// in some block whose nu - 2 <= 0 (the check of DESIGN 4.15.1 with cmax = 1).
void predict_leave_one_out(lcc::Context& ctx, const lce::Model& model, const int* groups, bool want_var = false);
// E[pi_k] (K values) and the mass beyond the truncation E[pi_rest] of a weight distribution in its updated state:
//   Dirichlet:  alpha_k / sum(alpha), no rest
//   StickBreak: E[v_k] prod_{i before k} E[1 - v_i] in ordvec order (distributions.cpp:139-165), rest prod_i E[1 - v_i]
//   GDirichlet: the same with v = 1 for the last stick of ordvec (:184-194): no rest
void weights_predictive(const lch::WeightState& w, double* Epi, double* Erest);
// The whole prediction of `model` on the observations in ctx: block b is scored with the weights of group groups[b]
// (null: 0).  sparse: vbexpectation's Kful rule (cluster.cpp:107-112).  Leaves label / logZ / logp in the context's
// per-row outputs and, with keep_qz, the responsibilities in its qZ.  Throws std::invalid_argument for a negative
// observation of an exponential model.
void predict(lcc::Context& ctx, const lce::Model& model, bool sparse, const int* groups, bool keep_qz);
// Exemplars: predict(..., keep_qz = false), then per cluster k the mtop rows labelled k with the largest
// Eloglike_k(x_n) -- ranked on the raw columns the prediction leaves in qZ, the cluster's constant added on the host.
// Outputs as Context::top_rows with C = K.
void exemplars(lcc::Context& ctx, const lce::Model& model, bool sparse, const int* groups, int mtop, int32_t* count,
               int32_t* group, int64_t* row, double* score);
}  // namespace lcp
