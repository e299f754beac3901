// Prediction with a learned mixture: VB responsibilities, per-row log normaliser, label and posterior
// predictive log density of observations that were not in the training set.  Nothing in the reference corresponds: its
// users call clusters[k].Eloglike(Xnew) per cluster (distributions.cpp:356-370, 483-492, 568-572) and do the
// log-sum-exp of vbexpectation (cluster.cpp:91-138) themselves.
//
// Launch structs of lc_kernels_predict.hip (device pointers, enqueue only) and the host side of the pass.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

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
