// Prediction with a learned mixture: the host arithmetic (expected weights, the per-cluster predictive
// constants of the three families, the zero-constant parameter sets of the raw E-step) and the context's side of the
// pass.  Kernels: lc_kernels_predict.hip.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "lc_ctx.hpp"
#include "lc_engine.hpp"
#include "lc_host.hpp"
#include "lc_predict.hpp"

namespace lcc {

void Context::predict_rows(int K, int Kp, const double* c, const double* pc, const double* ps, const double* pe,
                           bool keep_q) {
  use_device();
  if (K < 1 || Kp < 0) throw std::invalid_argument("K must be >= 1");
  pred_vb_ = false;
  if (NP_ == 0) {
    qz_[cur_].K = K;
    pred_vb_ = true;
    pred_logp_ = pred_logp_ || Kp > 0;
    return;
  }
  if (qz_[cur_].cap < std::max(K, Kp) || !qz_[cur_].buf.p) throw std::logic_error("predict_rows: no raw E-step columns");
  plabel_.reserve((size_t)NP_);
  plogz_.reserve((size_t)NP_);
  if (Kp > 0) plogp_.reserve((size_t)NP_);
  // tables: [c J x K | pc J x Kp | ps Kp | pe Kp]
  const size_t nc = (size_t)J_ * K, np = (size_t)J_ * Kp;
  hpack_.resize(nc + np + 2 * (size_t)Kp);
  std::copy(c, c + nc, hpack_.data());
  if (Kp > 0) {
    std::copy(pc, pc + np, hpack_.data() + nc);
    std::copy(ps, ps + Kp, hpack_.data() + nc + np);
    std::copy(pe, pe + Kp, hpack_.data() + nc + np + Kp);
  }
  ptab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(ptab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  lck::PredictRowsLaunch a;
  a.col = qz_[cur_].buf.p;
  a.qcol = qz_[cur_].buf.p;
  a.ldq = NP_;
  a.K = K;
  a.Kp = Kp;
  a.nrg = NP_ / lck::RG;
  a.rginfo = J_ > 1 ? rginfo_.p : nullptr;
  a.nrows = Nj_[0];
  a.ctab = ptab_.p;
  a.ptab = ptab_.p + nc;
  a.pscale = ptab_.p + nc + np;
  a.pexp = ptab_.p + nc + np + Kp;
  a.keep_q = keep_q ? 1 : 0;
  a.label = plabel_.p;
  a.logZ = plogz_.p;
  a.logp = Kp > 0 ? plogp_.p : nullptr;
  LC_HIP(lck::launch_predict_rows(a, stream_));
  LC_HIP(hipStreamSynchronize(stream_));  // (hpack_ and ptab_ are free again)
  qz_[cur_].K = K;
  qz_[cur_].hash_ok = false;
  qz_written(qz_[cur_]);
  pred_vb_ = true;
  pred_logp_ = pred_logp_ || Kp > 0;
}

bool Context::predict_diag(int mode, int Kp, const double* av, const double* w, const double* pc, const double* pe) {
  use_device();
  if (Kp < 1) throw std::invalid_argument("K must be >= 1");
  pred_logp_ = false;
  if (NP_ == 0) {
    pred_logp_ = true;
    return true;
  }
  const int D = D_, DP = DP_;
  plogp_.reserve((size_t)NP_);
  pflag_.reserve(1);
  // tables: [a Kp x DP | w Kp x DP | pc J x Kp | pe Kp], pad columns zero (a factor of exactly one)
  const size_t nw = (size_t)Kp * DP, np = (size_t)J_ * Kp;
  hpack_.assign(2 * nw + np + (size_t)Kp, 0.0);
  for (int k = 0; k < Kp; ++k) {
    std::copy(av + (size_t)k * D, av + (size_t)(k + 1) * D, hpack_.data() + (size_t)k * DP);
    std::copy(w + (size_t)k * D, w + (size_t)(k + 1) * D, hpack_.data() + nw + (size_t)k * DP);
  }
  std::copy(pc, pc + np, hpack_.data() + 2 * nw);
  std::copy(pe, pe + Kp, hpack_.data() + 2 * nw + np);
  ptab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(ptab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  LC_HIP(hipMemsetAsync(pflag_.p, 0, sizeof(int), stream_));
  lck::PredictDiagLaunch a;
  a.mode = mode;
  a.X = X_.p;
  a.DP = DP;
  a.nrg = NP_ / lck::RG;
  a.rginfo = J_ > 1 ? rginfo_.p : nullptr;
  a.nrows = Nj_[0];
  a.Kp = Kp;
  a.a = ptab_.p;
  a.w = ptab_.p + nw;
  a.ptab = ptab_.p + 2 * nw;
  a.pexp = ptab_.p + 2 * nw + np;
  a.logp = plogp_.p;
  a.flag = pflag_.p;
  LC_HIP(lck::launch_predict_diag(a, stream_));
  int flag = 0;
  LC_HIP(hipMemcpyAsync(&flag, pflag_.p, sizeof(int), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  if (flag) return false;
  pred_logp_ = true;
  return true;
}

void Context::get_predictions(int j, int64_t row0, int64_t n, int32_t* label, double* logZ, double* logp) const {
  use_device();
  if (j < 0 || j >= J_ || row0 < 0 || n < 0 || row0 + n > Nj_[j]) throw std::invalid_argument("row range out of bounds");
  if (!pred_vb_) throw std::invalid_argument("the context holds no prediction (lc_model_predict)");
  if (logp && !pred_logp_) throw std::invalid_argument("the context's prediction has no log density");
  if (n == 0) return;
  const size_t at = (size_t)(goff_[j] + row0);
  if (label) LC_HIP(hipMemcpyAsync(label, plabel_.p + at, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream_));
  if (logZ) LC_HIP(hipMemcpyAsync(logZ, plogz_.p + at, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  if (logp) LC_HIP(hipMemcpyAsync(logp, plogp_.p + at, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
}

void Context::predict_cond(int Kp, int Db, const double* tt, const double* ps, const double* pe, const double* ma,
                           const double* B, const double* mb) {
  use_device();
  if (Kp < 1 || Db < 1) throw std::invalid_argument("K and the number of target columns must be >= 1");
  pred_cond_ = 0;
  if (NP_ == 0) {
    pred_cond_ = Db;
    return;
  }
  if (qz_[cur_].cap < Kp || !qz_[cur_].buf.p) throw std::logic_error("predict_cond: no raw E-step columns");
  const int Da = D_, Dae = (Da + 1 + 3) / 4 * 4, Dbp = (Db + 3) / 4 * 4;
  pcmean_.reserve((size_t)NP_ * Db);
  pclogp_.reserve((size_t)NP_);
  // tables: [tt J x Kp | ps Kp | pe Kp | mext Kp x Dae | T Kp x Dae x Dbp], the pads zero
  const size_t nt = (size_t)J_ * Kp, nm = (size_t)Kp * Dae, nT = nm * Dbp;
  hpack_.assign(nt + 2 * (size_t)Kp + nm + nT, 0.0);
  double* h = hpack_.data();
  std::copy(tt, tt + nt, h);
  std::copy(ps, ps + Kp, h + nt);
  std::copy(pe, pe + Kp, h + nt + Kp);
  double* hm = h + nt + 2 * (size_t)Kp;
  double* hT = hm + nm;
  for (int k = 0; k < Kp; ++k) {
    std::copy(ma + (size_t)k * Da, ma + (size_t)(k + 1) * Da, hm + (size_t)k * Dae);
    double* Tk = hT + (size_t)k * Dae * Dbp;
    for (int t = 0; t < Db; ++t) {
      for (int c = 0; c < Da; ++c) Tk[(size_t)c * Dbp + t] = B[((size_t)k * Db + t) * Da + c];
      Tk[(size_t)Da * Dbp + t] = mb[(size_t)k * Db + t];  // the row of the ones column
    }
  }
  ptab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(ptab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  LC_HIP(lck::launch_predict_cond(predict_cond_args(Kp, Db), stream_));
  LC_HIP(hipStreamSynchronize(stream_));  // (hpack_ is free again; ptab_ keeps the tables for predict_cond_var)
  qz_[cur_].K = Kp;
  qz_[cur_].hash_ok = false;
  qz_written(qz_[cur_]);
  pred_cond_ = Db;
}

lck::PredictCondLaunch Context::predict_cond_args(int Kp, int Db) const {
  const int Da = D_, Dae = (Da + 1 + 3) / 4 * 4, Dbp = (Db + 3) / 4 * 4;
  const size_t nt = (size_t)J_ * Kp, nm = (size_t)Kp * Dae;  // (the layout predict_cond packs into ptab_)
  lck::PredictCondLaunch a;
  a.X = X_.p;
  a.DP = DP_;
  a.Da = Da;
  a.Dae = Dae;
  a.Db = Db;
  a.Dbp = Dbp;
  a.Kp = Kp;
  a.col = qz_[cur_].buf.p;
  a.ldq = NP_;
  a.nrg = NP_ / lck::RG;
  a.rginfo = J_ > 1 ? rginfo_.p : nullptr;
  a.nrows = Nj_[0];
  a.ttab = ptab_.p;
  a.pscale = ptab_.p + nt;
  a.pexp = ptab_.p + nt + Kp;
  a.mext = ptab_.p + nt + 2 * (size_t)Kp;
  a.T = a.mext + nm;
  a.mean = pcmean_.p;
  a.logp = pclogp_.p;
  return a;
}

void Context::predict_cond_var(int Kp, int Db, const double* S, const double* g) {
  use_device();
  pred_cond_var_ = false;
  if (pred_cond_ != Db || Kp < 1) throw std::logic_error("predict_cond_var: no conditional prediction of this width");
  if (NP_ == 0) {
    pred_cond_var_ = true;
    return;
  }
  if (qz_[cur_].K != Kp) throw std::logic_error("predict_cond_var: the columns of predict_cond are gone");
  const int Dbp = (Db + 3) / 4 * 4;
  pcvar_.reserve((size_t)NP_ * Db);
  // tables: [g Kp | S Kp x Dbp], the pads zero
  hpack_.assign((size_t)Kp + (size_t)Kp * Dbp, 0.0);
  std::copy(g, g + Kp, hpack_.data());
  for (int k = 0; k < Kp; ++k) std::copy(S + (size_t)k * Db, S + (size_t)(k + 1) * Db, hpack_.data() + Kp + (size_t)k * Dbp);
  pvtab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(pvtab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  lck::PredictCondVarLaunch v;
  v.c = predict_cond_args(Kp, Db);
  v.g = pvtab_.p;
  v.S = pvtab_.p + Kp;
  v.var = pcvar_.p;
  LC_HIP(lck::launch_predict_cond_var(v, stream_));
  LC_HIP(hipStreamSynchronize(stream_));  // (hpack_ is free again)
  pred_cond_var_ = true;
}

void Context::get_conditional_var(int j, int64_t row0, int64_t n, double* var, int64_t row_stride) const {
  use_device();
  if (pred_cond_ < 1) throw std::invalid_argument("the context holds no conditional prediction (lc_model_predict_conditional_var)");
  if (!pred_cond_var_)
    throw std::invalid_argument("the context's conditional prediction has no variance (lc_model_predict_conditional_var)");
  if (j < 0 || j >= J_ || row0 < 0 || n < 0 || row0 + n > Nj_[j]) throw std::invalid_argument("row range out of bounds");
  if (var && row_stride < pred_cond_) throw std::invalid_argument("row_stride is smaller than the number of target columns");
  if (n == 0 || !var) return;
  const size_t at = (size_t)(goff_[j] + row0), w = (size_t)pred_cond_ * sizeof(double);
  LC_HIP(hipMemcpy2DAsync(var, (size_t)row_stride * sizeof(double), pcvar_.p + at * pred_cond_, w, w, (size_t)n,
                          hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
}

void Context::get_conditional(int j, int64_t row0, int64_t n, double* mean, int64_t row_stride, double* logp) const {
  use_device();
  if (pred_cond_ < 1) throw std::invalid_argument("the context holds no conditional prediction (lc_model_predict_conditional)");
  if (j < 0 || j >= J_ || row0 < 0 || n < 0 || row0 + n > Nj_[j]) throw std::invalid_argument("row range out of bounds");
  if (mean && row_stride < pred_cond_) throw std::invalid_argument("row_stride is smaller than the number of target columns");
  if (n == 0) return;
  const size_t at = (size_t)(goff_[j] + row0), w = (size_t)pred_cond_ * sizeof(double);
  if (mean)
    LC_HIP(hipMemcpy2DAsync(mean, (size_t)row_stride * sizeof(double), pcmean_.p + at * pred_cond_, w, w, (size_t)n,
                            hipMemcpyDeviceToHost, stream_));
  if (logp) LC_HIP(hipMemcpyAsync(logp, pclogp_.p + at, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
}

void Context::predict_cond_draws(int Kp, int Db, int ndraws, uint64_t seed, const double* L, const double* cq) {
  use_device();
  pred_cond_draws_ = 0;
  if (pred_cond_ != Db || Kp < 1) throw std::logic_error("predict_cond_draws: no conditional prediction of this width");
  if (ndraws < 1 || ndraws > lck::DRAWS_MAX) throw std::invalid_argument("ndraws must be in 1 ... 64");
  if (NP_ == 0) {
    pred_cond_draws_ = ndraws;
    return;
  }
  if (qz_[cur_].K != Kp) throw std::logic_error("predict_cond_draws: the columns of predict_cond are gone");
  const int Dbp = (Db + 3) / 4 * 4;
  pcdraws_.reserve((size_t)NP_ * ndraws * Db);
  pcdlabel_.reserve((size_t)NP_ * ndraws);
  // tables: [cq Kp | Lt Kp x Dbp x Dbp] (the factor transposed: a wave reads one column of L_k side by side), the pads zero
  hpack_.assign((size_t)Kp + (size_t)Kp * Dbp * Dbp, 0.0);
  std::copy(cq, cq + Kp, hpack_.data());
  for (int k = 0; k < Kp; ++k) {
    double* Lt = hpack_.data() + Kp + (size_t)k * Dbp * Dbp;
    for (int t = 0; t < Db; ++t)
      for (int c = 0; c <= t; ++c) Lt[(size_t)c * Dbp + t] = L[((size_t)k * Db + t) * Db + c];
  }
  pdtab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(pdtab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  lck::PredictCondDrawsLaunch v;
  v.c = predict_cond_args(Kp, Db);
  v.goff = J_ > 1 ? goff_d_.p : nullptr;
  v.cq = pdtab_.p;
  v.Lt = pdtab_.p + Kp;
  v.ndraws = ndraws;
  v.seed = seed;
  v.draws = pcdraws_.p;
  v.label = pcdlabel_.p;
  LC_HIP(lck::launch_predict_cond_draws(v, stream_));
  LC_HIP(hipStreamSynchronize(stream_));  // (hpack_ is free again)
  pred_cond_draws_ = ndraws;
}

void Context::get_conditional_draws(int j, int64_t row0, int64_t n, double* draws, int32_t* label) const {
  use_device();
  if (pred_cond_ < 1 || pred_cond_draws_ < 1)
    throw std::invalid_argument("the context holds no draws of a conditional prediction (lc_model_predict_conditional_draws)");
  if (j < 0 || j >= J_ || row0 < 0 || n < 0 || row0 + n > Nj_[j]) throw std::invalid_argument("row range out of bounds");
  if (n == 0) return;
  const size_t at = (size_t)(goff_[j] + row0) * pred_cond_draws_, cnt = (size_t)n * pred_cond_draws_;
  static_assert(sizeof(int) == sizeof(int32_t), "the components are int32");
  if (draws)
    LC_HIP(hipMemcpyAsync(draws, pcdraws_.p + at * pred_cond_, cnt * pred_cond_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
  if (label) LC_HIP(hipMemcpyAsync(label, pcdlabel_.p + at, cnt * sizeof(int), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
}

void Context::sample(int mode, int J, const int64_t* Nj, int D, int Kp, const double* cdf, const int* klast, const double* loc,
                     const double* fac, const double* shape, uint64_t seed, int64_t row_offset) {
  use_device();
  if (Kp < 1) throw std::invalid_argument("K must be >= 1");
  build_layout(J, Nj, D);  // (whatever the context held is gone: data, qZ and predictions)
  if (mode == 0) require_gw_width();
  if (NP_ == 0) {
    sampled_ = true;
    return;
  }
  slabel_.reserve((size_t)NP_);
  DevBuf<int> dlast;
  dlast.reserve((size_t)J);
  LC_HIP(hipMemcpyAsync(dlast.p, klast, (size_t)J * sizeof(int), hipMemcpyHostToDevice, stream_));
  // tables: [cdf J x Kp | loc Kp x D | fac Kp x D (x D) | shape Kp]
  const size_t nc = (size_t)J * Kp, nl = (size_t)Kp * D, nf = mode == 0 ? nl * D : nl;
  hpack_.assign(nc + nl + nf + (size_t)Kp, 0.0);
  double* h = hpack_.data();
  std::copy(cdf, cdf + nc, h);
  if (loc) std::copy(loc, loc + nl, h + nc);
  std::copy(fac, fac + nf, h + nc + nl);
  std::copy(shape, shape + Kp, h + nc + nl + nf);
  ptab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(ptab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  lck::SampleLaunch a;
  a.mode = mode;
  a.DP = DP_;
  a.D = D;
  a.Kp = Kp;
  a.X = X_.p;
  a.label = slabel_.p;
  a.nrows = Nj[0];
  a.NP = NP_;
  a.row_offset = row_offset;
  a.seed = seed;
  a.rginfo = J > 1 ? rginfo_.p : nullptr;
  a.goff = J > 1 ? goff_d_.p : nullptr;
  a.cdf = ptab_.p;
  a.klast = dlast.p;
  a.loc = ptab_.p + nc;
  a.fac = ptab_.p + nc + nl;
  a.shape = ptab_.p + nc + nl + nf;
  LC_HIP(lck::launch_sample(a, stream_));
  LC_HIP(hipStreamSynchronize(stream_));  // (hpack_, ptab_ and the local table are free again)
  sampled_ = true;
}

void Context::get_sample_labels(int j, int64_t row0, int64_t n, int32_t* label) const {
  use_device();
  if (!sampled_) throw std::invalid_argument("the context's rows do not come from lc_model_sample");
  if (j < 0 || j >= J_ || row0 < 0 || n < 0 || row0 + n > Nj_[j]) throw std::invalid_argument("row range out of bounds");
  if (n == 0 || !label) return;
  static_assert(sizeof(int) == sizeof(int32_t), "the components are int32");
  LC_HIP(hipMemcpyAsync(label, slabel_.p + (size_t)(goff_[j] + row0), (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
}

void Context::holes_scan(int64_t* holed_rows, int* max_count, int* bad_block, int64_t* bad_row, int* bad_count) {
  use_device();
  pred_holes_ = false;
  *holed_rows = 0;
  *max_count = 0;
  *bad_block = -1;
  *bad_row = -1;
  *bad_count = 0;
  if (NP_ == 0) return;
  hcount_.reserve((size_t)NP_);
  hcols_.reserve((size_t)NP_ * lck::HOLES_MAX);
  hscan_.reserve(3);
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the scan's integers travel in int64 slots");
  lck::HolesScanLaunch a;
  a.X = X_.p;
  a.DP = DP_;
  a.D = D_;
  a.nrg = NP_ / lck::RG;
  a.rginfo = J_ > 1 ? rginfo_.p : nullptr;
  a.nrows = Nj_[0];
  a.count = hcount_.p;
  a.cols = hcols_.p;
  a.out = reinterpret_cast<unsigned long long*>(hscan_.p);
  LC_HIP(lck::launch_holes_scan(a, stream_));
  int64_t out[3];
  LC_HIP(hipMemcpyAsync(out, hscan_.p, sizeof(out), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  *holed_rows = out[0];
  *max_count = (int)out[1];
  if (out[2] < 0) return;  // (~0: no offending row)
  const int64_t pos = out[2];
  const int j = (int)(std::upper_bound(goff_.begin(), goff_.end(), pos) - goff_.begin()) - 1;
  if (pos >= NP_ || j < 0 || j >= J_ || pos - goff_[(size_t)j] >= Nj_[(size_t)j])
    throw std::logic_error("holes_scan: the offending position is no observation");
  int cnt = 0;
  LC_HIP(hipMemcpyAsync(&cnt, hcount_.p + pos, sizeof(int), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  *bad_block = j;
  *bad_row = pos - goff_[(size_t)j];
  *bad_count = cnt;
}

void Context::first_holed_row(int* block, int64_t* row) const {
  use_device();
  *block = -1;
  *row = -1;
  if (NP_ == 0) return;
  if (!hcount_.p) throw std::logic_error("first_holed_row: no hole records");
  std::vector<int> cnt((size_t)NP_);  // (an error path: the counts come to the host whole)
  LC_HIP(hipMemcpyAsync(cnt.data(), hcount_.p, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  for (int j = 0; j < J_; ++j)
    for (int64_t r = 0; r < Nj_[(size_t)j]; ++r)  // (the counts of pad rows are not written: valid rows only)
      if (cnt[(size_t)(goff_[(size_t)j] + r)] > 0) {
        *block = j;
        *row = r;
        return;
      }
}

void Context::holes_fill(const double* fill) {
  use_device();
  if (NP_ == 0) return;
  if (!hcount_.p || !hcols_.p) throw std::logic_error("holes_fill: no hole records");
  hpack_.resize((size_t)D_);
  std::copy(fill, fill + D_, hpack_.data());
  ptab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(ptab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  lck::HolesFillLaunch a;
  a.X = X_.p;
  a.DP = DP_;
  a.nrg = NP_ / lck::RG;
  a.rginfo = J_ > 1 ? rginfo_.p : nullptr;
  a.nrows = Nj_[0];
  a.count = hcount_.p;
  a.cols = hcols_.p;
  a.fill = ptab_.p;
  LC_HIP(lck::launch_holes_fill(a, stream_));
  LC_HIP(hipStreamSynchronize(stream_));  // (hpack_ and ptab_ are free again)
  dcache_invalidate();                    // (the observations changed)
  range_ok_ = false;
}

void Context::predict_holes(int Kp, const double* tt, const double* ps, const double* pe, const double* mean,
                            const double* P, const double* gnu, const double* cqnu, int ndraws, uint64_t seed) {
  use_device();
  if (Kp < 1) throw std::invalid_argument("K must be >= 1");
  pred_holes_ = false;
  pred_holes_var_ = false;
  pred_holes_draws_ = 0;
  if (ndraws < 0 || ndraws > lck::DRAWS_MAX) throw std::invalid_argument("ndraws must be in 1 ... 64");
  if (ndraws > 0 && (gnu || !cqnu)) throw std::logic_error("predict_holes: draws come with cqnu and without the variance");
  if (NP_ == 0) {
    pred_holes_ = true;
    pred_holes_var_ = gnu != nullptr;
    pred_holes_draws_ = ndraws;
    return;
  }
  if (qz_[cur_].cap < Kp || !qz_[cur_].buf.p) throw std::logic_error("predict_holes: no raw E-step columns");
  if (!hcount_.p || !hcols_.p) throw std::logic_error("predict_holes: no hole records");
  constexpr int NH = lck::HOLES_MAX + 1;
  const int D = D_, DP = DP_;
  hlogp_.reserve((size_t)NP_);
  if (gnu) hvar_.reserve((size_t)NP_ * lck::HOLES_MAX);
  // tables: [tt J x NH x Kp | ps Kp | pe NH x Kp | mean Kp x DP | P Kp x DP x DP], the pads zero; with gnu: [... | gnu NH x Kp],
  // with draws: [... | cqnu Kp]
  const size_t nt = (size_t)J_ * NH * Kp, ne = (size_t)NH * Kp, nm = (size_t)Kp * DP, nP = nm * DP;
  hpack_.assign(nt + (size_t)Kp + ne + nm + nP + (gnu ? ne : 0) + (ndraws > 0 ? (size_t)Kp : 0), 0.0);
  double* h = hpack_.data();
  if (gnu) std::copy(gnu, gnu + ne, h + nt + Kp + ne + nm + nP);
  if (ndraws > 0) std::copy(cqnu, cqnu + Kp, h + nt + Kp + ne + nm + nP);
  std::copy(tt, tt + nt, h);
  std::copy(ps, ps + Kp, h + nt);
  std::copy(pe, pe + ne, h + nt + Kp);
  double* hm = h + nt + Kp + ne;
  double* hP = hm + nm;
  for (int k = 0; k < Kp; ++k) {
    std::copy(mean + (size_t)k * D, mean + (size_t)(k + 1) * D, hm + (size_t)k * DP);
    for (int r = 0; r < D; ++r)
      std::copy(P + ((size_t)k * D + r) * D, P + ((size_t)k * D + r + 1) * D, hP + ((size_t)k * DP + r) * DP);
  }
  ptab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(ptab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  lck::PredictHolesLaunch a;
  a.X = X_.p;
  a.DP = DP;
  a.Kp = Kp;
  a.col = qz_[cur_].buf.p;
  a.ldq = NP_;
  a.nrg = NP_ / lck::RG;
  a.rginfo = J_ > 1 ? rginfo_.p : nullptr;
  a.nrows = Nj_[0];
  a.count = hcount_.p;
  a.cols = hcols_.p;
  a.ttab = ptab_.p;
  a.pscale = ptab_.p + nt;
  a.pexp = ptab_.p + nt + Kp;
  a.mean = ptab_.p + nt + Kp + ne;
  a.P = a.mean + nm;
  a.logp = hlogp_.p;
  if (gnu) {
    lck::PredictHolesVarLaunch v;
    v.h = a;
    v.gnu = a.P + nP;
    v.var = hvar_.p;
    LC_HIP(lck::launch_predict_holes_var(v, stream_));
  } else if (ndraws > 0) {
    // every valid row's slots on every call: draws 0 and components -1 (all bits set), then the rows with holes over them
    hdraws_.reserve((size_t)NP_ * ndraws * lck::HOLES_MAX);
    hdlabel_.reserve((size_t)NP_ * ndraws);
    LC_HIP(hipMemsetAsync(hdraws_.p, 0, (size_t)NP_ * ndraws * lck::HOLES_MAX * sizeof(double), stream_));
    LC_HIP(hipMemsetAsync(hdlabel_.p, 0xff, (size_t)NP_ * ndraws * sizeof(int), stream_));
    lck::PredictHolesKeepLaunch kp;
    kp.h = a;
    kp.tcol = qz_[cur_].buf.p;
    LC_HIP(lck::launch_predict_holes_keep(kp, stream_));
    lck::HolesDrawsLaunch v;
    v.h = a;
    v.goff = J_ > 1 ? goff_d_.p : nullptr;
    v.cqnu = a.P + nP;
    v.ndraws = ndraws;
    v.seed = seed;
    v.draws = hdraws_.p;
    v.label = hdlabel_.p;
    LC_HIP(lck::launch_holes_draws(v, stream_));
  } else {
    LC_HIP(lck::launch_predict_holes(a, stream_));
  }
  LC_HIP(hipStreamSynchronize(stream_));  // (hpack_ and ptab_ are free again)
  qz_[cur_].K = Kp;
  qz_[cur_].hash_ok = false;
  qz_written(qz_[cur_]);
  dcache_invalidate();  // (the observations changed)
  range_ok_ = false;
  pred_holes_ = true;
  pred_holes_var_ = gnu != nullptr;
  pred_holes_draws_ = ndraws;
}

void Context::get_completed_draws(int j, int64_t row0, int64_t n, double* draws, int32_t* label) const {
  use_device();
  if (!pred_holes_ || pred_holes_draws_ < 1)
    throw std::invalid_argument("the context holds no draws of completed rows (lc_model_predict_incomplete_draws)");
  if (j < 0 || j >= J_ || row0 < 0 || n < 0 || row0 + n > Nj_[j]) throw std::invalid_argument("row range out of bounds");
  if (n == 0) return;
  const size_t at = (size_t)(goff_[j] + row0) * pred_holes_draws_, cnt = (size_t)n * pred_holes_draws_;
  static_assert(sizeof(int) == sizeof(int32_t), "the components are int32");
  if (draws)
    LC_HIP(hipMemcpyAsync(draws, hdraws_.p + at * lck::HOLES_MAX, cnt * lck::HOLES_MAX * sizeof(double), hipMemcpyDeviceToHost,
                          stream_));
  if (label) LC_HIP(hipMemcpyAsync(label, hdlabel_.p + at, cnt * sizeof(int), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
}

void Context::get_completed_var(int j, int64_t row0, int64_t n, double* var, int64_t row_stride) const {
  use_device();
  if (!pred_holes_) throw std::invalid_argument("the context holds no completed rows (lc_model_predict_incomplete_var)");
  if (!pred_holes_var_)
    throw std::invalid_argument("the context's completed rows have no variance (lc_model_predict_incomplete_var)");
  if (j < 0 || j >= J_ || row0 < 0 || n < 0 || row0 + n > Nj_[j]) throw std::invalid_argument("row range out of bounds");
  if (row_stride < lck::HOLES_MAX) throw std::invalid_argument("row_stride is smaller than LC_HOLES_MAX");
  if (n == 0 || !var) return;
  const size_t at = (size_t)(goff_[j] + row0), w = (size_t)lck::HOLES_MAX * sizeof(double);
  LC_HIP(hipMemcpy2DAsync(var, (size_t)row_stride * sizeof(double), hvar_.p + at * lck::HOLES_MAX, w, w, (size_t)n,
                          hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
}

void Context::get_completed(int j, int64_t row0, int64_t n, double* rows, int64_t row_stride, double* logp, int32_t* count,
                            int32_t* cols) const {
  use_device();
  if (!pred_holes_) throw std::invalid_argument("the context holds no completed rows (lc_model_predict_incomplete)");
  if (j < 0 || j >= J_ || row0 < 0 || n < 0 || row0 + n > Nj_[j]) throw std::invalid_argument("row range out of bounds");
  if (rows && row_stride < D_) throw std::invalid_argument("row_stride is smaller than the number of columns");
  if (n == 0) return;
  const size_t at = (size_t)(goff_[j] + row0);
  static_assert(sizeof(int) == sizeof(int32_t), "the hole records are int32");
  if (rows)
    LC_HIP(hipMemcpy2DAsync(rows, (size_t)row_stride * sizeof(double), X_.p + at * DP_, (size_t)DP_ * sizeof(double),
                            (size_t)D_ * sizeof(double), (size_t)n, hipMemcpyDeviceToHost, stream_));
  if (logp) LC_HIP(hipMemcpyAsync(logp, hlogp_.p + at, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  if (count) LC_HIP(hipMemcpyAsync(count, hcount_.p + at, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream_));
  if (cols)
    LC_HIP(hipMemcpyAsync(cols, hcols_.p + at * lck::HOLES_MAX, (size_t)n * lck::HOLES_MAX * sizeof(int),
                          hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
}

void Context::predict_loo(int Kp, const double* pc, const double* ps, const double* pe0, const double* tt1, const double* pe1,
                          const double* gnu1, const double* mean, const double* P) {
  use_device();
  if (Kp < 1) throw std::invalid_argument("K must be >= 1");
  pred_loo_ = false;
  pred_loo_var_ = false;
  if (NP_ == 0) {
    pred_loo_ = true;
    pred_loo_var_ = gnu1 != nullptr;
    return;
  }
  if (qz_[cur_].cap < Kp || !qz_[cur_].buf.p) throw std::logic_error("predict_loo: no raw E-step columns");
  const int D = D_, DP = DP_;
  const size_t NP = (size_t)NP_;
  llogp_.reserve(NP);
  lcond_.reserve(NP * DP);
  lmean_.reserve(NP * DP);
  if (gnu1) lvar_.reserve(NP * DP);
  lworst_.reserve(NP);
  lworstv_.reserve(NP);
  // tables: [pc J x Kp | ps Kp | pe0 Kp | tt1 J x Kp | pe1 Kp | gnu1 Kp | mean Kp x DP | hlogp Kp x DP | ipd Kp x DP |
  // P Kp x DP x DP], the pads zero
  const size_t nt = (size_t)J_ * Kp, nm = (size_t)Kp * DP, nP = nm * DP;
  hpack_.assign(2 * nt + 4 * (size_t)Kp + 3 * nm + nP, 0.0);
  double* h = hpack_.data();
  std::copy(pc, pc + nt, h);
  std::copy(ps, ps + Kp, h + nt);
  std::copy(pe0, pe0 + Kp, h + nt + Kp);
  double* ht1 = h + nt + 2 * (size_t)Kp;
  std::copy(tt1, tt1 + nt, ht1);
  std::copy(pe1, pe1 + Kp, ht1 + nt);
  if (gnu1) std::copy(gnu1, gnu1 + Kp, ht1 + nt + Kp);
  double* hm = ht1 + nt + 2 * (size_t)Kp;
  double *hl = hm + nm, *hi = hl + nm, *hP = hi + nm;
  for (int k = 0; k < Kp; ++k) {
    std::copy(mean + (size_t)k * D, mean + (size_t)(k + 1) * D, hm + (size_t)k * DP);
    for (int r = 0; r < D; ++r) {
      std::copy(P + ((size_t)k * D + r) * D, P + ((size_t)k * D + r + 1) * D, hP + ((size_t)k * DP + r) * DP);
      const double pdd = P[((size_t)k * D + r) * D + r];  // (> 0: the diagonal of a positive definite matrix)
      hl[(size_t)k * DP + r] = 0.5 * std::log(pdd);
      hi[(size_t)k * DP + r] = 1.0 / pdd;
    }
  }
  ptab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(ptab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  const double* d1 = ptab_.p + nt + 2 * (size_t)Kp;
  // log p(x): predict_rows_kernel over the nb = 0 tables with no VB column (its label and logZ outputs go to the buffers
  // the worst column and its value overwrite below)
  lck::PredictRowsLaunch r;
  r.col = qz_[cur_].buf.p;
  r.qcol = qz_[cur_].buf.p;
  r.ldq = NP_;
  r.K = 0;
  r.Kp = Kp;
  r.nrg = NP_ / lck::RG;
  r.rginfo = J_ > 1 ? rginfo_.p : nullptr;
  r.nrows = Nj_[0];
  r.ctab = ptab_.p;
  r.ptab = ptab_.p;
  r.pscale = ptab_.p + nt;
  r.pexp = ptab_.p + nt + Kp;
  r.keep_q = 0;
  r.label = lworst_.p;
  r.logZ = lworstv_.p;
  r.logp = llogp_.p;
  LC_HIP(lck::launch_predict_rows(r, stream_));
  lck::LooRowsLaunch a;
  a.X = X_.p;
  a.DP = DP;
  a.D = D;
  a.Kp = Kp;
  a.col = qz_[cur_].buf.p;
  a.ldq = NP_;
  a.nrg = r.nrg;
  a.rginfo = r.rginfo;
  a.nrows = r.nrows;
  a.ttab = d1;
  a.pscale = r.pscale;
  a.pexp = d1 + nt;
  a.gnu = gnu1 ? d1 + nt + Kp : nullptr;
  a.mean = d1 + nt + 2 * (size_t)Kp;
  a.hlogp = a.mean + nm;
  a.ipd = a.hlogp + nm;
  a.P = a.ipd + nm;
  a.logp = llogp_.p;
  a.cond = lcond_.p;
  a.cmean = lmean_.p;
  a.var = gnu1 ? lvar_.p : nullptr;
  LC_HIP(lck::launch_loo_rows(a, stream_));
  lck::LooWorstLaunch w;
  w.cond = lcond_.p;
  w.DP = DP;
  w.D = D;
  w.nrg = r.nrg;
  w.rginfo = r.rginfo;
  w.nrows = r.nrows;
  w.worst = lworst_.p;
  w.value = lworstv_.p;
  LC_HIP(lck::launch_loo_worst(w, stream_));
  LC_HIP(hipStreamSynchronize(stream_));  // (hpack_ and ptab_ are free again)
  qz_[cur_].K = Kp;
  qz_[cur_].hash_ok = false;
  qz_written(qz_[cur_]);
  pred_loo_ = true;
  pred_loo_var_ = gnu1 != nullptr;
}

void Context::get_leave_one_out(int j, int64_t row0, int64_t n, double* logp, double* cond, double* mean, double* var,
                                int64_t row_stride, int32_t* worst) const {
  use_device();
  if (!pred_loo_) throw std::invalid_argument("the context holds no leave-one-out prediction (lc_model_predict_leave_one_out)");
  if (var && !pred_loo_var_)
    throw std::invalid_argument("the context's leave-one-out prediction has no variance (lc_model_predict_leave_one_out "
                                "with variance != 0)");
  if (j < 0 || j >= J_ || row0 < 0 || n < 0 || row0 + n > Nj_[j]) throw std::invalid_argument("row range out of bounds");
  if ((cond || mean || var) && row_stride < D_) throw std::invalid_argument("row_stride is smaller than the number of columns");
  if (n == 0) return;
  const size_t at = (size_t)(goff_[j] + row0);
  static_assert(sizeof(int) == sizeof(int32_t), "the worst columns are int32");
  const size_t dpitch = (size_t)row_stride * sizeof(double), spitch = (size_t)DP_ * sizeof(double), w = (size_t)D_ * sizeof(double);
  if (cond) LC_HIP(hipMemcpy2DAsync(cond, dpitch, lcond_.p + at * DP_, spitch, w, (size_t)n, hipMemcpyDeviceToHost, stream_));
  if (mean) LC_HIP(hipMemcpy2DAsync(mean, dpitch, lmean_.p + at * DP_, spitch, w, (size_t)n, hipMemcpyDeviceToHost, stream_));
  if (var) LC_HIP(hipMemcpy2DAsync(var, dpitch, lvar_.p + at * DP_, spitch, w, (size_t)n, hipMemcpyDeviceToHost, stream_));
  if (logp) LC_HIP(hipMemcpyAsync(logp, llogp_.p + at, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  if (worst) LC_HIP(hipMemcpyAsync(worst, lworst_.p + at, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
}

Context::RankColumns Context::rank_columns(int what, int ncols, bool by_label) const {
  if (J_ < 1) throw std::invalid_argument("the context holds no observations (lc_ctx_set_data / lc_ctx_synth)");
  if (what < 0 || what > 2) throw std::invalid_argument("unknown ranking source (LC_RANK_QZ, LC_RANK_LOGZ, LC_RANK_LOGP)");
  RankColumns rc;
  if (what == 0) {
    const int K = qz_[cur_].K;
    if (ncols < 1 || ncols > K) throw std::invalid_argument("ncols must be in 1 ... K, the columns of the context's qZ (" + std::to_string(K) + ")");
    if (by_label && !pred_vb_) throw std::invalid_argument("the context holds no prediction (lc_model_predict): no labels to rank by");
    rc.C = ncols;
    rc.col = qz_[cur_].buf.p;
  } else {
    if (by_label) throw std::invalid_argument("by_label ranks the columns of qZ, not logZ / logp");
    if (!pred_vb_) throw std::invalid_argument("the context holds no prediction (lc_model_predict)");
    if (what == 2 && !pred_logp_) throw std::invalid_argument("the context's prediction has no log density");
    rc.col = what == 1 ? plogz_.p : plogp_.p;
  }
  return rc;
}

lck::ScoreColumns Context::score_columns(const RankColumns& rc, bool by_label, const char* who) const {
  if (!rc.col || (by_label && !plabel_.p)) throw std::logic_error(std::string(who) + ": the column is not on the device");
  lck::ScoreColumns s;
  s.col = rc.col;
  s.ld = NP_;
  s.C = rc.C;
  s.NP = NP_;
  s.rginfo = J_ > 1 ? rginfo_.p : nullptr;
  s.nrows = Nj_[0];
  s.label = by_label ? plabel_.p : nullptr;
  return s;
}

void Context::score_quantiles(int what, int ncols, bool by_label, const double* probs, int nprobs, int64_t* count,
                              int64_t* rank, double* value) {
  use_device();
  const RankColumns rc = rank_columns(what, ncols, by_label);
  if (nprobs < 1 || nprobs > lck::SEL_MAX) throw std::invalid_argument("nprobs must be in 1 ... 16");
  for (int i = 0; i < nprobs; ++i)
    if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) throw std::invalid_argument("every prob must be in [0, 1]");
  const size_t C = (size_t)rc.C, n = C * (size_t)nprobs;
  std::fill(count, count + C, (int64_t)0);
  std::fill(rank, rank + n, (int64_t)-1);
  std::fill(value, value + n, std::numeric_limits<double>::quiet_NaN());
  if (NP_ == 0) return;
  lck::ScoreSelectLaunch a;
  a.s = score_columns(rc, by_label, "score_quantiles");
  a.nprobs = nprobs;
  std::copy(probs, probs + nprobs, a.probs);
  const size_t nhist = C * lck::SEL_HIST_WORDS, nstate = C * lck::SEL_STATE_WORDS, nout = C + 2 * n;
  toppos_.reserve(nhist + nstate + nout);
  static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(double) == sizeof(int64_t), "the results travel in 8-byte slots");
  a.hist = reinterpret_cast<unsigned long long*>(toppos_.p);
  a.state = reinterpret_cast<long long*>(toppos_.p + nhist);
  a.out = reinterpret_cast<long long*>(toppos_.p + nhist + nstate);
  LC_HIP(lck::launch_score_select(a, stream_));
  hred_.resize(nout);
  LC_HIP(hipMemcpyAsync(hred_.data(), a.out, nout * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  std::memcpy(count, hred_.data(), C * sizeof(int64_t));
  std::memcpy(rank, hred_.data() + C, n * sizeof(int64_t));
  for (size_t i = 0; i < n; ++i)
    if (rank[i] >= 0) std::memcpy(value + i, hred_.data() + C + n + i, sizeof(double));  // (the bits of one of the scores)
}

void Context::score_counts(int what, int ncols, bool by_label, const double* thr, int nthr, int64_t* count, int64_t* atmost) {
  use_device();
  const RankColumns rc = rank_columns(what, ncols, by_label);
  if (nthr < 1 || nthr > lck::SEL_MAX) throw std::invalid_argument("nthr must be in 1 ... 16");
  for (int i = 0; i < nthr; ++i)
    if (thr[i] != thr[i]) throw std::invalid_argument("a threshold is NaN");
  const size_t C = (size_t)rc.C, n = C * (size_t)nthr;
  std::fill(count, count + C, (int64_t)0);
  std::fill(atmost, atmost + n, (int64_t)0);
  if (NP_ == 0) return;
  lck::ScoreCountsLaunch a;
  a.s = score_columns(rc, by_label, "score_counts");
  a.nthr = nthr;
  std::copy(thr, thr + nthr, a.thr);
  toppos_.reserve(C + n);
  a.out = reinterpret_cast<unsigned long long*>(toppos_.p);
  LC_HIP(lck::launch_score_counts(a, stream_));
  hred_.resize(C + n);
  LC_HIP(hipMemcpyAsync(hred_.data(), a.out, (C + n) * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  for (size_t c = 0; c < C; ++c) {
    std::memcpy(count + c, hred_.data() + c * (1 + (size_t)nthr), sizeof(int64_t));
    std::memcpy(atmost + c * (size_t)nthr, hred_.data() + c * (1 + (size_t)nthr) + 1, (size_t)nthr * sizeof(int64_t));
  }
}

void Context::rows_beyond(int what, int ncols, int col, bool by_label, double thr, bool above, int64_t capacity,
                          int64_t* total, int32_t* group, int64_t* row, double* score) {
  use_device();
  RankColumns rc = rank_columns(what, ncols, by_label);
  if (col < 0 || col >= rc.C) throw std::invalid_argument("col must be in 0 ... ncols - 1 (0 for logZ / logp)");
  if (capacity < 0) throw std::invalid_argument("capacity must not be negative");
  if (thr != thr) throw std::invalid_argument("a threshold is NaN");
  *total = 0;
  if (NP_ == 0) return;
  lck::RowsBeyondLaunch a;
  a.s = score_columns(rc, by_label, "rows_beyond");
  a.s.col += (size_t)col * (size_t)NP_;
  a.s.C = 1;
  a.s.label0 = col;
  a.thr = thr;
  a.above = above ? 1 : 0;
  a.capacity = std::min<int64_t>(capacity, NP_);  // (no more rows than the context pads to can qualify)
  if (!group && !row && !score) a.capacity = 0;   // the count only
  a.nchunks = lck::top_rows_chunks(NP_);
  const size_t cap = (size_t)a.capacity;
  toppos_.reserve((size_t)a.nchunks + 1 + cap);
  topkey_.reserve(cap);
  a.chunkoff = reinterpret_cast<long long*>(toppos_.p);
  a.total = reinterpret_cast<long long*>(toppos_.p + a.nchunks);
  a.pos = reinterpret_cast<long long*>(toppos_.p + a.nchunks + 1);
  a.score = topkey_.p;
  LC_HIP(lck::launch_rows_beyond(a, stream_));
  hred_.resize(1);
  LC_HIP(hipMemcpyAsync(hred_.data(), a.total, sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  std::memcpy(total, hred_.data(), sizeof(int64_t));
  const size_t nw = (size_t)std::min<int64_t>(*total, a.capacity);
  if (nw == 0) return;
  if (group || row) {
    hred_.resize(nw);
    LC_HIP(hipMemcpyAsync(hred_.data(), a.pos, nw * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
  }
  if (score) LC_HIP(hipMemcpyAsync(score, a.score, nw * sizeof(double), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  if (!group && !row) return;
  size_t j = 0;  // (the positions ascend: the block only moves forward)
  for (size_t i = 0; i < nw; ++i) {
    int64_t pos;
    std::memcpy(&pos, hred_.data() + i, sizeof(pos));
    while (j + 1 < (size_t)J_ && pos >= goff_[j + 1]) ++j;
    if (pos < goff_[j] || pos - goff_[j] >= Nj_[j]) throw std::logic_error("rows_beyond: a flagged position is no observation");
    if (group) group[i] = (int32_t)j;
    if (row) row[i] = pos - goff_[j];
  }
}

void Context::top_rows(int what, int ncols, int m, bool largest, bool by_label, int32_t* count, int32_t* group,
                       int64_t* row, double* score) {
  use_device();
  if (J_ < 1) throw std::invalid_argument("the context holds no observations (lc_ctx_set_data / lc_ctx_synth)");
  if (m < 1 || m > lck::TOP_MAX_M) throw std::invalid_argument("m must be in 1 ... 64");
  const RankColumns rc = rank_columns(what, ncols, by_label);
  const double* col = rc.col;
  const int C = rc.C;
  const size_t n = (size_t)C * m;
  std::fill(count, count + C, 0);
  std::fill(group, group + n, -1);
  std::fill(row, row + n, (int64_t)-1);
  std::fill(score, score + n, std::numeric_limits<double>::quiet_NaN());
  if (NP_ == 0) return;
  if (!col || (by_label && !plabel_.p)) throw std::logic_error("top_rows: the column is not on the device");
  lck::TopRowsLaunch a;
  a.col = col;
  a.ld = NP_;
  a.C = C;
  a.NP = NP_;
  a.rginfo = J_ > 1 ? rginfo_.p : nullptr;
  a.nrows = Nj_[0];
  a.label = by_label ? plabel_.p : nullptr;
  a.m = m;
  a.largest = largest ? 1 : 0;
  a.nchunks = lck::top_rows_chunks(NP_);
  topkey_.reserve((size_t)a.nchunks * n);
  toppos_.reserve((size_t)a.nchunks * n);
  topout_.reserve(2 * n);
  static_assert(sizeof(long long) == sizeof(double) && sizeof(int64_t) == sizeof(long long), "positions travel in double slots");
  a.pkey = topkey_.p;
  a.ppos = reinterpret_cast<long long*>(toppos_.p);
  a.out_score = topout_.p;
  a.out_pos = reinterpret_cast<long long*>(topout_.p + n);
  LC_HIP(lck::launch_top_rows(a, stream_));
  hred_.resize(2 * n);
  LC_HIP(hipMemcpyAsync(hred_.data(), topout_.p, 2 * n * sizeof(double), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < m; ++i) {
      const size_t at = (size_t)c * m + i;
      int64_t pos;
      std::memcpy(&pos, hred_.data() + n + at, sizeof(pos));
      if (pos < 0) break;  // (best first: the empty slots are the last)
      const int j = (int)(std::upper_bound(goff_.begin(), goff_.end(), pos) - goff_.begin()) - 1;
      if (j < 0 || j >= J_ || pos - goff_[(size_t)j] >= Nj_[(size_t)j]) throw std::logic_error("top_rows: a selected position is no observation");
      group[at] = j;
      row[at] = pos - goff_[(size_t)j];
      score[at] = hred_[at];
      count[c] = i + 1;
    }
}

}  // namespace lcc

namespace lcp {

void weights_predictive(const lch::WeightState& w, double* Epi, double* Erest) {
  const int K = (int)w.alpha1.size();
  if (w.kind == lch::W_DIRICHLET) {
    double asum = 0.0;
    for (int k = 0; k < K; ++k) asum += w.alpha1[(size_t)k];
    for (int k = 0; k < K; ++k) Epi[k] = w.alpha1[(size_t)k] / asum;
    *Erest = 0.0;
    return;
  }
  // the sticks in ordvec order (equal counts in the order of the reference's sort, which update() repeats)
  double rest = 1.0;
  for (size_t idx = 0; idx < w.ordvec.size(); ++idx) {
    const int k = w.ordvec[idx].first;
    const double a1 = w.alpha1[(size_t)k], a2 = w.alpha2[(size_t)k];
    if (w.kind == lch::W_GDIRICHLET && idx + 1 == w.ordvec.size()) {  // v = 1 (distributions.cpp:184-194)
      Epi[k] = rest;
      rest = 0.0;
      break;
    }
    Epi[k] = a1 / (a1 + a2) * rest;
    rest *= a2 / (a1 + a2);
  }
  *Erest = rest;
}

namespace {

// the family's predictive of one cluster: log P(x) = lc - e * sum_d log1p(term_d(x)) (Gauss-Wishart: term = s d^2)
struct Predictive {
  double lc = 0.0, e = 0.0, s = 0.0;
  std::vector<double> a, w;  // separable families: term_d = w_d (x_d - a_d)^2 (NormGamma) / w_d x_d (ExpGamma)
};

Predictive gw_predictive(const lch::GaussWishState& g) {
  const int D = g.D;
  const double nup = g.nu + 1 - D;  // Student-t degrees of freedom
  Predictive p;
  p.lc = lch::lgam((g.nu + 1) / 2) - lch::lgam(nup / 2) - 0.5 * D * std::log(nup * lch::PI) +
         0.5 * (D * std::log(nup * g.beta / (1 + g.beta)) + g.logdW);
  p.s = g.beta / ((1 + g.beta) * g.nu);  // d^2 = nu maha_W(x): the distance the E-step forms
  p.e = (g.nu + 1) / 2;
  return p;
}

Predictive ng_predictive(const lch::NormGammaState& g) {
  const int D = g.D;
  Predictive p;
  p.lc = D * (lch::lgam(g.nu + 0.5) - lch::lgam(g.nu) - 0.5 * std::log(2 * lch::PI * (1 + g.beta) / g.beta)) -
         0.5 * g.logL;
  p.e = g.nu + 0.5;
  p.a = g.m;
  p.w.resize((size_t)D);
  for (int d = 0; d < D; ++d) p.w[(size_t)d] = g.beta / (2 * (1 + g.beta) * g.L[(size_t)d]);
  return p;
}

Predictive eg_predictive(const lch::ExpGammaState& g) {
  Predictive p;
  p.lc = g.D * std::log(g.a) - g.logb;
  p.e = g.a + 1;
  p.a.assign((size_t)g.D, 0.0);
  p.w = g.ib;
  return p;
}

Predictive predictive(const lch::ClusterAny& c) {
  return c.kind == lch::C_GAUSSWISH ? gw_predictive(c.gw) : c.kind == lch::C_NORMGAMMA ? ng_predictive(c.ng)
                                                                                        : eg_predictive(c.eg);
}

}  // namespace

void predict(lcc::Context& ctx, const lce::Model& model, bool sparse, const int* groups, bool keep_qz) {
  const int K = (int)model.clusters.size(), J = (int)model.weights.size(), D = ctx.D(), Jc = ctx.J();
  if (K < 1) throw std::invalid_argument("the model has no clusters");
  ctx.predict_clear();  // (whatever an earlier prediction left must not outlive a failure of this one)
  const int ck = model.ckind;
  // expected weights of every learned group; the prior component takes the mass beyond the truncation (StickBreak)
  std::vector<double> Epi((size_t)J * K), Erest((size_t)J);
  bool rest = false;
  for (int j = 0; j < J; ++j) {
    if ((int)model.weights[(size_t)j].alpha1.size() != K) throw std::invalid_argument("weights and clusters disagree");
    weights_predictive(model.weights[(size_t)j], Epi.data() + (size_t)j * K, &Erest[(size_t)j]);
    rest = rest || Erest[(size_t)j] > 0.0;
  }
  const int Kp = K + (rest ? 1 : 0);
  std::vector<Predictive> pr((size_t)Kp);
  std::vector<double> cst((size_t)K);
  for (int k = 0; k < K; ++k) {
    pr[(size_t)k] = predictive(model.clusters[(size_t)k]);
    cst[(size_t)k] = model.clusters[(size_t)k].eloglike_const();
  }
  const lch::ClusterAny prior(ck, model.clusters[0].prior(), D);  // clearobs state: a cluster that saw no data
  if (rest) pr[(size_t)K] = predictive(prior);

  // per block of the context: VB constants c (vbexpectation, cluster.cpp:91-138) and predictive constants pc
  constexpr double NINF = -std::numeric_limits<double>::infinity();
  std::vector<double> c((size_t)Jc * K), pc((size_t)Jc * Kp), pe((size_t)Kp), ps((size_t)Kp);
  for (int b = 0; b < Jc; ++b) {
    const int j = groups ? groups[b] : 0;
    const lch::WeightState& w = model.weights[(size_t)j];
    for (int k = 0; k < K; ++k) {
      const bool active = !sparse || w.Nk[(size_t)k] >= lch::ZEROCUTOFF;  // Kful, cluster.cpp:107-112
      c[(size_t)b * K + k] = active ? w.Elogpi[(size_t)k] + cst[(size_t)k] : NINF;
      pc[(size_t)b * Kp + k] = std::log(Epi[(size_t)j * K + k]) + pr[(size_t)k].lc;
    }
    if (rest) pc[(size_t)b * Kp + K] = std::log(Erest[(size_t)j]) + pr[(size_t)K].lc;
  }
  for (int k = 0; k < Kp; ++k) {
    pe[(size_t)k] = pr[(size_t)k].e;
    ps[(size_t)k] = pr[(size_t)k].s;
  }

  if (ck == lch::C_GAUSSWISH) {
    // one raw E-step over the K clusters (+ the prior's whitener): -d^2 / 2 per column
    std::vector<double> A((size_t)Kp * D * D), m((size_t)Kp * D), zero((size_t)Jc * Kp, 0.0);
    for (int k = 0; k < Kp; ++k) {
      const lch::GaussWishState& g = k < K ? model.clusters[(size_t)k].gw : prior.gw;
      const std::vector<double> Ak = g.whitener();
      std::copy(Ak.begin(), Ak.end(), A.begin() + (size_t)k * D * D);
      std::copy(g.m.begin(), g.m.end(), m.begin() + (size_t)k * D);
    }
    ctx.estep(Kp, A.data(), m.data(), zero.data(), nullptr, nullptr, /*raw=*/true);
    ctx.predict_rows(K, Kp, c.data(), pc.data(), ps.data(), pe.data(), keep_qz);
    return;
  }
  // separable families: the predictive first (it also checks ExpGamma's domain), then the raw E-step's data terms
  std::vector<double> av((size_t)Kp * D), wv((size_t)Kp * D);
  for (int k = 0; k < Kp; ++k) {
    std::copy(pr[(size_t)k].a.begin(), pr[(size_t)k].a.end(), av.begin() + (size_t)k * D);
    std::copy(pr[(size_t)k].w.begin(), pr[(size_t)k].w.end(), wv.begin() + (size_t)k * D);
  }
  if (!ctx.predict_diag(ck == lch::C_NORMGAMMA ? 0 : 1, Kp, av.data(), wv.data(), pc.data(), pe.data()))
    throw std::invalid_argument("X has to be in the range [0, inf)!");  // cluster.cpp:742
  std::vector<double> ra((size_t)K * D), rw2((size_t)K * D), rw1((size_t)K * D), zero((size_t)Jc * K, 0.0);
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < D; ++d) {  // the E-step parameters of vbem (lc_engine.cpp), distributions.cpp:486-491, 570-571
      const size_t i = (size_t)k * D + d;
      if (ck == lch::C_NORMGAMMA) {
        const lch::NormGammaState& g = model.clusters[(size_t)k].ng;
        ra[i] = g.m[(size_t)d];
        rw2[i] = -0.5 * g.nu / g.L[(size_t)d];
        rw1[i] = 0.0;
      } else {
        const lch::ExpGammaState& g = model.clusters[(size_t)k].eg;
        ra[i] = 0.0;
        rw2[i] = 0.0;
        rw1[i] = -g.a * g.ib[(size_t)d];
      }
    }
  ctx.estep_diag(K, ra.data(), rw2.data(), rw1.data(), zero.data(), nullptr, nullptr, /*raw=*/true);
  ctx.predict_rows(K, 0, c.data(), nullptr, nullptr, nullptr, keep_qz);
}

std::vector<int> conditional_split(int D, const int* given, int ngiven, const int* target, int ntarget) {
  if (ngiven < 1 || !given) throw std::invalid_argument("given needs at least one column");
  std::vector<char> seen((size_t)D, 0);
  for (int i = 0; i < ngiven; ++i) {
    const int c = given[i];
    if (c < 0 || c >= D) throw std::invalid_argument("given column " + std::to_string(c) + " is outside [0, D = " + std::to_string(D) + ")");
    if (seen[(size_t)c]) throw std::invalid_argument("given column " + std::to_string(c) + " appears twice");
    seen[(size_t)c] = 1;
  }
  std::vector<int> tg;
  if (!target) {
    for (int c = 0; c < D; ++c)
      if (!seen[(size_t)c]) tg.push_back(c);
    if (tg.empty()) throw std::invalid_argument("target needs at least one column: every column of the model is given");
    return tg;
  }
  if (ntarget < 1) throw std::invalid_argument("target needs at least one column");
  for (int i = 0; i < ntarget; ++i) {
    const int c = target[i];
    if (c < 0 || c >= D) throw std::invalid_argument("target column " + std::to_string(c) + " is outside [0, D = " + std::to_string(D) + ")");
    if (seen[(size_t)c] == 1) throw std::invalid_argument("column " + std::to_string(c) + " is both given and target");
    if (seen[(size_t)c]) throw std::invalid_argument("target column " + std::to_string(c) + " appears twice");
    seen[(size_t)c] = 2;
    tg.push_back(c);
  }
  return tg;
}

namespace {
// gw_conditional and gw_conditional_var on ONE Cholesky factor of iW_aa; S and gv (the variance tables) may be null, and
// the existence of the variance is looked at only when one of them is asked for
void conditional_tables(int D, double nu, double beta, const double* m, const double* iW, const std::vector<int>& given,
                        const std::vector<int>& target, double* A, double* ma, double* B, double* mb, double* G, double* s,
                        double* e, double* S, double* gv, double* Scov = nullptr, double* Lcov = nullptr) {
  const int Da = (int)given.size(), Db = (int)target.size();
  const double nup = nu + 1 - D;  // Student-t degrees of freedom: of the FULL model's width (the marginal keeps them)
  if (!(nup > 0.0) || !(beta > 0.0)) throw std::invalid_argument("nu must exceed D - 1 and beta must be positive");
  if ((S || gv) && !(nup + Da > 2.0))  // the conditional Student-t has nu' + Da degrees of freedom
    throw std::domain_error("the conditional variance does not exist: nu + 1 - D + ngiven = " + std::to_string(nup + Da) +
                            " is not above 2");
  std::vector<double> L((size_t)Da * Da);
  for (int i = 0; i < Da; ++i)
    for (int c = 0; c < Da; ++c) L[(size_t)i * Da + c] = iW[(size_t)given[(size_t)i] * D + given[(size_t)c]];
  if (!lch::cholesky(L, Da)) throw std::invalid_argument("Matrix A is not positive definite");  // (iW_aa = L L^T)
  double logdet = 0.0;
  for (int i = 0; i < Da; ++i) logdet += std::log(L[(size_t)i * Da + i]);
  logdet *= 2.0;
  if (A) {  // GaussWishState::whitener() of the sub-block
    const std::vector<double> Li = lch::tril_inverse(L, Da);
    const double sq = std::sqrt(nu);
    for (size_t i = 0; i < Li.size(); ++i) A[i] = sq * Li[i];
  }
  if (ma)
    for (int i = 0; i < Da; ++i) ma[i] = m[given[(size_t)i]];
  if (mb)
    for (int t = 0; t < Db; ++t) mb[t] = m[target[(size_t)t]];
  const bool cov = Scov || Lcov;
  std::vector<double> Y(cov ? (size_t)Db * Da : 0);  // Y^T: row t = L^-1 iW_a,t (the full Schur complement needs them all)
  if (B || S || cov) {  // row t of B solves iW_aa b = iW_a,t: L y = iW_a,t, then L^T b = y; the Schur complement's diagonal needs y only
    std::vector<double> y((size_t)Da);
    for (int t = 0; t < Db; ++t) {
      const int ct = target[(size_t)t];
      for (int i = 0; i < Da; ++i) {
        double v = iW[(size_t)ct * D + given[(size_t)i]];
        for (int c = 0; c < i; ++c) v -= L[(size_t)i * Da + c] * y[(size_t)c];
        y[(size_t)i] = v / L[(size_t)i * Da + i];
      }
      if (S) {  // iW_tt - iW_ta iW_aa^-1 iW_at = iW_tt - ||y||^2
        double v = iW[(size_t)ct * D + ct];
        for (int i = 0; i < Da; ++i) v -= y[(size_t)i] * y[(size_t)i];
        S[t] = v;
      }
      if (cov) std::copy(y.begin(), y.end(), Y.begin() + (size_t)t * Da);
      if (!B) continue;
      double* b = B + (size_t)t * Da;
      for (int i = Da - 1; i >= 0; --i) {
        double v = y[(size_t)i];
        for (int c = i + 1; c < Da; ++c) v -= L[(size_t)c * Da + i] * b[c];
        b[i] = v / L[(size_t)i * Da + i];
      }
    }
  }
  if (G)
    *G = lch::lgam((nup + Da) / 2) - lch::lgam(nup / 2) - 0.5 * Da * std::log(nup * lch::PI) +
         0.5 * (Da * std::log(nup * beta / (1 + beta)) - logdet);
  if (s) *s = beta / ((1 + beta) * nu);
  if (e) *e = (nup + Da) / 2;
  if (gv) *gv = (1 + beta) / (beta * (nup + Da - 2.0));
  if (cov) {  // S = iW_bb - Y^T Y, entry by entry as its diagonal above; then its own Cholesky factor
    std::vector<double> Sf((size_t)Db * Db);
    for (int t = 0; t < Db; ++t)
      for (int u = 0; u <= t; ++u) {
        double v = iW[(size_t)target[(size_t)t] * D + target[(size_t)u]];
        for (int i = 0; i < Da; ++i) v -= Y[(size_t)t * Da + i] * Y[(size_t)u * Da + i];
        Sf[(size_t)t * Db + u] = Sf[(size_t)u * Db + t] = v;
      }
    if (Scov) std::copy(Sf.begin(), Sf.end(), Scov);
    // (factored whichever output is wanted: an S that is not positive definite is an error, not a result)
    if (!lch::cholesky(Sf, Db))
      throw std::domain_error("the Schur complement iW_bb - iW_ba iW_aa^-1 iW_ab is not numerically positive definite");
    if (Lcov) std::copy(Sf.begin(), Sf.end(), Lcov);
  }
}
}  // namespace

void gw_conditional_cov(int D, double nu, double beta, const double* iW, const std::vector<int>& given,
                        const std::vector<int>& target, double* S, double* L) {
  std::vector<double> tmp(S || L ? 0 : (size_t)target.size() * target.size());  // (neither wanted: the checks still run)
  conditional_tables(D, nu, beta, nullptr, iW, given, target, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                     nullptr, nullptr, S || L ? S : tmp.data(), L);
}

void gw_conditional(int D, double nu, double beta, const double* m, const double* iW, const std::vector<int>& given,
                    const std::vector<int>& target, double* A, double* ma, double* B, double* mb, double* G, double* s,
                    double* e) {
  conditional_tables(D, nu, beta, m, iW, given, target, A, ma, B, mb, G, s, e, nullptr, nullptr);
}

void gw_conditional_var(int D, double nu, double beta, const double* iW, const std::vector<int>& given,
                        const std::vector<int>& target, double* S, double* g) {
  double gdummy;  // (the existence check runs even when neither output is wanted)
  conditional_tables(D, nu, beta, nullptr, iW, given, target, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, S,
                     g ? g : &gdummy);
}

void predict_conditional(lcc::Context& ctx, const lce::Model& model, const int* groups, const int* given, int ngiven,
                         const int* target, int ntarget, bool want_var, int ndraws, uint64_t seed) {
  ctx.predict_clear();  // (whatever an earlier prediction left must not outlive a failure of this one)
  const int K = (int)model.clusters.size(), J = (int)model.weights.size(), Jc = ctx.J();
  if (K < 1) throw std::invalid_argument("the model has no clusters");
  if (model.ckind != lch::C_GAUSSWISH)
    throw std::invalid_argument("conditional prediction needs Gauss-Wishart clusters: the columns of NormGamma / ExpGamma "
                                "clusters are independent within a cluster (not supported)");
  const int D = model.clusters[0].gw.D;
  const std::vector<int> gv(given, given + (ngiven > 0 && given ? ngiven : 0));
  const std::vector<int> tg = conditional_split(D, given, ngiven, target, ntarget);
  const int Da = ngiven, Db = (int)tg.size();
  if (ndraws < 0 || ndraws > lck::DRAWS_MAX) throw std::invalid_argument("ndraws must be in 1 ... 64");
  if (ctx.D() != Da)
    throw std::invalid_argument("the context has " + std::to_string(ctx.D()) + " columns, given names " + std::to_string(Da));
  for (int b = 0; b < Jc; ++b) {
    const int j = groups ? groups[b] : 0;
    if (j < 0 || j >= J) throw std::invalid_argument("group index out of range");
  }
  std::vector<double> Epi((size_t)J * K), Erest((size_t)J);
  bool rest = false;
  for (int j = 0; j < J; ++j) {
    if ((int)model.weights[(size_t)j].alpha1.size() != K) throw std::invalid_argument("weights and clusters disagree");
    weights_predictive(model.weights[(size_t)j], Epi.data() + (size_t)j * K, &Erest[(size_t)j]);
    rest = rest || Erest[(size_t)j] > 0.0;
  }
  const int Kp = K + (rest ? 1 : 0);
  const lch::ClusterAny prior(model.ckind, model.clusters[0].prior(), D);  // clearobs state: a cluster that saw no data
  std::vector<double> A((size_t)Kp * Da * Da), ma((size_t)Kp * Da), B((size_t)Kp * Db * Da), mb((size_t)Kp * Db),
      G((size_t)Kp), ps((size_t)Kp), pe((size_t)Kp), S(want_var ? (size_t)Kp * Db : 0, 0.0), gvar(want_var ? (size_t)Kp : 0, 0.0);
  std::vector<double> Lcov(ndraws > 0 ? (size_t)Kp * Db * Db : 0), cq(ndraws > 0 ? (size_t)Kp : 0);
  for (int k = 0; k < Kp; ++k) {
    const lch::GaussWishState& g = k < K ? model.clusters[(size_t)k].gw : prior.gw;
    bool var_k = want_var;
    if (want_var && !(g.nu + 1 - D + Da > 2.0)) {
      // the variance of this component does not exist: an error when a row can give it weight, nothing when none can
      // (its g and S stay 0, and the kernel skips a component whose responsibility is 0)
      bool weighted = false;
      for (int b = 0; b < Jc; ++b) {
        const int j = groups ? groups[b] : 0;
        weighted = weighted || (k < K ? Epi[(size_t)j * K + k] : Erest[(size_t)j]) > 0.0;
      }
      if (weighted)
        throw std::domain_error("the conditional variance does not exist: " +
                                (k < K ? "cluster " + std::to_string(k) : std::string("the prior component")) +
                                " has nu + 1 - D + ngiven = " + std::to_string(g.nu + 1 - D + Da) +
                                ", which is not above 2 (the mean and logp of lc_model_predict_conditional do exist)");
      var_k = false;
    }
    conditional_tables(D, g.nu, g.beta, g.m.data(), g.iW.data(), gv, tg, A.data() + (size_t)k * Da * Da,
                       ma.data() + (size_t)k * Da, B.data() + (size_t)k * Db * Da, mb.data() + (size_t)k * Db, &G[(size_t)k],
                       &ps[(size_t)k], &pe[(size_t)k], var_k ? S.data() + (size_t)k * Db : nullptr,
                       var_k ? &gvar[(size_t)k] : nullptr, nullptr, ndraws > 0 ? Lcov.data() + (size_t)k * Db * Db : nullptr);
    if (ndraws > 0) cq[(size_t)k] = (1 + g.beta) / (2 * g.beta);  // c_k eta / 2: the draw divides by G = chi^2_eta / 2
  }
  std::vector<double> tt((size_t)Jc * Kp), zero((size_t)Jc * Kp, 0.0);
  for (int b = 0; b < Jc; ++b) {
    const int j = groups ? groups[b] : 0;
    for (int k = 0; k < K; ++k) tt[(size_t)b * Kp + k] = std::log(Epi[(size_t)j * K + k]) + G[(size_t)k];
    if (rest) tt[(size_t)b * Kp + K] = std::log(Erest[(size_t)j]) + G[(size_t)K];
  }
  // one raw E-step over the given columns with the marginal whiteners: -d^2 / 2 per column
  ctx.estep(Kp, A.data(), ma.data(), zero.data(), nullptr, nullptr, /*raw=*/true);
  ctx.predict_cond(Kp, Db, tt.data(), ps.data(), pe.data(), ma.data(), B.data(), mb.data());
  if (want_var) ctx.predict_cond_var(Kp, Db, S.data(), gvar.data());
  if (ndraws > 0) ctx.predict_cond_draws(Kp, Db, ndraws, seed, Lcov.data(), cq.data());
}

void sample(lcc::Context& ctx, const lce::Model& model, int Jc, const int64_t* Nj, const int* groups, uint64_t seed,
            int64_t row_offset) {
  const int K = (int)model.clusters.size(), J = (int)model.weights.size();
  if (K < 1) throw std::invalid_argument("the model has no clusters");
  if (Jc < 1 || !Nj) throw std::invalid_argument("need at least one block of rows");
  for (int b = 0; b < Jc; ++b) {
    if (Nj[b] < 0) throw std::invalid_argument("negative block size");
    const int j = groups ? groups[b] : 0;
    if (j < 0 || j >= J) throw std::invalid_argument("group index out of range");
  }
  const int ck = model.ckind, D = model.clusters[0].D();
  if (ck == lch::C_GAUSSWISH && lck::padded_dim_wide(D) > lck::GW_MAX_DP)
    throw std::invalid_argument("D > 1024 is not supported by the Gauss-Wishart kernels (the diagonal and exponential "
                                "families take any D)");
  std::vector<double> Epi((size_t)J * K), Erest((size_t)J);
  bool rest = false;
  for (int j = 0; j < J; ++j) {
    if ((int)model.weights[(size_t)j].alpha1.size() != K) throw std::invalid_argument("weights and clusters disagree");
    weights_predictive(model.weights[(size_t)j], Epi.data() + (size_t)j * K, &Erest[(size_t)j]);
    rest = rest || Erest[(size_t)j] > 0.0;
  }
  const int Kp = K + (rest ? 1 : 0);
  // per block: the running sums of the weights in the order 0 ... K - 1, then the prior component
  std::vector<double> cdf((size_t)Jc * Kp);
  std::vector<int> klast((size_t)Jc, 0);
  for (int b = 0; b < Jc; ++b) {
    const int j = groups ? groups[b] : 0;
    double run = 0.0;
    for (int k = 0; k < Kp; ++k) {
      const double w = k < K ? Epi[(size_t)j * K + k] : Erest[(size_t)j];
      run += w;
      cdf[(size_t)b * Kp + k] = run;
      if (w > 0.0) klast[(size_t)b] = k;
    }
  }
  const lch::ClusterAny prior(ck, model.clusters[0].prior(), D);  // clearobs state: a cluster that saw no data
  std::vector<double> loc((size_t)Kp * D, 0.0), shape((size_t)Kp);
  std::vector<double> fac(ck == lch::C_GAUSSWISH ? (size_t)Kp * D * D : (size_t)Kp * D);
  for (int k = 0; k < Kp; ++k) {
    const lch::ClusterAny& c = k < K ? model.clusters[(size_t)k] : prior;
    if (ck == lch::C_GAUSSWISH) {
      // the Student-t of gw_predictive: nu' degrees of freedom, scale matrix (1 + beta) / (beta nu') iW; with
      // chi^2_nu' = 2 G the row is m + sqrt((1 + beta) / (2 beta)) chol(iW) z / sqrt(G), G ~ Gamma(nu' / 2)
      const lch::GaussWishState& g = c.gw;
      const double nup = g.nu + 1 - D;
      if (!(nup > 0.0) || !(g.beta > 0.0)) throw std::invalid_argument("nu must exceed D - 1 and beta must be positive");
      std::vector<double> L(g.iW);
      if (!lch::cholesky(L, D)) throw std::invalid_argument("Matrix A is not positive definite");
      const double sc = std::sqrt((1 + g.beta) / (2 * g.beta));
      for (size_t i = 0; i < L.size(); ++i) fac[(size_t)k * D * D + i] = sc * L[i];
      std::copy(g.m.begin(), g.m.end(), loc.begin() + (size_t)k * D);
      shape[(size_t)k] = nup / 2;
      continue;
    }
    // separable families, from the density predict() scores: prod_d (1 + term_d)^-e
    const Predictive p = predictive(c);
    for (int d = 0; d < D; ++d) {
      const size_t i = (size_t)k * D + d;
      if (ck == lch::C_NORMGAMMA) {
        // (1 + w (x - a)^2)^-e is a Student-t with n = 2 e - 1 degrees of freedom and scale^2 = 1 / (n w):
        // x = a + z / sqrt(2 w G), G ~ Gamma(n / 2)
        loc[i] = p.a[(size_t)d];
        fac[i] = 1.0 / std::sqrt(2 * p.w[(size_t)d]);
      } else {
        // (1 + w x)^-e is a Lomax with shape e - 1 and scale 1 / w: x = ((1 - u)^(-1 / (e - 1)) - 1) / w
        fac[i] = 1.0 / p.w[(size_t)d];
      }
    }
    shape[(size_t)k] = ck == lch::C_NORMGAMMA ? p.e - 0.5 : p.e - 1.0;
  }
  ctx.sample(ck == lch::C_GAUSSWISH ? 0 : ck == lch::C_NORMGAMMA ? 1 : 2, Jc, Nj, D, Kp, cdf.data(), klast.data(), loc.data(),
             fac.data(), shape.data(), seed, row_offset);
}

void gw_precision(int D, double nu, double beta, const double* iW, double* P, double* G, double* s, double* e) {
  constexpr int NH = lck::HOLES_MAX + 1;
  const double nup = nu + 1 - D;  // Student-t degrees of freedom: of the FULL model's width (a marginal keeps them)
  if (!(nup > 0.0) || !(beta > 0.0)) throw std::invalid_argument("nu must exceed D - 1 and beta must be positive");
  std::vector<double> L(iW, iW + (size_t)D * D);
  if (!lch::cholesky(L, D)) throw std::invalid_argument("Matrix A is not positive definite");  // (iW = L L^T)
  double logdet = 0.0;
  for (int i = 0; i < D; ++i) logdet += std::log(L[(size_t)i * D + i]);
  logdet *= 2.0;
  if (P) {  // nu Li^T Li: the square of GaussWishState::whitener()
    const std::vector<double> Li = lch::tril_inverse(L, D);
    for (int i = 0; i < D; ++i)
      for (int c = 0; c <= i; ++c) {
        double v = 0.0;
        for (int k = i; k < D; ++k) v += Li[(size_t)k * D + i] * Li[(size_t)k * D + c];
        P[(size_t)i * D + c] = P[(size_t)c * D + i] = nu * v;
      }
  }
  for (int nb = 0; nb < NH; ++nb) {
    const int Da = D - nb;
    if (G)
      G[nb] = Da < 0 ? std::numeric_limits<double>::quiet_NaN()
                     : lch::lgam((nup + Da) / 2) - lch::lgam(nup / 2) - 0.5 * Da * std::log(nup * lch::PI) +
                           0.5 * (Da * std::log(nup * beta / (1 + beta)) - (logdet - nb * std::log(nu)));
    if (e) e[nb] = (nup + Da) / 2;
  }
  if (s) *s = beta / ((1 + beta) * nu);
}

void gw_precision_var(int D, double nu, double beta, double* g) {
  constexpr int NH = lck::HOLES_MAX + 1;
  const double nup = nu + 1 - D;  // (the checks of gw_precision)
  if (!(nup > 0.0) || !(beta > 0.0)) throw std::invalid_argument("nu must exceed D - 1 and beta must be positive");
  for (int nb = 0; nb < NH; ++nb) {
    const double dof2 = nu - 1 - nb;  // nu' + Da - 2 with Da = D - nb
    g[nb] = nb >= D || !(dof2 > 0.0) ? std::numeric_limits<double>::quiet_NaN() : (1 + beta) / (beta * dof2);
  }
}

void predict_incomplete(lcc::Context& ctx, const lce::Model& model, const int* groups, bool want_var, int ndraws,
                        uint64_t seed) {
  ctx.predict_clear();  // (whatever an earlier prediction left must not outlive a failure of this one)
  if (ndraws < 0 || ndraws > lck::DRAWS_MAX) throw std::invalid_argument("ndraws must be in 1 ... 64");
  if (ndraws > 0 && want_var) throw std::invalid_argument("draws and the variance are two calls");
  constexpr int NH = lck::HOLES_MAX + 1;
  const int K = (int)model.clusters.size(), J = (int)model.weights.size(), Jc = ctx.J();
  if (K < 1) throw std::invalid_argument("the model has no clusters");
  if (model.ckind != lch::C_GAUSSWISH)
    throw std::invalid_argument("conditional prediction needs Gauss-Wishart clusters: the columns of NormGamma / ExpGamma "
                                "clusters are independent within a cluster (not supported)");
  const int D = model.clusters[0].gw.D;
  if (Jc > 0 && ctx.D() != D) throw std::invalid_argument("Mismatched dims. of cluster params and obs.!");
  for (int b = 0; b < Jc; ++b) {
    const int j = groups ? groups[b] : 0;
    if (j < 0 || j >= J) throw std::invalid_argument("group index out of range");
  }
  if (Jc < 1) return;  // (a context without observations: nothing to complete, nothing to read)
  if (ctx.DP() > lck::GW_MAX_DP)  // (what the E-step below would refuse, said before the holes are filled)
    throw std::invalid_argument("D > 1024 is not supported by the Gauss-Wishart kernels (the diagonal and exponential "
                                "families take any D)");
  std::vector<double> Epi((size_t)J * K), Erest((size_t)J);
  bool rest = false;
  for (int j = 0; j < J; ++j) {
    if ((int)model.weights[(size_t)j].alpha1.size() != K) throw std::invalid_argument("weights and clusters disagree");
    weights_predictive(model.weights[(size_t)j], Epi.data() + (size_t)j * K, &Erest[(size_t)j]);
    rest = rest || Erest[(size_t)j] > 0.0;
  }
  const int Kp = K + (rest ? 1 : 0);
  const lch::ClusterAny prior(model.ckind, model.clusters[0].prior(), D);  // clearobs state: a cluster that saw no data
  std::vector<double> P((size_t)Kp * D * D), G((size_t)Kp * NH), ps((size_t)Kp), ek((size_t)Kp * NH);
  std::vector<double> A((size_t)Kp * D * D), m((size_t)Kp * D);
  for (int k = 0; k < Kp; ++k) {
    const lch::GaussWishState& g = k < K ? model.clusters[(size_t)k].gw : prior.gw;
    gw_precision(D, g.nu, g.beta, g.iW.data(), P.data() + (size_t)k * D * D, &G[(size_t)k * NH], &ps[(size_t)k],
                 &ek[(size_t)k * NH]);
    const std::vector<double> Ak = g.whitener();
    std::copy(Ak.begin(), Ak.end(), A.begin() + (size_t)k * D * D);
    std::copy(g.m.begin(), g.m.end(), m.begin() + (size_t)k * D);
  }
  // tables by hole count: tt [Jc x NH x Kp], pe [NH x Kp]
  std::vector<double> tt((size_t)Jc * NH * Kp), pe((size_t)NH * Kp), zero((size_t)Jc * Kp, 0.0);
  for (int nb = 0; nb < NH; ++nb) {
    for (int k = 0; k < Kp; ++k) pe[(size_t)nb * Kp + k] = ek[(size_t)k * NH + nb];
    for (int b = 0; b < Jc; ++b) {
      const int j = groups ? groups[b] : 0;
      double* t = tt.data() + ((size_t)b * NH + nb) * Kp;
      for (int k = 0; k < K; ++k) t[k] = std::log(Epi[(size_t)j * K + k]) + G[(size_t)k * NH + nb];
      if (rest) t[K] = std::log(Erest[(size_t)j]) + G[(size_t)K * NH + nb];
    }
  }
  // what goes into the holes before the E-step: any finite value gives the same answer in exact arithmetic; one close to
  // the data (the N_k-weighted mean of the cluster means) keeps an offset far from the origin out of d_full^2 - u^T H^-1 u
  std::vector<double> fill((size_t)D, 0.0);
  double wsum = 0.0;
  for (int k = 0; k < K; ++k) wsum += model.clusters[(size_t)k].gw.N;
  for (int k = 0; k < K; ++k) {
    const lch::GaussWishState& g = model.clusters[(size_t)k].gw;
    const double w = wsum > 0.0 ? g.N / wsum : 1.0 / K;
    for (int d = 0; d < D; ++d) fill[(size_t)d] += w * g.m[(size_t)d];
  }

  int64_t holed = 0, bad_row = -1;
  int max_count = 0, bad_block = -1, bad_count = 0;
  ctx.holes_scan(&holed, &max_count, &bad_block, &bad_row, &bad_count);
  if (bad_block >= 0)  // (nothing was written to X so far)
    throw std::invalid_argument("row " + std::to_string(bad_row) + " of block " + std::to_string(bad_block) + " has " +
                                std::to_string(bad_count) + " unknown values (NaN) among its " + std::to_string(D) +
                                " columns: at most " + std::to_string(lck::HOLES_MAX) +
                                " per row, and at least one known column (lc_model_predict_conditional takes a pattern "
                                "shared by all rows, of any size)");
  // the variance's table g_k(nb) nu_k, 0 where the variance does not exist: an error when a row can meet such an entry
  // (a component with weight in some block, at the largest hole count of the context), never read otherwise
  std::vector<double> gnu;
  if (want_var) {
    gnu.assign((size_t)NH * Kp, 0.0);
    for (int k = 0; k < Kp; ++k) {
      const lch::GaussWishState& g = k < K ? model.clusters[(size_t)k].gw : prior.gw;
      if (holed > 0 && !(g.nu - 1 - max_count > 0.0)) {
        bool weighted = false;
        for (int b = 0; b < Jc; ++b) {
          const int j = groups ? groups[b] : 0;
          weighted = weighted || (k < K ? Epi[(size_t)j * K + k] : Erest[(size_t)j]) > 0.0;
        }
        if (weighted)  // (nothing was written to X so far)
          throw std::domain_error("the variance of the filled values does not exist: " +
                                  (k < K ? "cluster " + std::to_string(k) : std::string("the prior component")) + " has nu - 1 - " +
                                  std::to_string(max_count) + " = " + std::to_string(g.nu - 1 - max_count) +
                                  ", which is not above 0, and a row of the context has " + std::to_string(max_count) +
                                  " unknown values (the completed rows and logp of lc_model_predict_incomplete do exist)");
      }
      double gk[NH];
      gw_precision_var(D, g.nu, g.beta, gk);
      for (int nb = 0; nb < NH; ++nb)
        if (gk[nb] == gk[nb]) gnu[(size_t)nb * Kp + k] = gk[nb] * g.nu;
    }
  }
  if (holed > 0) ctx.holes_fill(fill.data());
  // one raw E-step at full width over the K clusters (+ the prior's whitener): -d_full^2 / 2 per column
  ctx.estep(Kp, A.data(), m.data(), zero.data(), nullptr, nullptr, /*raw=*/true);
  // the draws' table: cqnu_k = (1 + beta_k) nu_k / (2 beta_k), no moment has to exist
  std::vector<double> cqnu;
  if (ndraws > 0) {
    cqnu.resize((size_t)Kp);
    for (int k = 0; k < Kp; ++k) {
      const lch::GaussWishState& g = k < K ? model.clusters[(size_t)k].gw : prior.gw;
      cqnu[(size_t)k] = (1 + g.beta) * g.nu / (2 * g.beta);
    }
  }
  ctx.predict_holes(Kp, tt.data(), ps.data(), pe.data(), m.data(), P.data(), want_var ? gnu.data() : nullptr,
                    ndraws > 0 ? cqnu.data() : nullptr, ndraws, seed);
}

void predict_leave_one_out(lcc::Context& ctx, const lce::Model& model, const int* groups, bool want_var) {
  ctx.predict_clear();  // (whatever an earlier prediction left must not outlive a failure of this one)
  constexpr int NH = lck::HOLES_MAX + 1;
  const int K = (int)model.clusters.size(), J = (int)model.weights.size(), Jc = ctx.J();
  if (K < 1) throw std::invalid_argument("the model has no clusters");
  if (model.ckind != lch::C_GAUSSWISH)
    throw std::invalid_argument("leave-one-out conditionals need Gauss-Wishart clusters: the columns of NormGamma / ExpGamma "
                                "clusters are independent within a cluster (not supported)");
  const int D = model.clusters[0].gw.D;
  if (Jc > 0 && ctx.D() != D) throw std::invalid_argument("Mismatched dims. of cluster params and obs.!");
  if (D < 2) throw std::invalid_argument("leave-one-out conditionals need D >= 2: with one column no known column is left");
  for (int b = 0; b < Jc; ++b) {
    const int j = groups ? groups[b] : 0;
    if (j < 0 || j >= J) throw std::invalid_argument("group index out of range");
  }
  if (Jc < 1) return;  // (a context without observations: nothing to score)
  if (ctx.DP() > lck::GW_MAX_DP)
    throw std::invalid_argument("D > 1024 is not supported by the Gauss-Wishart kernels (the diagonal and exponential "
                                "families take any D)");
  std::vector<double> Epi((size_t)J * K), Erest((size_t)J);
  bool rest = false;
  for (int j = 0; j < J; ++j) {
    if ((int)model.weights[(size_t)j].alpha1.size() != K) throw std::invalid_argument("weights and clusters disagree");
    weights_predictive(model.weights[(size_t)j], Epi.data() + (size_t)j * K, &Erest[(size_t)j]);
    rest = rest || Erest[(size_t)j] > 0.0;
  }
  const int Kp = K + (rest ? 1 : 0);
  const lch::ClusterAny prior(model.ckind, model.clusters[0].prior(), D);  // clearobs state: a cluster that saw no data
  // nb = 0: predict()'s own constants, so that logp is its logp to the bit; nb = 1: the row of predict_incomplete's tables
  std::vector<double> P((size_t)Kp * D * D), ps((size_t)Kp), pe0((size_t)Kp), pe1((size_t)Kp), lc0((size_t)Kp), G1((size_t)Kp);
  std::vector<double> A((size_t)Kp * D * D), m((size_t)Kp * D), gnu1;
  if (want_var) gnu1.assign((size_t)Kp, 0.0);
  for (int k = 0; k < Kp; ++k) {
    const lch::GaussWishState& g = k < K ? model.clusters[(size_t)k].gw : prior.gw;
    double G[NH], e[NH], s;
    gw_precision(D, g.nu, g.beta, g.iW.data(), P.data() + (size_t)k * D * D, G, &s, e);
    const Predictive p0 = gw_predictive(g);
    lc0[(size_t)k] = p0.lc;
    ps[(size_t)k] = p0.s;
    pe0[(size_t)k] = p0.e;
    G1[(size_t)k] = G[1];
    pe1[(size_t)k] = e[1];
    const std::vector<double> Ak = g.whitener();
    std::copy(Ak.begin(), Ak.end(), A.begin() + (size_t)k * D * D);
    std::copy(g.m.begin(), g.m.end(), m.begin() + (size_t)k * D);
    if (want_var) {
      // the check of DESIGN 4.15.1 with cmax = 1: g_k(1) = (1 + beta) / (beta (nu - 2)) has to exist wherever a row can meet it
      if (!(g.nu - 2 > 0.0)) {
        bool weighted = false;
        for (int b = 0; b < Jc; ++b) {
          const int j = groups ? groups[b] : 0;
          weighted = weighted || (k < K ? Epi[(size_t)j * K + k] : Erest[(size_t)j]) > 0.0;
        }
        if (weighted)
          throw std::domain_error("the leave-one-out variance does not exist: " +
                                  (k < K ? "cluster " + std::to_string(k) : std::string("the prior component")) +
                                  " has nu - 2 = " + std::to_string(g.nu - 2) +
                                  ", which is not above 0 (lc_model_predict_leave_one_out without variance does exist)");
      } else {
        double gk[NH];
        gw_precision_var(D, g.nu, g.beta, gk);
        gnu1[(size_t)k] = gk[1] * g.nu;
      }
    }
  }
  std::vector<double> pc((size_t)Jc * Kp), tt1((size_t)Jc * Kp), zero((size_t)Jc * Kp, 0.0);
  for (int b = 0; b < Jc; ++b) {
    const int j = groups ? groups[b] : 0;
    for (int k = 0; k < Kp; ++k) {
      const double lw = std::log(k < K ? Epi[(size_t)j * K + k] : Erest[(size_t)j]);
      pc[(size_t)b * Kp + k] = lw + lc0[(size_t)k];
      tt1[(size_t)b * Kp + k] = lw + G1[(size_t)k];
    }
  }
  int64_t holed = 0, bad_row = -1;
  int max_count = 0, bad_block = -1, bad_count = 0;
  ctx.holes_scan(&holed, &max_count, &bad_block, &bad_row, &bad_count);
  if (holed > 0) {  // (nothing was written so far)
    int64_t row = -1;
    int block = -1;
    ctx.first_holed_row(&block, &row);
    throw std::invalid_argument("row " + std::to_string(row) + " of block " + std::to_string(block) +
                                " holds an unknown value (NaN): leave-one-out conditionals need complete rows "
                                "(lc_model_predict_incomplete takes rows with unknown values)");
  }
  // one raw E-step at full width over the K clusters (+ the prior's whitener), as predict() runs it: -d^2 / 2 per column
  ctx.estep(Kp, A.data(), m.data(), zero.data(), nullptr, nullptr, /*raw=*/true);
  ctx.predict_loo(Kp, pc.data(), ps.data(), pe0.data(), tt1.data(), pe1.data(), want_var ? gnu1.data() : nullptr, m.data(),
                  P.data());
}

void exemplars(lcc::Context& ctx, const lce::Model& model, bool sparse, const int* groups, int mtop, int32_t* count,
               int32_t* group, int64_t* row, double* score) {
  if (mtop < 1 || mtop > lck::TOP_MAX_M) throw std::invalid_argument("m must be in 1 ... 64");  // (before the prediction runs)
  if (ctx.J() < 1) throw std::invalid_argument("the context holds no observations (lc_ctx_set_data / lc_ctx_synth)");
  // Without keep_qz, predict_rows_kernel only READS the raw columns (it writes label, logZ, logp): when predict() returns,
  // columns 0 .. K - 1 of qZ still hold the raw E-step's data terms, Eloglike_k(x_n) minus the cluster's constant.
  predict(ctx, model, sparse, groups, /*keep_qz=*/false);
  const int K = (int)model.clusters.size();
  ctx.top_rows(0, K, mtop, /*largest=*/true, /*by_label=*/true, count, group, row, score);
  for (int k = 0; k < K; ++k) {
    const double cst = model.clusters[(size_t)k].eloglike_const();
    for (int i = 0; i < count[k]; ++i) score[(size_t)k * mtop + i] += cst;
  }
}

}  // namespace lcp
