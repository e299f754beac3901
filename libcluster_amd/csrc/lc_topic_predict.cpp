// Inference for new documents with a learned SCM / MCM model: the host tables (a_t per document, E_tk,
// the bottom-level whiteners and Eloglike constants) and the context's side of the pass.  Kernel: lc_kernels_topic.hip.
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "lc_ctx.hpp"
#include "lc_host.hpp"
#include "lc_topic.hpp"

namespace lcc {

void Context::topic_infer(int K, int T, const double* a, const double* E, int max_sweeps, double tol, bool keep_q) {
  use_device();
  if (K < 1 || T < 1) throw std::invalid_argument("qZ and qY must have at least one column");
  if (max_sweeps < 1) throw std::invalid_argument("max_sweeps must be at least 1");
  predict_clear();
  if (NP_ > 0 && (qz_[cur_].cap < K || !qz_[cur_].buf.p)) throw std::logic_error("topic_infer: no raw E-step columns");
  const int64_t maxN = *std::max_element(Nj_.begin(), Nj_.end());
  lck::TopicInferLaunch l;
  l.threads = maxN <= 64 ? 64 : maxN <= 128 ? 128 : 256;
  const size_t lds = lck::topic_infer_lds(K, T, l.threads, Nj_.data(), J_, &l.tile_cap, &l.e_lds);
  if (lds == 0) throw std::invalid_argument("the model is too large for the inference kernel (K and T against its LDS)");
  plabel_.reserve((size_t)std::max<int64_t>(NP_, 1));
  plogz_.reserve((size_t)std::max<int64_t>(NP_, 1));
  tqy_.reserve((size_t)J_ * T);
  tf_.reserve((size_t)J_ * 2);
  tint_.reserve((size_t)J_ * 2);
  tnrows_.reserve((size_t)J_);
  // tables: [a J x T | E T x K]
  const size_t na = (size_t)J_ * T, ne = (size_t)T * K;
  hpack_.resize(na + ne);
  std::copy(a, a + na, hpack_.data());
  std::copy(E, E + ne, hpack_.data() + na);
  ptab_.reserve(hpack_.size());
  LC_HIP(hipMemcpyAsync(ptab_.p, hpack_.data(), hpack_.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
  LC_HIP(hipMemcpyAsync(tnrows_.p, Nj_.data(), (size_t)J_ * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
  l.col = qz_[cur_].buf.p;
  l.ldq = NP_;
  l.K = K;
  l.T = T;
  l.docs = J_;
  l.goff = goff_d_.p;
  l.nrows = tnrows_.p;
  l.a = ptab_.p;
  l.E = ptab_.p + na;
  l.max_sweeps = max_sweeps;
  l.tol = tol;
  l.keep_q = keep_q ? 1 : 0;
  l.label = plabel_.p;
  l.logZ = plogz_.p;
  l.qY = tqy_.p;
  l.F = tf_.p;
  l.dint = tint_.p;
  LC_HIP(lck::launch_topic_infer(l, lds, stream_));
  LC_HIP(hipStreamSynchronize(stream_));  // (hpack_, ptab_ and Nj_ are free again)
  qz_[cur_].K = K;
  qz_[cur_].hash_ok = false;
  qz_written(qz_[cur_]);
  pred_vb_ = true;
  pred_docs_T_ = T;
}

void Context::get_doc_predictions(int doc0, int n, double* qY, int32_t* label_t, double* Fyz, double* Fz,
                                  int32_t* sweeps) const {
  use_device();
  if (doc0 < 0 || n < 0 || (int64_t)doc0 + n > J_) throw std::invalid_argument("document range out of bounds");
  if (pred_docs_T_ < 1) throw std::invalid_argument("the context holds no document prediction (lc_tmodel_predict)");
  if (n == 0) return;
  const int T = pred_docs_T_;
  std::vector<double> f((size_t)n * 2);
  std::vector<int> di((size_t)n * 2);
  if (qY)
    LC_HIP(hipMemcpyAsync(qY, tqy_.p + (size_t)doc0 * T, (size_t)n * T * sizeof(double), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipMemcpyAsync(f.data(), tf_.p + (size_t)doc0 * 2, f.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipMemcpyAsync(di.data(), tint_.p + (size_t)doc0 * 2, di.size() * sizeof(int), hipMemcpyDeviceToHost, stream_));
  LC_HIP(hipStreamSynchronize(stream_));
  for (int i = 0; i < n; ++i) {
    if (Fyz) Fyz[i] = f[(size_t)i * 2];
    if (Fz) Fz[i] = f[(size_t)i * 2 + 1];
    if (label_t) label_t[i] = di[(size_t)i * 2];
    if (sweeps) sweeps[i] = di[(size_t)i * 2 + 1];
  }
}

}  // namespace lcc

namespace lce {

void topic_predict(lcc::Context& ctx, const TopicModel& model, const int* groups, const double* W, int max_sweeps,
                   double tol, bool keep_qz) {
  const int I = ctx.J(), D = ctx.D(), T = model.T, K = (int)model.clusters.size();
  const bool mcm = !model.clusters_t.empty();
  if (K < 1 || T < 1) throw std::invalid_argument("the model has no clusters");
  ctx.predict_clear();  // (whatever an earlier prediction left must not outlive a failure of this one)

  // a_t = E[log pi_gt] (+ GaussWish::Eloglike of the document observation, distributions.cpp:356-370, as vbeY of
  // mcluster.cpp:49-92 forms it), E_tk = E[log pi_tk]
  std::vector<double> a((size_t)I * T), E((size_t)T * K);
  for (int t = 0; t < T; ++t) std::copy(model.weights_t[(size_t)t].Elogpi.begin(), model.weights_t[(size_t)t].Elogpi.end(),
                                        E.begin() + (size_t)t * K);
  std::vector<std::vector<double>> At;
  std::vector<double> ctt;
  const int Dt = mcm ? model.clusters_t[0].D : 0;
  for (int t = 0; mcm && t < T; ++t) {
    At.push_back(model.clusters_t[(size_t)t].whitener());
    ctt.push_back(model.clusters_t[(size_t)t].eloglike_const());
  }
  for (int i = 0; i < I; ++i) {
    const lch::WeightState& wj = model.weights_j[(size_t)(groups ? groups[i] : 0)];
    for (int t = 0; t < T; ++t) {
      double v = wj.Elogpi[(size_t)t];
      if (mcm) {
        const double* w = W + (size_t)i * Dt;
        const double* at = At[(size_t)t].data();
        const std::vector<double>& mt = model.clusters_t[(size_t)t].m;
        double d2 = 0.0;
        for (int r = 0; r < Dt; ++r) {
          double s = 0.0;
          for (int cc = 0; cc <= r; ++cc) s += at[(size_t)r * Dt + cc] * (w[cc] - mt[(size_t)cc]);
          d2 += s * s;
        }
        v += ctt[(size_t)t] - 0.5 * d2;
      }
      a[(size_t)i * T + t] = v;
    }
  }

  // one raw E-step over all documents with the clusters' own constants: L_nk = Eloglike_k(x_n) in the qZ columns
  std::vector<double> A((size_t)K * D * D), m((size_t)K * D), c((size_t)I * K);
  for (int k = 0; k < K; ++k) {
    const lch::GaussWishState& g = model.clusters[(size_t)k];
    const std::vector<double> Ak = g.whitener();
    std::copy(Ak.begin(), Ak.end(), A.begin() + (size_t)k * D * D);
    std::copy(g.m.begin(), g.m.end(), m.begin() + (size_t)k * D);
    const double cst = g.eloglike_const();
    for (int i = 0; i < I; ++i) c[(size_t)i * K + k] = cst;
  }
  ctx.estep(K, A.data(), m.data(), c.data(), nullptr, nullptr, /*raw=*/true);
  ctx.topic_infer(K, T, a.data(), E.data(), max_sweeps, tol, keep_qz);
}

}  // namespace lce
