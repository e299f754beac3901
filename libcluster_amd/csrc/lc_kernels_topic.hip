// Inference with a learned two-level model: topic_infer_kernel finds, for every document of the
// context, its class responsibilities qY and its rows' segment responsibilities qZ with the model held fixed -- the
// per-document fixed point of vbeY / vbeZ (scluster.cpp:50-124, mcluster.cpp:49-135).  The expected log-likelihoods
// L_nk = Eloglike_k(x_n) do not change between sweeps: a raw E-step leaves them in the context's qZ columns, and one
// workgroup per document then runs that document's sweeps to its own stopping point, out of LDS where the document's
// L tile fits.  Nothing is accumulated with atomics: every sum has a fixed order, two runs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>

#include "lc_device.hpp"
#include "lc_kernels.h"

namespace lck {
namespace {

constexpr int TI_MAX_THREADS = 256;
constexpr int TI_KR = 16;  // K <= TI_KR: a row's K terms stay in registers (one exponential per responsibility)

// doubles of LDS in front of the E table and the tile
__host__ __device__ inline int64_t ti_fixed(int K, int T, int nw) {
  return 64 + 4 * (int64_t)T + 2 * (int64_t)K + (int64_t)nw * (K + 1) + 4;
}

// softmax over T values by ONE thread (T is the number of classes: a handful); returns the log normaliser
__device__ __forceinline__ double softmax_serial(const double* v, const double* add, double* out, int T,
                                                 const double* etab) {
  double m = -std::numeric_limits<double>::infinity();
  for (int t = 0; t < T; ++t) m = fmax(m, add ? v[t] + add[t] : v[t]);
  double s = 0.0;
  for (int t = 0; t < T; ++t) s += exp_nonpos((add ? v[t] + add[t] : v[t]) - m, etab);
  const double lz = m + log(s);  // probutils::logsumexp (probutils.cpp:141-150)
  for (int t = 0; t < T; ++t) out[t] = exp_nonpos((add ? v[t] + add[t] : v[t]) - lz, etab);
  return lz;
}

struct TiShared {
  double *etab, *qy, *qyn, *av, *like, *cv, *nk, *part, *scal;
  const double* E;  // LDS or global
};

// vbeZ of one document with the class responsibilities in s.qy (scluster.cpp:93-124): c_k = sum_t qY_t E_tk,
// q_nk = softmax_k(c_k + L_nk).  FINAL = false: N_k = sum_n q_nk into s.nk.  FINAL = true: label, logZ (and q with
// keep_q) per row, sum_n logZ_n into s.scal[2].  Ends with a barrier.
// Order of the sums, a function of N and the workgroup size only.  sum logZ, and N_k for K <= KR: a thread's rows in
// ascending order (in a register), the 64 lanes of a wave by the butterfly of wave_sum once per pass, the waves in
// ascending order.  N_k for larger K (no registers for K running sums): per batch of blockDim rows the butterfly,
// the batches in ascending order by lane 0 of every wave, then the waves in ascending order.
template <bool TILED, int KR, bool FINAL>
__device__ __forceinline__ void vbez_pass(const TopicInferLaunch& a, const TiShared& s, const double* tile, double* col,
                                          int64_t N, int64_t row0) {
  const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nth >> 6;
  const int K = a.K, T = a.T;
  for (int k = tid; k < K; k += nth) {
    double c = 0.0;
    for (int t = 0; t < T; ++t) c = fma(s.qy[t], s.E[(size_t)t * K + k], c);
    s.cv[k] = c;
  }
  for (int i = tid; i < nw * (K + 1); i += nth) s.part[i] = 0.0;
  __syncthreads();
  double* mypart = s.part + (size_t)wv * (K + 1);
  const int64_t ldl = TILED ? N : a.ldq;
  const double* Lp = TILED ? tile : col;
  constexpr double NINF = -std::numeric_limits<double>::infinity();
  double lzsum = 0.0;
  double acc[KR > 0 ? KR : 1];  // (K <= KR, sweeps) this thread's share of N_k
#pragma unroll
  for (int k = 0; k < (KR > 0 ? KR : 1); ++k) acc[k] = 0.0;
  for (int64_t n0 = 0; n0 < N; n0 += nth) {  // (block-uniform trip count: every wave meets the shuffles below)
    const int64_t n = n0 + tid;
    const bool valid = n < N;
    const int64_t nn = valid ? n : 0;  // (idle lanes read row 0 and contribute nothing)
    double m = NINF, sum = 0.0;
    int lab = 0;
    if constexpr (KR > 0) {
      double v[KR];
#pragma unroll
      for (int k = 0; k < KR; ++k)
        if (k < K) {
          v[k] = s.cv[k] + Lp[(size_t)k * ldl + nn];
          if (v[k] > m) {  // first maximum: the lowest k on ties
            m = v[k];
            lab = k;
          }
        }
#pragma unroll
      for (int k = 0; k < KR; ++k)
        if (k < K) {
          v[k] = exp_nonpos(v[k] - m, s.etab);
          sum += v[k];
        }
      const double rs = rcp_pos(sum);
#pragma unroll
      for (int k = 0; k < KR; ++k)
        if (k < K) {
          const double q = v[k] * rs;
          if constexpr (FINAL) {
            if (a.keep_q && valid) col[(size_t)k * a.ldq + n] = q;
          } else {
            acc[k] += valid ? q : 0.0;
          }
        }
    } else {
      for (int k = 0; k < K; ++k) {
        const double v = s.cv[k] + Lp[(size_t)k * ldl + nn];
        if (v > m) {
          m = v;
          lab = k;
        }
      }
      for (int k = 0; k < K; ++k) sum += exp_nonpos(s.cv[k] + Lp[(size_t)k * ldl + nn] - m, s.etab);
      const double rs = rcp_pos(sum);
      for (int k = 0; k < K; ++k) {
        const double q = exp_nonpos(s.cv[k] + Lp[(size_t)k * ldl + nn] - m, s.etab) * rs;
        if constexpr (FINAL) {
          if (a.keep_q && valid) col[(size_t)k * a.ldq + n] = q;
        } else {
          const double w = wave_sum(valid ? q : 0.0);
          if (lane == 0) mypart[k] += w;
        }
      }
    }
    if constexpr (FINAL) {
      if (valid) {
        const double lz = m + log(sum);
        lzsum += lz;
        a.label[row0 + n] = lab;
        a.logZ[row0 + n] = lz;
      }
    }
  }
  if constexpr (FINAL) {
    const double w = wave_sum(lzsum);
    if (lane == 0) mypart[K] = w;
  } else if constexpr (KR > 0) {
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (k < K) {
        const double w = wave_sum(acc[k]);
        if (lane == 0) mypart[k] = w;
      }
  }
  __syncthreads();
  if constexpr (FINAL) {
    if (tid == 0) {
      double f = 0.0;
      for (int w = 0; w < nw; ++w) f += s.part[(size_t)w * (K + 1) + K];
      s.scal[2] = f;
    }
  } else {
    for (int k = tid; k < K; k += nth) {
      double f = 0.0;
      for (int w = 0; w < nw; ++w) f += s.part[(size_t)w * (K + 1) + k];
      s.nk[k] = f;
    }
  }
  __syncthreads();
}

template <bool TILED, int KR>
__device__ __forceinline__ void infer_document(const TopicInferLaunch& a, const TiShared& s, double* tile, double* col,
                                               int64_t N, int64_t row0, int doc) {
  const int tid = threadIdx.x, nth = blockDim.x;
  const int K = a.K, T = a.T;
  if constexpr (TILED) {  // the one read of the document's L columns
    for (int k = 0; k < K; ++k)
      for (int64_t n = tid; n < N; n += nth) tile[(size_t)k * N + n] = col[(size_t)k * a.ldq + n];
  }
  if (tid == 0) softmax_serial(s.av, nullptr, s.qy, T, s.etab);  // qY^0: the group's weights
  __syncthreads();
  int R = 0;
  for (int r = 1; r <= a.max_sweeps; ++r) {
    vbez_pass<TILED, KR, false>(a, s, tile, col, N, row0);
    // vbeY (scluster.cpp:50-85 / mcluster.cpp:49-92)
    for (int t = tid; t < T; t += nth) {
      double l = 0.0;
      for (int k = 0; k < K; ++k) l = fma(s.nk[k], s.E[(size_t)t * K + k], l);
      s.like[t] = l;
    }
    __syncthreads();
    if (tid == 0) {
      const double lzy = softmax_serial(s.av, s.like, s.qyn, T, s.etab);
      double delta = 0.0, acc = 0.0;
      for (int t = 0; t < T; ++t) {
        delta = fmax(delta, fabs(s.qyn[t] - s.qy[t]));
        acc = fma(s.qyn[t], s.like[t], acc);
        s.qy[t] = s.qyn[t];
      }
      s.scal[0] = delta;
      s.scal[1] = acc - lzy;
    }
    __syncthreads();
    R = r;
    // (s.scal[0] is one LDS word read by every thread after the barrier: the exit is block-uniform, and the next
    //  write to it lies behind the barriers of the next pass)
    if (a.tol >= 0.0 && s.scal[0] <= a.tol) break;
  }
  vbez_pass<TILED, KR, true>(a, s, tile, col, N, row0);
  for (int t = tid; t < T; t += nth) a.qY[(size_t)doc * T + t] = s.qy[t];
  if (tid == 0) {
    int lt = 0;
    for (int t = 1; t < T; ++t)
      if (s.qy[t] > s.qy[lt]) lt = t;
    a.F[(size_t)doc * 2] = s.scal[1];
    a.F[(size_t)doc * 2 + 1] = -s.scal[2];
    a.dint[(size_t)doc * 2] = lt;
    a.dint[(size_t)doc * 2 + 1] = R;
  }
}

// (four waves per SIMD: at most 128 VGPRs -- the K <= 16 instance asked for 135 without the bound, one wave fewer)
template <int KR>
__global__ __launch_bounds__(TI_MAX_THREADS, 4) void topic_infer_kernel(TopicInferLaunch a) {
  extern __shared__ double ti_sm[];
  const int tid = threadIdx.x, nth = blockDim.x, nw = nth >> 6;
  const int K = a.K, T = a.T;
  TiShared s;
  s.etab = ti_sm;
  s.qy = s.etab + 64;
  s.qyn = s.qy + T;
  s.av = s.qyn + T;
  s.like = s.av + T;
  s.cv = s.like + T;
  s.nk = s.cv + K;
  s.part = s.nk + K;
  s.scal = s.part + (size_t)nw * (K + 1);
  double* Es = s.scal + 4;
  double* tile = Es + (a.e_lds ? (size_t)T * K : 0);
  const int doc = blockIdx.x;
  const int64_t N = a.nrows[doc], row0 = a.goff[doc];
  double* col = a.col + row0;
  fill_exp_table(s.etab, tid, nth);
  for (int t = tid; t < T; t += nth) s.av[t] = a.a[(size_t)doc * T + t];
  if (a.e_lds)
    for (int i = tid; i < T * K; i += nth) Es[i] = a.E[i];
  s.E = a.e_lds ? Es : a.E;
  if (tid < 4) s.scal[tid] = 0.0;
  __syncthreads();
  if (N * K <= a.tile_cap)  // (block-uniform)
    infer_document<true, KR>(a, s, tile, col, N, row0, doc);
  else
    infer_document<false, KR>(a, s, tile, col, N, row0, doc);
}

}  // namespace

size_t topic_infer_lds(int K, int T, int threads, const int64_t* nrows, int docs, int64_t* tile_cap, int* e_lds) {
  const int nw = threads / 64;
  const int el = (int64_t)T * K <= TOPIC_E_LDS ? 1 : 0;
  const int64_t fixed = ti_fixed(K, T, nw) + (el ? (int64_t)T * K : 0), budget = TOPIC_LDS_BYTES / 8;
  if (fixed > budget) return 0;
  int64_t cap = 0;  // the largest tile among the documents that fit
  for (int i = 0; i < docs; ++i) {
    const int64_t want = nrows[i] * K;
    if (want <= budget - fixed) cap = std::max(cap, want);
  }
  *tile_cap = cap;
  *e_lds = el;
  return (size_t)(fixed + cap) * sizeof(double);
}

hipError_t launch_topic_infer(const TopicInferLaunch& a, size_t lds_bytes, hipStream_t stream) {
  if (a.docs < 1) return hipSuccess;
  if (a.K < 1 || a.T < 1 || a.max_sweeps < 1 || (a.threads != 64 && a.threads != 128 && a.threads != 256) ||
      lds_bytes > (size_t)TOPIC_LDS_BYTES)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.docs), block((unsigned)a.threads);
  if (a.K <= TI_KR)
    hipLaunchKernelGGL((topic_infer_kernel<TI_KR>), grid, block, lds_bytes, stream, a);
  else
    hipLaunchKernelGGL((topic_infer_kernel<0>), grid, block, lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace lck
