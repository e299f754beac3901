// Prediction kernels: what a learned mixture says about observations that were not in the training set.
//
// predict_rows_kernel finishes the raw E-step (estep_kernel / estep_wide_kernel / estep_diag_kernel with zero
// constants) the way vbexpectation does (cluster.cpp:91-138) -- E[log pi_jk] + Eloglike_k(x_n), log-sum-exp over
// Kful, q = exp(. - logZ) -- and, for Gauss-Wishart clusters, turns the same distances into the posterior predictive
// (multivariate Student-t per cluster, mixed with E[pi_jk]).  predict_diag_kernel forms the predictive of the separable
// families (product of Student-t / Lomax densities per dimension), which has no GEMM form.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "lc_device.hpp"
#include "lc_predict.hpp"

namespace lck {
namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_COLS = 8;  // predict_rows_kernel: columns loaded per batch

// (row_valid and lse_push: lc_device.hpp, shared with lc_kernels_holes.hip)

__global__ __launch_bounds__(PR_THREADS) void predict_rows_kernel(PredictRowsLaunch a) {
  __shared__ double etab[64];
  __shared__ LogEntry ltab[128];
  fill_exp_table(etab, threadIdx.x, PR_THREADS);
  fill_log_table(ltab, threadIdx.x, PR_THREADS);
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  int j = 0;
  if (row >= a.nrg * RG || !row_valid(row, a.rginfo, a.nrows, j)) return;
  const double* __restrict__ ct = a.ctab + (size_t)j * a.K;
  const double* __restrict__ pt = a.ptab + (size_t)j * a.Kp;
  const double* __restrict__ col = a.col + row;
  constexpr double NINF = -std::numeric_limits<double>::infinity();
  double m = NINF, s = 0.0, best = NINF, mp = NINF, sp = 0.0;
  int lab = 0;
  const int Kmax = a.K > a.Kp ? a.K : a.Kp;
  for (int k0 = 0; k0 < Kmax; k0 += PR_COLS) {  // the one read of the row's columns
    // PR_COLS independent loads in flight per lane before the arithmetic that consumes them (one at a time left the
    // kernel waiting on memory latency)
    double r[PR_COLS];
#pragma unroll
    for (int i = 0; i < PR_COLS; ++i) r[i] = k0 + i < Kmax ? col[(size_t)(k0 + i) * a.ldq] : 0.0;
#pragma unroll
    for (int i = 0; i < PR_COLS; ++i) {
      const int k = k0 + i;
      if (k < a.K) {
        const double v = ct[k] + r[i];
        if (v > best) {  // first maximum: the lowest k on ties
          best = v;
          lab = k;
        }
        lse_push(v, m, s, etab);
      }
      if (k < a.Kp) lse_push(pt[k] - a.pexp[k] * log1p_nonneg(a.pscale[k] * (-2.0 * r[i]), ltab), mp, sp, etab);
    }
  }
  const double lz = m + log(s);
  a.label[row] = lab;
  a.logZ[row] = lz;
  if (a.Kp > 0) a.logp[row] = mp + log(sp);
  if (a.keep_q) {
    double* q = a.qcol + row;
    for (int k = 0; k < a.K; ++k) q[(size_t)k * a.ldq] = exp_nonpos(ct[k] + q[(size_t)k * a.ldq] - lz, etab);
  }
}

// log of a product of factors >= 1 taken PRED_RENORM at a time, the binary exponent moved out after every group
__device__ __forceinline__ double log_scaled(double p, int ex) {
  return fma((double)ex, 0x1.62e42fefa39efp-1, log(p)) + (double)ex * 0x1.abc9e3b39803fp-56;
}

template <int MODE>
__device__ __forceinline__ double pred_factor(double x, double ad, double wd) {
  if constexpr (MODE == 0) {
    const double t = x - ad;
    return fma(wd * t, t, 1.0);
  } else {
    return fma(wd, x, 1.0);
  }
}

// DPT > 0: the padded width is DPT and the row's x lives in registers; DPT = 0: any DP, x re-read from the cache
template <int MODE, int DPT>
__global__ __launch_bounds__(PR_THREADS) void predict_diag_kernel(PredictDiagLaunch a) {
  __shared__ double etab[64];
  fill_exp_table(etab, threadIdx.x, PR_THREADS);
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  int j = 0;
  if (row >= a.nrg * RG || !row_valid(row, a.rginfo, a.nrows, j)) return;
  const int DP = DPT > 0 ? DPT : a.DP;
  const double* __restrict__ xr = a.X + (size_t)row * DP;
  double xv[DPT > 0 ? DPT : 1];
  bool neg = false;
  if constexpr (DPT > 0) {
#pragma unroll
    for (int d = 0; d < DPT; d += 2) {
      const double2 v = *reinterpret_cast<const double2*>(xr + d);
      xv[d] = v.x;
      xv[d + 1] = v.y;
      neg = neg || v.x < 0.0 || v.y < 0.0;
    }
  } else {
    for (int d = 0; d < DP; ++d) neg = neg || xr[d] < 0.0;
  }
  if (MODE == 1 && neg) *a.flag = 1;  // (ExpGamma's domain, cluster.cpp:742; every writer stores the same value)
  const double* __restrict__ pt = a.ptab + (size_t)j * a.Kp;
  double m = -std::numeric_limits<double>::infinity(), s = 0.0;
  for (int k = 0; k < a.Kp; ++k) {  // wave-uniform: the cluster's parameters are the same for every lane
    const double* __restrict__ ak = a.a + (size_t)k * DP;
    const double* __restrict__ wk = a.w + (size_t)k * DP;
    // two running products over alternate groups of PRED_RENORM factors, each group multiplied as a tree: the chain of
    // dependent fp64 operations is a third of the serial product's (the kernel runs at 2-3 waves per SIMD)
    double p[2] = {1.0, 1.0};
    int ex[2] = {0, 0};
    auto group = [&](int h, double f0, double f1, double f2, double f3) {
      int e;
      p[h] = frexp(p[h] * ((f0 * f1) * (f2 * f3)), &e);
      ex[h] += e;
    };
    static_assert(PRED_RENORM == 4, "group() takes four factors");
    if constexpr (DPT > 0) {
      static_for<DPT / PRED_RENORM>([&](auto c) {
        const int d = c * PRED_RENORM;
        group(c & 1, pred_factor<MODE>(xv[d], MODE == 0 ? ak[d] : 0.0, wk[d]),
              pred_factor<MODE>(xv[d + 1], MODE == 0 ? ak[d + 1] : 0.0, wk[d + 1]),
              pred_factor<MODE>(xv[d + 2], MODE == 0 ? ak[d + 2] : 0.0, wk[d + 2]),
              pred_factor<MODE>(xv[d + 3], MODE == 0 ? ak[d + 3] : 0.0, wk[d + 3]));
      });
    } else {
      for (int d = 0; d < DP; d += PRED_RENORM)
        group((d / PRED_RENORM) & 1, pred_factor<MODE>(xr[d], MODE == 0 ? ak[d] : 0.0, wk[d]),
              pred_factor<MODE>(xr[d + 1], MODE == 0 ? ak[d + 1] : 0.0, wk[d + 1]),
              pred_factor<MODE>(xr[d + 2], MODE == 0 ? ak[d + 2] : 0.0, wk[d + 2]),
              pred_factor<MODE>(xr[d + 3], MODE == 0 ? ak[d + 3] : 0.0, wk[d + 3]));
    }
    lse_push(pt[k] - a.pexp[k] * log_scaled(p[0] * p[1], ex[0] + ex[1]), m, s, etab);
  }
  a.logp[row] = m + log(s);
}

// Conditional mean.  Lane = lo2 + 4 blk + 16 hi of v_mfma_f64_4x4x4_4b (lc_device.hpp): MFMA block blk of
// row group g multiplies the rows 16 g + 4 blk + {0..3} of the wave (A: row lo2, column hi of the k-step) with a 4 x 4 piece
// of the table (B: given column hi, target lo2 -- the same in all four blocks) into D (row hi, target lo2).  In the first
// part lane l scores row l of the wave, which is row 4 blk + lo2 of row group hi: the r_k of row group g sit in the lanes
// with hi = g, and one __shfl per row group hands them to the lanes that build the A operands.
__global__ __launch_bounds__(PC_THREADS) void predict_cond_kernel(PredictCondLaunch a) {
  __shared__ double etab[64];
  __shared__ LogEntry ltab[128];
  fill_exp_table(etab, threadIdx.x, PC_THREADS);
  fill_log_table(ltab, threadIdx.x, PC_THREADS);
  __syncthreads();  // (the only barrier: from here on the waves do not meet)
  constexpr int NG = PC_WAVE_ROWS / RG, NS = PC_CHUNK / 4, NQ = PC_PANEL / 4;
  static_assert(RG == 16 && NG == 4, "one MFMA block per quad of rows, one shuffle source per row group");
  const int lane = threadIdx.x & 63, lo2 = lane & 3, blk = (lane >> 2) & 3, hi = lane >> 4;
  const int64_t NP = a.nrg * RG;
  const int64_t wrow0 = ((int64_t)blockIdx.x * (PC_THREADS / 64) + (threadIdx.x >> 6)) * PC_WAVE_ROWS;
  if (wrow0 >= NP) return;
  // NP is a multiple of 16, not of 64: rows past the end are clamped for reading and never written
  const int64_t row = wrow0 + lane, rrow = row < NP ? row : NP - 1;
  int j = 0;
  const bool valid = row_valid(rrow, a.rginfo, a.nrows, j) && row < NP;
  if (!valid) j = 0;  // (a pad row is scored like any other, so that the wave stays whole, and nothing of it is written)
  constexpr double NINF = -std::numeric_limits<double>::infinity();
  double* __restrict__ col = a.col + rrow;
  double logp;
  {  // log p(x_a) as predict_rows_kernel forms logp; t_k replaces the raw column
    const double* __restrict__ tt = a.ttab + (size_t)j * a.Kp;
    double m = NINF, s = 0.0;
    for (int k0 = 0; k0 < a.Kp; k0 += PR_COLS) {
      double r[PR_COLS];
#pragma unroll
      for (int i = 0; i < PR_COLS; ++i) r[i] = k0 + i < a.Kp ? col[(size_t)(k0 + i) * a.ldq] : 0.0;
#pragma unroll
      for (int i = 0; i < PR_COLS; ++i) {
        const int k = k0 + i;
        if (k < a.Kp) {
          const double t = tt[k] - a.pexp[k] * log1p_nonneg(a.pscale[k] * (-2.0 * r[i]), ltab);
          lse_push(t, m, s, etab);
          if (valid) col[(size_t)k * a.ldq] = t;
        }
      }
    }
    logp = m + log(s);
    if (valid) a.logp[row] = logp;
  }
  // rows of the A operands (row lo2 of block blk) and of the results (row hi of block blk), per row group
  int64_t xrow[NG];
  bool ovalid[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int64_t ra = wrow0 + g * RG + 4 * blk + lo2, ro = wrow0 + g * RG + 4 * blk + hi;
    xrow[g] = ra < NP ? ra : NP - 1;
    int jo;
    ovalid[g] = ro < NP && row_valid(ro < NP ? ro : NP - 1, a.rginfo, a.nrows, jo);
  }
  for (int t0 = 0; t0 < a.Db; t0 += PC_PANEL) {  // the accumulators of one panel of targets are resident
    const int nq = (a.Dbp - t0) / 4 < NQ ? (a.Dbp - t0) / 4 : NQ;
    double acc[NG][NQ];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[g][q] = 0.0;
    for (int c0 = 0; c0 < a.Dae; c0 += PC_CHUNK) {  // the x of one chunk of given columns is resident
      const int ns = (a.Dae - c0) / 4 < NS ? (a.Dae - c0) / 4 : NS;
      double x[NG][NS];
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const int c = c0 + 4 * s + hi;
          x[g][s] = c < a.Da ? a.X[(size_t)xrow[g] * a.DP + c] : c == a.Da ? 1.0 : 0.0;  // (the ones column carries m_b)
        }
      for (int k = 0; k < a.Kp; ++k) {
        // the tables stream from the cache cluster by cluster: Kp (Da + 1) Db doubles do not fit the LDS
        const double t = valid ? col[(size_t)k * a.ldq] : NINF;
        const double r = valid ? exp_nonpos(t - logp, etab) : 0.0;
        double rg[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) rg[g] = __shfl(r, g * RG + 4 * blk + lo2);
        const double* __restrict__ mk = a.mext + (size_t)k * a.Dae + c0 + hi;
        const double* __restrict__ Tk = a.T + ((size_t)k * a.Dae + c0 + hi) * a.Dbp + t0 + lo2;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (s < ns) {
            // the four scaled, centred operands of a k-step first, then its MFMAs in one run (a VALU
            // instruction between MFMAs is paid per switch)
            const double mv = mk[4 * s];
            double av[NG], bv[NQ];
#pragma unroll
            for (int g = 0; g < NG; ++g) av[g] = rg[g] * (x[g][s] - mv);
#pragma unroll
            for (int q = 0; q < NQ; ++q) bv[q] = q < nq ? Tk[(size_t)(4 * s) * a.Dbp + 4 * q] : 0.0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
              if (q < nq) {
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g][q] = mfma4(av[g], bv[q], acc[g][q]);
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int64_t ro = wrow0 + g * RG + 4 * blk + hi;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int tcol = t0 + 4 * q + lo2;
        if (ovalid[g] && tcol < a.Db) a.mean[(size_t)ro * a.Db + tcol] = acc[g][q];
      }
    }
  }
}

// Predictive variance, after predict_cond_kernel and in its lane layout.  Lane l owns row l of the wave in
// the first part of a cluster's step (r_k and h_k from the t_k and logp that kernel left); the lanes that hold row hi of
// block blk in the D operand fetch them with one __shfl per row group each.  The tile M_k of a cluster is complete -- all
// chunks of given columns contracted -- before it is squared: the loop order is panel, cluster, chunk, and x stays in
// registers across the clusters only when one chunk holds all given columns (Dae <= PC_CHUNK: RES); otherwise it is re-read
// per cluster from the cache.  With the 16-wide panel (80 resident doubles per lane) both instances fit the 256 registers
// of two waves per SIMD without scratch; the 32-wide panel (128 doubles) runs at one wave.
template <bool RES>  // RES: one chunk holds all given columns, x is loaded once
__global__ __launch_bounds__(PC_THREADS, PCV_PANEL == 16 ? 2 : 1) void predict_cond_var_kernel(PredictCondVarLaunch v) {
  __shared__ double etab[64];
  fill_exp_table(etab, threadIdx.x, PC_THREADS);
  __syncthreads();  // (the only barrier)
  const PredictCondLaunch& a = v.c;
  // (x that is re-read per cluster anyway is held half a chunk at a time: 32 registers less)
  constexpr int CH = RES ? PC_CHUNK : PC_CHUNK / 2;
  constexpr int NG = PC_WAVE_ROWS / RG, NS = CH / 4, NQ = PCV_PANEL / 4;
  static_assert(RG == 16 && NG == 4, "one MFMA block per quad of rows, one shuffle source per row group");
  const int lane = threadIdx.x & 63, lo2 = lane & 3, blk = (lane >> 2) & 3, hi = lane >> 4;
  const int64_t NP = a.nrg * RG;
  const int64_t wrow0 = ((int64_t)blockIdx.x * (PC_THREADS / 64) + (threadIdx.x >> 6)) * PC_WAVE_ROWS;
  if (wrow0 >= NP) return;
  // rows past the end and pad rows: clamped for reading, scored with r = h = 0, never written
  const int64_t row = wrow0 + lane, rrow = row < NP ? row : NP - 1;
  int j = 0;
  const bool valid = row_valid(rrow, a.rginfo, a.nrows, j) && row < NP;
  if (!valid) j = 0;
  const double* __restrict__ col = a.col + rrow;
  const double* __restrict__ tt = a.ttab + (size_t)j * a.Kp;
  const double logp = valid ? a.logp[rrow] : 0.0;
  int64_t xrow[NG];
  bool ovalid[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int64_t ra = wrow0 + g * RG + 4 * blk + lo2, ro = wrow0 + g * RG + 4 * blk + hi;
    xrow[g] = ra < NP ? ra : NP - 1;
    int jo;
    ovalid[g] = ro < NP && row_valid(ro < NP ? ro : NP - 1, a.rginfo, a.nrows, jo);
  }
  const unsigned toff = (unsigned)(hi * a.Dbp + lo2);  // of (given column hi, target lo2) inside a k-step's piece of T
  constexpr bool resident = RES;
  double x[NG][NS];
  auto load_x = [&](int c0) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int c = c0 + 4 * s + hi;
        x[g][s] = c < a.Da ? a.X[(size_t)xrow[g] * a.DP + c] : c == a.Da ? 1.0 : 0.0;  // (the ones column carries m_b)
      }
  };
  if (resident) load_x(0);
  for (int t0 = 0; t0 < a.Db; t0 += PCV_PANEL) {  // accumulators, mean and tile of one panel of targets are resident
    const int nq = (a.Dbp - t0) / 4 < NQ ? (a.Dbp - t0) / 4 : NQ;
    double acc[NG][NQ], mu[NG][NQ];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int64_t ro = wrow0 + g * RG + 4 * blk + hi, orow = ro < NP ? ro : NP - 1;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int tcol = t0 + 4 * q + lo2;
        acc[g][q] = 0.0;
        mu[g][q] = tcol < a.Db ? a.mean[(size_t)orow * a.Db + tcol] : 0.0;
      }
    }
    for (int k = 0; k < a.Kp; ++k) {
      const double t = col[(size_t)k * a.ldq];
      const double r = valid ? exp_nonpos(t - logp, etab) : 0.0;
      // 1 + s_k d_k^2 back from t_k = ttab_jk - e_k log1p(s_k d_k^2); a component without weight (t = -inf) adds nothing
      // (as the reciprocal of the table exponential of the negated argument: half the instructions and registers of exp())
      const double h = r > 0.0 ? v.g[k] * rcp_pos(exp_nonpos((t - tt[k]) / a.pexp[k], etab)) : 0.0;
      double tile[NG][NQ];
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int q = 0; q < NQ; ++q) tile[g][q] = 0.0;
      for (int c0 = 0; c0 < a.Dae; c0 += CH) {
        if (!resident) load_x(c0);
        const int ns = (a.Dae - c0) / 4 < NS ? (a.Dae - c0) / 4 : NS;
        // wave-uniform bases and one 32-bit lane offset: the addresses stay in scalar registers
        const double* __restrict__ mk = a.mext + (size_t)k * a.Dae + c0;
        const double* __restrict__ Tk = a.T + ((size_t)k * a.Dae + c0) * a.Dbp + t0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (s < ns) {
            const double mv = (mk + 4 * s)[(unsigned)hi];
            double av[NG], bv[NQ];
#pragma unroll
            for (int g = 0; g < NG; ++g) av[g] = x[g][s] - mv;
#pragma unroll
            for (int q = 0; q < NQ; ++q) bv[q] = q < nq ? (Tk + (size_t)(4 * s) * a.Dbp + 4 * q)[toff] : 0.0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
              if (q < nq) {
#pragma unroll
                for (int g = 0; g < NG; ++g) tile[g][q] = mfma4(av[g], bv[q], tile[g][q]);
              }
            }
          }
        }
      }
      // the cluster's update in one group after its run of MFMAs; r_k and h_k cross to the D layout here,
      // not before the run, where they would be eight more doubles live under it.  Quads past the panel's end are skipped.
      double sv[NQ];
#pragma unroll
      for (int q = 0; q < NQ; ++q) sv[q] = q < nq ? (v.S + (size_t)k * a.Dbp + t0 + 4 * q)[(unsigned)lo2] : 0.0;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const double rD = __shfl(r, g * RG + 4 * blk + hi), hD = __shfl(h, g * RG + 4 * blk + hi);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          if (q < nq) {
            const double d = tile[g][q] - mu[g][q];
            acc[g][q] = fma(rD, fma(d, d, hD * sv[q]), acc[g][q]);
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int64_t ro = wrow0 + g * RG + 4 * blk + hi;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int tcol = t0 + 4 * q + lo2;
        if (ovalid[g] && tcol < a.Db) v.var[(size_t)ro * a.Db + tcol] = acc[g][q];
      }
    }
  }
}

template <int MODE>
hipError_t launch_diag_mode(const PredictDiagLaunch& a, dim3 grid, hipStream_t stream) {
  switch (a.DP) {
    case 16: hipLaunchKernelGGL((predict_diag_kernel<MODE, 16>), grid, dim3(PR_THREADS), 0, stream, a); break;
    case 32: hipLaunchKernelGGL((predict_diag_kernel<MODE, 32>), grid, dim3(PR_THREADS), 0, stream, a); break;
    case 48: hipLaunchKernelGGL((predict_diag_kernel<MODE, 48>), grid, dim3(PR_THREADS), 0, stream, a); break;
    case 64: hipLaunchKernelGGL((predict_diag_kernel<MODE, 64>), grid, dim3(PR_THREADS), 0, stream, a); break;
    default: hipLaunchKernelGGL((predict_diag_kernel<MODE, 0>), grid, dim3(PR_THREADS), 0, stream, a); break;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_predict_rows(const PredictRowsLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  const dim3 grid((unsigned)((rows + PR_THREADS - 1) / PR_THREADS));
  hipLaunchKernelGGL(predict_rows_kernel, grid, dim3(PR_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_predict_diag(const PredictDiagLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0 || a.DP % PRED_RENORM != 0) return rows == 0 ? hipSuccess : hipErrorInvalidValue;
  const dim3 grid((unsigned)((rows + PR_THREADS - 1) / PR_THREADS));
  return a.mode == 0 ? launch_diag_mode<0>(a, grid, stream) : launch_diag_mode<1>(a, grid, stream);
}

hipError_t launch_predict_cond(const PredictCondLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (a.Kp < 1 || a.Da < 1 || a.Db < 1 || a.DP < a.Da || a.Dae < a.Da + 1 || a.Dae % 4 != 0 || a.Dbp < a.Db || a.Dbp % 4 != 0)
    return hipErrorInvalidValue;
  const int64_t per = (int64_t)(PC_THREADS / 64) * PC_WAVE_ROWS;
  hipLaunchKernelGGL(predict_cond_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(PC_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_predict_cond_var(const PredictCondVarLaunch& v, hipStream_t stream) {
  const PredictCondLaunch& a = v.c;
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (a.Kp < 1 || a.Da < 1 || a.Db < 1 || a.DP < a.Da || a.Dae < a.Da + 1 || a.Dae % 4 != 0 || a.Dbp < a.Db ||
      a.Dbp % 4 != 0 || !v.S || !v.g || !v.var)
    return hipErrorInvalidValue;
  const int64_t per = (int64_t)(PC_THREADS / 64) * PC_WAVE_ROWS;
  const dim3 grid((unsigned)((rows + per - 1) / per));
  if (a.Dae <= PC_CHUNK)
    hipLaunchKernelGGL(predict_cond_var_kernel<true>, grid, dim3(PC_THREADS), 0, stream, v);
  else
    hipLaunchKernelGGL(predict_cond_var_kernel<false>, grid, dim3(PC_THREADS), 0, stream, v);
  return hipGetLastError();
}

}  // namespace lck
