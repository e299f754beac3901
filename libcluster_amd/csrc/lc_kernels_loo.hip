// Leave-one-out conditionals: every column of a complete row scored given the row's other columns.
//
// With y = x - m_k, P_k = nu_k iW_k^-1 and v = P_k y, the rank-nb correction of DESIGN 4.15 for the single hole b = {d} is a
// scalar: H = P_k,dd, u = v_d.  All D columns of a row share v, so the whole pass is one GEMM per cluster, V_k = Y_k P_k, on
// the fp64 matrix pipe (v_mfma_f64_4x4x4_4b, the E-step's instruction), and an elementwise epilogue in the accumulator
// layout that folds cluster k into an online log-sum-exp per (row, column).  loo_worst_kernel then names the column a row's
// model likes least.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "lc_device.hpp"
#include "lc_predict.hpp"

namespace lck {
namespace {

// Lane = lo2 + 4 blk + 16 hi (lc_device.hpp).  MFMA block blk of row group g multiplies rows 16 g + 4 blk + {0..3} (A: row
// lo2, contraction column hi of the k-step) with a 4 x 4 piece of P_k (B: contraction column hi, output column lo2, the same
// in all four blocks) into D (row hi, output column lo2).  A lane therefore reads x of row 4 blk + lo2 and owns the results of
// row 4 blk + hi, LOO_NG row groups times LOO_NQ quads of output columns of them.
constexpr int LOO_NG = LOO_WAVE_ROWS / RG, LOO_NQ = LOO_PANEL / 4;
static_assert(RG == 16 && LOO_NG >= 1 && LOO_PANEL % 4 == 0, "one MFMA per row group and quad of output columns");

// P_k reaches the waves through LDS: the block's four waves share the panel, so the 64 contraction rows x LOO_PANEL columns
// of one (cluster, chunk) step are fetched once per block, into registers while the step before is multiplied, and
// written to the other of two buffers behind it -- one barrier per step, and no wave waits on the cache inside its MFMA
// run (at one wave per SIMD nothing else would hide that wait).  m_k travels with the chunk, log(P_dd) / 2 and 1 / P_dd with
// a cluster's first chunk.  The centred operand x - m_k is formed per cluster: no offset sits in P x - P m.  The rows' x
// fragments stay in registers when one chunk covers the contraction (DP <= 64) and are read again per step otherwise.
constexpr int LOO_CHUNK = 64;             // contraction rows per step: 16 k-steps
constexpr int LOO_LDP = LOO_PANEL + 8;    // row stride of a staged chunk: the four rows of a k-step on disjoint banks
constexpr int LOO_NS = LOO_CHUNK / 4;
constexpr int LOO_PF = LOO_CHUNK * LOO_PANEL / LOO_THREADS;  // doubles of a chunk one thread fetches
static_assert(LOO_CHUNK * LOO_PANEL % LOO_THREADS == 0 && LOO_THREADS >= LOO_CHUNK && LOO_THREADS >= 2 * LOO_PANEL, "the fetch is dealt evenly");

template <bool VAR>
__global__ __launch_bounds__(LOO_THREADS, 2) void loo_rows_kernel(LooRowsLaunch a) {
  __shared__ double etab[64];
  __shared__ LogEntry ltab[128];
  __shared__ double Ps[2][LOO_CHUNK * LOO_LDP];
  __shared__ double ms[2][LOO_CHUNK];
  __shared__ double hls[2][LOO_PANEL], ips[2][LOO_PANEL];
  const int tid = threadIdx.x;
  fill_exp_table(etab, tid, LOO_THREADS);
  fill_log_table(ltab, tid, LOO_THREADS);
  const int lane = tid & 63, lo2 = lane & 3, blk = (lane >> 2) & 3, hi = lane >> 4;
  const int64_t rg0 = ((int64_t)blockIdx.x * (LOO_THREADS / 64) + (tid >> 6)) * LOO_NG;
  const int DP = a.DP, p0 = (int)blockIdx.y * LOO_PANEL;
  const int nq = (DP - p0) / 4 < LOO_NQ ? (DP - p0) / 4 : LOO_NQ;
  const int nch = (DP + LOO_CHUNK - 1) / LOO_CHUNK, nsteps = a.Kp * nch;
  // a row group past the end is clamped for reading and never written (its wave keeps step with the block's barriers)
  int64_t xrow[LOO_NG], orow[LOO_NG];
  bool ovalid[LOO_NG];
  int jg[LOO_NG];
#pragma unroll
  for (int g = 0; g < LOO_NG; ++g) {
    const bool in = rg0 + g < a.nrg;
    const int64_t r0 = (in ? rg0 + g : a.nrg - 1) * RG + 4 * blk;
    xrow[g] = r0 + lo2;
    orow[g] = r0 + hi;
    int j = 0;
    ovalid[g] = row_valid(orow[g], a.rginfo, a.nrows, j) && in;
    jg[g] = j;
  }
  // the fetch of step (k, c): LOO_PF doubles of P_k per thread, m_k by the first LOO_CHUNK threads, the two diagonals of the
  // panel by the first 2 LOO_PANEL threads at c = 0
  double fP[LOO_PF], fm = 0.0, fd = 0.0;
  auto fetch = [&](int k, int c) {
#pragma unroll
    for (int i = 0; i < LOO_PF; ++i) {
      const int idx = tid + LOO_THREADS * i, r = c * LOO_CHUNK + idx / LOO_PANEL, col = p0 + idx % LOO_PANEL;
      fP[i] = r < DP && col < DP ? a.P[((size_t)k * DP + r) * DP + col] : 0.0;
    }
    if (tid < LOO_CHUNK) fm = c * LOO_CHUNK + tid < DP ? a.mean[(size_t)k * DP + c * LOO_CHUNK + tid] : 0.0;
    if (c == 0 && tid < 2 * LOO_PANEL) {
      const int col = p0 + (tid % LOO_PANEL);
      fd = col < DP ? (tid < LOO_PANEL ? a.hlogp : a.ipd)[(size_t)k * DP + col] : 0.0;
    }
  };
  auto stage = [&](int k, int c, int b) {
#pragma unroll
    for (int i = 0; i < LOO_PF; ++i) {
      const int idx = tid + LOO_THREADS * i;
      Ps[b][(idx / LOO_PANEL) * LOO_LDP + idx % LOO_PANEL] = fP[i];
    }
    if (tid < LOO_CHUNK) ms[b][tid] = fm;
    if (c == 0 && tid < 2 * LOO_PANEL) (tid < LOO_PANEL ? hls : ips)[k & 1][tid % LOO_PANEL] = fd;
  };
  fetch(0, 0);
  stage(0, 0, 0);
  __syncthreads();  // (the tables and the first step)
  double x[LOO_NG][LOO_NS];
  constexpr double NINF = -std::numeric_limits<double>::infinity();
  // the terms folded so far sum to S exp(mx); Sd and Sq carry the same factor
  double mx[LOO_NG][LOO_NQ], S[LOO_NG][LOO_NQ], Sd[LOO_NG][LOO_NQ], Sq[LOO_NG][VAR ? LOO_NQ : 1];
  double acc[LOO_NG][LOO_NQ], d2[LOO_NG], tk[LOO_NG];
#pragma unroll
  for (int g = 0; g < LOO_NG; ++g) {
    d2[g] = tk[g] = 0.0;
#pragma unroll
    for (int q = 0; q < LOO_NQ; ++q) {
      mx[g][q] = NINF;
      S[g][q] = 0.0;
      Sd[g][q] = 0.0;
      acc[g][q] = 0.0;
      if constexpr (VAR) Sq[g][q] = 0.0;
    }
  }
  int k = 0, c = 0;
  for (int it = 0; it < nsteps; ++it) {
    const int b = it & 1;
    const int kn = c + 1 < nch ? k : k + 1, cn = c + 1 < nch ? c + 1 : 0;
    if (it + 1 < nsteps) fetch(kn, cn);  // (in flight under this step's MFMAs)
    const int ns = (DP - c * LOO_CHUNK) / 4 < LOO_NS ? (DP - c * LOO_CHUNK) / 4 : LOO_NS;
    if (nch > 1 || it == 0) {
#pragma unroll
      for (int g = 0; g < LOO_NG; ++g)
#pragma unroll
        for (int s = 0; s < LOO_NS; ++s) x[g][s] = s < ns ? a.X[(size_t)xrow[g] * DP + c * LOO_CHUNK + 4 * s + hi] : 0.0;
    }
    if (c == 0) {  // what the cluster's epilogue needs from memory, asked for before its MFMAs
#pragma unroll
      for (int g = 0; g < LOO_NG; ++g) {
        d2[g] = -2.0 * a.col[(size_t)k * a.ldq + orow[g]];
        tk[g] = a.ttab[(size_t)jg[g] * a.Kp + k];
#pragma unroll
        for (int q = 0; q < LOO_NQ; ++q) acc[g][q] = 0.0;
      }
    }
    const double* __restrict__ Pb = Ps[b] + hi * LOO_LDP + lo2;
    const double* __restrict__ mb = ms[b] + hi;
#pragma unroll
    for (int s = 0; s < LOO_NS; ++s) {
      if (s < ns) {
        // one k-step: the centred operands and the pieces of P_k first, then the MFMAs in one run
        const double mv = mb[4 * s];
        double av[LOO_NG], bv[LOO_NQ];
#pragma unroll
        for (int g = 0; g < LOO_NG; ++g) av[g] = x[g][s] - mv;
#pragma unroll
        for (int q = 0; q < LOO_NQ; ++q) bv[q] = q < nq ? Pb[4 * s * LOO_LDP + 4 * q] : 0.0;
#pragma unroll
        for (int q = 0; q < LOO_NQ; ++q) {
          if (q < nq) {
#pragma unroll
            for (int g = 0; g < LOO_NG; ++g) acc[g][q] = mfma4(av[g], bv[q], acc[g][q]);
          }
        }
      }
    }
    if (c == nch - 1) {  // epilogue of cluster k, elementwise in the accumulator layout
      const double sk = a.pscale[k], ek = a.pexp[k];
      double gk = 0.0;
      if constexpr (VAR) gk = a.gnu[k];
#pragma unroll
      for (int q = 0; q < LOO_NQ; ++q) {
        if (q < nq) {
          // (a pad column: 0 and 0 -- no division by P_dd = 0 anywhere)
          const double hl = hls[k & 1][4 * q + lo2], ip = ips[k & 1][4 * q + lo2];
#pragma unroll
          for (int g = 0; g < LOO_NG; ++g) {
            const double v = acc[g][q];
            const double vi = v * ip;
            const double z = sk * fmax(fma(-v, vi, d2[g]), 0.0);  // s_k d_a^2, clamped
            const double t = tk[g] - hl - ek * log1p_nonneg(z, ltab);
            const double dl = -vi;  // M_k,d - x_d
            const double df = t - mx[g][q];
            const bool up = df > 0.0;
            const double e = exp_nonpos(up ? -df : df, etab);
            // (up: what was folded so far is scaled down and the new term enters with weight 1)
            const double wo = up ? e : 1.0, wn = up ? 1.0 : e;
            S[g][q] = fma(S[g][q], wo, wn);
            Sd[g][q] = fma(Sd[g][q], wo, wn * dl);
            if constexpr (VAR) Sq[g][q] = fma(Sq[g][q], wo, wn * fma(gk * ip, 1.0 + z, dl * dl));  // Cov_k,d + delta^2
            mx[g][q] = up ? t : mx[g][q];
          }
        }
      }
    }
    if (it + 1 < nsteps) stage(kn, cn, b ^ 1);
    __syncthreads();  // (buffer b is free for step it + 2, buffer b ^ 1 holds step it + 1)
    k = kn;
    c = cn;
  }
#pragma unroll
  for (int g = 0; g < LOO_NG; ++g) {
    if (!ovalid[g]) continue;
    const double lp = a.logp[orow[g]];
#pragma unroll
    for (int q = 0; q < LOO_NQ; ++q) {
      const int col = p0 + 4 * q + lo2;
      if (q < nq && col < a.D) {
        const size_t at = (size_t)orow[g] * DP + col;
        const double rs = rcp_pos(S[g][q]);
        const double dm = Sd[g][q] * rs;  // mean - x_d
        a.cond[at] = lp - (mx[g][q] + log(S[g][q]));
        a.cmean[at] = a.X[at] + dm;
        if constexpr (VAR) a.var[at] = fma(-dm, dm, Sq[g][q] * rs);
      }
    }
  }
}

// LPR lanes read one row of cond: lane sl takes the columns sl, sl + LPR, ... and keeps its smallest value (the lowest
// column on ties; a NaN never wins a comparison), then a fixed butterfly over the row's lanes with the same rule.
template <int LPR>
__global__ __launch_bounds__(LOO_THREADS) void loo_worst_kernel(LooWorstLaunch a) {
  const int lane = threadIdx.x & 63, sg = lane / LPR, sl = lane % LPR;
  const int64_t NP = a.nrg * RG;
  const int64_t row = ((int64_t)blockIdx.x * (LOO_THREADS / 64) + (threadIdx.x >> 6)) * (64 / LPR) + sg;
  int j;
  const bool valid = row < NP && row_valid(row, a.rginfo, a.nrows, j);
  const double* __restrict__ cr = a.cond + (size_t)(valid ? row : 0) * a.DP;
  double best = 0.0;
  int bc = -1;  // (no column so far)
  if (valid)
    for (int c = sl; c < a.D; c += LPR) {
      const double v = cr[c];
      if (v == v && (bc < 0 || v < best)) {
        best = v;
        bc = c;
      }
    }
  for (int d = 1; d < LPR; d <<= 1) {  // (every lane of the wave takes every step)
    const double ov = __shfl_xor(best, d);
    const int oc = __shfl_xor(bc, d);
    if (oc >= 0 && (bc < 0 || ov < best || (ov == best && oc < bc))) {
      best = ov;
      bc = oc;
    }
  }
  if (valid && sl == 0) {
    a.worst[row] = bc;
    a.value[row] = bc >= 0 ? best : std::numeric_limits<double>::quiet_NaN();
  }
}

}  // namespace

hipError_t launch_loo_rows(const LooRowsLaunch& a, hipStream_t stream) {
  if (a.nrg == 0) return hipSuccess;
  if (a.Kp < 1 || a.D < 1 || a.DP < a.D || a.DP % 4 != 0 || a.nrg < 0 || a.ldq < a.nrg * RG || !a.X || !a.col || !a.ttab ||
      !a.pscale || !a.pexp || !a.mean || !a.P || !a.hlogp || !a.ipd || !a.logp || !a.cond || !a.cmean || (a.var && !a.gnu))
    return hipErrorInvalidValue;
  const int64_t per = (int64_t)(LOO_THREADS / 64) * LOO_NG;
  const int64_t gx = (a.nrg + per - 1) / per;
  const int gy = (a.D + LOO_PANEL - 1) / LOO_PANEL;  // (a panel of pad columns only is not launched)
  if (gx > 0x7fffffff || gy > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (a.var)
    hipLaunchKernelGGL(loo_rows_kernel<true>, grid, dim3(LOO_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(loo_rows_kernel<false>, grid, dim3(LOO_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_loo_worst(const LooWorstLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (a.D < 1 || a.DP < a.D || !a.cond || !a.worst || !a.value) return hipErrorInvalidValue;
  const int lpr = a.DP <= 16 ? 16 : a.DP <= 32 ? 32 : 64;
  const int64_t per = (int64_t)(LOO_THREADS / 64) * (64 / lpr);
  const dim3 grid((unsigned)((rows + per - 1) / per));
  switch (lpr) {
    case 16: hipLaunchKernelGGL(loo_worst_kernel<16>, grid, dim3(LOO_THREADS), 0, stream, a); break;
    case 32: hipLaunchKernelGGL(loo_worst_kernel<32>, grid, dim3(LOO_THREADS), 0, stream, a); break;
    default: hipLaunchKernelGGL(loo_worst_kernel<64>, grid, dim3(LOO_THREADS), 0, stream, a); break;
  }
  return hipGetLastError();
}

}  // namespace lck
