// Rows whose unknown columns differ from row to row: a NaN marks a hole, every row has its own set.
//
// holes_scan_kernel finds the holes in one read of X, holes_fill_kernel puts a finite value into them so that the raw
// E-step (estep_kernel / estep_wide_kernel, as they are) can run at full width, and predict_holes_kernel takes the holes
// out of the distances again -- per (row, cluster) a rank-nb correction with the cluster's precision matrix
// P_k = nu_k iW_k^-1 -- and writes the mixture of the clusters' linear experts into the holes.  Rows without holes take
// predict_rows_kernel's predictive loop.
// holes_draws_kernel then draws the unknown values: per draw a component by its responsibility and a
// value from that component's conditional Student-t, on the factor of (P_k)_bb that predict_holes_kernel forms as well.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>
#include <type_traits>

#include "lc_device.hpp"
#include "lc_philox.hpp"
#include "lc_predict.hpp"

namespace lck {
namespace {

constexpr int HS_THREADS = 256;
constexpr int HS_STEPS = 64;  // rows one sub-group of a wave scans, one after the other
constexpr int PH_COLS = 8;    // predict_holes_kernel, rows without holes: columns loaded per batch (predict_rows_kernel's)

// LPR lanes read one row: lane sl of a sub-group takes the columns sl, sl + LPR, ... -- consecutive lanes read consecutive
// doubles.  A ballot per column step ranks the NaNs of a row in ascending column order.
template <int LPR>
__global__ __launch_bounds__(HS_THREADS) void holes_scan_kernel(HolesScanLaunch a) {
  constexpr int SUB = 64 / LPR;
  const int lane = threadIdx.x & 63, sg = lane / LPR, sl = lane % LPR;
  const int64_t NP = a.nrg * RG;
  const int64_t wave = (int64_t)blockIdx.x * (HS_THREADS / 64) + (threadIdx.x >> 6);
  const int64_t row0 = wave * (HS_STEPS * SUB);
  int nholed = 0, cmax = 0;
  unsigned long long bad = ~0ull;
  for (int s = 0; s < HS_STEPS; ++s) {
    if (row0 + (int64_t)s * SUB >= NP) break;  // (the same in every lane)
    const int64_t row = row0 + (int64_t)s * SUB + sg;
    int j;
    const bool valid = row < NP && row_valid(row, a.rginfo, a.nrows, j);
    const double* __restrict__ xr = a.X + (size_t)(valid ? row : 0) * a.DP;
    int cnt = 0;
    for (int c0 = 0; c0 < a.D; c0 += LPR) {  // (every lane of the wave takes every step: the ballot needs them all)
      const int c = c0 + sl;
      const bool hole = valid && c < a.D && isnan(xr[c]);
      const unsigned long long all = __ballot(hole);
      unsigned long long mine = all;
      if constexpr (LPR < 64) mine = (all >> (sg * LPR)) & ((1ull << LPR) - 1);
      const int rank = cnt + __popcll(mine & ((1ull << sl) - 1));
      if (hole && rank < HOLES_MAX) a.cols[(size_t)row * HOLES_MAX + rank] = c;
      cnt += __popcll(mine);
    }
    if (valid) {
      if (sl < HOLES_MAX && sl >= cnt) a.cols[(size_t)row * HOLES_MAX + sl] = -1;
      if (sl == 0) {
        a.count[row] = cnt;
        nholed += cnt > 0 ? 1 : 0;
        cmax = cnt > cmax ? cnt : cmax;
        if ((cnt > HOLES_MAX || cnt >= a.D) && (unsigned long long)row < bad) bad = (unsigned long long)row;
      }
    }
  }
  // one atomic of each kind per block at the most (every block hammering the same three words cost 13 ms at 10M rows
  // with holes): the block's lanes meet in LDS first.  Integer atomics: the same three values whatever the order.
  __shared__ unsigned int blk_holed, blk_max;
  __shared__ unsigned long long blk_bad;
  if (threadIdx.x == 0) {
    blk_holed = 0;
    blk_max = 0;
    blk_bad = ~0ull;
  }
  __syncthreads();
  if (sl == 0) {
    if (nholed) atomicAdd(&blk_holed, (unsigned int)nholed);
    if (cmax) atomicMax(&blk_max, (unsigned int)cmax);
    if (bad != ~0ull) atomicMin(&blk_bad, bad);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (blk_holed) atomicAdd(a.out, (unsigned long long)blk_holed);
    if (blk_max) atomicMax(a.out + 1, (unsigned long long)blk_max);
    if (blk_bad != ~0ull) atomicMin(a.out + 2, blk_bad);
  }
}

__global__ __launch_bounds__(HS_THREADS) void holes_fill_kernel(HolesFillLaunch a) {
  const int64_t row = (int64_t)blockIdx.x * HS_THREADS + threadIdx.x;
  int j;
  if (row >= a.nrg * RG || !row_valid(row, a.rginfo, a.nrows, j)) return;
  const int cnt = a.count[row];
  if (cnt == 0) return;
  double* __restrict__ xr = a.X + (size_t)row * a.DP;
  const int* __restrict__ cr = a.cols + (size_t)row * HOLES_MAX;
#pragma unroll
  for (int i = 0; i < HOLES_MAX; ++i) {
    if (i < cnt) {
      const int c = cr[i];
      xr[c] = a.fill[c];
    }
  }
}

// The fold of predict_holes_kernel's u loop (described there) for the variance sums: eight sums over the wave in ten
// exchanges, a fixed tree.  Lane l ends with the sum of acc[i], i = bit5 + 2 bit4 + 4 bit3 of l.  (The u loop keeps its
// own copy of these lines: with a call to this function there the mean-only instance takes 236 registers, not 222.)
static_assert(HOLES_MAX == 8, "the fold below halves eight values three times");
__device__ __forceinline__ double fold8(const double (&acc)[HOLES_MAX], int lane) {
  const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
  double v4[4], v2[2];
#pragma unroll
  for (int p = 0; p < 4; ++p)
    v4[p] = (b5 ? acc[2 * p + 1] : acc[2 * p]) + __shfl_xor(b5 ? acc[2 * p] : acc[2 * p + 1], 32);
#pragma unroll
  for (int p = 0; p < 2; ++p)
    v2[p] = (b4 ? v4[2 * p + 1] : v4[2 * p]) + __shfl_xor(b4 ? v4[2 * p] : v4[2 * p + 1], 16);
  double v1 = (b3 ? v2[1] : v2[0]) + __shfl_xor(b3 ? v2[0] : v2[1], 8);
  v1 += __shfl_xor(v1, 4);
  v1 += __shfl_xor(v1, 2);
  v1 += __shfl_xor(v1, 1);
  return v1;
}

// predict_holes_kernel<false> is the kernel of DESIGN 4.15 as it was (222 registers, two waves per SIMD, no scratch):
// every addition sits behind if constexpr.  <true> also forms the variance of the filled values; it is
// held to two waves per SIMD, which it reaches without scratch (248 registers) with the fill values in scalar registers.
__device__ __forceinline__ const PredictHolesLaunch& holes_args(const PredictHolesLaunch& x) { return x; }
__device__ __forceinline__ const PredictHolesLaunch& holes_args(const PredictHolesVarLaunch& x) { return x.h; }
__device__ __forceinline__ const PredictHolesLaunch& holes_args(const PredictHolesKeepLaunch& x) { return x.h; }
// <false, true> is <false> with one store more: the lane that owns cluster k keeps t_k of a row with holes
// where it read the raw column, for holes_draws_kernel.
template <bool VAR, bool KEEP = false>
__global__ __launch_bounds__(PH_THREADS, VAR ? 2 : 0) void predict_holes_kernel(
    std::conditional_t<KEEP, PredictHolesKeepLaunch, std::conditional_t<VAR, PredictHolesVarLaunch, PredictHolesLaunch>> aa) {
  static_assert(!(VAR && KEEP), "the draws call forms no variance");
  const PredictHolesLaunch& a = holes_args(aa);
  [[maybe_unused]] const double* __restrict__ gnu = nullptr;
  [[maybe_unused]] double* __restrict__ var = nullptr;
  if constexpr (VAR) {
    gnu = aa.gnu;
    var = aa.var;
  }
  __shared__ double etab[64];
  __shared__ LogEntry ltab[128];
  __shared__ double uslab[PH_THREADS / 64][64][HOLES_MAX];  // per wave: u of up to 64 clusters (16 KB in all)
  fill_exp_table(etab, threadIdx.x, PH_THREADS);
  fill_log_table(ltab, threadIdx.x, PH_THREADS);
  __syncthreads();  // (the only barrier: from here on the waves do not meet)
  double(*uw)[HOLES_MAX] = uslab[threadIdx.x >> 6];
  constexpr int NH = HOLES_MAX + 1;
  constexpr double NINF = -std::numeric_limits<double>::infinity();
  const int lane = threadIdx.x & 63;
  const int64_t NP = a.nrg * RG;
  const int64_t row = (int64_t)blockIdx.x * PH_THREADS + threadIdx.x, wrow0 = row - lane;
  if (wrow0 >= NP) return;  // (whole waves only: the reductions below need every lane)
  int j = 0;
  const bool valid = row < NP && row_valid(row, a.rginfo, a.nrows, j);
  const int cnt = valid ? a.count[row] : 0;
  const int DP = a.DP, Kp = a.Kp;

  if (valid && cnt == 0) {  // log p(x) as predict_rows_kernel forms it, with the tables of nb = 0
    const double* __restrict__ pt = a.ttab + (size_t)j * NH * Kp;
    const double* __restrict__ col = a.col + row;
    double mp = NINF, sp = 0.0;
    for (int k0 = 0; k0 < Kp; k0 += PH_COLS) {
      double r[PH_COLS];
#pragma unroll
      for (int i = 0; i < PH_COLS; ++i) r[i] = k0 + i < Kp ? col[(size_t)(k0 + i) * a.ldq] : 0.0;
#pragma unroll
      for (int i = 0; i < PH_COLS; ++i) {
        const int k = k0 + i;
        if (k < Kp) lse_push(pt[k] - a.pexp[k] * log1p_nonneg(a.pscale[k] * (-2.0 * r[i]), ltab), mp, sp, etab);
      }
    }
    a.logp[row] = mp + log(sp);
    if constexpr (VAR) {
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i) var[(size_t)row * HOLES_MAX + i] = 0.0;
    }
  }

  // The rows with holes of this wave, one after the other.  Everything a row decides -- its position, nb, the hole
  // columns -- is the same in every lane, and every lane takes every step.
  unsigned long long todo = __ballot(valid && cnt > 0);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t hr = wrow0 + src;
    const int nb = __builtin_amdgcn_readfirstlane(__shfl(cnt, src));
    const int jh = __builtin_amdgcn_readfirstlane(__shfl(j, src));
    double* __restrict__ xr = a.X + (size_t)hr * DP;
    int c[HOLES_MAX];
    double xb[HOLES_MAX];  // the filled values
#pragma unroll
    for (int i = 0; i < HOLES_MAX; ++i) {
      c[i] = i < nb ? __builtin_amdgcn_readfirstlane(a.cols[(size_t)hr * HOLES_MAX + i]) : 0;
      xb[i] = i < nb ? xr[c[i]] : 0.0;
      if constexpr (VAR)  // (the same value in every lane: into scalar registers, the vector ones are the tight spot)
        xb[i] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(xb[i])),
                                 __builtin_amdgcn_readfirstlane(__double2loint(xb[i])));
    }
    const double* __restrict__ tt = a.ttab + ((size_t)jh * NH + nb) * Kp;
    const double* __restrict__ pe = a.pexp + (size_t)nb * Kp;
    // online over chunks of 64 clusters: the terms so far sum to ssum exp(mrun), their experts to esum[i] exp(mrun)
    double mrun = NINF, ssum = 0.0, esum[HOLES_MAX];
#pragma unroll
    for (int i = 0; i < HOLES_MAX; ++i) esum[i] = 0.0;
    // VAR: lane l carries ONE more running sum, that of the hole fold8 leaves in l: sum_k e_k (Cov_k,ii + w_k,i^2)
    [[maybe_unused]] double vsum = 0.0;
    [[maybe_unused]] const double* __restrict__ gv = VAR ? gnu + (size_t)nb * Kp : nullptr;
    for (int k0 = 0; k0 < Kp; k0 += 64) {
      const int kc = Kp - k0 < 64 ? Kp - k0 : 64;
      // u = (P_k y)_b: the lanes own the columns of row b_i of P_k (a coalesced read), a sum over the wave per (i, k); the
      // u of cluster k0 + kk waits in row kk of the wave's LDS slab for the lane that owns the cluster
      for (int kk = 0; kk < kc; ++kk) {
        const double* __restrict__ Pk = a.P + (size_t)(k0 + kk) * DP * DP;
        const double* __restrict__ mk = a.mean + (size_t)(k0 + kk) * DP;
        double acc[HOLES_MAX];
#pragma unroll
        for (int i = 0; i < HOLES_MAX; ++i) acc[i] = 0.0;
        for (int d = lane; d < DP; d += 64) {
          const double y = xr[d] - mk[d];  // (pad columns: 0 - 0)
#pragma unroll
          for (int i = 0; i < HOLES_MAX; ++i)
            if (i < nb) acc[i] = fma(Pk[(size_t)c[i] * DP + d], y, acc[i]);
        }
        const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
        double v4[4], v2[2];
#pragma unroll
        for (int p = 0; p < 4; ++p)
          v4[p] = (b5 ? acc[2 * p + 1] : acc[2 * p]) + __shfl_xor(b5 ? acc[2 * p] : acc[2 * p + 1], 32);
#pragma unroll
        for (int p = 0; p < 2; ++p)
          v2[p] = (b4 ? v4[2 * p + 1] : v4[2 * p]) + __shfl_xor(b4 ? v4[2 * p] : v4[2 * p + 1], 16);
        double v1 = (b3 ? v2[1] : v2[0]) + __shfl_xor(b3 ? v2[0] : v2[1], 8);
        v1 += __shfl_xor(v1, 4);
        v1 += __shfl_xor(v1, 2);
        v1 += __shfl_xor(v1, 1);
        if ((lane & 7) == 0) uw[kk][((lane >> 5) & 1) | ((lane >> 3) & 2) | ((lane >> 1) & 4)] = v1;
      }
      __builtin_amdgcn_wave_barrier();  // (the wave's own LDS writes above, its reads below: issued in this order)
      // the small solve: lane kk owns cluster k0 + kk (the lanes past kc redo the chunk's first cluster and count for nothing)
      const bool on = lane < kc;
      const int k = on ? k0 + lane : k0;
      const double* __restrict__ Pk = a.P + (size_t)k * DP * DP;
      double u[HOLES_MAX];
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i) u[i] = on ? uw[lane][i] : 0.0;
      __builtin_amdgcn_wave_barrier();
      // H = P_bb padded with the identity, factored in place: H = L L^T
      double L[HOLES_MAX][HOLES_MAX];
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i)
#pragma unroll
        for (int jj = 0; jj <= i; ++jj) L[i][jj] = i < nb ? Pk[(size_t)c[i] * DP + c[jj]] : i == jj ? 1.0 : 0.0;
      double inv[HOLES_MAX], prod = 1.0;
#pragma unroll
      for (int jj = 0; jj < HOLES_MAX; ++jj) {
        inv[jj] = 1.0;
        if (jj < nb) {
          double sjj = L[jj][jj];
#pragma unroll
          for (int q = 0; q < jj; ++q) sjj = fma(-L[jj][q], L[jj][q], sjj);
          const double ljj = sqrt(sjj);
          inv[jj] = 1.0 / ljj;
          prod *= ljj;
#pragma unroll
          for (int i = jj + 1; i < HOLES_MAX; ++i) {
            double sij = L[i][jj];
#pragma unroll
            for (int q = 0; q < jj; ++q) sij = fma(-L[i][q], L[jj][q], sij);
            L[i][jj] = sij * inv[jj];
          }
        }
      }
      // L z = u, then L^T w = z: u^T H^-1 u = z^T z and H^-1 u = w (in place in u)
      double quad = 0.0;
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i) {
        double v = u[i];
#pragma unroll
        for (int q = 0; q < i; ++q) v = fma(-L[i][q], u[q], v);
        u[i] = v * inv[i];
        quad = fma(u[i], u[i], quad);
      }
#pragma unroll
      for (int i = HOLES_MAX - 1; i >= 0; --i) {
        double v = u[i];
#pragma unroll
        for (int q = i + 1; q < HOLES_MAX; ++q) v = fma(-L[q][i], u[q], v);
        u[i] = v * inv[i];
      }
      // VAR: (H^-1)_ii = ||L^-1 e_i||^2, one forward solve per hole on eight temporaries (L's last use); the identity
      // padding adds nothing, so the rows j >= nb are skipped
      [[maybe_unused]] double hd[HOLES_MAX];
      if constexpr (VAR) {
#pragma unroll
        for (int i = 0; i < HOLES_MAX; ++i) {
          hd[i] = 0.0;
          if (i < nb) {
            double x[HOLES_MAX];
            x[i] = inv[i];
            double s2 = x[i] * x[i];
#pragma unroll
            for (int r = i + 1; r < HOLES_MAX; ++r) {
              if (r < nb) {
                double v = 0.0;
#pragma unroll
                for (int q = i; q < r; ++q) v = fma(-L[r][q], x[q], v);
                x[r] = v * inv[r];
                s2 = fma(x[r], x[r], s2);
              }
            }
            hd[i] = s2;
          }
        }
      }
      const double d2full = -2.0 * a.col[(size_t)k * a.ldq + hr];
      const double d2a = fmax(d2full - quad, 0.0);
      const double t = on ? tt[k] - log(prod) - pe[k] * log1p_nonneg(a.pscale[k] * d2a, ltab) : NINF;
      if constexpr (KEEP) {
        if (on) aa.tcol[(size_t)k * a.ldq + hr] = t;
      }
      // fold the chunk into the running sums
      const double mnew = fmax(mrun, wave_max(t));
      const double f = exp_nonpos(mrun - mnew, etab), e = exp_nonpos(t - mnew, etab);
      ssum = fma(ssum, f, wave_sum(e));
      // VAR: Cov_k,ii = g_k(nb) nu_k (1 + s_k d_a^2) (H^-1)_ii, and the second moment of the expert about the fill value;
      // d_a^2 is multiplied, never exponentiated: a far row stays finite
      [[maybe_unused]] double hk = 0.0, vacc[HOLES_MAX];
      if constexpr (VAR) hk = gv[k] * fma(a.pscale[k], d2a, 1.0);
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i) {
        if constexpr (VAR) vacc[i] = 0.0;
        if (i < nb) {
          const double ex = xb[i] - u[i];  // the expert
          esum[i] = fma(esum[i], f, wave_sum(e * ex));
          // w_i is taken back out of the expert, the ONE value both instances form: u keeps the uses it has in the
          // mean-only instance, the compiler contracts the subtraction above alike in both, and X gets the same bits
          if constexpr (VAR) {
            const double wd = xb[i] - ex;
            vacc[i] = e * fma(hk, hd[i], wd * wd);
          }
        }
      }
      if constexpr (VAR) vsum = fma(vsum, f, fold8(vacc, lane));
      mrun = mnew;
    }
    if constexpr (VAR) {
      // lane 0 collects the eight sums from the lanes that hold them (lane 32 holds hole 1, 16 hole 2, 48 hole 3, 8 hole 4, ...)
      double vs[HOLES_MAX];
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i) vs[i] = __shfl(vsum, ((i & 1) << 5) | ((i & 2) << 3) | ((i & 4) << 1));
      if (lane == 0) {
        // var_i = sum_k r_k (Cov_k,ii + w_k,i^2) - (sum_k r_k w_k,i)^2 with sum_k r_k w_k,i = fill_i - mean_i: centred
        // on the mean through deviations from the fill value, which lies among the data
#pragma unroll
        for (int i = 0; i < HOLES_MAX; ++i) {
          const double dw = xb[i] - esum[i] / ssum;
          var[(size_t)hr * HOLES_MAX + i] = i < nb ? fma(-dw, dw, vs[i] / ssum) : 0.0;
        }
      }
    }
    if (lane == 0) {
      a.logp[hr] = mrun + log(ssum);
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i)
        if (i < nb) xr[c[i]] = esum[i] / ssum;
    }
  }
}

// Draws of the unknown values of rows with holes (the arithmetic is in lc_predict.hpp).  The rows with holes
// of a wave one after the other, as in predict_holes_kernel: nb, the hole columns and the block are wave-uniform.
__global__ __launch_bounds__(PH_THREADS) void holes_draws_kernel(HolesDrawsLaunch v) {
  const PredictHolesLaunch& a = v.h;
  constexpr int NH = HOLES_MAX + 1;
  const int lane = threadIdx.x & 63;
  const int64_t NP = a.nrg * RG;
  const int64_t row = (int64_t)blockIdx.x * PH_THREADS + threadIdx.x, wrow0 = row - lane;
  if (wrow0 >= NP) return;  // (whole waves only: the ballots and the fold below need every lane)
  int j = 0;
  const bool valid = row < NP && row_valid(row, a.rginfo, a.nrows, j);
  const int cnt = valid ? a.count[row] : 0;
  const int DP = a.DP, Kp = a.Kp, m = v.ndraws;
  const bool mine = lane < m;  // lane i = draw i
  unsigned long long todo = __ballot(valid && cnt > 0);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t hr = wrow0 + src;
    const int nb = __builtin_amdgcn_readfirstlane(__shfl(cnt, src));
    const int jh = __builtin_amdgcn_readfirstlane(__shfl(j, src));
    const double* __restrict__ xr = a.X + (size_t)hr * DP;  // the mean-completed row
    int c[HOLES_MAX];
    double xb[HOLES_MAX];
#pragma unroll
    for (int i = 0; i < HOLES_MAX; ++i) {
      c[i] = i < nb ? __builtin_amdgcn_readfirstlane(a.cols[(size_t)hr * HOLES_MAX + i]) : 0;
      xb[i] = i < nb ? xr[c[i]] : 0.0;
    }
    const double* __restrict__ tt = a.ttab + ((size_t)jh * NH + nb) * Kp;
    const double* __restrict__ pe = a.pexp + (size_t)nb * Kp;
    const double* __restrict__ tc = a.col + hr;  // t_k at tc[k * ldq]
    const double logp = a.logp[hr];
    const uint64_t g = ((uint64_t)jh << 40) + (uint64_t)(hr - (v.goff ? v.goff[jh] : 0));
    const RngStream st = rng_stream(g, v.seed, (uint32_t)lane);
    uint32_t o[4];
    // the component: lane kk forms r of cluster k0 + kk once, every lane walks the running sum (the same in all) against its own u
    st.block(RNG_TAG_CHOICE, 0u, o);
    const double uu = u01(o[0], o[1]);
    double cum = 0.0;
    int k1 = -1, last = 0;
    for (int k0 = 0; k0 < Kp; k0 += 64) {
      const int kc = Kp - k0 < 64 ? Kp - k0 : 64;
      const double rl = lane < kc ? exp(tc[(size_t)(k0 + lane) * a.ldq] - logp) : 0.0;
      for (int kk = 0; kk < kc; ++kk) {
        const double r = readlane_f64(rl, kk);
        if (r > 0.0) {
          cum += r;
          if (k1 < 0) {  // still looking: remember the last component with weight, take the first whose sum exceeds u
            last = k0 + kk;
            if (cum > uu) k1 = k0 + kk;
          }
        }
      }
    }
    if (k1 < 0) k1 = last;
    const double G = mine ? gamma_draw(st, pe[k1]) : 1.0;
    double z[HOLES_MAX];
#pragma unroll
    for (int p = 0; p < HOLES_MAX / 2; ++p) {
      z[2 * p] = 0.0;
      z[2 * p + 1] = 0.0;
      if (2 * p < nb) {
        st.block(RNG_TAG_NORMAL, (uint32_t)p, o);
        box_muller(o, z[2 * p], z[2 * p + 1]);
      }
    }
    if (mine) v.label[(size_t)hr * m + lane] = k1;
    // the distinct components the draws chose, one after the other (a hard row has one)
    unsigned long long rem = __ballot(mine);
    while (rem) {
      const int k = __builtin_amdgcn_readlane(k1, __ffsll((long long)rem) - 1);
      const bool sel = mine && k1 == k;
      rem &= ~__ballot(sel);
      const double* __restrict__ Pk = a.P + (size_t)k * DP * DP;
      const double* __restrict__ mk = a.mean + (size_t)k * DP;
      // u = (P_k y)_b: predict_holes_kernel's reads and fold, then the eight sums into every lane
      double acc[HOLES_MAX];
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i) acc[i] = 0.0;
      for (int d = lane; d < DP; d += 64) {
        const double y = xr[d] - mk[d];  // (pad columns: 0 - 0)
#pragma unroll
        for (int i = 0; i < HOLES_MAX; ++i)
          if (i < nb) acc[i] = fma(Pk[(size_t)c[i] * DP + d], y, acc[i]);
      }
      const double us = fold8(acc, lane);
      double u[HOLES_MAX];
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i) u[i] = readlane_f64(us, ((i & 1) << 5) | ((i & 2) << 3) | ((i & 4) << 1));
      // H = P_bb padded with the identity, H = L L^T (the same in every lane: a SIMD does it once for all of them)
      double L[HOLES_MAX][HOLES_MAX];
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i)
#pragma unroll
        for (int jj = 0; jj <= i; ++jj) L[i][jj] = i < nb ? Pk[(size_t)c[i] * DP + c[jj]] : i == jj ? 1.0 : 0.0;
      double inv[HOLES_MAX], prod = 1.0;
#pragma unroll
      for (int jj = 0; jj < HOLES_MAX; ++jj) {
        inv[jj] = 1.0;
        if (jj < nb) {
          double sjj = L[jj][jj];
#pragma unroll
          for (int q = 0; q < jj; ++q) sjj = fma(-L[jj][q], L[jj][q], sjj);
          const double ljj = sqrt(sjj);
          inv[jj] = 1.0 / ljj;
          prod *= ljj;
#pragma unroll
          for (int i = jj + 1; i < HOLES_MAX; ++i) {
            double sij = L[i][jj];
#pragma unroll
            for (int q = 0; q < jj; ++q) sij = fma(-L[i][q], L[jj][q], sij);
            L[i][jj] = sij * inv[jj];
          }
        }
      }
      // w = H^-1 u (in place in u): M_k = x_b - w
#pragma unroll
      for (int i = 0; i < HOLES_MAX; ++i) {
        double s = u[i];
#pragma unroll
        for (int q = 0; q < i; ++q) s = fma(-L[i][q], u[q], s);
        u[i] = s * inv[i];
      }
#pragma unroll
      for (int i = HOLES_MAX - 1; i >= 0; --i) {
        double s = u[i];
#pragma unroll
        for (int q = i + 1; q < HOLES_MAX; ++q) s = fma(-L[q][i], u[q], s);
        u[i] = s * inv[i];
      }
      // 1 + s_k d_a^2 back from t_k = ttab - log prod L_ii - e_k log1p(s_k d_a^2), as cond_draws_kernel recovers it
      const double h = fmax(exp((tt[k] - log(prod) - tc[(size_t)k * a.ldq]) / pe[k]), 1.0);
      const double f = sqrt(v.cqnu[k] * h / G);
      // L^T x = z with the lane's own z: sqrt(nu) L^-T is a factor of S_k = nu H^-1 (nu is in cqnu)
      double x[HOLES_MAX];
#pragma unroll
      for (int i = HOLES_MAX - 1; i >= 0; --i) {
        double s = z[i];
#pragma unroll
        for (int q = i + 1; q < HOLES_MAX; ++q) s = fma(-L[q][i], x[q], s);
        x[i] = s * inv[i];
      }
      if (sel) {
        double* __restrict__ dr = v.draws + ((size_t)hr * m + lane) * HOLES_MAX;
#pragma unroll
        for (int i = 0; i < HOLES_MAX; ++i)
          if (i < nb) dr[i] = fma(f, x[i], xb[i] - u[i]);
      }
    }
  }
}

}  // namespace

hipError_t launch_predict_holes_keep(const PredictHolesKeepLaunch& a, hipStream_t stream) {
  const int64_t rows = a.h.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (a.h.Kp < 1 || a.h.DP < 1 || !a.tcol || a.tcol != a.h.col) return hipErrorInvalidValue;
  hipLaunchKernelGGL((predict_holes_kernel<false, true>), dim3((unsigned)((rows + PH_THREADS - 1) / PH_THREADS)), dim3(PH_THREADS), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_holes_draws(const HolesDrawsLaunch& v, hipStream_t stream) {
  const int64_t rows = v.h.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (v.h.Kp < 1 || v.h.DP < 1 || !v.cqnu || !v.draws || !v.label || v.ndraws < 1 || v.ndraws > DRAWS_MAX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(holes_draws_kernel, dim3((unsigned)((rows + PH_THREADS - 1) / PH_THREADS)), dim3(PH_THREADS), 0, stream, v);
  return hipGetLastError();
}

hipError_t launch_holes_scan(const HolesScanLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (a.D < 1 || a.DP < a.D) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.out, 0, 2 * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.out + 2, 0xff, sizeof(unsigned long long), stream);  // (~0: no offending row)
  if (e != hipSuccess) return e;
  const int lpr = a.DP <= 16 ? 16 : a.DP <= 32 ? 32 : 64;
  const int64_t per = (int64_t)(HS_THREADS / 64) * HS_STEPS * (64 / lpr);
  const dim3 grid((unsigned)((rows + per - 1) / per));
  switch (lpr) {
    case 16: hipLaunchKernelGGL(holes_scan_kernel<16>, grid, dim3(HS_THREADS), 0, stream, a); break;
    case 32: hipLaunchKernelGGL(holes_scan_kernel<32>, grid, dim3(HS_THREADS), 0, stream, a); break;
    default: hipLaunchKernelGGL(holes_scan_kernel<64>, grid, dim3(HS_THREADS), 0, stream, a); break;
  }
  return hipGetLastError();
}

hipError_t launch_holes_fill(const HolesFillLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(holes_fill_kernel, dim3((unsigned)((rows + HS_THREADS - 1) / HS_THREADS)), dim3(HS_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_predict_holes(const PredictHolesLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (a.Kp < 1 || a.DP < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(predict_holes_kernel<false>, dim3((unsigned)((rows + PH_THREADS - 1) / PH_THREADS)), dim3(PH_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_predict_holes_var(const PredictHolesVarLaunch& a, hipStream_t stream) {
  const int64_t rows = a.h.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (a.h.Kp < 1 || a.h.DP < 1 || !a.gnu || !a.var) return hipErrorInvalidValue;
  hipLaunchKernelGGL(predict_holes_kernel<true>, dim3((unsigned)((rows + PH_THREADS - 1) / PH_THREADS)), dim3(PH_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lck
