// Draws from a learned model: new rows (sample_gw_kernel, sample_diag_kernel) and draws of the unknown
// columns of a conditional prediction (cond_draws_kernel).  Random numbers: lc_philox.hpp; every value is a function of
// (seed, block, row, draw, slot) alone, so any shard of any block can be regenerated on its own.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lc_device.hpp"
#include "lc_philox.hpp"
#include "lc_predict.hpp"

namespace lck {
namespace {

// block and nvalid of a row group, and the counter of its first row
struct RowGroup {
  int grp, nvalid;
  uint64_t gbase;
};
__device__ __forceinline__ RowGroup sample_row_group(const SampleLaunch& a, int64_t row0, int64_t rg) {
  RowGroup o;
  o.grp = 0;
  if (a.rginfo) {
    const int info = a.rginfo[rg];
    o.grp = info >> 5;
    o.nvalid = info & 31;
  } else {
    const int64_t rem = a.nrows - row0;
    o.nvalid = rem >= RG ? RG : (rem > 0 ? (int)rem : 0);
  }
  const int64_t ingrp0 = row0 - (a.goff ? a.goff[o.grp] : 0);
  o.gbase = ((uint64_t)o.grp << 40) + (uint64_t)(a.row_offset + ingrp0);
  return o;
}

// the component of u: the first k whose running sum exceeds u, else the last component with weight
__device__ __forceinline__ int choose_component(const double* __restrict__ cdf, int Kp, int klast, double u) {
  for (int k = 0; k < Kp; ++k)
    if (cdf[k] > u) return k;
  return klast;
}

__device__ __forceinline__ int sample_label(const SampleLaunch& a, const RowGroup& rg, uint64_t g) {
  uint32_t o[4];
  rng_stream(g, a.seed, 0u).block(RNG_TAG_CHOICE, 0u, o);
  return choose_component(a.cdf + (size_t)rg.grp * a.Kp, a.Kp, a.klast[rg.grp], u01(o[0], o[1]));
}

// Gauss-Wishart: 16 rows per block, the normals of the rows staged in LDS, then the triangular product of the row's
// component (synth_kernel's shape) scaled by the row's 1 / sqrt(G).
__global__ void __launch_bounds__(256) sample_gw_kernel(SampleLaunch a) {
  extern __shared__ double eps[];  // [16][DP]
  __shared__ int zlab[RG];
  __shared__ double rs[RG];
  const int DP = a.DP, D = a.D;
  const int64_t row0 = (int64_t)blockIdx.x * RG;
  const RowGroup rg = sample_row_group(a, row0, blockIdx.x);
  const int npair = (D + 1) / 2;
  for (int t = threadIdx.x; t < RG * npair; t += 256) {
    const int r = t / npair, p = t % npair;
    uint32_t o[4];
    rng_stream(rg.gbase + (uint64_t)r, a.seed, 0u).block(RNG_TAG_NORMAL, (uint32_t)p, o);
    double z0, z1;
    box_muller(o, z0, z1);
    eps[r * DP + 2 * p] = z0;
    if (2 * p + 1 < D) eps[r * DP + 2 * p + 1] = z1;
  }
  if (threadIdx.x < RG) {
    const int r = threadIdx.x;
    int z = -1;
    double s = 0.0;
    if (r < rg.nvalid) {
      const uint64_t g = rg.gbase + (uint64_t)r;
      z = sample_label(a, rg, g);
      s = 1.0 / sqrt(gamma_draw(rng_stream(g, a.seed, 0u), a.shape[z]));
    }
    zlab[r] = z;
    rs[r] = s;
    if (row0 + r < a.NP) a.label[row0 + r] = z;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < RG * DP; t += 256) {
    const int r = t / DP, i = t % DP;
    const int64_t row = row0 + r;
    if (row >= a.NP) continue;
    double v = 0.0;
    if (r < rg.nvalid && i < D) {
      const int z = zlab[r];
      const double* __restrict__ Fz = a.fac + ((size_t)z * D + i) * D;
      double acc = 0.0;
      for (int j = 0; j <= i; ++j) acc += Fz[j] * eps[r * DP + j];
      v = a.loc[(size_t)z * D + i] + rs[r] * acc;
    }
    a.X[(size_t)row * DP + i] = v;
  }
}

// The separable families: every entry is a draw of its own (no product, nothing staged): one thread per pair of columns.
template <int MODE>
__global__ void __launch_bounds__(256) sample_diag_kernel(SampleLaunch a) {
  __shared__ int zlab[RG];
  const int DP = a.DP, D = a.D;
  const int64_t row0 = (int64_t)blockIdx.x * RG;
  const RowGroup rg = sample_row_group(a, row0, blockIdx.x);
  if (threadIdx.x < RG) {
    const int r = threadIdx.x;
    const int z = r < rg.nvalid ? sample_label(a, rg, rg.gbase + (uint64_t)r) : -1;
    zlab[r] = z;
    if (row0 + r < a.NP) a.label[row0 + r] = z;
  }
  __syncthreads();
  const int npair = DP / 2;  // (DP is a multiple of 16)
  for (int t = threadIdx.x; t < RG * npair; t += 256) {
    const int r = t / npair, p = t % npair;
    const int64_t row = row0 + r;
    if (row >= a.NP) continue;
    double v[2] = {0.0, 0.0};
    if (r < rg.nvalid && 2 * p < D) {
      const int z = zlab[r];
      const uint64_t g = rg.gbase + (uint64_t)r;
      const double shape = a.shape[z];
      uint32_t o[4];
      if (MODE == 1) {
        rng_stream(g, a.seed, 0u).block(RNG_TAG_NORMAL, (uint32_t)p, o);
        double e[2];
        box_muller(o, e[0], e[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int d = 2 * p + h;
          if (d < D) {
            const double G = gamma_draw(rng_stream(g, a.seed, (uint32_t)d), shape);
            v[h] = a.loc[(size_t)z * D + d] + a.fac[(size_t)z * D + d] * e[h] / sqrt(G);
          }
        }
      } else {
        rng_stream(g, a.seed, (uint32_t)p).block(RNG_TAG_LOMAX, 0u, o);
        const double u[2] = {u01(o[0], o[1]), u01(o[2], o[3])};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int d = 2 * p + h;
          if (d < D) v[h] = a.fac[(size_t)z * D + d] * expm1(-log(u[h]) / shape);
        }
      }
    }
    a.X[(size_t)row * DP + 2 * p] = v[0];
    a.X[(size_t)row * DP + 2 * p + 1] = v[1];
  }
}

constexpr int CD_THREADS = PC_THREADS;
constexpr int CD_BATCH = 8;  // table values loaded side by side: the gathers come from L2, one at a time leaves the wave waiting
constexpr int CD_DRAWS = 4;  // draws of a row whose component and scale are resident between the two parts of the kernel

__global__ void __launch_bounds__(CD_THREADS) cond_draws_kernel(PredictCondDrawsLaunch v) {
  const PredictCondLaunch& a = v.c;
  const int lane = threadIdx.x & 63;
  const int64_t NP = a.nrg * RG;
  const int64_t wrow0 = ((int64_t)blockIdx.x * (CD_THREADS / 64) + (threadIdx.x >> 6)) * PC_WAVE_ROWS;
  if (wrow0 >= NP) return;
  const int m = v.ndraws, Kp = a.Kp, Db = a.Db, Dbp = a.Dbp, Da = a.Da, Dae = a.Dae;
  // first part, lane l = row l of the wave (as predict_cond_kernel scores them): rows past the end and pad rows are
  // clamped for reading, draw nothing and write nothing
  const int64_t myrow = wrow0 + lane, rrow = myrow < NP ? myrow : NP - 1;
  int jm = 0;
  const bool valid = row_valid(rrow, a.rginfo, a.nrows, jm) && myrow < NP;
  if (!valid) jm = 0;
  const uint64_t gm = ((uint64_t)jm << 40) + (uint64_t)(rrow - (v.goff ? v.goff[jm] : 0));
  const double* __restrict__ colm = a.col + rrow;
  const double logpm = a.logp[rrow];
  for (int i0 = 0; i0 < m; i0 += CD_DRAWS) {  // CD_DRAWS draws of every row at a time: their components and scales stay in registers
    int lab[CD_DRAWS];
    double f[CD_DRAWS];
#pragma unroll
    for (int q = 0; q < CD_DRAWS; ++q) {
      const int i = i0 + q;
      lab[q] = 0;
      f[q] = 0.0;
      if (i < m && valid) {
        const RngStream st = rng_stream(gm, v.seed, (uint32_t)i);
        uint32_t o[4];
        st.block(RNG_TAG_CHOICE, 0u, o);
        const double u = u01(o[0], o[1]);
        double cum = 0.0, tl = 0.0;
        int k1 = -1, last = 0;
        for (int k0 = 0; k0 < Kp; k0 += CD_BATCH) {  // CD_BATCH independent loads in flight before the arithmetic on them
          double tv[CD_BATCH];
#pragma unroll
          for (int b = 0; b < CD_BATCH; ++b) tv[b] = k0 + b < Kp ? colm[(size_t)(k0 + b) * a.ldq] : 0.0;
#pragma unroll
          for (int b = 0; b < CD_BATCH; ++b) {
            const int k = k0 + b;
            const double r = k < Kp ? exp(tv[b] - logpm) : 0.0;
            if (r > 0.0) {
              cum += r;
              if (k1 < 0) {  // still looking: remember the last component with weight, take the first whose sum exceeds u
                last = k;
                tl = tv[b];
                if (cum > u) k1 = k;
              }
            }
          }
        }
        if (k1 < 0) k1 = last;
        const double e = a.pexp[k1];
        // 1 + s d^2 back from t = ttab - e log1p(s d^2), as predict_cond_var_kernel recovers it
        const double h = exp((a.ttab[(size_t)jm * Kp + k1] - tl) / e);
        lab[q] = k1;
        f[q] = sqrt(v.cq[k1] * h / gamma_draw(st, e));
        v.label[(size_t)rrow * m + i] = k1;
      }
    }
    // second part, the wave's rows one after the other (everything about the row is wave-uniform): lane t = target column
    const int nq = m - i0 < CD_DRAWS ? m - i0 : CD_DRAWS;
    for (int rr = 0; rr < PC_WAVE_ROWS; ++rr) {
      const int64_t row = wrow0 + rr;
      if (row >= NP) break;
      int j = 0;
      if (!row_valid(row, a.rginfo, a.nrows, j)) continue;  // pad rows write nothing
      const uint64_t g = ((uint64_t)j << 40) + (uint64_t)(row - (v.goff ? v.goff[j] : 0));
      for (int t0 = 0; t0 < Db; t0 += 64) {
        const int tcol = t0 + lane;
        const bool tin = tcol < Dbp;
        const int jend = t0 + 64 < Db ? t0 + 64 : Db;  // (L_k is lower triangular: columns past the panel add nothing)
        int kprev = -1;
        double mk = 0.0;
#pragma unroll
        for (int q = 0; q < CD_DRAWS; ++q) {
          if (q < nq) {
            const int i = i0 + q;
            const int k = __builtin_amdgcn_readlane(lab[q], rr);
            const double fi = readlane_f64(f[q], rr);
            if (k != kprev) {  // the expert M_k(x_a): once for consecutive draws that chose k (a hard row's draws all do)
              kprev = k;
              mk = 0.0;
              for (int c0 = 0; c0 < Dae; c0 += 64) {
                const int c = c0 + lane;
                const double dv = c < Da ? a.X[(size_t)row * a.DP + c] - a.mext[(size_t)k * Dae + c] : (c == Da ? 1.0 : 0.0);
                const int nc = Dae - c0 < 64 ? Dae - c0 : 64;
                const double* __restrict__ Tk = a.T + ((size_t)k * Dae + c0) * Dbp;
                for (int cc = 0; cc < nc; cc += CD_BATCH) {  // (cc <= 56: cc + b stays a lane; dv is 0 past the ones column)
                  double tv[CD_BATCH];
#pragma unroll
                  for (int b = 0; b < CD_BATCH; ++b) tv[b] = tin && cc + b < nc ? Tk[(size_t)(cc + b) * Dbp + tcol] : 0.0;
#pragma unroll
                  for (int b = 0; b < CD_BATCH; ++b) mk = fma(readlane_f64(dv, cc + b), tv[b], mk);
                }
              }
            }
            const RngStream st = rng_stream(g, v.seed, (uint32_t)i);
            double s = 0.0;
            for (int j0 = 0; j0 < jend; j0 += 64) {
              const int jc = j0 + lane;  // lane l: the normal of column j0 + l (the two lanes of a pair form the same block)
              uint32_t o[4];
              st.block(RNG_TAG_NORMAL, (uint32_t)(jc >> 1), o);
              double z0, z1;
              box_muller(o, z0, z1);
              const double z = jc < Db ? ((jc & 1) ? z1 : z0) : 0.0;
              const int nj = jend - j0 < 64 ? jend - j0 : 64;
              const double* __restrict__ Lk = v.Lt + ((size_t)k * Dbp + j0) * Dbp;
              for (int jj = 0; jj < nj; jj += CD_BATCH) {
                double lv[CD_BATCH];
#pragma unroll
                for (int b = 0; b < CD_BATCH; ++b) lv[b] = tin && jj + b < nj ? Lk[(size_t)(jj + b) * Dbp + tcol] : 0.0;
#pragma unroll
                for (int b = 0; b < CD_BATCH; ++b) s = fma(readlane_f64(z, (jj + b) & 63), lv[b], s);
              }
            }
            if (tcol < Db) v.draws[((size_t)row * m + i) * Db + tcol] = mk + fi * s;
          }
        }
      }
    }
  }
}

}  // namespace

hipError_t launch_sample(const SampleLaunch& a, hipStream_t stream) {
  if (a.NP <= 0) return hipSuccess;
  if (a.Kp < 1 || a.D < 1 || a.DP < a.D || a.DP % 2 != 0 || !a.X || !a.label || !a.cdf || !a.klast || !a.fac || !a.shape ||
      a.mode < 0 || a.mode > 2 || (a.mode != 2 && !a.loc))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.NP + RG - 1) / RG));
  if (a.mode == 0) {
    const size_t shmem = (size_t)RG * a.DP * sizeof(double);
    static LdsGrant grant;  // wide rows (DP > 512): more dynamic LDS than a kernel gets without asking
    if (hipError_t e = grant_dynamic_lds(reinterpret_cast<const void*>(sample_gw_kernel), shmem, grant); e != hipSuccess) return e;
    hipLaunchKernelGGL(sample_gw_kernel, grid, dim3(256), shmem, stream, a);
  } else if (a.mode == 1) {
    hipLaunchKernelGGL(sample_diag_kernel<1>, grid, dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(sample_diag_kernel<2>, grid, dim3(256), 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_predict_cond_draws(const PredictCondDrawsLaunch& v, hipStream_t stream) {
  const PredictCondLaunch& a = v.c;
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (a.Kp < 1 || a.Da < 1 || a.Db < 1 || a.DP < a.Da || a.Dae < a.Da + 1 || a.Dae % 4 != 0 || a.Dbp < a.Db ||
      a.Dbp % 4 != 0 || !v.Lt || !v.cq || !v.draws || !v.label || v.ndraws < 1 || v.ndraws > DRAWS_MAX)
    return hipErrorInvalidValue;
  const int64_t per = (int64_t)(CD_THREADS / 64) * PC_WAVE_ROWS;
  hipLaunchKernelGGL(cond_draws_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(CD_THREADS), 0, stream, v);
  return hipGetLastError();
}

}  // namespace lck
