// Sufficient statistics of the Gauss-Wishart clusters: updateSS (src/cluster.cpp:53-82) -> GaussWish::addobs (src/distributions.cpp:301-313)
// (one translation unit per kernel family; the file header of lc_kernels_estep.hip maps kernels to the reference)
#include "lc_device.hpp"

// widths at which the feature-GEMM form of the statistics pass is the default for more than 16 clusters (measured:
// tools/ssfeat_check.py; LC_SS_FEAT=2 selects it wherever it exists, 0 nowhere)
#ifndef LC_SS_FEAT_MINK_ACTIVE
#define LC_SS_FEAT_MINK_ACTIVE 5
#endif
#ifndef LC_SS_FEAT_WIDTHS
#define LC_SS_FEAT_WIDTHS(DP) ((DP) >= 32 && (DP) <= 128)  // (every padded width: 80, 96, 112 fit their registers as 8-wave blocks, round 5)
#endif

namespace lck {

// ===========================================================================
// Sufficient statistics
// ===========================================================================
// S_k = sum_n q_nk x_n x_n^T is a GEMM whose reduction dimension is the data
// rows.  One wave owns CPW clusters and streams over a chunk of rows, four
// rows per step, with the (symmetric, lower-triangular 16x16-blocked)
// accumulators in registers for the whole chunk.  For every needed pair of
// 16-wide feature blocks (JBp >= JB) and every rotation s of the four 4-wide
// sub-blocks inside JBp the wave issues
//     D += A(x[., 16*JBp + 4*((blk+s)&3) + lo2]) * B(q_k * x[., 16*JB + 4*blk + lo2])
// so that MFMA block blk computes the 4x4 tile (i-tile (blk+s)&3, j-tile blk).
// Off-diagonal 16x16 blocks need s=0..3, diagonal ones s=0..2 (symmetry).
//
// fp64 VALU and fp64 MFMA share the issue pipe on gfx950 (a VALU block between
// MFMA streams is not hidden by the other resident wave:
// tools/mfma_issue_probe.hip, 97% -> 81% of peak), so the rotated operands are
// NOT formed with DPP moves: the workgroup stages BR rows of X in LDS (every
// wave of the group needs the same rows) and each wave reads all four
// rotations of a fragment straight from LDS with rotated addresses (LGKM
// path).  Row stride DP+16 doubles keeps the two rows a ds_read_b64 half-wave
// touches on disjoint banks.  q columns are staged per wave the same way.
// What remains on the VALU per cluster and step: NB multiplies (q*x), NB adds
// (s_k) and one add (N_k) against NACC MFMAs.
// Each (chunk, cluster) writes one partial record; launch_reduce_partials sums
// chunks in fixed order.
template <int NB>
struct SSAcc { static constexpr int N = NB * 3 + NB * (NB - 1) / 2 * 4; };

// SKIP: a (4-row step, cluster) pair whose four responsibilities are all exactly 0.0 contributes exactly nothing;
// the sparse mode (cluster.cpp:67-79: groups without mass in a cluster are left out) launches this variant so that
// "sparse" saves the work it saves in the reference.  The dense variant carries no test in its inner loop.
// HALF: 0 = the whole tile triangle in one launch; 1 / 2 = the first / second half of the 16x16 block pairs (balanced by
// MFMA count).  At D = 128 the 136 accumulators per cluster of the full triangle leave room for ONE wave per SIMD, and
// a lone wave cannot hide its own LDS latency; two half launches (68 / 69 accumulators, both re-read X, which the
// MFMA-bound kernel can afford) run two waves per SIMD with the simple step loop.  N_k and s_k ride with half 1.
template <int NB>
__host__ __device__ constexpr bool ss_in_half(int half, int jbp, int jb) {
  if (half == 0) return true;
  const bool first = NB == 8   ? (jbp < 5 || (jbp == 5 && jb < 3))    // 67 | 69 MFMAs
                     : NB == 7 ? (jbp < 4 || (jbp == 4 && jb < 4))    // 52 | 53
                     : NB == 6 ? (jbp < 4 || (jbp == 4 && jb < 1))    // 40 | 38
                               : (jbp == 1 || jbp == 2);              // 18 | 18 (NB = 4)
  return first == (half == 1);
}
// PAN (observations wider than 128 columns, DP = 64 only): the statistics of a wide X are assembled from 64-column
// panels, one launch per panel pair (P >= Q).  1 = diagonal pair (P, P): the triangle loop of the narrow kernel on
// columns [colA, colA + 64) of rows with stride ldx; N_k rides with panel 0, s_k with every diagonal pair.
// 2 = off-diagonal pair: A operands (all four rotations) from panel colA, q x from panel colB, the full 16 x 4 set of
// MFMAs, block written to (P, Q) and mirrored to (Q, P).  Records are DPW wide.
template <int PAN>
constexpr int ss_batch_rows() { return PAN == 2 ? 24 : SS_BR; }  // (two panels per batch: 24 rows keep two blocks per CU)
template <int DP, int CPW, bool SKIP, int HALF, int PAN = 0, bool RSP = false>
__global__ void __launch_bounds__(256, (DP <= 64 ? (HALF != 0 ? 3 : 2) : (HALF != 0 || DP <= 80 ? 2 : 1)))
    suffstat_kernel(SuffstatLaunch a) {
  static_assert(PAN == 0 || (DP == 64 && HALF == 0), "panel variants are built on the D = 64 kernel");
  constexpr int NB = DP / 16;
  constexpr int NACC = PAN == 2 ? NB * NB * 4 : SSAcc<NB>::N;
  constexpr int BR = ss_batch_rows<PAN>();
  constexpr int LD = lds_row_stride(DP);  // padded LDS row stride (doubles)
  constexpr int NPB = PAN == 2 ? 2 : 1;  // column panels staged per batch
  constexpr bool SORD = DP == 64;        // rotation-major MFMA order in the step loop (see there)
  // step loop with the next step's unrotated fragments and q prefetched (see there); -2...4 % at every width but
  // 16 (+20 %: four clusters per wave on 10 MFMAs each leave nothing to hide the extra reads behind)
  constexpr bool PFETCH = DP >= 32 && (DP <= 80 || HALF != 0);
  constexpr int XBUF = NPB * BR * LD;    // doubles per X buffer
  constexpr int NV2 = BR * DP / 2;       // double2 elements per staged batch and panel
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int nwaves = 4, nthr = 256;  // always launched with 4 waves; surplus waves only help staging
  double* xbuf = lds;                              // [2][NPB][BR][LD]
  double* qbuf = lds + 2 * XBUF;                   // [2][nwaves][CPW][BR]
  const int64_t ldx = PAN ? a.ldx : DP;            // row stride of X
  const int DPW = PAN ? a.DPW : DP;                // record width
  const int colA = PAN ? a.colA : 0, colB = PAN == 2 ? a.colB : colA;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo4 = lane & 15, hi = lane >> 4, blk = (lane >> 2) & 3, lo2 = lane & 3;
  const int K = a.K;
  // Workgroup -> (row chunk, cluster slice).  Every slice of a chunk re-reads the
  // same X rows, so the slices of one chunk are placed back-to-back on ONE XCD
  // (block b runs on XCD b % 8, each XCD has its own L2): seq = b / 8 walks
  // (chunk-in-XCD, slice) with the slice fastest.  Pure speed; any placement is correct.
  int chunk, slice;
  {
    const int nslice = a.nslice, nchunks = a.nchunks;
    const int b = blockIdx.x;
    const int full = (nchunks / 8) * 8;
    if (b < full * nslice) {
      const int xcd = b & 7, seq = b >> 3;
      chunk = (seq / nslice) * 8 + xcd;
      slice = seq % nslice;
    } else {
      const int t = b - full * nslice;
      chunk = full + t / nslice;
      slice = t % nslice;
    }
  }
  // RSP (row split, launched for a last slice that fills only one or two waves): the idle waves share the rows of
  // the active ones -- wave w works on the clusters of wave w % f, 4-row steps st = rcls mod RS, and writes its own record
  int wslot = wave, rcls = 0;
  if constexpr (RSP) {
    slice += a.slice0;
    const int f = nwaves / a.rs;
    wslot = wave % f;
    rcls = wave / f;
  }
  const int KR = a.KR;                                // records per chunk (K, or K + extra row-split records)
  const int kbase = (slice * nwaves + wslot) * CPW;   // may be >= K: the wave still helps staging
  int nk = kbase >= K ? 0 : ((K - kbase) < CPW ? (K - kbase) : CPW);
  int64_t r0 = (int64_t)chunk * a.chunk_rows;
  int64_t r1 = (r0 + a.chunk_rows) < a.NP ? (r0 + a.chunk_rows) : a.NP;
  int kidx[CPW];      // cluster of accumulator set c
  int64_t recidx[CPW];  // its partial record
#pragma unroll
  for (int c = 0; c < CPW; ++c) {
    kidx[c] = kbase + c;
    recidx[c] = (int64_t)chunk * KR + kbase + c;
    if (RSP && rcls > 0) recidx[c] = (int64_t)chunk * KR + K + (rcls - 1) * a.nklast + (kbase + c - a.klast0);
  }
  if (a.items) {
    // sparse work list: one block = (row range inside ONE group, up to 4*CPW clusters of that group's active
    // list); work is proportional to the active (row, cluster) pairs, records exist only for those pairs
    const SSItem it = a.items[blockIdx.x];
    r0 = it.r0;
    r1 = it.r1;
    const int first = wave * CPW;
    nk = first >= it.kcnt ? 0 : ((it.kcnt - first) < CPW ? (it.kcnt - first) : CPW);
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
      kidx[c] = c < nk ? a.klist[it.kofs + first + c] : 0;
      recidx[c] = it.rec0 + first + c;
    }
  }

  double acc[CPW][NACC];
  double sacc[CPW][NB];
  double nacc[CPW];
#pragma unroll
  for (int c = 0; c < CPW; ++c) {
    nacc[c] = 0.0;
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[c][i] = 0.0;
#pragma unroll
    for (int i = 0; i < NB; ++i) sacc[c][i] = 0.0;
  }

  // ---- staging: registers hold the next batch while the current one is consumed
  constexpr int NPRE_MAX = (NV2 + nthr - 1) / nthr, npre = NPRE_MAX;
  double pre[NPB][NPRE_MAX][2];
  double qpre[CPW];
  auto gload = [&](int64_t b0) {
#pragma unroll
    for (int pn = 0; pn < NPB; ++pn) {
#pragma unroll
      for (int i = 0; i < NPRE_MAX; ++i) {
        if (i < npre) {
          const int idx = tid + i * nthr;          // double2 index inside the batch: row-major [BR][DP/2]
          const int row = idx / (DP / 2), c2 = idx % (DP / 2);
          double2 v = make_double2(0.0, 0.0);
          if (idx < NV2 && b0 + row < r1)
            v = *reinterpret_cast<const double2*>(a.X + (b0 + row) * ldx + (pn == 0 ? colA : colB) + 2 * c2);
          pre[pn][i][0] = v.x;
          pre[pn][i][1] = v.y;
        }
      }
    }
    // q: lanes 0..BR-1 of each wave fetch that wave's CPW columns (coalesced)
    int g = 0;
    const int64_t qrow = b0 + lane;
    const bool qok = lane < BR && qrow < r1;
    if (a.smask && qok) g = a.rginfo[qrow >> 4] >> 5;
#pragma unroll
    for (int c = 0; c < CPW; ++c) {
      double q = 0.0;
      if (c < nk && qok) {
        q = a.qZ[(int64_t)kidx[c] * a.ldq + qrow];
        if (a.smask && !a.smask[(int64_t)g * K + kidx[c]]) q = 0.0;
      }
      qpre[c] = q;
    }
  };
  auto lstore = [&](int buf) {
    double* xb = xbuf + buf * XBUF;
#pragma unroll
    for (int pn = 0; pn < NPB; ++pn) {
#pragma unroll
      for (int i = 0; i < NPRE_MAX; ++i) {
        if (i < npre) {
          const int idx = tid + i * nthr;
          const int row = idx / (DP / 2), c2 = idx % (DP / 2);
          if (idx < NV2)
            *reinterpret_cast<double2*>(xb + pn * BR * LD + row * LD + 2 * c2) = make_double2(pre[pn][i][0], pre[pn][i][1]);
        }
      }
    }
    if (lane < BR) {
      double* qb = qbuf + ((buf * nwaves + wave) * CPW) * BR;
#pragma unroll
      for (int c = 0; c < CPW; ++c) qb[c * BR + lane] = qpre[c];
    }
  };

  if (r0 < r1) {
    gload(r0);
    lstore(0);
  }
  __syncthreads();
  int buf = 0;
  for (int64_t b0 = r0; b0 < r1; b0 += BR, buf ^= 1) {
    const bool more = b0 + BR < r1;
    if (more) gload(b0 + BR);
    if (nk > 0) {
      const double* xb = xbuf + buf * XBUF + hi * LD + lo2;
      const double* qb = qbuf + ((buf * nwaves + wave) * CPW) * BR + hi;
      if constexpr (DP > 80 && HALF == 0) {
        // One wave per SIMD (the accumulators need > 256 registers): nothing else hides the LDS
        // latency, so the step loop is software-pipelined by hand, unrolled by two with two register
        // sets (unrotated fragments + q of a step) that swap roles -- no copies.  A step fetches its
        // rotated fragments at the top (first needed after the unrotated MFMAs) and the unrotated
        // fragments and q of the NEXT step; only the first step of a batch waits on LDS.  All BR/4
        // steps run (rows past the chunk end were staged as zeros with q = 0); the last step's prefetch
        // reads one step past the tile: inside the LDS allocation, never used.
        double xA[NB], qA[CPW], xB[NB], qB[CPW];
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) xA[jb] = xb[16 * jb + 4 * blk];
#pragma unroll
        for (int c = 0; c < CPW; ++c) qA[c] = qb[c * BR];
        auto step = [&](int st, const double (&x0)[NB], const double (&q)[CPW], double (&x0n)[NB],
                        double (&qn)[CPW]) {
          double xr[NB][4];
#pragma unroll
          for (int jb = 0; jb < NB; ++jb) {
            xr[jb][0] = x0[jb];
#pragma unroll
            for (int s2 = 1; s2 < 4; ++s2) xr[jb][s2] = xb[st * 4 * LD + 16 * jb + 4 * ((blk + s2) & 3)];
          }
#pragma unroll
          for (int jb = 0; jb < NB; ++jb) x0n[jb] = xb[(st + 1) * 4 * LD + 16 * jb + 4 * blk];
#pragma unroll
          for (int c = 0; c < CPW; ++c) qn[c] = qb[c * BR + (st + 1) * 4];
#pragma unroll
          for (int c = 0; c < CPW; ++c) {
            if (SKIP && __builtin_amdgcn_ballot_w64(q[c] != 0.0) == 0) continue;
            double qx[NB];
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
              qx[jb] = q[c] * xr[jb][0];
              sacc[c][jb] += qx[jb];
            }
            nacc[c] += q[c];
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {  // unrotated operands first
              int idx = 0;
#pragma unroll
              for (int jbp = 0; jbp < NB; ++jbp)
#pragma unroll
                for (int jb = 0; jb <= jbp; ++jb)
#pragma unroll
                  for (int s2 = 0; s2 < 4; ++s2)
                    if (s2 < 3 || jb < jbp) {
                      if ((pass == 0) == (s2 == 0)) acc[c][idx] = mfma4(xr[jbp][s2], qx[jb], acc[c][idx]);
                      ++idx;
                    }
            }
          }
        };
        static_assert((BR / 4) % 2 == 0, "step loop is unrolled by two");
#pragma unroll 1
        for (int st = 0; st < BR / 4; st += 2) {
          step(st, xA, qA, xB, qB);
          step(st + 1, xB, qB, xA, qA);
        }
      } else if constexpr (PAN == 2) {
        const int nstep = (int)(((r1 - b0) < BR ? (r1 - b0) : BR) / 4);
        for (int st = 0; st < nstep; ++st) {
          if (SKIP) {
            bool any = false;
#pragma unroll
            for (int c = 0; c < CPW; ++c) any = any || qb[c * BR + st * 4] != 0.0;
            if (__builtin_amdgcn_ballot_w64(any) == 0) continue;
          }
          // A side: all four rotations of panel colA; B side: the unrotated fragments of panel colB
          // (read in the order of use: the B side first, then the A side block row by block row, so that the
          // MFMAs of block row 0 start on a partial lgkmcnt wait)
          double xr[NB][4], xq[NB];
#pragma unroll
          for (int jb = 0; jb < NB; ++jb) xq[jb] = xb[BR * LD + st * 4 * LD + 16 * jb + 4 * blk];
#pragma unroll
          for (int jb = 0; jb < NB; ++jb)
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) xr[jb][s2] = xb[st * 4 * LD + 16 * jb + 4 * ((blk + s2) & 3)];
#pragma unroll
          for (int c = 0; c < CPW; ++c) {
            const double q = qb[c * BR + st * 4];
            if (SKIP && __builtin_amdgcn_ballot_w64(q != 0.0) == 0) continue;
            double qx[NB];
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) qx[jb] = q * xq[jb];
#pragma unroll
            for (int jbp = 0; jbp < NB; ++jbp)
#pragma unroll
              for (int jb = 0; jb < NB; ++jb)
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2)
                  acc[c][(jbp * NB + jb) * 4 + s2] = mfma4(xr[jbp][s2], qx[jb], acc[c][(jbp * NB + jb) * 4 + s2]);
          }
        }
      } else if constexpr (RSP) {
        const int nstep = (int)(((r1 - b0) < BR ? (r1 - b0) : BR) / 4);
        for (int st = rcls; st < nstep; st += a.rs) {
          double xr[NB][4];
#pragma unroll
          for (int jb = 0; jb < NB; ++jb)
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) xr[jb][s2] = xb[st * 4 * LD + 16 * jb + 4 * ((blk + s2) & 3)];
#pragma unroll
          for (int c = 0; c < CPW; ++c) {
            const double q = qb[c * BR + st * 4];
            double qx[NB];
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
              qx[jb] = q * xr[jb][0];
              if (HALF != 2) sacc[c][jb] += qx[jb];
            }
            if (HALF != 2) nacc[c] += q;
            int idx = 0;
#pragma unroll
            for (int jbp = 0; jbp < NB; ++jbp)
#pragma unroll
              for (int jb = 0; jb <= jbp; ++jb)
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2)
                  if (s2 < 3 || jb < jbp) {
                    if (ss_in_half<NB>(HALF, jbp, jb)) acc[c][idx] = mfma4(xr[jbp][s2], qx[jb], acc[c][idx]);
                    ++idx;
                  }
          }
        }
      } else if constexpr (PFETCH && !SKIP) {
        // Dense: the unrotated fragments and q of step st + 1 are fetched under the MFMAs of step st (12 registers at
        // D = 64), so a step starts its rotation-0 MFMAs at once and its own rotated fragments arrive under them.
        // All BR/4 steps run (rows past the chunk end were staged as zeros with q = 0).
        double x0[NB], qv[CPW];
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) x0[jb] = xb[16 * jb + 4 * blk];
#pragma unroll
        for (int c = 0; c < CPW; ++c) qv[c] = qb[c * BR];
#pragma unroll 1
        for (int st = 0; st < BR / 4; ++st) {
          double xr[NB][4], x0n[NB], qn[CPW];
#pragma unroll
          for (int s2 = 1; s2 < 4; ++s2)
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) xr[jb][s2] = xb[st * 4 * LD + 16 * jb + 4 * ((blk + s2) & 3)];
          const int sn = st + 1 < BR / 4 ? st + 1 : st;  // (the last step re-reads its own operands; not used)
#pragma unroll
          for (int jb = 0; jb < NB; ++jb) {
            xr[jb][0] = x0[jb];
            x0n[jb] = xb[sn * 4 * LD + 16 * jb + 4 * blk];
          }
#pragma unroll
          for (int c = 0; c < CPW; ++c) qn[c] = qb[c * BR + sn * 4];
#pragma unroll
          for (int c = 0; c < CPW; ++c) {
            double qx[NB];
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
              qx[jb] = qv[c] * xr[jb][0];
              if (HALF != 2) sacc[c][jb] += qx[jb];
            }
            if (HALF != 2) nacc[c] += qv[c];
#pragma unroll
            for (int sp = 0; sp < 4; ++sp) {
              int idx = 0;
#pragma unroll
              for (int jbp = 0; jbp < NB; ++jbp)
#pragma unroll
                for (int jb = 0; jb <= jbp; ++jb)
#pragma unroll
                  for (int s2 = 0; s2 < 4; ++s2)
                    if (s2 < 3 || jb < jbp) {
                      if (s2 == sp && ss_in_half<NB>(HALF, jbp, jb)) acc[c][idx] = mfma4(xr[jbp][s2], qx[jb], acc[c][idx]);
                      ++idx;
                    }
            }
          }
#pragma unroll
          for (int jb = 0; jb < NB; ++jb) x0[jb] = x0n[jb];
#pragma unroll
          for (int c = 0; c < CPW; ++c) qv[c] = qn[c];
        }
      } else {
        const int nstep = (int)(((r1 - b0) < BR ? (r1 - b0) : BR) / 4);
        for (int st = 0; st < nstep; ++st) {
          if (SKIP) {  // nothing to do for any of this wave's clusters: do not even fetch the fragments
            bool any = false;
#pragma unroll
            for (int c = 0; c < CPW; ++c) any = any || qb[c * BR + st * 4] != 0.0;
            if (__builtin_amdgcn_ballot_w64(any) == 0) continue;
          }
          // fragments: xr[jb][s] = x[row 4*st+hi][16*jb + 4*((blk+s)&3) + lo2]
          double xr[NB][4];
  #pragma unroll
          for (int t = 0; t < 4 * NB; ++t) {
            const int jb = SORD ? t % NB : t / 4, s = SORD ? t / NB : t % 4;
            xr[jb][s] = xb[st * 4 * LD + 16 * jb + 4 * ((blk + s) & 3)];
          }
  #pragma unroll
          for (int c = 0; c < CPW; ++c) {
            const double q = qb[c * BR + st * 4];
            if (SKIP && __builtin_amdgcn_ballot_w64(q != 0.0) == 0) continue;
            double qx[NB];
  #pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
              qx[jb] = q * xr[jb][0];
              if (HALF != 2) sacc[c][jb] += qx[jb];
            }
            if (HALF != 2) nacc[c] += q;
            // D = 64: rotation-major order -- the unrotated fragments (the first reads of the step) are consumed
            // first, so the compiler can start the MFMAs on partial lgkmcnt waits while the rotated fragments are
            // still in flight (23.5 -> 22.9 ms at the north-star shape; the other widths are 2-5 % slower that way)
  #pragma unroll
            for (int sp = 0; sp < (SORD ? 4 : 1); ++sp) {
              int idx = 0;
  #pragma unroll
              for (int jbp = 0; jbp < NB; ++jbp) {
  #pragma unroll
                for (int jb = 0; jb <= jbp; ++jb) {
  #pragma unroll
                  for (int s = 0; s < 4; ++s) {
                    if (s < 3 || jb < jbp) {
                      if ((!SORD || s == sp) && ss_in_half<NB>(HALF, jbp, jb))
                        acc[c][idx] = mfma4(xr[jbp][s], qx[jb], acc[c][idx]);
                      ++idx;
                    }
                  }
                }
              }
            }
          }
        }
      }
    }
    if (more) lstore(buf ^ 1);
    __syncthreads();
  }
  if (nk == 0) return;

  const int64_t SS = 1 + (int64_t)DPW + (int64_t)DPW * DPW;
#pragma unroll
  for (int c = 0; c < CPW; ++c) {
    if (c < nk) {
      double* out = a.partial + recidx[c] * SS;
      if (HALF != 2 && PAN != 2) {
        if (PAN == 0 || colA == 0) {
          const double nsum = sum_over_hi(nacc[c]);
          if (lane == 0) out[0] = nsum;
        }
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
          const double s = sum_over_hi(sacc[c][jb]);
          if (hi == 0) out[1 + colA + 16 * jb + lo4] = s;
        }
      }
      double* S = out + 1 + DPW;
      if constexpr (PAN == 2) {
#pragma unroll
        for (int jbp = 0; jbp < NB; ++jbp)
#pragma unroll
          for (int jb = 0; jb < NB; ++jb)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const int gi = colA + 16 * jbp + 4 * ((blk + s) & 3) + hi, gj = colB + 16 * jb + 4 * blk + lo2;
              const double v = acc[c][(jbp * NB + jb) * 4 + s];
              S[(int64_t)gi * DPW + gj] = v;
              S[(int64_t)gj * DPW + gi] = v;
            }
      } else {
      int idx = 0;
#pragma unroll
      for (int jbp = 0; jbp < NB; ++jbp) {
#pragma unroll
        for (int jb = 0; jb <= jbp; ++jb) {
          const int ns = jb < jbp ? 4 : 3;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            if (s < ns) {
              const int ti = (blk + s) & 3, tj = blk;
              const int gi = colA + 16 * jbp + 4 * ti + hi, gj = colA + 16 * jb + 4 * tj + lo2;
              const bool diag = jb == jbp;
              // diagonal 16x16 blocks: s=0 gives the diagonal tiles, s=1 every pair {t,t+1 mod 4}
              // once, s=2 the pairs {0,2},{1,3} twice (keep the lower copy); s=3 is never issued
              const bool wr = (!diag || ti == tj || s == 1 || ti > tj) && ss_in_half<NB>(HALF, jbp, jb);
              const double v = acc[c][idx];
              if (wr) {
                S[(int64_t)gi * DPW + gj] = v;
                if (!diag || ti != tj) S[(int64_t)gj * DPW + gi] = v;
              }
              ++idx;
            }
          }
        }
      }
      }
    }
  }
}

// ===========================================================================
// Sufficient statistics as a feature GEMM (32 <= D <= 128, more than 16 clusters, dense)
// ===========================================================================
// suffstat_kernel forms q_k x per cluster: 9 fp64 VALU instructions per 36 MFMAs, and an fp64 VALU instruction inside a
// stream of fp64 MFMAs costs the matrix pipe about 11 clocks (tools/mfma_mix_probe.hip) -- its ceiling is ~81 % of the
// pipe, and it sits there.  Here the cluster index moves into the MFMA:  T = Q^T Phi(x), Phi(x) = [x_i x_j (i <= j) | x_i | 1]:
//   A operand = q[row 4 st + hi][cluster k0 + 4 c + lo2]     (one LDS read per cluster quad and step, all tiles share it)
//   B operand = x[row][u] * x[row][w]                         (ONE multiply per 16 features, shared by ALL cluster quads)
//   D[i = hi][lane (lo2, blk)] = sum over the rows of q_{k0 + 4c + hi} x_u x_w
// i.e. one v_mul_f64 per NQ MFMAs (NQ = cluster quads per launch, up to 8: 1 : 8 against 1 : 4) and nothing else on the
// VALU: s_k and N_k are the features x_i * 1 and 1 * 1 (a column of ones rides in the staged X rows).  A "tile" is 16
// features, each the product of one lane's own two columns (u, w): the features of the active width, packed (ft_feature
// in lc_kernels.h: 135 tiles at D = 64); a wave owns up to 9 tiles x NQ quads (<= 72 accumulators), nslice blocks cover a
// row chunk (as the cluster slices of suffstat_kernel do), and the tiles are dealt so that no SIMD carries more than its
// share (ft_deal).  Every tile reads its two operand fragments itself (LDS broadcast reads cost the matrix pipe nothing;
// no operand sharing to schedule).  More than 32 clusters: one launch per range of <= 32.  Same partial records, same
// reduction, deterministic; a feature's accumulator sees the same MFMAs over the same rows wherever in a tile it sits,
// and the one accumulator of x_i x_j is written to S[i][j] and S[j][i], so S_k comes out exactly symmetric.
// (DC: the ACTIVE width, estep_active_width in lc_kernels.h -- the features of the columns past it are products of zeros
//  and are not dealt out at all; their record entries are never written)
#ifndef LC_FT_BR
#define LC_FT_BR 32
#endif
#ifndef LC_FT_BR64
#define LC_FT_BR64 48
#endif
#ifndef LC_FT_BR128
#define LC_FT_BR128 32
#endif
// Loop order of the instances that skip specks (suffstat_feat_kernel<..., SPECK>) at the grouped widths.  Quad-major
// (ft_quad_major): all products of a step first, then ONE guarded block of NT MFMAs per quad -- 8 branches per step of 9
// tiles x 8 quads.  Timed on one box against tile groups with one branch per (group, quad) -- pairs 40, threes 24 branches
// per step -- at the north star (profiles/stats_speck_skip_quad_major.txt): pairs 15.7, threes 13.84, quad-major 12.31 ms per
// hard pass.  D = 48 keeps tile pairs (ft_group_speck): <48,40,5> spills 8 registers in quad-major order, and with threes
// <48,44,8> and <48,40,5> spill.  -DLC_FT_QUAD_MAJOR=0 (tools/variants.py) builds the tile-group layout everywhere, with
// LC_FT_GROUP_SPECK tiles per group at D = 64.
#ifndef LC_FT_GROUP_SPECK
#define LC_FT_GROUP_SPECK 3
#endif
#ifndef LC_FT_QUAD_MAJOR
#define LC_FT_QUAD_MAJOR 1
#endif
__host__ __device__ constexpr bool ft_quad_major(int DP) { return LC_FT_QUAD_MAJOR != 0 && DP >= 64 && DP <= 112; }
// -DLC_FT_SPECK_SORT=0 (tools/variants.py): the context's skipping passes leave the rows of a batch as they come
#ifndef LC_FT_SPECK_SORT
#define LC_FT_SPECK_SORT 1
#endif
int speck_skip_mode() { return LC_FT_SPECK_SORT != 0 ? 2 : 1; }
// tiles whose products are formed together in front of their MFMAs (suffstat_feat_kernel's step loop)
// (round 5, K = 20 / 40 at D = 64: threes and fours for the launches of <= 6 quads measure the same as pairs, gpurun_out/r05y2)
__host__ __device__ constexpr int ft_group(int DP) { return DP >= 48 && DP <= 112 ? 2 : 1; }
__host__ __device__ constexpr int ft_group_speck(int DP) { return DP == 64 ? LC_FT_GROUP_SPECK : ft_group(DP); }
// (160 KB of LDS per CU: two blocks of 4 waves or one of 8)
__host__ __device__ constexpr int ft_batch_rows(int DP) {
  return DP == 128 && ft_waves(DP) == 8 ? LC_FT_BR128 : DP > 96 ? 24 : DP == 64 && ft_waves(DP) == 8 ? LC_FT_BR64 : LC_FT_BR;
}
// row stride of the staged q quads (32 or 64 cluster columns + 4): the rows of a half-wave 8 banks apart
__host__ __device__ constexpr int ft_qld(int NQ) { return NQ > 8 ? 68 : 36; }
// cluster range of one launch: 32 (up to 8 quads), or -- D = 128 -- 64 in ONE pass over X (16 quads, 4 tiles per wave:
// one multiply per 16 MFMAs; config 5's K = 64 used to take two launches of 8 quads, each re-reading and re-staging X)
inline int ft_range(int DP, int K) { return DP == 128 && K % 64 == 0 ? 64 : DP == 128 && K % 64 >= 57 ? 64 : 32; }
// the instance (its NQ) that serves a launch of nq cluster quads: launch_ss_feat_d's dispatch and suffstat_plan's fill search
constexpr int ft_instance_quads(int nq) { return nq > 8 ? 16 : nq > 4 ? nq : nq > 2 ? 4 : 2; }
inline bool ss_feat_eligible(int DP, int K, int DC) {
  // (tests, libcluster_hip_testhooks.so only: 0 off, 1 where it wins, 2 everywhere it exists)
  static const int mode = test_switch("LC_SS_FEAT") ? atoi(test_switch("LC_SS_FEAT")) : 1;
  if (mode == 0 || DP < 32 || DP > 128) return false;
  if (mode == 2) return true;
  // active width below the padded one (round 6): this kernel skips the idle patches (D = 23: 24 of 39 tiles), the per-cluster
  // kernel works in 16 x 16 blocks and cannot -- from two cluster quads up the feature GEMM is the faster one there
  if (DC > 0 && DC < DP && K >= LC_SS_FEAT_MINK_ACTIVE) return true;
  // few clusters (one launch of <= 4 quads): the per-cluster kernel holds its own up to K = 12 everywhere and at D = 64 /
  // 128 up to 16 (tools/ss_smallk_probe.py, round 5: D = 64, K = 16 0.685 against 0.672 of the peak); a full fourth quad
  // pays at the widths whose per-cluster instances are the weak ones: D = 96, K = 16 0.64 -> 0.75, D = 32 0.56 -> 0.61
  if (K <= 16) return K >= 13 && (DP == 32 || DP == 80 || DP == 96 || DP == 112);
  // measured (tools/ssfeat_check.py, MI355X): it wins where EVERY launch carries 7 or 8 cluster quads (one multiply per
  // 7-8 MFMAs): K = 28..32, 60..64, ...; a remainder launch with few quads costs a whole pass over X at a poor ratio
  // (K = 33: 6.8 against 5.8 ms at N = 2M), and with 5-6 quads the two kernels are level
  // round 4, with chunk counts that fill the last round of resident blocks (suffstat_plan): at D <= 64 a remainder launch
  // of 1 ... 7 quads pays as soon as it carries a whole quad's worth of clusters (D = 64: K = 36 +2 %, 40 +9 %, 48 +2 %,
  // 56 +17 %; D = 48, K = 48 +12 %; D = 32, K = 40 +21 %; K = 33 still loses 12 %); D = 128 keeps the round-3 rule
  // (K = 40 level, 48 -5 %) next to the 64-cluster ranges
  const int rem = K % 32;
  if (!LC_SS_FEAT_WIDTHS(DP)) return false;
  if (DP == 128) return rem == 0 || rem >= 28 || (ft_range(DP, K) == 64 && K >= 57);
  return rem == 0 || rem >= 4;
}
// SPECK (speck skipping): a (4-row step, cluster quad) pair whose sixteen responsibilities are ALL below
// SPECK_TAU issues no MFMA -- once the posteriors have sharpened every row has one owner and K - 1 specks of 1e-100 and
// less, and most of a step's quads hold nothing else.  The A operand is the same sixteen values for every tile and every
// wave of the block, so the decision is wave-uniform and all waves skip the same quads (ft_deal's balance stands).  The
// staging threads form the step's mask (a thread holds the four rows of one cluster, a wave 32 clusters x 2 row quads or
// 64 x 1: one compare per value and a ballot) and one lane per step stores it -- a byte, two at 16 quads -- in the spare
// columns of the staged q batch's first row; the batch body fetches the 16 bytes once into four SGPRs, and the step loop
// tests compile-time bits of them: no VALU work in the loop.  "Kept" is "not (q < tau)": a NaN is kept and poisons its
// record as it always did; specks inside a kept pair are accumulated as before.
template <int DP, int DC, int NQ, bool SPECK>
__global__ void __launch_bounds__(64 * ft_waves(DP), 2) suffstat_feat_kernel(SuffstatLaunch a) {
  static_assert(DC % 4 == 0 && DC <= DP && DC > DP - 16, "active width");
  constexpr int FTW = ft_waves(DP);
  constexpr int BR = ft_batch_rows(DP), LD = lds_row_stride(DP), QLD = ft_qld(NQ), XBUF = BR * LD, QBUF = BR * QLD;
  constexpr int TPW = ft_tpw(DP, DC, NQ), NSL = ft_nslice(DP, DC, NQ);
  constexpr int ONE = DP;  // column of the staged rows that holds 1.0
  static_assert(LD > DP, "the staged rows need a spare column");
  static_assert(TPW * NQ <= 72, "accumulators");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* xbuf = lds;              // [2][BR][LD]
  double* qbuf = lds + 2 * XBUF;   // [2][BR][QLD]   q[row][cluster - k0], clusters past the range are zero
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 4, blk = (lane >> 2) & 3, lo2 = lane & 3;
  const int k0 = a.klast0;                                  // first cluster of this launch's range
  const int KC = a.K - k0 < 4 * NQ ? a.K - k0 : 4 * NQ;     // clusters in the range
  int chunk, slice;
  {  // (chunk, slice) placement as in suffstat_kernel: the slices of a chunk back-to-back on one XCD
    const int nslice = NSL, nchunks = a.nchunks, b = blockIdx.x, full = (nchunks / 8) * 8;
    if (b < full * nslice) {
      const int xcd = b & 7, seq = b >> 3;
      chunk = (seq / nslice) * 8 + xcd;
      slice = seq % nslice;
    } else {
      const int t = b - full * nslice;
      chunk = full + t / nslice;
      slice = t % nslice;
    }
  }
  const int64_t r0 = (int64_t)chunk * a.chunk_rows;
  const int64_t r1 = (r0 + a.chunk_rows) < a.NP ? (r0 + a.chunk_rows) : a.NP;
  // this wave's tiles (ft_deal) and, per lane, where their two operand fragments sit in a staged batch (in doubles,
  // step 0).  8 waves: TPW or TPW - 1 tiles (two instances of the batch body); 4 waves: TPW everywhere, the tiles past
  // the last one (idle) read 1 * 1 and are not stored
  constexpr bool UNEVEN = FTW == 8 && ft_nt_min(DP, DC, NQ) < TPW;
  constexpr int TPWL = UNEVEN ? TPW - 1 : TPW;
  static_assert(FTW != 8 || (TPWL >= 1 && ft_nt_min(DP, DC, NQ) == TPWL), "tile deal");
  int T0 = 0, nt = 0;
  ft_deal(DP, DC, NQ, slice, wave, &T0, &nt);
  const double* pu[TPW];
  const double* pw[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const FtFeature f = ft_feature(DC, ONE, 16 * (T0 + t) + lo2 + 4 * blk);
    pu[t] = xbuf + hi * LD + f.u;
    pw[t] = xbuf + hi * LD + f.w;
  }
  double acc[TPW][NQ];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int c = 0; c < NQ; ++c) acc[t][c] = 0.0;

  // ---- staging: registers hold the next batch while the current one is consumed.
  // X batch: thread -> 16 bytes of NPRE consecutive rows (row group tid / TPR, column pair tid % TPR): one address
  // register on either side, the rows are immediate offsets.  q batch: thread -> (cluster tid % QCL, row quad tid / QCL),
  // QCL = 32 or 64 cluster columns: clusters fastest, so that the 16-lane groups of a ds_write_b64 fill one LDS row (rows
  // fastest would put all the row quads of a group on one bank)
  constexpr int NTHR = 64 * FTW;
  constexpr int TPR = DP / 2, NV2 = BR * TPR, NPRE = (NV2 + NTHR - 1) / NTHR;  // double2 per row / per batch / per thread
  constexpr int RPP = NTHR / TPR;                                               // rows covered by one pass of the block
  static_assert(NTHR % TPR == 0 || NPRE * NTHR >= NV2, "staging");
  constexpr int QCL = NQ > 8 ? 64 : 32;
  static_assert(BR / 4 <= NTHR / QCL && 2 * BR <= NTHR, "q staging / ones column");
  // the steps' masks: bytes (16 quads: shorts) in the spare columns QCL ... QCL + 3 of the batch's first q row
  constexpr int MBITS = NQ > 8 ? 16 : 8;
  static_assert(QLD - QCL == 4 && (BR / 4) * MBITS <= 128, "room for the step masks");
  double pre[NPRE][2], qpre[4];
  const int qcl = tid % QCL, qrq = tid / QCL;
  const bool qthr = qrq < BR / 4;
  const int xr0 = tid / TPR, xc2 = tid % TPR;  // (DP = 80, 112: 256 is not a multiple of TPR -- the generic index below)
  double* const qdst = qbuf + (4 * qrq) * QLD + qcl;
  // Sorted batches (SuffstatLaunch::speck_skip == 2): the batch's rows are PLACED by the one quad that keeps
  // them, so that the four rows of a step share their owner and the step keeps one quad, not four.  Row masks (bit c: the
  // row has a value of quad c that is not below SPECK_TAU) go through the row's own spare q columns; behind one more block
  // barrier every wave works out the same slots for itself: a stable counting sort by owning quad, rows that keep nothing
  // last -- or, when ANY row of the batch keeps more than one quad, the rows as they come (slot = row: the steps and sums
  // of the unsorted rule).  A step's mask is the OR of the masks of the rows placed in it, so every kept value is summed
  // wherever its row lands; the placement decides only how much is skipped.
  [[maybe_unused]] const bool sortb = SPECK && a.speck_skip == 2;
  auto lstore_sorted = [&](int buf) {
    if constexpr (SPECK) {
      // the thread's places are worked out again from an opaque copy of its index: hoisted in front of the batch body, the
      // addresses and lane tests below would sit in registers next to the accumulators
      int ts = tid;
      asm volatile("" : "+v"(ts));
      const int ln = ts & 63, sqcl = ts % QCL, sqrq = ts / QCL;
      const bool sqthr = sqrq < BR / 4;
      // a row's mask: ballot of its kept values (one lane per cluster), then lane n < 16 tests nibble n = quad n of that word
      // (32 cluster columns: the low byte of the second ballot belongs to the wave's first row quad, the high byte to its second)
      unsigned rm[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned long long bal = __ballot(!(qpre[i] < SPECK_TAU));
        rm[i] = (unsigned)__ballot(ln < 16 && ((bal >> (4 * (ln & 15))) & 0xfull) != 0);
      }
      if (sqthr && sqcl < 4) {
        unsigned v = sqcl == 0 ? rm[0] : sqcl == 1 ? rm[1] : sqcl == 2 ? rm[2] : rm[3];
        if constexpr (QCL == 32) v = (v >> (8 * (ln >> 5))) & 0xffu;
        *reinterpret_cast<unsigned*>(qbuf + buf * QBUF + (4 * sqrq + sqcl) * QLD + QCL + 2) = v;
      }
      __syncthreads();
      const bool valid = ln < BR;
      const unsigned mask = valid ? *reinterpret_cast<const unsigned*>(qbuf + buf * QBUF + ln * QLD + QCL + 2) : 0u;
      const bool mixed = __ballot(__popc(mask) > 1) != 0;
      int slot = ln;
      if (!mixed) {
        const int myq = mask ? __ffs(mask) - 1 : NQ;  // (NQ: the bin of the rows that keep nothing, padding rows among them)
        int start = 0;
#pragma unroll
        for (int c = 0; c <= NQ; ++c) {
          const unsigned long long b = __ballot(valid && myq == c);
          const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
          if (valid && myq == c) slot = start + rank;
          start += __popcll(b);
        }
      }
      if ((ts >> 6) == FTW - 1) {
        // the step masks, where the batch body reads them: every row's mask to the lane of its slot, OR over four lanes
        unsigned m = (unsigned)__builtin_amdgcn_ds_permute(4 * slot, (int)mask);
        m |= (unsigned)__shfl_xor((int)m, 1);
        m |= (unsigned)__shfl_xor((int)m, 2);
        if (valid && (ln & 3) == 0) {
          if constexpr (MBITS == 8) reinterpret_cast<unsigned char*>(qbuf + buf * QBUF + QCL)[ln >> 2] = (unsigned char)m;
          else reinterpret_cast<unsigned short*>(qbuf + buf * QBUF + QCL)[ln >> 2] = (unsigned short)m;
        }
      }
#pragma unroll
      for (int i = 0; i < NPRE; ++i) {
        const int idx = ts + i * NTHR;
        const int row = idx / TPR, c2 = idx % TPR;
        const int srow = mixed ? row : __shfl(slot, row);
        if (row < BR) *reinterpret_cast<double2*>(xbuf + buf * XBUF + srow * LD + 2 * c2) = make_double2(pre[i][0], pre[i][1]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int srow = mixed ? 4 * sqrq + i : __shfl(slot, 4 * sqrq + i);
        if (sqthr && sqcl < 4 * NQ) qbuf[buf * QBUF + srow * QLD + sqcl] = qpre[i];
      }
    }
  };
  auto gload = [&](int64_t b0) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      int row, c2;
      if constexpr (NTHR % TPR == 0) {
        row = xr0 + i * RPP, c2 = xc2;
      } else {
        const int idx = tid + i * NTHR;
        row = idx / TPR, c2 = idx % TPR;
      }
      double2 v = make_double2(0.0, 0.0);
      if (row < BR && b0 + row < r1) v = *reinterpret_cast<const double2*>(a.X + (b0 + row) * DP + 2 * c2);
      pre[i][0] = v.x;
      pre[i][1] = v.y;
    }
    const int64_t qrow = b0 + 4 * qrq;
#pragma unroll
    for (int i = 0; i < 4; ++i) qpre[i] = 0.0;
    if (qthr && qcl < KC && qrow < r1) {  // (a row quad lies inside the chunk or outside it: chunk_rows is a multiple of 4)
      const double2* qp = reinterpret_cast<const double2*>(a.qZ + (int64_t)(k0 + qcl) * a.ldq + qrow);
      const double2 v0 = qp[0], v1 = qp[1];
      qpre[0] = v0.x, qpre[1] = v0.y, qpre[2] = v1.x, qpre[3] = v1.y;
    }
  };
  auto lstore = [&](int buf) {
    if constexpr (SPECK) {
      if (sortb) {  // (block-uniform)
        lstore_sorted(buf);
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      int row, c2;
      if constexpr (NTHR % TPR == 0) {
        row = xr0 + i * RPP, c2 = xc2;
      } else {
        const int idx = tid + i * NTHR;
        row = idx / TPR, c2 = idx % TPR;
      }
      if (row < BR) *reinterpret_cast<double2*>(xbuf + buf * XBUF + row * LD + 2 * c2) = make_double2(pre[i][0], pre[i][1]);
    }
    if (qthr && qcl < 4 * NQ) {
#pragma unroll
      for (int i = 0; i < 4; ++i) qdst[buf * QBUF + i * QLD] = qpre[i];
    }
    if constexpr (SPECK) {
      // (threads that stage nothing, clusters past the range and rows past the chunk hold zeros: not kept)
      const bool keep = !(qpre[0] < SPECK_TAU) || !(qpre[1] < SPECK_TAU) || !(qpre[2] < SPECK_TAU) || !(qpre[3] < SPECK_TAU);
      unsigned long long bal = __ballot(keep);
      if constexpr (QCL == 32) bal = (bal >> (32 * (lane >> 5))) & 0xffffffffull;  // this thread's row quad
      unsigned m = 0;
#pragma unroll
      for (int c = 0; c < NQ; ++c) m |= ((bal >> (4 * c)) & 0xfull) != 0 ? 1u << c : 0u;
      if (qthr && qcl == 0) {
        if constexpr (MBITS == 8) reinterpret_cast<unsigned char*>(qbuf + buf * QBUF + QCL)[qrq] = (unsigned char)m;
        else reinterpret_cast<unsigned short*>(qbuf + buf * QBUF + QCL)[qrq] = (unsigned short)m;
      }
    }
  };
  if (tid < 2 * BR) xbuf[(tid / BR) * XBUF + (tid % BR) * LD + ONE] = 1.0;
  if (r0 < r1) {
    gload(r0);
    lstore(0);
  }
  __syncthreads();
  const double* pq = qbuf + hi * QLD + lo2;
  // One batch from buffer B, for a wave of NT tiles (two instances: the fuller waves and the others).  All BR / 4 steps
  // run (rows past the chunk end were staged as zeros with q = 0): nothing in the loop depends on run-time counts.  The next tile's fragments -- behind the last tile the next step's first tile and its
  // q quads -- are issued BEFORE this tile's MFMAs and arrive under them (two register sets that swap roles; the fences
  // keep hipcc from sinking the reads to their uses).
  // 16 quads: two sets of q quads would be 64 registers next to 128 of accumulators -- ONE set, refilled in place during
  // the step's last tile (quad c's register takes the next step's quad c right behind the MFMA that read it)
  constexpr bool ONEQ = NQ > 8;
  auto batch = [&](auto bsel, auto ntsel) {
    constexpr int B = decltype(bsel)::value, XO = B * XBUF, QO = B * QBUF, NT = decltype(ntsel)::value;
    // the batch's step masks in four SGPRs; on(st, c): does step st issue the MFMAs of quad c (a compile-time bit)
    unsigned mw0 = 0u, mw1 = 0u, mw2 = 0u, mw3 = 0u;
    if constexpr (SPECK) {
      const uint4 mv = *reinterpret_cast<const uint4*>(qbuf + QO + QCL);
      mw0 = __builtin_amdgcn_readfirstlane(mv.x), mw1 = __builtin_amdgcn_readfirstlane(mv.y);
      mw2 = __builtin_amdgcn_readfirstlane(mv.z), mw3 = __builtin_amdgcn_readfirstlane(mv.w);
    }
    // the test of quad c's bit of step st: s_bitcmp + s_cbranch_scc on a compile-time bit, no VALU work.  (The word is made
    // opaque for EVERY test: hipcc otherwise threads the tests of one bit by a step's tile groups into each other and carries
    // the outcomes as lane masks, with VALU selects between the MFMAs -- and with one opaque word per group it moves the
    // MFMAs out of line, two taken branches per active quad.)
    auto on = [&](int st, int c) {
      if constexpr (!SPECK) return true;
      const int bit = st * MBITS + c;
      unsigned w = bit < 32 ? mw0 : bit < 64 ? mw1 : bit < 96 ? mw2 : mw3;
      asm volatile("" : "+s"(w));
      return ((w >> (bit & 31)) & 1u) != 0;
    };
    if constexpr (!ONEQ && ft_group(DP) > 1) {
      // Tiles in groups of G: the group's products first, then its G x NQ MFMAs.  Next to the matrix pipe a VALU
      // instruction is paid per switch between the two kinds, not per instruction (tools/mfma_batch_probe.hip: ~ 12 clocks
      // for a lone multiply between MFMAs, 8 each in pairs, 5.7 in fours); the fragments of the next group are read into
      // the registers the multiplies have just freed and arrive under the MFMAs.  ONE set of q quads, refilled in place
      // during the last tile of a step (as the 16-quad instance does): the second set's 16 registers pay for the group.
      // Measured (N = 10M, D = 64, K = 32; gpurun_out/r05e): pairs 21.61 -> 21.22 ms, threes 21.30, fours 21.51, fives 21.79
      // -- the multiplies were a third of what the step loses, and larger groups expose the fragment reads; D = 48 gains
      // 1 % with pairs, D = 80 ... 112 1-2 %, D = 32 and D = 128 nothing (ft_group).
      if constexpr (SPECK && ft_quad_major(DP)) {
        // the step's NT products (fragments read one tile ahead), then per quad one test and NT MFMAs; quad c's register
        // takes the next step's quad c right behind its block, whatever was skipped
        double qa[NQ], u[2], w[2], pp[NT];
        u[0] = pu[0][XO];
        w[0] = pw[0][XO];
#pragma unroll
        for (int c = 0; c < NQ; ++c) qa[c] = pq[QO + 4 * c];
#pragma unroll
        for (int st = 0; st < BR / 4; ++st) {
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const int cur = (st * NT + t) & 1, nxt = cur ^ 1;
            pp[t] = u[cur] * w[cur];
            if (t + 1 < NT) {
              u[nxt] = pu[t + 1][XO + st * 4 * LD];
              w[nxt] = pw[t + 1][XO + st * 4 * LD];
            } else if (st + 1 < BR / 4) {
              u[nxt] = pu[0][XO + (st + 1) * 4 * LD];
              w[nxt] = pw[0][XO + (st + 1) * 4 * LD];
            }
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int c = 0; c < NQ; ++c) {
            if (on(st, c)) {
#pragma unroll
              for (int t = 0; t < NT; ++t) acc[t][c] = mfma4(qa[c], pp[t], acc[t][c]);
            }
            if (st + 1 < BR / 4) qa[c] = pq[QO + (st + 1) * 4 * QLD + 4 * c];
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        return;
      }
      constexpr int G = SPECK ? ft_group_speck(DP) : ft_group(DP), TOT = (BR / 4) * NT;
      double qa[NQ], u[G], w[G], pp[G];
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (g < TOT && g < NT) {
          u[g] = pu[g][XO];
          w[g] = pw[g][XO];
        }
#pragma unroll
      for (int c = 0; c < NQ; ++c) qa[c] = pq[QO + 4 * c];
#pragma unroll
      for (int st = 0; st < BR / 4; ++st) {
        // (groups never straddle a step: the step's q quads change there)
#pragma unroll
        for (int t0 = 0; t0 < NT; t0 += G) {
          const int ng = NT - t0 < G ? NT - t0 : G;
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (g < ng) pp[g] = u[g] * w[g];
          // the next group: the rest of this step, or the head of the next one
          const int nt0 = t0 + G < NT ? t0 + G : 0, nst = t0 + G < NT ? st : st + 1;
          if (nst < BR / 4) {
            const int nng = NT - nt0 < G ? NT - nt0 : G;
#pragma unroll
            for (int g = 0; g < G; ++g)
              if (g < nng) {
                u[g] = pu[nt0 + g][XO + nst * 4 * LD];
                w[g] = pw[nt0 + g][XO + nst * 4 * LD];
              }
          }
          const bool refill = nst != st && nst < BR / 4;
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (SPECK) {
            // one scalar branch around each quad's MFMAs of the group; the q quads are refilled whatever was skipped
#pragma unroll
            for (int c4 = 0; c4 < NQ; c4 += 4) {
#pragma unroll
              for (int c = c4; c < c4 + 4 && c < NQ; ++c)
                if (on(st, c)) {
#pragma unroll
                  for (int g = 0; g < G; ++g)
                    if (g < ng) acc[t0 + g][c] = mfma4(qa[c], pp[g], acc[t0 + g][c]);
                }
              if (refill) {
#pragma unroll
                for (int c = c4; c < c4 + 4 && c < NQ; ++c) qa[c] = pq[QO + nst * 4 * QLD + 4 * c];
              }
              __builtin_amdgcn_sched_barrier(0);
            }
            continue;
          }
#pragma unroll
          for (int g = 0; g < G; ++g)
            if (g < ng) {
              if (refill && g + 1 == ng) {
#pragma unroll
                for (int c4 = 0; c4 < NQ; c4 += 4) {
#pragma unroll
                  for (int c = c4; c < c4 + 4 && c < NQ; ++c) acc[t0 + g][c] = mfma4(qa[c], pp[g], acc[t0 + g][c]);
#pragma unroll
                  for (int c = c4; c < c4 + 4 && c < NQ; ++c) qa[c] = pq[QO + nst * 4 * QLD + 4 * c];
                  __builtin_amdgcn_sched_barrier(0);
                }
              } else {
#pragma unroll
                for (int c = 0; c < NQ; ++c) acc[t0 + g][c] = mfma4(qa[c], pp[g], acc[t0 + g][c]);
              }
            }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      return;
    }
    double qa[ONEQ ? 1 : 2][NQ], u[2], w[2];
    u[0] = pu[0][XO];
    w[0] = pw[0][XO];
#pragma unroll
    for (int c = 0; c < NQ; ++c) qa[0][c] = pq[QO + 4 * c];
#pragma unroll
    for (int st = 0; st < BR / 4; ++st) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int cur = (st * NT + t) & 1, nxt = cur ^ 1;
        const double p = u[cur] * w[cur];
        const bool refill = t + 1 == NT && st + 1 < BR / 4;
        if (t + 1 < NT) {
          u[nxt] = pu[t + 1][XO + st * 4 * LD];
          w[nxt] = pw[t + 1][XO + st * 4 * LD];
        } else if (st + 1 < BR / 4) {
          u[nxt] = pu[0][XO + (st + 1) * 4 * LD];
          w[nxt] = pw[0][XO + (st + 1) * 4 * LD];
          if constexpr (!ONEQ) {
#pragma unroll
            for (int c = 0; c < NQ; ++c) qa[(st + 1) & 1][c] = pq[QO + (st + 1) * 4 * QLD + 4 * c];
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ONEQ) {
#pragma unroll
          for (int c4 = 0; c4 < NQ; c4 += 4) {
#pragma unroll
            for (int c = c4; c < c4 + 4; ++c)
              if (on(st, c)) acc[t][c] = mfma4(qa[0][c], p, acc[t][c]);
            if (refill) {
#pragma unroll
              for (int c = c4; c < c4 + 4; ++c) qa[0][c] = pq[QO + (st + 1) * 4 * QLD + 4 * c];
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {
#pragma unroll
          for (int c = 0; c < NQ; ++c)
            if (on(st, c)) acc[t][c] = mfma4(qa[st & 1][c], p, acc[t][c]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  };
  for (int64_t b0 = r0; b0 < r1; b0 += 2 * BR) {  // two batches per trip: the buffer index is a compile-time constant
    const bool more1 = b0 + BR < r1, more2 = b0 + 2 * BR < r1;
    if (more1) gload(b0 + BR);
    if (!UNEVEN || nt == TPW) batch(std::integral_constant<int, 0>{}, std::integral_constant<int, TPW>{});
    else batch(std::integral_constant<int, 0>{}, std::integral_constant<int, TPWL>{});
    if (more1) lstore(1);
    __syncthreads();
    if (!more1) break;
    if (more2) gload(b0 + 2 * BR);
    if (!UNEVEN || nt == TPW) batch(std::integral_constant<int, 1>{}, std::integral_constant<int, TPW>{});
    else batch(std::integral_constant<int, 1>{}, std::integral_constant<int, TPWL>{});
    if (more2) lstore(0);
    __syncthreads();
  }

  // ---- partial records: [N_k, s_k[DP], S_k[DP x DP]] per (chunk, cluster), as suffstat_kernel writes them
  const int64_t SS = 1 + (int64_t)DP + (int64_t)DP * DP;
  // (the deal and the features are worked out again here, not kept: an opaque copy of the slice keeps the compiler from
  //  hoisting them in front of the step loop, where their results would sit in registers next to the accumulators)
  int sle = slice, T0e = 0, nte = 0;
  asm volatile("" : "+v"(sle));
  ft_deal(DP, DC, NQ, sle, wave, &T0e, &nte);
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    if (t >= nte) continue;
    const FtFeature f = ft_feature(DC, ONE, 16 * (T0e + t) + lo2 + 4 * blk);
    if (f.kind == FT_SPARE) continue;
#pragma unroll
    for (int c = 0; c < NQ; ++c) {
      const int kk = 4 * c + hi;
      if (kk >= KC) continue;
      double* out = a.partial + ((int64_t)chunk * a.KR + k0 + kk) * SS;
      const double v = acc[t][c];
      if (f.kind == FT_PRODUCT) {
        double* S = out + 1 + DP;
        S[(int64_t)f.u * DP + f.w] = v;
        S[(int64_t)f.w * DP + f.u] = v;
      } else if (f.kind == FT_LINEAR) {
        out[1 + f.u] = v;
      } else {
        out[0] = v;
      }
    }
  }
}

// launch_speck_probe: one thread per (sampled step, cluster quad), one atomic per wave
// (a step's quads sit in nqp consecutive lanes, nqp = the power of two >= nq: lanes c >= nq idle.  The second count -- rows
// that keep exactly one quad -- is a popcount over those lanes of the row's "kept" ballot; nqp > 64: not counted)
// rk: bit i = row i of this thread's (step, quad c) keeps a value of the quad -> the two counts (all lanes of the block call)
__device__ __forceinline__ void speck_probe_count(unsigned rk, int c, int nqp, int* active) {
  const int lane = threadIdx.x & 63;
  const unsigned long long b = __ballot(rk != 0);
  if (lane == 0 && b != 0) atomicAdd(active, __popcll(b));
  if (nqp <= 64) {
    const unsigned long long grp = (nqp == 64 ? ~0ull : ((1ull << nqp) - 1ull)) << (lane & ~(nqp - 1));
    int single = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned long long br = __ballot((rk >> i) & 1u);
      single += __popcll(__ballot(c == 0 && __popcll(br & grp) == 1));
    }
    if (lane == 0 && single != 0) atomicAdd(active + 1, single);
  }
}
__global__ void __launch_bounds__(256) speck_probe_kernel(const double* qZ, int64_t ldq, int K, int64_t stride, int nsteps, int nq,
                                                           int nqp, int* active) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % nqp);
  unsigned rk = 0;  // bit i: row i of the step keeps a value of quad c
  if (t / nqp < nsteps && c < nq) {
    const int64_t row = 4 * stride * (t / nqp);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 4 * c + i;
      if (k < K) {
        const double2* qp = reinterpret_cast<const double2*>(qZ + (int64_t)k * ldq + row);
        const double2 v0 = qp[0], v1 = qp[1];
        rk |= (!(v0.x < SPECK_TAU) ? 1u : 0u) | (!(v0.y < SPECK_TAU) ? 2u : 0u) | (!(v1.x < SPECK_TAU) ? 4u : 0u) |
              (!(v1.y < SPECK_TAU) ? 8u : 0u);
      }
    }
  }
  speck_probe_count(rk, c, nqp, active);
}
// the same sample read off the kept-quad masks of an E-step (EstepLaunch::qmask): a step's four rows are four bits of one
// 16-bit word (a step starts on a multiple of four rows), bit i of rk what speck_probe_kernel computes from qZ
__global__ void __launch_bounds__(256) speck_probe_masks_kernel(const unsigned short* __restrict__ qmask, int64_t nrg, int64_t stride,
                                                                 int nsteps, int nq, int nqp, int* active) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)(t % nqp);
  unsigned rk = 0;
  if (t / nqp < nsteps && c < nq) {
    const int64_t row = 4 * stride * (t / nqp);
    rk = ((unsigned)qmask[(int64_t)c * nrg + (row >> 4)] >> (unsigned)(row & 15)) & 0xfu;
  }
  speck_probe_count(rk, c, nqp, active);
}
// the sample of both probes: steps looked at, their stride, quads and quads rounded up to a power of two; false: nothing to look at
static bool speck_probe_sample(int K, int64_t NP, int64_t* pairs, int64_t* rows, int* nsteps, int64_t* stride, int* nq, int* nqp) {
  const int64_t steps = NP / 4;
  *pairs = 0;
  if (rows) *rows = 0;
  if (steps < 1 || K < 1) return false;
  *nsteps = (int)(steps < SPECK_PROBE_STEPS ? steps : SPECK_PROBE_STEPS), *nq = (K + 3) / 4;
  *stride = steps / *nsteps;  // (the last sampled step: stride * (nsteps - 1) < steps)
  *nqp = 1;
  while (*nqp < *nq) *nqp *= 2;
  *pairs = (int64_t)*nsteps * *nq;
  if (rows && *nqp <= 64) *rows = 4 * (int64_t)*nsteps;
  return true;
}
hipError_t launch_speck_probe(const double* qZ, int64_t ldq, int K, int64_t NP, int* active, int64_t* pairs, hipStream_t stream,
                              int64_t* rows) {
  int nsteps = 0, nq = 0, nqp = 0;
  int64_t stride = 0;
  const bool any = speck_probe_sample(K, NP, pairs, rows, &nsteps, &stride, &nq, &nqp);
  if (hipError_t e = hipMemsetAsync(active, 0, 2 * sizeof(int), stream); e != hipSuccess) return e;
  if (!any) return hipSuccess;
  hipLaunchKernelGGL(speck_probe_kernel, dim3((unsigned)(((int64_t)nsteps * nqp + 255) / 256)), dim3(256), 0, stream, qZ, ldq, K, stride,
                     nsteps, nq, nqp, active);
  return hipGetLastError();
}
hipError_t launch_speck_probe_masks(const unsigned short* qmask, int64_t nrg, int K, int64_t NP, int* active, int64_t* pairs,
                                    hipStream_t stream, int64_t* rows) {
  int nsteps = 0, nq = 0, nqp = 0;
  int64_t stride = 0;
  if (!qmask || !active || !pairs || nrg * RG < NP) return hipErrorInvalidValue;
  const bool any = speck_probe_sample(K, NP, pairs, rows, &nsteps, &stride, &nq, &nqp);
  if (hipError_t e = hipMemsetAsync(active, 0, 2 * sizeof(int), stream); e != hipSuccess) return e;
  if (!any) return hipSuccess;
  hipLaunchKernelGGL(speck_probe_masks_kernel, dim3((unsigned)(((int64_t)nsteps * nqp + 255) / 256)), dim3(256), 0, stream, qmask, nrg,
                     stride, nsteps, nq, nqp, active);
  return hipGetLastError();
}

template <int DP, int DC, int NQ, bool SPECK>
static hipError_t launch_ss_feat_i(const SuffstatLaunch& b, hipStream_t stream) {
  constexpr int BR = ft_batch_rows(DP), LD = lds_row_stride(DP);
  const size_t shmem = (size_t)(2 * BR * LD + 2 * BR * ft_qld(NQ)) * sizeof(double);
  auto kern = suffstat_feat_kernel<DP, DC, NQ, SPECK>;
  static LdsGrant grant;
  if (hipError_t e = grant_dynamic_lds(reinterpret_cast<const void*>(kern), shmem, grant); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(b.nchunks * ft_nslice(DP, DC, NQ))), dim3(64 * ft_waves(DP)), shmem, stream, b);
  return hipGetLastError();
}
template <int DP, int DC, int NQ>
static hipError_t launch_ss_feat_q(const SuffstatLaunch& b, hipStream_t stream) {
  return b.speck_skip ? launch_ss_feat_i<DP, DC, NQ, true>(b, stream) : launch_ss_feat_i<DP, DC, NQ, false>(b, stream);
}
template <int DP, int DC>
static hipError_t launch_ss_feat_d(const SuffstatLaunch& a, hipStream_t stream) {
  // cluster ranges: as many full ranges of 32 (8 quads: one multiply per 8 MFMAs) as there are, the remainder in a last
  // range of its own -- near-equal ranges (K = 48 as 24 + 24) put BOTH launches at the poor 5-6 quad ratio.  Every range
  // re-reads X, which an MFMA-bound pass affords.
  SuffstatLaunch b = a;
  const int range = ft_range(DP, a.K);
  for (int k0 = 0; k0 < a.K; k0 += range) {
    b.klast0 = k0;
    const int nq = ((a.K - k0 < range ? a.K - k0 : range) + 3) / 4;
    hipError_t e = hipErrorInvalidValue;
    switch (ft_instance_quads(nq)) {
      case 2: e = launch_ss_feat_q<DP, DC, 2>(b, stream); break;
      case 4: e = launch_ss_feat_q<DP, DC, 4>(b, stream); break;
      case 5: e = launch_ss_feat_q<DP, DC, 5>(b, stream); break;
      case 6: e = launch_ss_feat_q<DP, DC, 6>(b, stream); break;
      case 7: e = launch_ss_feat_q<DP, DC, 7>(b, stream); break;
      case 8: e = launch_ss_feat_q<DP, DC, 8>(b, stream); break;
      case 16:  // (ranges of 64 clusters: D = 128 only, ft_range)
        if constexpr (DP == 128) e = launch_ss_feat_q<DP, DC, 16>(b, stream);
        break;
    }
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
template <int DP>
static hipError_t launch_ss_feat_w(const SuffstatLaunch& a, hipStream_t stream) {
  if constexpr (DP <= 48) {
    if (a.DC == DP - 4) return launch_ss_feat_d<DP, DP - 4>(a, stream);
    if (a.DC == DP - 12) return launch_ss_feat_d<DP, DP - 12>(a, stream);
  }
  if (a.DC == DP - 8) return launch_ss_feat_d<DP, DP - 8>(a, stream);
  if (a.DC != 0 && a.DC != DP) return hipErrorInvalidValue;
  return launch_ss_feat_d<DP, DP>(a, stream);
}
static hipError_t launch_ss_feat(const SuffstatLaunch& a, hipStream_t stream) {
  switch (a.DP) {
    case 32: return launch_ss_feat_w<32>(a, stream);
    case 48: return launch_ss_feat_w<48>(a, stream);
    case 64: return launch_ss_feat_w<64>(a, stream);
    case 80: return launch_ss_feat_w<80>(a, stream);
    case 96: return launch_ss_feat_w<96>(a, stream);
    case 112: return launch_ss_feat_w<112>(a, stream);
    case 128: return launch_ss_feat_w<128>(a, stream);
  }
  return hipErrorInvalidValue;
}

// ===========================================================================
// The list route of a skipping pass: per-quad row lists, one block per list
// ===========================================================================
// suffstat_feat_kernel<..., SPECK> decides what to skip per (4-row step, quad) inside a walk over ALL rows with all eight
// quads' accumulators live; once the rows are hard the work that matters is one (row, quad) pair per row.  Here a first
// kernel writes, per (row chunk, quad), the ascending list of the rows that keep a value of the quad, and a second one
// sums one list per block: the feature GEMM for NQ = 1 over gathered rows, all tiles of the width in one block (X staged
// once), no masks and no tests in the loop.  A cluster's accumulator sees its kept rows in ascending order, four per MFMA
// as ever -- the terms of the dense pass minus specks -- so the records equal those of the other skipping modes bit for bit
// wherever those equal the dense ones.
// -DLC_FT_SPECK_LISTS=0 (tools/variants.py): the context ignores the route
#ifndef LC_FT_SPECK_LISTS
#define LC_FT_SPECK_LISTS 1
#endif
#ifndef LC_FTL_BR
#define LC_FTL_BR 48  // rows per staged batch of the list kernel (64: the second buffer leaves the 16-bit offset of a ds_read)
#endif
// The list kernel's step reads the NEXT step's fragments while its MFMAs run.  LC_FTL_SPREAD = G > 0: the reads go out in
// G near-equal portions, one behind each of the step's first G MFMAs, in the order the next step's multiplies take them
// (ftl_read), so that a wave that pushes reads into the LDS queue keeps issuing MFMAs and the last MFMAs cover the last
// read's latency.  -DLC_FTL_SPREAD=0 (tools/variants.py): all of them in one burst ahead of the MFMAs, as before.
#ifndef LC_FTL_SPREAD
#define LC_FTL_SPREAD 12
#endif
// the r-th LDS read of a step: t >= 0: the `u` fragment of tile t; -1 - i: `w` fragment i (ahead of the first tile that
// multiplies by it); ftl_tpw: the step's q value, which the MFMAs need and no multiply does
__host__ __device__ constexpr int ftl_read(int DC, int r) {
  int n = 0;
  for (int t = 0; t < ftl_tpw(DC); ++t) {
    if (t == 0 || ftl_wi(DC, t) != ftl_wi(DC, t - 1)) {
      if (n == r) return -1 - ftl_wi(DC, t);
      ++n;
    }
    if (n == r) return t;
    ++n;
  }
  return ftl_tpw(DC);
}
bool speck_lists_enabled() { return LC_FT_SPECK_LISTS != 0; }
// Share of one-quad rows (in 64ths) from which a skipping pass takes the list route.  A row that keeps several quads is
// gathered and multiplied once per quad; with the other rows soft in EVERY quad the list pass loses to the sorted instance
// at 56 / 64 (11.19 against 10.61 ms at the north star) and wins at 58 / 64 (10.09 against 10.61): DESIGN 4.2b has the sweep.
#ifndef LC_FT_LIST_SHARE64
#define LC_FT_LIST_SHARE64 58
#endif
bool speck_probe_says_lists(int64_t single, int64_t rows) { return rows > 0 && 64 * single >= (int64_t)LC_FT_LIST_SHARE64 * rows; }
bool suffstat_list_instance(int DP, int DC) { return DP == 64 && (DC == 0 || DC == 64 || DC == 56); }

// One block per row chunk walks the chunk 256 rows at a time, quads in groups of 32 (128 columns of qZ, each read coalesced,
// every column once).  Per tile and quad: a ballot of the rows that keep the quad; the four waves' counts meet in LDS, lane c
// of every wave carries the running length of quad c's list, and a row's place is that base + the counts of the waves before
// its own + its rank in the ballot: ascending row order, no atomics at all.  A segment holds chunk_rows entries.
template <typename IT>
__global__ void __launch_bounds__(256) ss_list_build_kernel(const double* __restrict__ qZ, int64_t ldq, int K, int64_t NP,
                                                             int64_t chunk_rows, int nq, int* __restrict__ lens, IT* __restrict__ ent) {
  __shared__ int wcnt[2][32][4];
  const int chunk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)chunk * chunk_rows;
  const int64_t r1 = (r0 + chunk_rows) < NP ? (r0 + chunk_rows) : NP;
  if (r0 >= r1) {
    for (int c = tid; c < nq; c += 256) lens[(int64_t)chunk * nq + c] = 0;
    return;
  }
  for (int q0 = 0; q0 < nq; q0 += 32) {
    const int nqg = nq - q0 < 32 ? nq - q0 : 32;
    int base = 0, par = 0;
    for (int64_t t0 = r0; t0 < r1; t0 += 256, par ^= 1) {
      const int64_t row = t0 + tid;
      const bool valid = row < r1;
      const double* qr = qZ + (valid ? row : r1 - 1);  // (rows past the chunk: a valid address, the value is not used)
      unsigned m = 0;
      for (int c8 = 0; c8 < nqg; c8 += 8) {  // 32 loads in flight per thread
        double v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) {
          const int k = 4 * (q0 + c8) + i;
          v[i] = qr[(int64_t)(k < K ? k : K - 1) * ldq];
        }
#pragma unroll
        for (int i = 0; i < 32; ++i) {
          const int k = 4 * (q0 + c8) + i;
          if (valid && k < K && speck_keeps(v[i])) m |= 1u << (c8 + i / 4);
        }
      }
      int mycnt = 0;
      for (int c = 0; c < nqg; ++c) {
        const unsigned long long bal = __ballot((m >> c) & 1u);
        if (lane == c) mycnt = __popcll(bal);
      }
      if (lane < nqg) wcnt[par][lane][wave] = mycnt;
      __syncthreads();  // (one barrier per tile: the counts alternate between two buffers)
      int mybase = 0;
      if (lane < nqg) {
        int tot = 0, before = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const int n = wcnt[par][lane][w];
          before += w < wave ? n : 0;
          tot += n;
        }
        mybase = base + before;
        base += tot;
      }
      for (int c = 0; c < nqg; ++c) {
        const unsigned long long bal = __ballot((m >> c) & 1u);
        const int at = __shfl(mybase, c) + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
        if ((m >> c) & 1u) ent[((int64_t)chunk * nq + q0 + c) * chunk_rows + at] = (IT)(row - r0);
      }
    }
    if (wave == 0 && lane < nqg) lens[(int64_t)chunk * nq + q0 + lane] = base;
    __syncthreads();  // (the next group starts with the first count buffer again)
  }
}

// One block = one (row chunk, cluster quad): 8 waves, all tiles of the width (ftl_feature: at DC = 64 the shared deal, a
// wave's off-diagonal tiles are two stars that read their common factor once a step -- 22 fragment reads per 17 MFMAs where
// ft_deal_one's deal takes 35; the products, their order per accumulator and the records are the same bit for bit).
// A staged batch is LC_FTL_BR rows
// of the list: X rows gathered whole (row-major: one contiguous row each), the quad's four q values per row, zeros with
// q = 0 past the list's end.  The row offsets of a batch are fetched TWO batches ahead (their loads would otherwise stand
// in front of the gather's), the rows one batch ahead into registers.  Step loop: the step's products in one group (their
// fragments were read a whole step ahead), then its MFMAs with the next step's reads spread behind the first
// LC_FTL_SPREAD of them (ftl_read) -- one v_mul_f64 and one or two ds_read_b64 per MFMA, and nothing else.
template <int DP, int DC, typename IT>
__global__ void __launch_bounds__(512, 2) suffstat_list_kernel(SuffstatLaunch a, const int* __restrict__ lens, const IT* __restrict__ ent,
                                                                int nq) {
  static_assert(DC % 4 == 0 && DC <= DP && DC > DP - 16, "active width");
  constexpr int NTHR = 512, BR = LC_FTL_BR, LD = lds_row_stride(DP), QLD = 4, XBUF = BR * LD, QBUF = BR * QLD;
  constexpr int ONE = DP, NT = ftl_tpw(DC);
  constexpr int TPR = DP / 2, RPP = NTHR / TPR, NPRE = BR / RPP;
  static_assert(LD > DP && NTHR % TPR == 0 && BR % RPP == 0 && BR % 4 == 0 && 4 * BR <= NTHR, "staging");
  static_assert((XBUF + (BR - 4) * LD + LD) * 8 <= 65536, "fragment reads: one address register per tile, the rest immediate");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* xbuf = lds;             // [2][BR][LD]
  double* qbuf = lds + 2 * XBUF;  // [2][BR][4]: q[row][cluster of the quad], clusters past K zero
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 4, blk = (lane >> 2) & 3, lo2 = lane & 3;
  const int chunk = blockIdx.x / nq, quad = blockIdx.x % nq;
  const int64_t r0 = (int64_t)chunk * a.chunk_rows;
  const int len = lens[blockIdx.x];
  const IT* li = ent + (int64_t)blockIdx.x * a.chunk_rows;
  // the wave's tiles (ftl_feature): tile t multiplies fragment t of `u` by fragment ftl_wi(t) of `w` -- one per tile in
  // ft_deal_one's deal; in the shared deal one per star, read once a step, and one per free tile
  constexpr int NW = ftl_nw(DC);
  constexpr int NRD = NT + NW + 1, SPREAD = LC_FTL_SPREAD < 0 ? 0 : LC_FTL_SPREAD < NT ? LC_FTL_SPREAD : NT;  // (ftl_read)
  const double* pu[NT];
  const double* pw[NW];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const FtlFeature f = ftl_feature(DC, ONE, wave, t, lo2 + 4 * blk);
    pu[t] = xbuf + hi * LD + f.u;
    int ow = hi * LD + f.w;
    // (the shared deal: the two stars' fragments lie 32 columns apart and hipcc joins their reads into one ds_read2_b64,
    //  which takes 8 cycles of the LDS array where two ds_read_b64 take 4 -- the offset is hidden from it)
    if constexpr (ftl_shared(DC)) asm volatile("" : "+v"(ow));
    pw[ftl_wi(DC, t)] = xbuf + ow;
  }
  double acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = 0.0;

  const int xr0 = tid / TPR, xc2 = tid % TPR, qrow = tid / 4, qcl = tid % 4;
  const bool qthr = tid < 4 * BR;
  const int kq = 4 * quad + qcl;
  const double* qcol = a.qZ + (int64_t)(kq < a.K ? kq : a.K - 1) * a.ldq + r0;
  int xi[NPRE], qi = -1;
  double pre[NPRE][2], qpre = 0.0;
  // What a place past the list's end loaded becomes zero where the batch is STORED, a whole batch after its loads went
  // out: a select next to the load waits for the load, and the fences of the step loop keep that wait in front of the
  // batch's first MFMA -- the gather's whole latency, once per batch (LC_FTL_SPREAD = 0 selects there, as before).
  constexpr bool LATE = SPREAD != 0;
  bool xok[NPRE], qok = false;
  auto iload = [&](int p0) {  // list places p0 ... p0 + BR - 1 -> row offsets (-1 past the end)
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int p = p0 + xr0 + i * RPP;
      xi[i] = p < len ? (int)li[p] : -1;
    }
    qi = qthr && p0 + qrow < len ? (int)li[p0 + qrow] : -1;
  };
  auto gload = [&]() {  // (every load is issued: a place past the end reads the chunk's first row and keeps zeros)
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const double2 v = *reinterpret_cast<const double2*>(a.X + (r0 + (xi[i] < 0 ? 0 : xi[i])) * DP + 2 * xc2);
      xok[i] = xi[i] >= 0;
      pre[i][0] = LATE || xok[i] ? v.x : 0.0;
      pre[i][1] = LATE || xok[i] ? v.y : 0.0;
    }
    const double q = qcol[qi < 0 ? 0 : qi];
    qok = qi >= 0 && kq < a.K;
    qpre = LATE || qok ? q : 0.0;
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i)
      *reinterpret_cast<double2*>(xbuf + buf * XBUF + (xr0 + i * RPP) * LD + 2 * xc2) =
          make_double2(!LATE || xok[i] ? pre[i][0] : 0.0, !LATE || xok[i] ? pre[i][1] : 0.0);
    if (qthr) qbuf[buf * QBUF + qrow * QLD + qcl] = !LATE || qok ? qpre : 0.0;
  };
  if (tid < 2 * BR) xbuf[(tid / BR) * XBUF + (tid % BR) * LD + ONE] = 1.0;
  if (len > 0) {
    iload(0);
    gload();
    iload(BR);
    lstore(0);
  }
  __syncthreads();
  const double* pq = qbuf + hi * QLD + lo2;
  auto batch = [&](auto bsel) {
    constexpr int B = decltype(bsel)::value, XO = B * XBUF, QO = B * QBUF;
    double uf[NT], wf[NW], pp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) uf[t] = pu[t][XO];
#pragma unroll
    for (int i = 0; i < NW; ++i) wf[i] = pw[i][XO];
    double qa = pq[QO];
    // (the shared deal: without the fence hipcc joins every fragment's reads of steps 0 and 1 into a ds_read2st64_b64 --
    //  8 LDS cycles where two ds_read_b64 take 4, once per fragment and batch)
    if constexpr (ftl_shared(DC)) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int st = 0; st < BR / 4; ++st) {
#pragma unroll
      for (int t = 0; t < NT; ++t) pp[t] = uf[t] * wf[ftl_wi(DC, t)];
      const double qc = qa;
      if constexpr (SPREAD == 0) {
        if (st + 1 < BR / 4) {
#pragma unroll
          for (int t = 0; t < NT; ++t) uf[t] = pu[t][XO + (st + 1) * 4 * LD];
#pragma unroll
          for (int i = 0; i < NW; ++i) wf[i] = pw[i][XO + (st + 1) * 4 * LD];
          qa = pq[QO + (st + 1) * 4 * QLD];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma4(qc, pp[t], acc[t]);
        __builtin_amdgcn_sched_barrier(0);
      } else {
        // (uf and wf are dead once the products exist: the next step's fragments land in the same registers.  A fence
        //  per MFMA: the scheduler would otherwise gather the reads into one burst again)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          acc[t] = mfma4(qc, pp[t], acc[t]);
          if (st + 1 < BR / 4 && t < SPREAD) {
#pragma unroll
            for (int r = t * NRD / SPREAD; r < (t + 1) * NRD / SPREAD; ++r) {
              const int what = ftl_read(DC, r);
              if (what == NT)
                qa = pq[QO + (st + 1) * 4 * QLD];
              else if (what >= 0)
                uf[what] = pu[what][XO + (st + 1) * 4 * LD];
              else
                wf[-1 - what] = pw[-1 - what][XO + (st + 1) * 4 * LD];
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }
  };
  if constexpr (LATE) {
    // The next batch is fetched and stored whether it exists or not (past the list's end: the chunk's first row, stored as
    // zeros into a buffer nobody reads again).  Under a condition the offsets and rows in flight meet their old values
    // in register copies at the join, and a copy of a loaded register waits for every load in front of the batch.
    for (int p0 = 0; p0 < len; p0 += 2 * BR) {  // two batches per trip: the buffer index is a compile-time constant
      gload();
      iload(p0 + 2 * BR);
      batch(std::integral_constant<int, 0>{});
      lstore(1);
      __syncthreads();
      if (p0 + BR >= len) break;
      gload();
      iload(p0 + 3 * BR);
      batch(std::integral_constant<int, 1>{});
      lstore(0);
      __syncthreads();
    }
  } else {
    for (int p0 = 0; p0 < len; p0 += 2 * BR) {
      const bool more1 = p0 + BR < len, more2 = p0 + 2 * BR < len;
      if (more1) {
        gload();
        iload(p0 + 2 * BR);
      }
      batch(std::integral_constant<int, 0>{});
      if (more1) lstore(1);
      __syncthreads();
      if (!more1) break;
      if (more2) {
        gload();
        iload(p0 + 3 * BR);
      }
      batch(std::integral_constant<int, 1>{});
      if (more2) lstore(0);
      __syncthreads();
    }
  }

  // ---- partial records, as suffstat_feat_kernel writes them (an empty list: exact zeros)
  const int64_t SS = 1 + (int64_t)DP + (int64_t)DP * DP;
  int wv = wave;
  asm volatile("" : "+v"(wv));  // (the map is worked out again, not kept in registers across the step loop)
  const int kk = 4 * quad + hi;
  if (kk >= a.K) return;
  double* out = a.partial + ((int64_t)chunk * a.KR + kk) * SS;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const FtlFeature f = ftl_feature(DC, ONE, wv, t, lo2 + 4 * blk);
    if (f.kind == FT_SPARE) continue;
    const double v = acc[t];
    if (f.kind == FT_PRODUCT) {
      double* S = out + 1 + DP;
      S[(int64_t)f.u * DP + f.w] = v;
      S[(int64_t)f.w * DP + f.u] = v;
    } else if (f.kind == FT_LINEAR) {
      out[1 + f.u] = v;
    } else {
      out[0] = v;
    }
  }
}

// ---- hard rows at DC = DP = 64: one wave per cluster, the products on the VALU -------------------------------
// On a hard row one of a quad's four clusters holds a value and the MFMA's other three blocks multiply specks or zeros.  The
// fp64 MFMA adds a step's four rows to an accumulator as a chain in row order, rounding after each row, so for ONE cluster
// the accumulator of feature (u, w) receives, per kept row in ascending order, acc = fma(q, rnd(x_u x_w), acc): one
// v_mul_f64 and one v_fma_f64 per 64 features, no matrix pipe.
// One block = one (row chunk, cluster quad) as before, 4 waves, wave c = cluster 4 quad + c; the waves share nothing (no
// __syncthreads).  A wave walks the quad's list 64 places at a time: lane l loads entry p0 + l and the wave's own q at that
// row; a row is the wave's if speck_keeps(q) -- the rule is now per (listed row, cluster), DESIGN 4.4 -- and the kept rows of
// the ballot are taken in ascending order, offset and q through readlane, lane w loading X[row][w] (one 512-byte load).
// The deal is fto_feature's diagonals: the row goes to a wave-private LDS slot TWICE (128 doubles), so the rotated factor of
// accumulator t is slot[w + t] with t as the read's immediate offset.  The entries of a window are fetched two windows
// ahead and their q one ahead; the rows of LC_FTO_DEPTH kept places are in flight while the group before them is summed.
// -DLC_FTL_OWNER=0 (tools/variants.py): the list kernel at DC = 64 too, as before.
#ifndef LC_FTL_OWNER
#define LC_FTL_OWNER 1
#endif
#ifndef LC_FTO_DEPTH
#define LC_FTO_DEPTH 4  // rows of a group (two groups are in flight)
#endif
#ifndef LC_FTO_FUSED
#define LC_FTO_FUSED 1  // 0: rnd(q p) + acc in place of fma(q, p, acc)
#endif
bool suffstat_owner_instance(int DP, int DC) { return LC_FTL_OWNER != 0 && DP == 64 && (DC == 0 || DC == 64); }
template <int DP, int DC, typename IT>
__global__ void __launch_bounds__(256, 4) suffstat_owner_kernel(SuffstatLaunch a, const int* __restrict__ lens, const IT* __restrict__ ent,
                                                                 int nq) {
  static_assert(DP == 64 && DC == 64, "lane w owns column w");
  constexpr int G = LC_FTO_DEPTH, NSLOT = 2, ND = FTO_DIAGS;
  static_assert(G >= 1 && G <= 8, "rows in flight");
  __shared__ double slots[4][NSLOT][2 * DP];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int chunk = blockIdx.x / nq, quad = blockIdx.x % nq;
  const int k = 4 * quad + wave;
  if (k >= a.K) return;
  const int64_t r0 = (int64_t)chunk * a.chunk_rows;
  // (what the builders wrote: 0 <= len <= rows of the chunk, entries below that; clamped all the same, so that no
  //  address leaves X or qZ whatever the buffer holds)
  const int64_t rows64 = a.NP - r0 < a.chunk_rows ? a.NP - r0 : a.chunk_rows;
  const int rows = rows64 > 0 ? (int)rows64 : 0;
  int len = lens[blockIdx.x];
  len = len < 0 ? 0 : len > rows ? rows : len;
  const int nwin = (len + 63) / 64;
  const IT* li = ent + (int64_t)blockIdx.x * a.chunk_rows;
  const int64_t rb = rows > 0 ? r0 : 0;  // (a chunk behind the last row: nothing is summed, and nothing is read there)
  const double* qcol = a.qZ + (int64_t)k * a.ldq + rb;
  const double* xl = a.X + rb * DP + lane;
  double* slot = &slots[wave][0][lane];

  double acc[ND], lin = 0.0, cnt = 0.0;
#pragma unroll
  for (int t = 0; t < ND; ++t) acc[t] = 0.0;

  // windows: `cur` is summed, n1 has its q on the way, n2 its entries (a place past the end: offset 0, masked out)
  auto ld_off = [&](int w) {
    const int p = 64 * w + lane;
    const int o = p < len ? (int)li[p] : 0;
    return o < rows ? o : 0;
  };
  int widx = -1;
  unsigned long long mask = 0ull;
  int cur_off = 0, n1_off = ld_off(0), n2_off = ld_off(1);
  double cur_q = 0.0, n1_q = qcol[n1_off];
  auto advance = [&]() {
    ++widx;
    cur_off = n1_off, cur_q = n1_q;
    n1_off = n2_off;
    n1_q = qcol[n1_off];
    n2_off = ld_off(widx + 2);
    mask = __ballot(64 * widx + lane < len && speck_keeps(cur_q));
  };
  // the next G kept places (fewer at a window's end: a group lies within one window): every load is issued, a missing
  // place reads the chunk's first row and is not summed
  auto fetch = [&](double(&gx)[G], double(&gq)[G], int& n) {
    while (mask == 0ull && widx + 1 < nwin) advance();
    n = 0;
#pragma unroll
    for (int i = 0; i < G; ++i) {
      const bool has = mask != 0ull;
      const int l = has ? __builtin_ctzll(mask) : 0;
      mask &= mask - (has ? 1ull : 0ull);
      const int off = has ? __builtin_amdgcn_readlane(cur_off, l) : 0;
      gq[i] = readlane_f64(cur_q, l);
      gx[i] = xl[(int64_t)off * DP];
      n += has ? 1 : 0;
    }
  };
  auto row = [&](double x, double q, int s) {
    double* sl = slot + s * 2 * DP;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the slot's earlier reads stay in front of the stores)
    __builtin_amdgcn_wave_barrier();
    sl[0] = x;
    sl[DP] = x;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    double y[ND];
    y[0] = x;
#pragma unroll
    for (int t = 1; t < ND; ++t) {
      y[t] = sl[t];
      // (neighbouring reads would be joined into ds_read2_b64, which takes the LDS array twice as long as the two reads
      //  it replaces: an empty statement that may touch memory stands between them)
      asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int t = 0; t < ND; ++t) {
      const double p = x * y[t];
#if LC_FTO_FUSED
      acc[t] = fma(q, p, acc[t]);
#else
      acc[t] = __dadd_rn(__dmul_rn(q, p), acc[t]);
#endif
    }
#if LC_FTO_FUSED
    lin = fma(q, x, lin);
    cnt = fma(q, 1.0, cnt);
#else
    lin = __dadd_rn(__dmul_rn(q, x), lin);
    cnt = __dadd_rn(q, cnt);
#endif
  };
  auto sum = [&](const double(&gx)[G], const double(&gq)[G], int n) {
#pragma unroll
    for (int i = 0; i < G; ++i)
      if (i < n) row(gx[i], gq[i], i % NSLOT);
  };
  double ax[G], aq[G], bx[G], bq[G];
  int an = 0, bn = 0;
  fetch(ax, aq, an);
  while (an > 0) {
    fetch(bx, bq, bn);
    sum(ax, aq, an);
    if (bn == 0) break;
    fetch(ax, aq, an);
    sum(bx, bq, bn);
  }

  // ---- the cluster's partial record (an empty list, a cluster without kept rows: exact zeros); S_k from ONE accumulator
  // per pair, so it is exactly symmetric
  const int64_t SS = 1 + (int64_t)DP + (int64_t)DP * DP;
  double* out = a.partial + ((int64_t)chunk * a.KR + k) * SS;
  double* S = out + 1 + DP;
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    const FtFeature f = fto_feature(lane, t);
    if (f.kind == FT_PRODUCT) {
      S[f.u * DP + f.w] = acc[t];
      if (t != 0) S[f.w * DP + f.u] = acc[t];
    }
  }
  out[1 + fto_feature(lane, ND).u] = lin;
  if (fto_feature(lane, ND + 1).kind == FT_COUNT) out[0] = cnt;
}

// the checks both launchers share; *lay: the buffer's layout
static hipError_t ss_list_check(const SuffstatLaunch& a, const SuffstatPlan& p, const void* lists, size_t bytes, SsListLayout* lay) {
  if (a.K <= 0 || p.nchunks <= 0 || !lists || !a.qZ || !a.X) return hipErrorInvalidValue;
  if (p.route != SS_FEAT || a.mode != SS_DENSE || a.smask || a.items || p.extra != 0) return hipErrorInvalidValue;
  if (a.nchunks != p.nchunks || a.chunk_rows != p.chunk_rows || a.KR != p.KR || a.KR != a.K) return hipErrorInvalidValue;
  if (!suffstat_list_instance(a.DP, a.DC)) return hipErrorInvalidValue;
  if (a.chunk_rows < 4 || a.chunk_rows % 4 || a.chunk_rows > (int64_t)1 << 30 || (int64_t)a.nchunks * a.chunk_rows < a.NP) return hipErrorInvalidValue;
  *lay = ss_list_layout(a.nchunks, a.chunk_rows, a.K);
  if ((int64_t)a.nchunks * lay->nq > (int64_t)1 << 30 || bytes < lay->bytes) return hipErrorInvalidValue;
  return hipSuccess;
}
hipError_t launch_suffstat_list_build(const SuffstatLaunch& a, const SuffstatPlan& p, void* lists, size_t bytes, hipStream_t stream) {
  SsListLayout lay;
  if (hipError_t e = ss_list_check(a, p, lists, bytes, &lay); e != hipSuccess) return e;
  int* lens = static_cast<int*>(lists);
  void* ent = static_cast<char*>(lists) + lay.ent_off;
  if (lay.wide)
    hipLaunchKernelGGL(ss_list_build_kernel<unsigned>, dim3((unsigned)a.nchunks), dim3(256), 0, stream, a.qZ, a.ldq, a.K, a.NP,
                       a.chunk_rows, lay.nq, lens, static_cast<unsigned*>(ent));
  else
    hipLaunchKernelGGL(ss_list_build_kernel<unsigned short>, dim3((unsigned)a.nchunks), dim3(256), 0, stream, a.qZ, a.ldq, a.K, a.NP,
                       a.chunk_rows, lay.nq, lens, static_cast<unsigned short*>(ent));
  return hipGetLastError();
}
template <int DP, int DC, typename IT>
static hipError_t launch_ss_list_i(const SuffstatLaunch& a, const SsListLayout& lay, const void* lists, hipStream_t stream) {
  constexpr int BR = LC_FTL_BR;
  const size_t shmem = (size_t)(2 * BR * lds_row_stride(DP) + 2 * BR * 4) * sizeof(double);
  auto kern = suffstat_list_kernel<DP, DC, IT>;
  static LdsGrant grant;
  if (hipError_t e = grant_dynamic_lds(reinterpret_cast<const void*>(kern), shmem, grant); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.nchunks * lay.nq)), dim3(512), shmem, stream, a, static_cast<const int*>(lists),
                     reinterpret_cast<const IT*>(static_cast<const char*>(lists) + lay.ent_off), lay.nq);
  return hipGetLastError();
}
template <typename IT>
static hipError_t launch_ss_owner_i(const SuffstatLaunch& a, const SsListLayout& lay, const void* lists, hipStream_t stream) {
  hipLaunchKernelGGL((suffstat_owner_kernel<64, 64, IT>), dim3((unsigned)(a.nchunks * lay.nq)), dim3(256), 0, stream, a,
                     static_cast<const int*>(lists), reinterpret_cast<const IT*>(static_cast<const char*>(lists) + lay.ent_off), lay.nq);
  return hipGetLastError();
}
// the sums over lists that exist: DC = 64 the owner kernel (unless built with -DLC_FTL_OWNER=0), DC = 56 the list kernel
static hipError_t launch_ss_list_sums(const SuffstatLaunch& a, const SsListLayout& lay, const void* lists, hipStream_t stream) {
  if (a.DC == 56) return lay.wide ? launch_ss_list_i<64, 56, unsigned>(a, lay, lists, stream) : launch_ss_list_i<64, 56, unsigned short>(a, lay, lists, stream);
  if (suffstat_owner_instance(a.DP, a.DC)) return lay.wide ? launch_ss_owner_i<unsigned>(a, lay, lists, stream) : launch_ss_owner_i<unsigned short>(a, lay, lists, stream);
  return lay.wide ? launch_ss_list_i<64, 64, unsigned>(a, lay, lists, stream) : launch_ss_list_i<64, 64, unsigned short>(a, lay, lists, stream);
}
hipError_t launch_suffstat_lists(const SuffstatLaunch& a, const SuffstatPlan& p, void* lists, size_t bytes, hipStream_t stream) {
  SsListLayout lay;
  if (hipError_t e = ss_list_check(a, p, lists, bytes, &lay); e != hipSuccess) return e;
  if (hipError_t e = launch_suffstat_list_build(a, p, lists, bytes, stream); e != hipSuccess) return e;
  return launch_ss_list_sums(a, lay, lists, stream);
}

// ---- the lists from the kept-quad masks of the E-step that wrote qZ (EstepLaunch::qmask) ------------------------------------
// One block per (row chunk, cluster quad) walks the chunk's bits of the quad 4096 rows at a time: thread t takes the sixteen
// rows from r0 + 16 t on -- a chunk starts on a multiple of 4 rows, not of 16, so the sixteen bits come out of two words --,
// a popcount per thread, a scan over the wave and the four waves' totals through LDS give every kept row its place: ascending
// row order, no atomics, and qZ is not read (10 MB of masks against 2.56 GB at the north star).
template <typename IT>
__global__ void __launch_bounds__(256) ss_list_build_masks_kernel(const unsigned short* __restrict__ qmask, int64_t nrg, int64_t NP,
                                                                   int64_t chunk_rows, int nq, int* __restrict__ lens, IT* __restrict__ ent) {
  __shared__ int wcnt[2][4];
  const int chunk = blockIdx.x / nq, c = blockIdx.x % nq, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)chunk * chunk_rows;
  const int64_t r1 = (r0 + chunk_rows) < NP ? (r0 + chunk_rows) : NP;
  if (r0 >= r1) {
    if (tid == 0) lens[blockIdx.x] = 0;
    return;
  }
  const unsigned short* mq = qmask + (int64_t)c * nrg;
  IT* seg = ent + (int64_t)blockIdx.x * chunk_rows;
  int base = 0, par = 0;
  for (int64_t t0 = r0; t0 < r1; t0 += 4096, par ^= 1) {
    const int64_t row = t0 + 16 * tid;
    unsigned m = 0;
    if (row < r1) {  // (row < NP <= 16 nrg: the first word exists; the second one only where it is needed)
      const int64_t w = row >> 4;
      const unsigned sh = (unsigned)(row & 15);
      const unsigned lo = mq[w], hi = sh != 0 && w + 1 < nrg ? mq[w + 1] : 0u;
      m = ((lo | (hi << 16)) >> sh) & 0xffffu;
      if (r1 - row < 16) m &= (1u << (unsigned)(r1 - row)) - 1u;
    }
    const int cnt = __popc(m);
    int inc = cnt;  // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(inc, d);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wcnt[par][wave] = inc;
    __syncthreads();  // (one barrier per tile: the counts alternate between two buffers)
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int n = wcnt[par][w];
      before += w < wave ? n : 0;
      tot += n;
    }
    int at = base + before + inc - cnt;
    while (m) {
      const int i = __ffs((int)m) - 1;
      m &= m - 1;
      seg[at++] = (IT)(row - r0 + i);
    }
    base += tot;
  }
  if (tid == 0) lens[blockIdx.x] = base;
}
// the rule itself: the masks of what a qZ buffer holds (one thread per (row, quad); a wave's ballot is four words)
__global__ void __launch_bounds__(256) qmask_from_qz_kernel(const double* __restrict__ qZ, int64_t ldq, int K, int64_t nrg,
                                                             unsigned short* __restrict__ qmask) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y, lane = threadIdx.x & 63;
  bool keep = false;
  if (row < nrg * RG) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = 4 * c + i;
      if (k < K && speck_keeps(qZ[(int64_t)k * ldq + row])) keep = true;
    }
  }
  const unsigned long long b = __ballot(keep);
  if ((lane & 15) == 0 && row < nrg * RG) qmask[(int64_t)c * nrg + (row >> 4)] = (unsigned short)((b >> lane) & 0xffffull);
}
hipError_t launch_qmask_from_qz(const double* qZ, int64_t ldq, int K, int64_t nrg, unsigned short* qmask, hipStream_t stream) {
  if (!qZ || !qmask || K < 1 || nrg < 1 || ldq < nrg * RG || (K + 3) / 4 > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(qmask_from_qz_kernel, dim3((unsigned)((nrg * RG + 255) / 256), (unsigned)((K + 3) / 4)), dim3(256), 0, stream, qZ, ldq,
                     K, nrg, qmask);
  return hipGetLastError();
}
hipError_t launch_suffstat_list_build_masks(const SuffstatLaunch& a, const SuffstatPlan& p, const unsigned short* qmask, int64_t nrg,
                                            void* lists, size_t bytes, hipStream_t stream) {
  SsListLayout lay;
  if (hipError_t e = ss_list_check(a, p, lists, bytes, &lay); e != hipSuccess) return e;
  if (!qmask || nrg * RG < a.NP) return hipErrorInvalidValue;
  int* lens = static_cast<int*>(lists);
  void* ent = static_cast<char*>(lists) + lay.ent_off;
  const dim3 grid((unsigned)(a.nchunks * lay.nq));
  if (lay.wide)
    hipLaunchKernelGGL(ss_list_build_masks_kernel<unsigned>, grid, dim3(256), 0, stream, qmask, nrg, a.NP, a.chunk_rows, lay.nq, lens,
                       static_cast<unsigned*>(ent));
  else
    hipLaunchKernelGGL(ss_list_build_masks_kernel<unsigned short>, grid, dim3(256), 0, stream, qmask, nrg, a.NP, a.chunk_rows, lay.nq, lens,
                       static_cast<unsigned short*>(ent));
  return hipGetLastError();
}
hipError_t launch_suffstat_lists_masks(const SuffstatLaunch& a, const SuffstatPlan& p, const unsigned short* qmask, int64_t nrg,
                                       void* lists, size_t bytes, hipStream_t stream) {
  SsListLayout lay;
  if (hipError_t e = launch_suffstat_list_build_masks(a, p, qmask, nrg, lists, bytes, stream); e != hipSuccess) return e;
  if (hipError_t e = ss_list_check(a, p, lists, bytes, &lay); e != hipSuccess) return e;
  return launch_ss_list_sums(a, lay, lists, stream);
}

// ===========================================================================
// Sufficient statistics for FEW clusters (K <= 16) at D <= 64: four clusters in the four blocks of one MFMA (round 6)
// ===========================================================================
// Few clusters leave both forms above short of operands to share: suffstat_kernel forms q_k x per cluster and 16 x 16
// block (D = 32: five fp64 VALU instructions per ten MFMAs), the feature GEMM shares one product among NQ <= 4 cluster
// quads and reads two LDS fragments for it (NQ = 2: the LDS port is the bound).  Here the MFMA's four blocks are the four
// CLUSTERS of a quad and its output tile a 4 x 4 patch of the scatter matrix:
//   A operand = x[row 4 st + hi][4 ia + lo2]                        (the same in all four blocks: one LDS read per ia and step)
//   B operand = q[row 4 st + hi][cluster 4 c + blk] * x[row][4 ja + lo2]   (ONE v_mul_f64 per ja and step, used by ja + 1 patches;
//                                                                    s_k adds the same product up on the VALU)
//   D[i = hi][j = lo2] of block blk = S_{4c + blk}[4 ia + hi][4 ja + lo2]
// -- NT multiplies, NT + 1 additions and NT + 1 LDS reads per NT (NT + 1) / 2 MFMAs and step (D = 48: 25 : 78, D = 24: 13 : 21), no
// rotated reads, cross-lane sums in the epilogue only.  A quad's work list (patches ia <= ja in ja-major order, each ja followed by its s_k
// tile, N_k last) is cut into NPART contiguous parts of equal length, one wave each: K <= 4 runs as 4 parts, K <= 8 as 2 x 2,
// 12 as 3 x 4 (three blocks per row chunk), 16 as 4 x 1 (D <= 32) or 4 x 2; D = 64 always in 4 parts (39 accumulators).  Same staging, chunks, partial records and
// fixed-order reduction as the other two kernels; a diagonal patch stores its lower triangle only (and mirrors it): the two
// halves come from differently rounded products, and the host reads the lower triangle.  Dense only.
struct SqItem {
  int kind, ia, ja;  // kind 0: patch (ia, ja); 1: s_k tile of ja; 2: N_k
};
__host__ __device__ constexpr int sq_items(int DC) { return (DC / 4) * (DC / 4 + 1) / 2 + DC / 4 + 1; }
__host__ __device__ constexpr SqItem sq_item(int DC, int n) {
  for (int ja = 0; ja < DC / 4; ++ja) {
    if (n <= ja) return SqItem{0, n, ja};
    n -= ja + 1;
    if (n == 0) return SqItem{1, 0, ja};
    n -= 1;
  }
  return SqItem{2, 0, 0};
}
__host__ __device__ constexpr int sq_part_lo(int DC, int NPART, int p) { return (sq_items(DC) * p + NPART - 1) / NPART; }
__host__ __device__ constexpr int sq_part_max(int DC, int NPART) {
  int m = 0;
  for (int p = 0; p < NPART; ++p) {
    const int n = sq_part_lo(DC, NPART, p + 1) - sq_part_lo(DC, NPART, p);
    m = n > m ? n : m;
  }
  return m;
}
constexpr int SQ_BR = 32, SQ_QLD = 18;  // (rows per staged batch: 16 measures 1-7 % slower, 64 3-20 % -- the blocks a CU holds)
inline int sq_npart(int DP, int K) {  // parts per cluster quad (the instances launch_ss_quad has)
  const int nq = (K + 3) / 4;
  if (DP > 48) return 4;  // (D = 64: two parts per quad need more than 256 registers)
  return nq == 2 ? 2 : nq == 4 ? (DP <= 32 ? 1 : 2) : 4;
}
inline int sq_nslice(int DP, int K) { return (((K + 3) / 4) * sq_npart(DP, K) + 3) / 4; }
inline bool ss_quad_eligible(int DP, int K) {
  // (tests, libcluster_hip_testhooks.so only: 0 never, 1 wherever an instance exists)
  static const int mode = test_switch("LC_SS_QUAD") ? atoi(test_switch("LC_SS_QUAD")) : -1;
  if (mode == 0 || DP < 32 || DP > 64 || K < 1 || K > 16) return false;
  if (mode == 1) return true;
  // a quad's four MFMA blocks are four clusters whether they exist or not: K = 2 does twice the work of the per-cluster
  // kernel and loses (D = 64: 1.30 against 0.98 ms at N = 4M; cluster()'s two-cluster sub-problems: 403 launches, 107 against
  // 73 ms); from three clusters on the form wins although blocks idle (D = 48, K = 5: 1.76 against 2.04 ms, D = 32, K = 6:
  // 1.10 against 1.28; gpurun_out/r06i)
  return K >= 3;
}
template <int DP, int DC, int NPART>
__global__ void __launch_bounds__(256, 2) suffstat_quad_kernel(SuffstatLaunch a) {
  static_assert(DC % 4 == 0 && DC <= DP && DC > DP - 16, "active width");
  constexpr int NT = DC / 4, BR = SQ_BR, LD = lds_row_stride(DP), QLD = SQ_QLD, XBUF = BR * LD, QBUF = BR * QLD, NTHR = 256;
  constexpr int NACC = sq_part_max(DC, NPART);
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* xbuf = lds;             // [2][BR][LD]
  double* qbuf = lds + 2 * XBUF;  // [2][BR][QLD]: q[row][cluster], clusters past K zero
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 4, blk = (lane >> 2) & 3, lo2 = lane & 3;
  const int K = a.K, NQ = (K + 3) / 4;
  int chunk, slice;
  {  // (chunk, slice) placement as in suffstat_kernel: the slices of a chunk back-to-back on one XCD
    const int nslice = a.nslice, nchunks = a.nchunks, b = blockIdx.x, full = (nchunks / 8) * 8;
    if (b < full * nslice) {
      const int xcd = b & 7, seq = b >> 3;
      chunk = (seq / nslice) * 8 + xcd;
      slice = seq % nslice;
    } else {
      const int t = b - full * nslice;
      chunk = full + t / nslice;
      slice = t % nslice;
    }
  }
  const int64_t r0 = (int64_t)chunk * a.chunk_rows;
  const int64_t r1 = (r0 + a.chunk_rows) < a.NP ? (r0 + a.chunk_rows) : a.NP;
  const int unit = slice * 4 + wave, quad = unit / NPART, part = unit % NPART;
  const bool busy = quad < NQ;

  // ---- staging (as suffstat_feat_kernel): registers hold the next batch while the current one is consumed
  constexpr int TPR = DP / 2, NV2 = BR * TPR, NPRE = (NV2 + NTHR - 1) / NTHR;
  double pre[NPRE][2], qpre[4];
  const int qcl = tid % 16, qrq = tid / 16;
  const bool qthr = qrq < BR / 4;
  auto gload = [&](int64_t b0) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int idx = tid + i * NTHR;
      const int row = idx / TPR, c2 = idx % TPR;
      double2 v = make_double2(0.0, 0.0);
      if (row < BR && b0 + row < r1) v = *reinterpret_cast<const double2*>(a.X + (b0 + row) * DP + 2 * c2);
      pre[i][0] = v.x;
      pre[i][1] = v.y;
    }
    const int64_t qrow = b0 + 4 * qrq;
#pragma unroll
    for (int i = 0; i < 4; ++i) qpre[i] = 0.0;
    if (qthr && qcl < K && qrow < r1) {  // (a row quad lies inside the chunk or outside it: chunk_rows is a multiple of 4)
      const double2* qp = reinterpret_cast<const double2*>(a.qZ + (int64_t)qcl * a.ldq + qrow);
      const double2 v0 = qp[0], v1 = qp[1];
      qpre[0] = v0.x, qpre[1] = v0.y, qpre[2] = v1.x, qpre[3] = v1.y;
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NPRE; ++i) {
      const int idx = tid + i * NTHR;
      const int row = idx / TPR, c2 = idx % TPR;
      if (row < BR) *reinterpret_cast<double2*>(xbuf + buf * XBUF + row * LD + 2 * c2) = make_double2(pre[i][0], pre[i][1]);
    }
    if (qthr) {
#pragma unroll
      for (int i = 0; i < 4; ++i) qbuf[buf * QBUF + (4 * qrq + i) * QLD + qcl] = qpre[i];
    }
  };

  double acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
  const double* px = xbuf + hi * LD + lo2;
  const double* pq = qbuf + hi * QLD + 4 * (busy ? quad : 0) + blk;

  // one part's work on one staged batch (buffer B): all BR / 4 steps run (rows past the chunk end were staged as zeros with
  // q = 0).  The next step's fragments are read before this step's MFMAs (two register sets); the products stand together
  // in front of them (a VALU instruction next to the matrix pipe is paid per switch).
  auto batch = [&](auto bsel, auto psel) {
    constexpr int B = decltype(bsel)::value, P = decltype(psel)::value, XO = B * XBUF, QO = B * QBUF;
    constexpr int LO = sq_part_lo(DC, NPART, P), HI = sq_part_lo(DC, NPART, P + 1);
    constexpr int JA0 = sq_item(DC, LO).kind == 2 ? NT - 1 : sq_item(DC, LO).ja;
    constexpr int JA1 = sq_item(DC, HI - 1).kind == 2 ? NT - 1 : sq_item(DC, HI - 1).ja;  // fragments 0 .. JA1, products JA0 .. JA1
    double xa[2][JA1 + 1], qa[2];
#pragma unroll
    for (int t = 0; t <= JA1; ++t) xa[0][t] = px[XO + 4 * t];
    qa[0] = pq[QO];
#pragma unroll
    for (int st = 0; st < BR / 4; ++st) {
      const int cur = st & 1, nxt = cur ^ 1;
      double pr[JA1 - JA0 + 1];
#pragma unroll
      for (int j = JA0; j <= JA1; ++j) pr[j - JA0] = qa[cur] * xa[cur][j];
      if (st + 1 < BR / 4) {
#pragma unroll
        for (int t = 0; t <= JA1; ++t) xa[nxt][t] = px[XO + (st + 1) * 4 * LD + 4 * t];
        qa[nxt] = pq[QO + (st + 1) * 4 * QLD];
      }
      // s_k and N_k on the VALU, next to the products (one v_add_f64 each: as MFMA tiles they were 7 of 28 matrix
      // instructions at D = 24, 13 of 91 at D = 48); the four hi lanes' partial sums meet in the epilogue
      static_for<HI - LO>([&](auto ic) {
        constexpr SqItem it = sq_item(DC, LO + ic);
        if constexpr (it.kind == 1) acc[ic] += pr[it.ja - JA0];
        else if constexpr (it.kind == 2) acc[ic] += qa[cur];
      });
      __builtin_amdgcn_sched_barrier(0);
      static_for<HI - LO>([&](auto ic) {
        constexpr SqItem it = sq_item(DC, LO + ic);
        if constexpr (it.kind == 0) acc[ic] = mfma4(xa[cur][it.ia], pr[it.ja - JA0], acc[ic]);
      });
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto run = [&](auto psel) {
    if (r0 < r1) {
      gload(r0);
      lstore(0);
    }
    __syncthreads();
    for (int64_t b0 = r0; b0 < r1; b0 += 2 * BR) {  // two batches per trip: the buffer index is a compile-time constant
      const bool more1 = b0 + BR < r1, more2 = b0 + 2 * BR < r1;
      if (more1) gload(b0 + BR);
      if (busy) batch(std::integral_constant<int, 0>{}, psel);
      if (more1) lstore(1);
      __syncthreads();
      if (!more1) break;
      if (more2) gload(b0 + 2 * BR);
      if (busy) batch(std::integral_constant<int, 1>{}, psel);
      if (more2) lstore(0);
      __syncthreads();
    }
    if (!busy) return;
    // ---- partial records: [N_k, s_k[DP], S_k[DP x DP]] per (chunk, cluster), as the other kernels write them
    constexpr int P = decltype(psel)::value, LO = sq_part_lo(DC, NPART, P), HI = sq_part_lo(DC, NPART, P + 1);
    const int kk = 4 * quad + blk;
    if (kk >= K) return;
    const int64_t SS = 1 + (int64_t)DP + (int64_t)DP * DP;
    double* out = a.partial + ((int64_t)chunk * a.KR + kk) * SS;
    double* S = out + 1 + DP;
    static_for<HI - LO>([&](auto ic) {
      constexpr SqItem it = sq_item(DC, LO + ic);
      const double v = acc[ic];
      if constexpr (it.kind == 0) {
        const int gi = 4 * it.ia + hi, gj = 4 * it.ja + lo2;
        if constexpr (it.ia == it.ja) {
          if (hi >= lo2) S[(int64_t)gi * DP + gj] = v;   // lower triangle of the diagonal patch ...
          if (hi > lo2) S[(int64_t)gj * DP + gi] = v;    // ... and its mirror image
        } else {
          S[(int64_t)gi * DP + gj] = v;
          S[(int64_t)gj * DP + gi] = v;
        }
      } else if constexpr (it.kind == 1) {
        const double t = sum_over_hi(v);
        if (hi == 0) out[1 + 4 * it.ja + lo2] = t;
      } else {
        const double t = sum_over_hi(v);
        if (hi == 0 && lo2 == 0) out[0] = t;
      }
    });
  };
  if constexpr (NPART == 1) {
    run(std::integral_constant<int, 0>{});
  } else if constexpr (NPART == 2) {
    if (part == 0) run(std::integral_constant<int, 0>{});
    else run(std::integral_constant<int, 1>{});
  } else {
    static_assert(NPART == 4, "parts per quad");
    if (part == 0) run(std::integral_constant<int, 0>{});
    else if (part == 1) run(std::integral_constant<int, 1>{});
    else if (part == 2) run(std::integral_constant<int, 2>{});
    else run(std::integral_constant<int, 3>{});
  }
}

// the instance <DP, DC, NPART> of a shape, handed to f as three integral constants (only the instances sq_npart can ask for exist)
template <int DP, int DC, class F>
static hipError_t sq_instance_d(int K, F& f) {
  const int np = sq_npart(DP, K);
  using dp = std::integral_constant<int, DP>;
  using dc = std::integral_constant<int, DC>;
  if constexpr (DP <= 32) {
    if (np == 1) return f(dp{}, dc{}, std::integral_constant<int, 1>{});
  }
  if constexpr (DP <= 48) {
    if (np == 2) return f(dp{}, dc{}, std::integral_constant<int, 2>{});
  }
  return np == 4 ? f(dp{}, dc{}, std::integral_constant<int, 4>{}) : hipErrorInvalidValue;
}
template <int DP, class F>
static hipError_t sq_instance_w(int DC, int K, F& f) {
  if constexpr (DP <= 48) {
    if (DC == DP - 4) return sq_instance_d<DP, DP - 4>(K, f);
    if (DC == DP - 12) return sq_instance_d<DP, DP - 12>(K, f);
  }
  if (DC == DP - 8) return sq_instance_d<DP, DP - 8>(K, f);
  if (DC != 0 && DC != DP) return hipErrorInvalidValue;
  return sq_instance_d<DP, DP>(K, f);
}
template <class F>
static hipError_t sq_instance(int DP, int DC, int K, F f) {
  switch (DP) {
    case 32: return sq_instance_w<32>(DC, K, f);
    case 48: return sq_instance_w<48>(DC, K, f);
    case 64: return sq_instance_w<64>(DC, K, f);
  }
  return hipErrorInvalidValue;
}
static size_t sq_lds_bytes(int DP) { return (size_t)(2 * SQ_BR * lds_row_stride(DP) + 2 * SQ_BR * SQ_QLD) * sizeof(double); }
static hipError_t launch_ss_quad(const SuffstatLaunch& a, hipStream_t stream) {
  return sq_instance(a.DP, a.DC, a.K, [&](auto dp, auto dc, auto np) {
    auto kern = suffstat_quad_kernel<decltype(dp)::value, decltype(dc)::value, decltype(np)::value>;
    const size_t shmem = sq_lds_bytes(a.DP);
    static LdsGrant grant;
    if (hipError_t e = grant_dynamic_lds(reinterpret_cast<const void*>(kern), shmem, grant); e != hipSuccess) return e;
    SuffstatLaunch b = a;
    b.nslice = sq_nslice(a.DP, a.K);
    hipLaunchKernelGGL(kern, dim3((unsigned)(b.nchunks * b.nslice)), dim3(256), shmem, stream, b);
    return hipGetLastError();
  });
}
// resident blocks per CU of the instance a shape takes (suffstat_plan's fill search): the runtime is asked once per instance
static int sq_blocks_per_cu(int DP, int DC, int K) {
  static std::atomic<int> cache[8 * 16 * 4];  // [layout][active-width step][parts]
  const int np = sq_npart(DP, K);
  std::atomic<int>& slot = cache[((DP / 16) % 8) * 64 + (((DP - DC) / 4) % 16) * 4 + (np == 1 ? 0 : np == 2 ? 1 : 2)];
  int per_cu = slot.load(std::memory_order_relaxed);
  if (per_cu > 0) return per_cu;
  const hipError_t e = sq_instance(DP, DC, K, [&](auto dp, auto dc, auto npc) {
    auto kern = suffstat_quad_kernel<decltype(dp)::value, decltype(dc)::value, decltype(npc)::value>;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, sq_lds_bytes(DP));  // (below 64 KB: no grant needed)
  });
  if (e != hipSuccess || per_cu < 1) per_cu = 2;
  slot.store(per_cu, std::memory_order_relaxed);
  return per_cu;
}

template <int DP>
struct SSCfg;
template <>
struct SSCfg<16> { static constexpr int CPW = 4; };
template <>
struct SSCfg<32> { static constexpr int CPW = 4; };
template <>
struct SSCfg<48> { static constexpr int CPW = 2; };  // (four clusters per wave spill at the 256-register budget)
template <>
struct SSCfg<64> { static constexpr int CPW = 2; };
template <>
struct SSCfg<80> { static constexpr int CPW = 1; };
template <>
struct SSCfg<96> { static constexpr int CPW = 1; };
template <>
struct SSCfg<128> { static constexpr int CPW = 1; };

static int ss_cpw(int DP, int K) {
  int cpw = DP == 16 ? SSCfg<16>::CPW : DP == 32 ? SSCfg<32>::CPW : DP == 48 ? SSCfg<48>::CPW : DP == 64 ? SSCfg<64>::CPW
                                                                                             : SSCfg<128>::CPW;  // (96, 128)
  // few clusters: spread them over more waves instead of stacking them in one
  while (cpw > 1 && (K + cpw - 1) / cpw < 4 && (K + cpw / 2 - 1) / (cpw / 2) <= 4) cpw /= 2;
  return cpw;
}

// row classes for a last slice with `active` of its four waves in use
static int ss_row_classes(int active) { return active == 1 ? 4 : active == 2 ? 2 : 1; }

// rec[(klast0 + e % nlast) * SS + i] += rec[(K + e) * SS + i], e = 0 .. extra-1 in order (deterministic)
__global__ void __launch_bounds__(256) fold_extra_kernel(double* rec, int64_t SS, int K, int klast0, int extra) {
  const int nlast = K - klast0;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)nlast * SS) return;
  const int kk = (int)(t / SS);
  const int64_t i = t % SS;
  double v = rec[(int64_t)(klast0 + kk) * SS + i];
  for (int e = kk; e < extra; e += nlast) v += rec[(int64_t)(K + e) * SS + i];
  rec[(int64_t)(klast0 + kk) * SS + i] = v;
}
hipError_t launch_fold_extra(double* rec, int64_t SS, int K, int klast0, int extra, hipStream_t stream) {
  if (extra <= 0) return hipSuccess;
  const int64_t n = (int64_t)(K - klast0) * SS;
  hipLaunchKernelGGL(fold_extra_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, rec, SS, K, klast0, extra);
  return hipGetLastError();
}

SuffstatPlan suffstat_plan(int DP, int DC, int64_t NP, int K, SuffstatMode mode) {
  SuffstatPlan p{SS_PER_CLUSTER, 0, 0, 0, K, K, 4, "suffstat_kernel"};
  if (K < 1 || NP < 1) return p;
  if (DC <= 0) DC = DP;
  // The kernel this SHAPE is eligible for -- the route of its dense pass.  The other modes run the per-cluster kernel, and
  // at a quad- or feature-eligible shape they run it on the chunking computed below as if the eligible kernel ran, and
  // without the row split of a ragged last slice (a masked dense pass elsewhere keeps the split): kept as it was found,
  // not a measured choice (open question).
  const bool wide = DP > 128, quad = !wide && ss_quad_eligible(DP, K), feat = !wide && !quad && ss_feat_eligible(DP, K, DC);
  p.route = wide ? SS_WIDE : mode != SS_DENSE ? SS_PER_CLUSTER : quad ? SS_QUAD : feat ? SS_FEAT : SS_PER_CLUSTER;
  p.name = p.route == SS_QUAD ? "suffstat_quad_kernel" : p.route == SS_FEAT ? "suffstat_feat_kernel" : "suffstat_kernel";
  const int cpw = wide ? 1 : ss_cpw(DP, K);  // wide: panel launches, one cluster per wave
  p.clusters_per_block = 4 * cpw;
  const int kwaves = (K + cpw - 1) / cpw;  // waves needed to cover the clusters
  if (!wide && !quad && !feat && (mode == SS_DENSE || mode == SS_MASKED_DENSE)) {  // (whole quads / any K of a range: no ragged last slice)
    const int nslice = (kwaves + 3) / 4, rs = ss_row_classes(kwaves - (nslice - 1) * 4);
    if (rs > 1) {
      p.klast0 = (nslice - 1) * 4 * cpw;
      p.extra = (rs - 1) * (K - p.klast0);
    }
  }
  p.KR = K + p.extra;
  // aim for ~8 waves per CU on 256 CUs, at least 256 rows per chunk
  int64_t want = (256 * 8 + kwaves - 1) / kwaves;
  if (quad) want = (256 * 8 / 4 + sq_nslice(DP, K) - 1) / sq_nslice(DP, K);  // blocks of four waves, nslice per chunk
  // four blocks per resident slot: the hardware back-fills slots as blocks retire, which evens out the
  // per-CU / per-XCD speed differences (measured 25.7 -> 24.9 ms at N=10M, D=64, K=32), while the partial
  // records (chunks x K x (1 + DP + DP^2) doubles) stay below 1 GiB
  const int rounds = 4;
  const int64_t rec = (int64_t)K * (1 + DP + (int64_t)DP * DP) * 8;
  // (wide records are large: allow 4 GiB of them so that the grid still covers the chip)
  const int64_t cap = ((int64_t)(wide ? 4 : 1) << 30) / rec;
  if (want * rounds <= cap) want *= rounds;
  else if (want < cap) want = cap;
  else if (want > cap && wide) want = cap > 1 ? cap : 1;
  // at least 1024 rows per chunk where that still leaves two chunks per CU (a chunk's K records are written and read
  // back by the reduction: at 256 rows they are half of a two-cluster sub-problem's traffic), 256 rows otherwise
  int64_t maxchunks = std::max<int64_t>((NP + 1023) / 1024, std::min<int64_t>((NP + 255) / 256, 512));
  if (want > maxchunks) want = maxchunks;
  if (want < 1) want = 1;
  auto plan = [&](int64_t w, int64_t* rows_out) {
    int64_t rows = (NP + w - 1) / w;
    rows = (rows + SS_BR - 1) / SS_BR * SS_BR;  // whole staging batches
    *rows_out = rows;
    return (NP + rows - 1) / rows;
  };
  int64_t rows = 0;
  int64_t n = plan(want, &rows);
  // share of the last round's resident slots that a grid of `chunks` x nslice blocks fills
  auto fill = [](int64_t chunks, int nslice, int64_t slots) {
    const int64_t blocks = chunks * nslice, rounds = (blocks + slots - 1) / slots;
    return (double)blocks / (double)(rounds * slots);
  };
  // Feature-GEMM launches put nslice blocks on every chunk and one (8 waves) or two (4 waves) blocks on a CU: a grid
  // whose last round of resident blocks is half empty loses that much of the launch.  Config 5 (D = 128, K = 64: 17 blocks
  // per chunk) ran 127 chunks = 2159 blocks = 8.43 rounds of 256 -- 6 % of the pass idle; 120 chunks are 7.97 rounds.
  // Among the chunk counts down to 80 % of the wanted one, take the fullest last round (the larger count on ties).
  if (feat && NP >= 64 * 1024) {
    const int range = ft_range(DP, K);
    const int nslice = ft_nslice(DP, DC, ft_instance_quads(((K < range ? K : range) + 3) / 4));
    if (nslice > 0) {
      const int64_t slots = (int64_t)current_device_cus() * (ft_waves(DP) == 8 ? 1 : 2);
      double best = fill(n, nslice, slots);
      for (int64_t w = want - 1; w >= 1 && w * 5 >= want * 4 && best < 0.985; --w) {
        int64_t r2 = 0;
        const int64_t n2 = plan(w, &r2);
        if (fill(n2, nslice, slots) > best + 1e-9) best = fill(n2, nslice, slots), n = n2, rows = r2;
      }
    }
  }
  // ... and the few-cluster kernel (sq_nslice blocks per chunk, 2 - 4 resident per CU): N = 5M, D = 48, K = 12 ran 684 chunks = 2052
  // blocks = 2.67 rounds of 768
  if (quad && NP >= 64 * 1024) {
    const int nslice = sq_nslice(DP, K);
    const int64_t slots = (int64_t)current_device_cus() * sq_blocks_per_cu(DP, DC, K);
    // (chunk counts from 80 % to 125 % of the wanted one, the nearest first: three blocks per chunk on 768 slots have no
    //  full round between 512 and 768 chunks)
    double best = fill(n, nslice, slots);
    for (int64_t d = 1; best < 0.985 && d * 4 <= want; ++d)
      for (int sgn = -1; sgn <= 1; sgn += 2) {
        const int64_t w = want + sgn * d;
        if (w < 1 || (sgn < 0 && w * 5 < want * 4) || w > maxchunks || (sgn > 0 && w > cap)) continue;  // (cap: the partial records' memory)
        int64_t r2 = 0;
        const int64_t n2 = plan(w, &r2);
        if (fill(n2, nslice, slots) > best + 1e-9) best = fill(n2, nslice, slots), n = n2, rows = r2;
      }
  }
  p.nchunks = (int)n;
  p.chunk_rows = rows;
  return p;
}

template <int DP, int CPW, bool SKIP, int HALF, int PAN = 0, bool RSP = false>
static hipError_t launch_ss_k(const SuffstatLaunch& b, unsigned grid, hipStream_t stream) {
  const int wpb = 4;
  constexpr int BR = ss_batch_rows<PAN>();
  const size_t shmem = (size_t)(2 * (PAN == 2 ? 2 : 1) * BR * lds_row_stride(DP) + 2 * wpb * CPW * BR) * sizeof(double);
  auto kern = suffstat_kernel<DP, CPW, SKIP, HALF, PAN, RSP>;
  static LdsGrant grant;
  if (hipError_t e = grant_dynamic_lds(reinterpret_cast<const void*>(kern), shmem, grant); e != hipSuccess) return e;
  if (grid == 0) return hipSuccess;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(wpb * 64), shmem, stream, b);
  return hipGetLastError();
}

template <int DP, int CPW, bool SKIP, int HALF, int PAN = 0>
static hipError_t launch_ss_h(const SuffstatLaunch& a, hipStream_t stream) {
  const int kwaves = (a.K + CPW - 1) / CPW;
  const int wpb = 4;
  const int nslice = (kwaves + wpb - 1) / wpb;
  SuffstatLaunch b = a;
  b.nslice = nslice;
  if constexpr (PAN == 0 && !SKIP && !(DP > 80 && HALF == 0)) {
    // ragged K: the last slice runs as its own launch with the idle waves sharing the rows (SuffstatPlan::extra)
    const int rs = ss_row_classes(kwaves - (nslice - 1) * wpb);
    if (!a.items && rs > 1 && b.KR > a.K) {
      b.nslice = nslice - 1;
      hipError_t e = launch_ss_k<DP, CPW, SKIP, HALF, PAN>(b, (unsigned)(a.nchunks * (nslice - 1)), stream);
      if (e != hipSuccess) return e;
      b.nslice = 1;
      b.slice0 = nslice - 1;
      b.rs = rs;
      b.klast0 = (nslice - 1) * wpb * CPW;
      b.nklast = a.K - b.klast0;
      return launch_ss_k<DP, CPW, SKIP, HALF, PAN, true>(b, (unsigned)a.nchunks, stream);
    }
  }
  return launch_ss_k<DP, CPW, SKIP, HALF, PAN>(b, a.items ? (unsigned)a.nitems : (unsigned)(a.nchunks * nslice), stream);
}

// Observations wider than 128 columns: one launch per pair of 64-column panels (P >= Q) over the same row chunks (and
// the same work list in sparse mode, built for four clusters per block: any clusters-per-wave serves it), all
// writing the same DP-wide records.  Two clusters per wave in the diagonal pairs (the D = 64 kernel as it is), one in
// the off-diagonal ones (64 accumulators per cluster).
template <bool SKIP>
static hipError_t launch_ss_wide(const SuffstatLaunch& a, hipStream_t stream) {
  SuffstatLaunch b = a;
  b.ldx = a.DP;
  b.DPW = a.DP;
  b.DP = 64;
  const int npan = a.DP / 64;
  for (int P = 0; P < npan; ++P)
    for (int Q = 0; Q <= P; ++Q) {
      b.colA = 64 * P;
      b.colB = 64 * Q;
      const hipError_t e = P == Q ? launch_ss_h<64, 2, SKIP, 0, 1>(b, stream) : launch_ss_h<64, 1, SKIP, 0, 2>(b, stream);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

template <int DP, int CPW, bool SKIP>
static hipError_t launch_ss_s(const SuffstatLaunch& a, hipStream_t stream) {
  if constexpr (DP > 80) {  // (at D = 64 the two-half variant is slower: 26.0 vs 23.6 ms; one launch at one wave per SIMD
                            //  measured 82.8 against 73.2 ms at D = 128: DESIGN 4.5.3)
    hipError_t e = launch_ss_h<DP, CPW, SKIP, 1>(a, stream);
    if (e != hipSuccess) return e;
    return launch_ss_h<DP, CPW, SKIP, 2>(a, stream);
  } else {
    return launch_ss_h<DP, CPW, SKIP, 0>(a, stream);
  }
}

template <int DP, int CPW>
static hipError_t launch_ss_t(const SuffstatLaunch& a, bool skip, hipStream_t stream) {
  return skip ? launch_ss_s<DP, CPW, true>(a, stream) : launch_ss_s<DP, CPW, false>(a, stream);
}

hipError_t launch_suffstat(const SuffstatLaunch& a, const SuffstatPlan& p, hipStream_t stream) {
  if (a.K <= 0 || p.nchunks <= 0) return hipSuccess;
  if (a.DP > 128 && a.DP % 64) return hipErrorInvalidValue;
  // the launch has to be the one its plan describes: mask and work list as the mode says, the plan's records and chunks
  if ((p.route == SS_WIDE) != (a.DP > 128) || (p.route != SS_WIDE && p.route != SS_PER_CLUSTER && a.mode != SS_DENSE)) return hipErrorInvalidValue;
  if (a.speck_skip && p.route != SS_FEAT) return hipErrorInvalidValue;  // (only the feature GEMM has a speck-skipping instance)
  if (a.speck_skip < 0 || a.speck_skip > 2) return hipErrorInvalidValue;
  const bool listed = a.mode == SS_WORK_LIST;
  if (listed != (a.items != nullptr) || a.KR != p.KR) return hipErrorInvalidValue;
  if (a.mode != SS_ZERO_SKIP && (a.smask != nullptr) != (a.mode == SS_MASKED_DENSE)) return hipErrorInvalidValue;
  if (!listed && (a.nchunks != p.nchunks || a.chunk_rows != p.chunk_rows)) return hipErrorInvalidValue;
  const bool skip = a.mode == SS_ZERO_SKIP || (listed && a.skip_listed);  // the variant that skips all-zero (step, cluster) pairs
  const int cpw = p.clusters_per_block / 4;
  switch (p.route) {
    case SS_WIDE: return skip ? launch_ss_wide<true>(a, stream) : launch_ss_wide<false>(a, stream);
    case SS_QUAD: return launch_ss_quad(a, stream);
    case SS_FEAT: return launch_ss_feat(a, stream);
    case SS_PER_CLUSTER: break;
  }
  switch (a.DP) {
    case 16:
      return cpw == 4 ? launch_ss_t<16, 4>(a, skip, stream) : cpw == 2 ? launch_ss_t<16, 2>(a, skip, stream)
                                                                : launch_ss_t<16, 1>(a, skip, stream);
    case 32:
      return cpw == 4 ? launch_ss_t<32, 4>(a, skip, stream) : cpw == 2 ? launch_ss_t<32, 2>(a, skip, stream)
                                                                : launch_ss_t<32, 1>(a, skip, stream);
    case 48: return cpw == 2 ? launch_ss_t<48, 2>(a, skip, stream) : launch_ss_t<48, 1>(a, skip, stream);
    case 64: return cpw == 2 ? launch_ss_t<64, 2>(a, skip, stream) : launch_ss_t<64, 1>(a, skip, stream);
    case 80: return launch_ss_t<80, 1>(a, skip, stream);
    case 96: return launch_ss_t<96, 1>(a, skip, stream);
    case 112: return launch_ss_t<112, 1>(a, skip, stream);
    case 128: return launch_ss_t<128, 1>(a, skip, stream);
  }
  return hipErrorInvalidValue;
}

}  // namespace lck
