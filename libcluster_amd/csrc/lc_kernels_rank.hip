// Ranking kernels: the m best rows of each of C device columns -- the exemplars of a cluster, the least
// likely rows of a prediction -- without bringing the columns to the host.
//
// The order is TOTAL: entry a is better than entry b when key_a > key_b, or the keys compare equal and pos_a < pos_b
// (key = the score for `largest`, its negation otherwise; +0.0 and -0.0 compare equal, a NaN compares with nothing and
// is never selected).  The m best entries of a set under a total order do not depend on how the set was split, so the
// answer is the same for every chunk length, grid and wave count.
//
// top_rows_chunk_kernel, one wave per (row chunk, column): the wave scans its chunk and keeps its best 64 entries in
// registers, one per lane, best first; the m-th of them is the wave-uniform threshold.  A step loads 4 x 16 bytes of
// consecutive rows per lane and asks with ONE ballot whether anything beats the threshold -- in steady state nothing does
// and the pass is a read.  A qualifier is inserted by rank: its rank is the number of list entries that are better (a
// ballot: the list is sorted, the better entries are a prefix), the lanes behind it shift by one (__shfl_up).  The wave
// writes its m best as the partial list of (chunk, column).  (One wave per chunk, not four that share it: a wave that
// scans R rows in random order inserts about m (1 + ln(R / m)) of them, so four short scans pay three times the
// insertions of one long one; a block of several waves would merge their lists through LDS as the merge kernel does.)
// top_rows_merge_kernel, one block of 16 waves per column, runs the same insertion over the partial lists; its waves'
// lists meet in LDS and wave 0 inserts the others' entries.
//
// Worst case: the qualifiers of a step are taken from the highest lane down and the ballot is renewed after every
// insertion, so a rising column inserts about 2 m rows per step of 512 and a falling one none after its first step; a
// column built against the scan order makes every row an insertion (about 30 wave instructions each) -- linear in the
// rows, no merge network (DESIGN 4.13 prices it).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>

#include "lc_kernels.h"

namespace lck {
namespace {

constexpr int TR_WAVES = 1;         // chunk kernel: waves per block (each scans TOP_CHUNK_ROWS / TR_WAVES rows)
constexpr int TR_MERGE_WAVES = 16;  // merge kernel
constexpr int TR_STEP = 512;        // rows per wave step: 4 loads of 2 consecutive rows per lane
constexpr int TR_WAVE_ROWS = TOP_CHUNK_ROWS / TR_WAVES;
static_assert(TR_WAVE_ROWS % TR_STEP == 0, "a wave's share of a chunk is whole steps");
constexpr long long TR_EMPTY = std::numeric_limits<long long>::max();  // position of a list slot that holds no row

__device__ __forceinline__ bool better(double ka, long long pa, double kb, long long pb) {
  return ka > kb || (ka == kb && pa < pb);
}
// value of lane `lane` (wave-uniform) in every lane
__device__ __forceinline__ double lane_value(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ long long lane_value(long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), lane);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// a wave's list: lane i holds its i-th best entry; (tk, tp) = the entry of lane m - 1, the same in every lane
struct TopList {
  double k;
  long long p;
  double tk;
  long long tp;
};
// The threshold is wave-uniform and lives in a pair of scalar registers.  Written as a constant, its start value -inf
// became `s_mov_b64 s[..], 0xfff0000000000000` with this compiler (ROCm 7's hipcc, gfx950), which the encoder stores as the
// 32-bit literal 0: a threshold of 0.0, and no negative score was ever selected.  The high word goes through an empty asm
// statement, so the value is put together at run time from a 32-bit move.
__device__ __forceinline__ TopList empty_list() {
  int hi = (int)0xfff00000u;
  asm volatile("" : "+s"(hi));
  const double ninf = __hiloint2double(hi, 0);
  return {ninf, TR_EMPTY, ninf, TR_EMPTY};
}
// every lane offers one candidate (q: it has one); those that beat the threshold are inserted, highest lane first
__device__ __forceinline__ void push(TopList& L, double ck, long long cp, bool q, int mlast, int lane) {
  unsigned long long mask = __ballot(q && better(ck, cp, L.tk, L.tp));
  while (mask) {
    const int src = __builtin_amdgcn_readfirstlane(63 - __clzll((long long)mask));
    const double k = lane_value(ck, src);
    const long long p = lane_value(cp, src);
    const int rank = __popcll(__ballot(better(L.k, L.p, k, p)));  // the sorted list's better entries are lanes 0 .. rank - 1
    const double uk = __shfl_up(L.k, 1);
    const long long up = __shfl_up(L.p, 1);
    if (lane == rank) {
      L.k = k;
      L.p = p;
    } else if (lane > rank) {
      L.k = uk;
      L.p = up;
    }
    L.tk = lane_value(L.k, mlast);
    L.tp = lane_value(L.p, mlast);
    mask = __ballot(q && better(ck, cp, L.tk, L.tp)) & ((1ull << src) - 1ull);
  }
}

// the lists of the block's waves -> wave 0's list holds the block's best (sk, sp: NW x 64 entries of LDS)
template <int NW>
__device__ __forceinline__ void merge_waves(TopList& L, double* sk, long long* sp, int m, int lane, int wave) {
  sk[wave * 64 + lane] = L.k;
  sp[wave * 64 + lane] = L.p;
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < NW; ++w) {
    const double ck = sk[w * 64 + lane];
    const long long cp = sp[w * 64 + lane];
    push(L, ck, cp, lane < m && cp != TR_EMPTY, m - 1, lane);
  }
}

template <bool FILTER>
__global__ __launch_bounds__(TR_WAVES * 64) void top_rows_chunk_kernel(TopRowsLaunch a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.y;
  const double* __restrict__ col = a.col + (size_t)c * a.ld;
  const int64_t w0 = (int64_t)blockIdx.x * TOP_CHUNK_ROWS + (int64_t)wave * TR_WAVE_ROWS;
  const int64_t wend = w0 + TR_WAVE_ROWS < a.NP ? w0 + TR_WAVE_ROWS : a.NP;  // (NP is a multiple of 16: rows come in pairs)
  TopList L = empty_list();
  for (int64_t base = w0; base < wend; base += TR_STEP) {
    double key[8];
    bool ok[8];
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t row = base + 128 * j + 2 * lane;
      const bool in = row < wend;
      double2 v = make_double2(0.0, 0.0);
      if (in) v = *reinterpret_cast<const double2*>(col + row);
      int nv = 0;  // observations in the pair's row group (the pad rows behind them are never selected)
      if (in) {
        if (a.rginfo) {
          nv = a.rginfo[row / RG] & 31;
        } else {
          const int64_t rem = a.nrows - row / RG * RG;
          nv = rem >= RG ? RG : rem > 0 ? (int)rem : 0;
        }
      }
      const int r = (int)(row % RG);
      bool o0 = r < nv, o1 = r + 1 < nv;
      if constexpr (FILTER) {
        int2 lab = make_int2(-1, -1);
        if (in) lab = *reinterpret_cast<const int2*>(a.label + row);
        o0 = o0 && lab.x == c;
        o1 = o1 && lab.y == c;
      }
      key[2 * j] = a.largest ? v.x : -v.x;
      key[2 * j + 1] = a.largest ? v.y : -v.y;
      ok[2 * j] = o0;
      ok[2 * j + 1] = o1;
      any = any || (o0 && better(key[2 * j], row, L.tk, L.tp)) || (o1 && better(key[2 * j + 1], row + 1, L.tk, L.tp));
    }
    if (!__ballot(any)) continue;
#pragma unroll
    for (int e = 7; e >= 0; --e)  // (the later rows first: a rising column raises the threshold soonest)
      push(L, key[e], base + 128 * (e / 2) + 2 * lane + (e & 1), ok[e], a.m - 1, lane);
  }
  if constexpr (TR_WAVES > 1) {
    __shared__ double sk[TR_WAVES * 64];
    __shared__ long long sp[TR_WAVES * 64];
    merge_waves<TR_WAVES>(L, sk, sp, a.m, lane, wave);
  }
  if (wave == 0 && lane < a.m) {
    const size_t at = ((size_t)blockIdx.x * a.C + c) * a.m + lane;
    a.pkey[at] = L.k;
    a.ppos[at] = L.p;
  }
}

__global__ __launch_bounds__(TR_MERGE_WAVES * 64) void top_rows_merge_kernel(TopRowsLaunch a) {
  __shared__ double sk[TR_MERGE_WAVES * 64];
  __shared__ long long sp[TR_MERGE_WAVES * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x;
  const unsigned n = (unsigned)a.nchunks * (unsigned)a.m;  // entries of the column's partial lists
  TopList L = empty_list();
  constexpr unsigned U = 4;  // loads in flight per lane
  for (unsigned e0 = (unsigned)wave * 64; e0 < n; e0 += TR_MERGE_WAVES * 64 * U) {
    double ck[U];
    long long cp[U];
#pragma unroll
    for (unsigned u = 0; u < U; ++u) {
      const unsigned e = e0 + u * TR_MERGE_WAVES * 64 + lane;
      ck[u] = 0.0;
      cp[u] = TR_EMPTY;
      if (e < n) {
        const unsigned chunk = e / (unsigned)a.m, i = e - chunk * (unsigned)a.m;
        const size_t at = ((size_t)chunk * a.C + c) * a.m + i;
        ck[u] = a.pkey[at];
        cp[u] = a.ppos[at];
      }
    }
#pragma unroll
    for (unsigned u = 0; u < U; ++u) push(L, ck[u], cp[u], cp[u] != TR_EMPTY, a.m - 1, lane);
  }
  merge_waves<TR_MERGE_WAVES>(L, sk, sp, a.m, lane, wave);
  if (wave == 0 && lane < a.m) {
    const bool has = L.p != TR_EMPTY;
    const size_t at = (size_t)c * a.m + lane;
    a.out_score[at] = !has ? std::numeric_limits<double>::quiet_NaN() : a.largest ? L.k : -L.k;
    a.out_pos[at] = has ? L.p : -1;
  }
}

}  // namespace

int top_rows_chunks(int64_t NP) { return (int)((NP + TOP_CHUNK_ROWS - 1) / TOP_CHUNK_ROWS); }

hipError_t launch_top_rows(const TopRowsLaunch& a, hipStream_t stream) {
  if (a.m < 1 || a.m > TOP_MAX_M || a.C < 1 || a.C > 65535 || a.NP < 0 || a.NP % RG != 0 || a.ld < a.NP) return hipErrorInvalidValue;
  if (a.nchunks != top_rows_chunks(a.NP) || (int64_t)a.nchunks * a.m > (int64_t)1 << 30) return hipErrorInvalidValue;
  if (a.nchunks > 0) {
    const dim3 grid((unsigned)a.nchunks, (unsigned)a.C);
    if (a.label) hipLaunchKernelGGL(top_rows_chunk_kernel<true>, grid, dim3(TR_WAVES * 64), 0, stream, a);
    else hipLaunchKernelGGL(top_rows_chunk_kernel<false>, grid, dim3(TR_WAVES * 64), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(top_rows_merge_kernel, dim3((unsigned)a.C), dim3(TR_MERGE_WAVES * 64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lck
