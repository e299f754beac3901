// Order and threshold queries over device-resident score columns: order statistics by radix select, counts
// at thresholds, and the rows beyond a threshold in context order.  The columns and the filters are those of
// top_rows_chunk_kernel (lc_kernels_rank.hip): pad rows never take part (row-group word, or nrows with one group), with
// `label` column c sees only the rows with label[row] == label0 + c, and a NaN score takes part in nothing.
//
// Radix select.  A double becomes a 64-bit key that is monotone in the total order -inf < ... < -0.0 < +0.0 < ... < +inf:
// all bits flipped for a negative value, the sign bit flipped otherwise (done on the 32-bit halves: no 64-bit constant with
// a zero low word appears, see the note on literals in lc_kernels_rank.hip).  The key is fixed 8 bits at a time, most
// significant first.  A pass is select_hist_kernel -- every block counts the rows of its chunks into LDS histograms, one of
// 256 bins per ACTIVE PREFIX, and adds its non-zero bins to the column's global histograms -- and select_pick_kernel, one
// block per column, which finds for every requested rank the bin that holds it, the rank within that bin, and the distinct
// prefixes the ranks follow next (at most SEL_MAX).  A row matches at most one prefix, so a pass is one read of the
// column and at most one LDS atomic per row whatever the number of ranks; when all rows a wave instruction holds fall into
// one bin, one lane adds their number.  All counts are integers: the result does not depend on the grid or on the order of
// the atomics.  Nothing is read by the host between the passes.
//
// Counts: one pass, per-thread counters against the wave-uniform thresholds, a wave reduction, one atomic per (block,
// column, threshold).  Rows beyond a threshold: count per chunk of TOP_CHUNK_ROWS rows, an exclusive scan of the chunk counts
// in one block, and a second pass in which the chunk's wave places its qualifiers at chunk offset + rank within the chunk (a
// ballot prefix): context order by construction.  Every store and atomic is a vector one.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lc_kernels.h"

namespace lck {
namespace {

constexpr int SEL_THREADS = 256;    // histogram / counts kernels: 4 waves share a chunk
constexpr int SEL_BINS = 256;       // 8-bit digits
constexpr int SEL_PASSES = 8;
constexpr int SEL_STEP = SEL_THREADS * 8;  // rows per block step: 4 loads of 2 consecutive rows per lane
static_assert(TOP_CHUNK_ROWS % SEL_STEP == 0, "a chunk is whole block steps");
constexpr int RB_STEP = 512;        // rows per wave step of the compaction kernels (one wave per chunk)
static_assert(TOP_CHUNK_ROWS % RB_STEP == 0, "a chunk is whole wave steps");
constexpr int SCAN_THREADS = 1024;

// per column, between the passes
struct SelectState {
  unsigned long long pref[SEL_MAX];  // the active prefixes: keys with the bits not yet fixed zero
  long long rem[SEL_MAX];            // per requested rank: its rank among the rows under its prefix
  long long rank[SEL_MAX];           // per requested rank: r_i, or -1 (no participating row)
  int slot[SEL_MAX];                 // per requested rank: the prefix it follows
  int nact;                          // active prefixes (0: no participating row)
  int pad_;
  long long n;                       // participating rows
};
static_assert(sizeof(SelectState) % 8 == 0 && sizeof(SelectState) / 8 == SEL_STATE_WORDS, "SEL_STATE_WORDS is the state's size");

__device__ __forceinline__ unsigned long long key_of(double v) {
  unsigned hi = (unsigned)__double2hiint(v), lo = (unsigned)__double2loint(v);
  const unsigned neg = (unsigned)((int)hi >> 31);  // all ones for a negative value
  lo ^= neg;
  hi ^= neg | 0x80000000u;
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long bits_of_key(unsigned long long key) {
  unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
  const unsigned neg = ~(unsigned)((int)hi >> 31);  // the key of a negative value has a clear top bit
  lo ^= neg;
  hi ^= neg | 0x80000000u;
  return ((unsigned long long)hi << 32) | lo;
}

// rows `row`, `row + 1` of column c (row even, below NP): the scores and whether each takes part
template <bool FILTER>
__device__ __forceinline__ void load_pair(const ScoreColumns& s, const double* __restrict__ col, int c, int64_t row, bool in,
                                          double2& v, bool& o0, bool& o1) {
  v = make_double2(0.0, 0.0);
  if (in) v = *reinterpret_cast<const double2*>(col + row);
  int nv = 0;  // observations in the pair's row group
  if (in) {
    if (s.rginfo) {
      nv = s.rginfo[row / RG] & 31;
    } else {
      const int64_t rem = s.nrows - row / RG * RG;
      nv = rem >= RG ? RG : rem > 0 ? (int)rem : 0;
    }
  }
  const int r = (int)(row % RG);
  o0 = r < nv && v.x == v.x;
  o1 = r + 1 < nv && v.y == v.y;
  if constexpr (FILTER) {
    int2 lab = make_int2(-1, -1);
    if (in) lab = *reinterpret_cast<const int2*>(s.label + row);
    o0 = o0 && lab.x == s.label0 + c;
    o1 = o1 && lab.y == s.label0 + c;
  }
}

// ---- radix select --------------------------------------------------------------------------------------------------------
template <bool FILTER>
__global__ __launch_bounds__(SEL_THREADS) void select_hist_kernel(ScoreSelectLaunch a, int pass) {
  __shared__ unsigned int h[SEL_MAX * SEL_BINS];
  __shared__ unsigned long long spref[SEL_MAX];
  const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const SelectState* st = reinterpret_cast<const SelectState*>(a.state) + c;
  const int nact = pass == 0 ? 1 : st->nact;  // (block-uniform)
  if (nact < 1) return;
  for (int i = tid; i < nact * SEL_BINS; i += SEL_THREADS) h[i] = 0u;
  if (tid < nact) spref[tid] = pass == 0 ? 0ull : st->pref[tid];
  __syncthreads();
  const int shift = 64 - 8 * (pass + 1);
  const unsigned long long himask = pass == 0 ? 0ull : ~0ull << (shift + 8);  // the bits the earlier passes fixed
  const double* __restrict__ col = a.s.col + (size_t)c * a.s.ld;
  const int nchunks = (int)((a.s.NP + TOP_CHUNK_ROWS - 1) / TOP_CHUNK_ROWS);
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t c0 = (int64_t)chunk * TOP_CHUNK_ROWS;
    const int64_t cend = c0 + TOP_CHUNK_ROWS < a.s.NP ? c0 + TOP_CHUNK_ROWS : a.s.NP;  // (NP is a multiple of 16)
    for (int64_t base = c0; base < cend; base += SEL_STEP) {
      unsigned long long key[8];
      int code[8];  // slot * 256 + bin of the row, -1: it takes part in nothing
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t row = base + 2 * SEL_THREADS * j + 2 * tid;
        double2 v;
        bool o0, o1;
        load_pair<FILTER>(a.s, col, c, row, row < cend, v, o0, o1);
        key[2 * j] = key_of(v.x);
        key[2 * j + 1] = key_of(v.y);
        code[2 * j] = o0 ? -2 : -1;  // -2: takes part, no prefix matched yet
        code[2 * j + 1] = o1 ? -2 : -1;
      }
      for (int s = 0; s < nact; ++s) {
        const unsigned long long p = spref[s];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (code[e] == -2 && ((key[e] ^ p) & himask) == 0ull) code[e] = s * SEL_BINS + (int)((key[e] >> shift) & 255ull);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bool q = code[e] >= 0;
        const unsigned long long act = __ballot(q);
        if (!act) continue;
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
        const int first = __builtin_amdgcn_readlane(code[e], src);
        if (__ballot(q && code[e] == first) == act) {  // one bin for the whole wave instruction: one add
          if (lane == src) atomicAdd(&h[first], (unsigned)__popcll(act));
        } else if (q) {
          atomicAdd(&h[code[e]], 1u);
        }
      }
    }
  }
  __syncthreads();
  unsigned long long* g = a.hist + (size_t)c * SEL_MAX * SEL_BINS;
  for (int i = tid; i < nact * SEL_BINS; i += SEL_THREADS) {
    const unsigned int v = h[i];
    if (v) atomicAdd(&g[i], (unsigned long long)v);
  }
}

// one block per column: the bins of the requested ranks, the prefixes of the next pass; the histograms are zero again after it
__global__ __launch_bounds__(SEL_BINS) void select_pick_kernel(ScoreSelectLaunch a, int pass) {
  __shared__ unsigned long long sc[2][SEL_BINS];
  __shared__ int sbin[SEL_MAX];
  __shared__ long long srem[SEL_MAX];
  __shared__ long long srank[SEL_MAX];
  const int c = blockIdx.x, tid = threadIdx.x;
  SelectState* st = reinterpret_cast<SelectState*>(a.state) + c;
  unsigned long long* g = a.hist + (size_t)c * SEL_MAX * SEL_BINS;
  const int nact = pass == 0 ? 1 : st->nact;
  const int shift = 64 - 8 * (pass + 1);
  if (tid < SEL_MAX) {
    sbin[tid] = -1;
    srem[tid] = 0;
    srank[tid] = pass == 0 ? -1 : st->rank[tid];
  }
  __syncthreads();
  for (int s = 0; s < nact; ++s) {
    const unsigned long long cnt = g[(size_t)s * SEL_BINS + tid];
    g[(size_t)s * SEL_BINS + tid] = 0ull;
    // inclusive scan of the 256 counts
    int cur = 0;
    sc[0][tid] = cnt;
    __syncthreads();
    for (int d = 1; d < SEL_BINS; d <<= 1) {
      const unsigned long long v = sc[cur][tid] + (tid >= d ? sc[cur][tid - d] : 0ull);
      sc[cur ^ 1][tid] = v;
      cur ^= 1;
      __syncthreads();
    }
    const long long incl = (long long)sc[cur][tid], excl = incl - (long long)cnt;
    const long long total = (long long)sc[cur][SEL_BINS - 1];
    for (int i = 0; i < a.nprobs; ++i) {
      long long r;
      if (pass == 0) {  // r_i = min(n - 1, max(0, ceil(p_i n) - 1)); every thread works it out, the bin's owner keeps it
        if (total == 0) continue;
        r = (long long)ceil(a.probs[i] * (double)total) - 1;
        r = r < 0 ? 0 : r;
        r = r > total - 1 ? total - 1 : r;
      } else {
        if (st->slot[i] != s || srank[i] < 0) continue;
        r = st->rem[i];
      }
      if (cnt != 0ull && excl <= r && r < incl) {
        sbin[i] = tid;
        srem[i] = r - excl;
        if (pass == 0) srank[i] = r;
      }
    }
    if (pass == 0 && tid == 0) st->n = total;
    __syncthreads();  // (sc is written again by the next prefix; st->slot / rem are read by all above, written below)
  }
  if (tid != 0) return;
  // the distinct (prefix, bin) pairs in the order of the ranks that first ask for them
  unsigned long long np[SEL_MAX];
  int nslot[SEL_MAX];
  int nn = 0;
  for (int i = 0; i < a.nprobs; ++i) {
    nslot[i] = -1;
    if (sbin[i] < 0) continue;
    const unsigned long long old = pass == 0 ? 0ull : st->pref[st->slot[i]];
    const unsigned long long p = old | ((unsigned long long)(unsigned)sbin[i] << shift);
    int j = 0;
    while (j < nn && np[j] != p) ++j;
    if (j == nn) np[nn++] = p;
    nslot[i] = j;
  }
  for (int i = 0; i < a.nprobs; ++i) {
    st->slot[i] = nslot[i];
    st->rem[i] = srem[i];
    if (nslot[i] < 0) srank[i] = -1;
    st->rank[i] = srank[i];
  }
  for (int j = 0; j < nn; ++j) st->pref[j] = np[j];
  st->nact = nn;
  if (pass == SEL_PASSES - 1) {  // the prefixes are whole keys now
    a.out[c] = st->n;
    for (int i = 0; i < a.nprobs; ++i) {
      const size_t at = (size_t)a.s.C + (size_t)c * a.nprobs + i;
      a.out[at] = srank[i];
      a.out[at + (size_t)a.s.C * a.nprobs] = nslot[i] < 0 ? 0ll : (long long)bits_of_key(np[nslot[i]]);
    }
  }
}

// ---- counts at thresholds ------------------------------------------------------------------------------------------------
template <bool FILTER>
__global__ __launch_bounds__(SEL_THREADS) void score_counts_kernel(ScoreCountsLaunch a) {
  __shared__ unsigned int sh[SEL_MAX + 1];
  const int c = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  if (tid <= SEL_MAX) sh[tid] = 0u;
  __syncthreads();
  unsigned int cnt[SEL_MAX + 1];  // [0 .. SEL_MAX): score <= thr[i]; [SEL_MAX]: participating rows
#pragma unroll
  for (int i = 0; i <= SEL_MAX; ++i) cnt[i] = 0u;
  const double* __restrict__ col = a.s.col + (size_t)c * a.s.ld;
  const int nchunks = (int)((a.s.NP + TOP_CHUNK_ROWS - 1) / TOP_CHUNK_ROWS);
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int64_t c0 = (int64_t)chunk * TOP_CHUNK_ROWS;
    const int64_t cend = c0 + TOP_CHUNK_ROWS < a.s.NP ? c0 + TOP_CHUNK_ROWS : a.s.NP;
    for (int64_t base = c0; base < cend; base += SEL_STEP) {
      double2 v[4];
      bool ok[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t row = base + 2 * SEL_THREADS * j + 2 * tid;
        load_pair<FILTER>(a.s, col, c, row, row < cend, v[j], ok[2 * j], ok[2 * j + 1]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cnt[SEL_MAX] += (unsigned)ok[2 * j] + (unsigned)ok[2 * j + 1];
#pragma unroll
        for (int i = 0; i < SEL_MAX; ++i)
          if (i < a.nthr) cnt[i] += (unsigned)(ok[2 * j] && v[j].x <= a.thr[i]) + (unsigned)(ok[2 * j + 1] && v[j].y <= a.thr[i]);
      }
    }
  }
  // (a block scans at most its share of the chunks: the 32-bit counters hold up to 2^32 rows per block)
#pragma unroll
  for (int i = 0; i <= SEL_MAX; ++i) {
    unsigned int x = cnt[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if (lane == 0 && x) atomicAdd(&sh[i], x);
  }
  __syncthreads();
  if (tid <= SEL_MAX && sh[tid]) {
    // out[c][0] = participating rows, out[c][1 + i] = those at most thr[i]
    const int at = tid == SEL_MAX ? 0 : 1 + tid;
    if (at <= a.nthr) atomicAdd(&a.out[(size_t)c * (1 + a.nthr) + at], (unsigned long long)sh[tid]);
  }
}

// ---- the rows beyond a threshold, in context order ----------------------------------------------------------------------
// one wave per chunk.  PLACE = false: the chunk's count; true: positions and scores at chunkoff[chunk] + rank within the chunk
template <bool FILTER, bool PLACE>
__global__ __launch_bounds__(64) void rows_beyond_kernel(RowsBeyondLaunch a) {
  const int lane = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * TOP_CHUNK_ROWS;
  const int64_t cend = c0 + TOP_CHUNK_ROWS < a.s.NP ? c0 + TOP_CHUNK_ROWS : a.s.NP;
  const unsigned long long below = (1ull << lane) - 1ull;
  long long at = 0;  // wave-uniform: qualifiers of the chunk so far (PLACE: plus the chunk's offset)
  if constexpr (PLACE) at = a.chunkoff[blockIdx.x];
  for (int64_t base = c0; base < cend; base += RB_STEP) {
    double2 v[4];
    bool q[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t row = base + 128 * j + 2 * lane;
      bool o0, o1;
      load_pair<FILTER>(a.s, a.s.col, 0, row, row < cend, v[j], o0, o1);
      q[2 * j] = o0 && (a.above ? v[j].x >= a.thr : v[j].x <= a.thr);
      q[2 * j + 1] = o1 && (a.above ? v[j].y >= a.thr : v[j].y <= a.thr);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long b0 = __ballot(q[2 * j]), b1 = __ballot(q[2 * j + 1]);
      if constexpr (PLACE) {
        // rows in order: lane 0's pair, lane 1's pair, ...
        const long long p0 = at + __popcll(b0 & below) + __popcll(b1 & below);
        const long long p1 = p0 + (q[2 * j] ? 1 : 0);
        const int64_t row = base + 128 * j + 2 * lane;
        if (q[2 * j] && p0 < a.capacity) {
          a.pos[p0] = row;
          a.score[p0] = v[j].x;
        }
        if (q[2 * j + 1] && p1 < a.capacity) {
          a.pos[p1] = row + 1;
          a.score[p1] = v[j].y;
        }
      }
      at += __popcll(b0) + __popcll(b1);
    }
  }
  if constexpr (!PLACE)
    if (lane == 0) a.chunkoff[blockIdx.x] = at;
}

// chunkoff[i] := the sum of chunkoff[0 .. i), *total := the sum of all (one block; a carry between its rounds)
__global__ __launch_bounds__(SCAN_THREADS) void rows_beyond_scan_kernel(RowsBeyondLaunch a) {
  __shared__ long long sc[2][SCAN_THREADS];
  __shared__ long long carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int b = 0; b < a.nchunks; b += SCAN_THREADS) {
    const int i = b + tid;
    const long long v = i < a.nchunks ? a.chunkoff[i] : 0;
    int cur = 0;
    sc[0][tid] = v;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {
      const long long x = sc[cur][tid] + (tid >= d ? sc[cur][tid - d] : 0);
      sc[cur ^ 1][tid] = x;
      cur ^= 1;
      __syncthreads();
    }
    const long long base = carry;
    if (i < a.nchunks) a.chunkoff[i] = base + sc[cur][tid] - v;
    __syncthreads();  // (everybody has read carry)
    if (tid == SCAN_THREADS - 1) carry = base + sc[cur][tid];
    __syncthreads();
  }
  if (tid == 0) *a.total = carry;
}

bool columns_ok(const ScoreColumns& s) {
  return s.C >= 1 && s.C <= 65535 && s.NP >= 0 && s.NP % RG == 0 && s.ld >= s.NP && s.NP / TOP_CHUNK_ROWS < (int64_t)1 << 30;
}
// blocks per column: enough to fill the chip with the columns together, never more than there are chunks
unsigned blocks_per_column(const ScoreColumns& s) {
  const int64_t nchunks = (s.NP + TOP_CHUNK_ROWS - 1) / TOP_CHUNK_ROWS;
  const int64_t want = (SEL_GRID_BLOCKS + s.C - 1) / s.C;
  return (unsigned)(nchunks < want ? nchunks : want);
}

}  // namespace

hipError_t launch_score_select(const ScoreSelectLaunch& a, hipStream_t stream) {
  if (!columns_ok(a.s) || a.nprobs < 1 || a.nprobs > SEL_MAX || !a.hist || !a.state || !a.out) return hipErrorInvalidValue;
  if (a.s.NP == 0) return hipErrorInvalidValue;  // (the caller answers an empty context itself)
  hipError_t e = hipMemsetAsync(a.hist, 0, (size_t)a.s.C * SEL_MAX * SEL_BINS * sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  const dim3 grid(blocks_per_column(a.s), (unsigned)a.s.C);
  for (int pass = 0; pass < SEL_PASSES; ++pass) {
    if (a.s.label) hipLaunchKernelGGL(select_hist_kernel<true>, grid, dim3(SEL_THREADS), 0, stream, a, pass);
    else hipLaunchKernelGGL(select_hist_kernel<false>, grid, dim3(SEL_THREADS), 0, stream, a, pass);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(select_pick_kernel, dim3((unsigned)a.s.C), dim3(SEL_BINS), 0, stream, a, pass);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_score_counts(const ScoreCountsLaunch& a, hipStream_t stream) {
  if (!columns_ok(a.s) || a.nthr < 1 || a.nthr > SEL_MAX || !a.out) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.out, 0, (size_t)a.s.C * (1 + a.nthr) * sizeof(unsigned long long), stream);
  if (e != hipSuccess || a.s.NP == 0) return e;
  const dim3 grid(blocks_per_column(a.s), (unsigned)a.s.C);
  if (a.s.label) hipLaunchKernelGGL(score_counts_kernel<true>, grid, dim3(SEL_THREADS), 0, stream, a);
  else hipLaunchKernelGGL(score_counts_kernel<false>, grid, dim3(SEL_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_rows_beyond(const RowsBeyondLaunch& a, hipStream_t stream) {
  if (!columns_ok(a.s) || a.s.C != 1 || a.capacity < 0 || a.nchunks != top_rows_chunks(a.s.NP) || !a.total) return hipErrorInvalidValue;
  if (a.nchunks > 0 && !a.chunkoff) return hipErrorInvalidValue;
  if (a.capacity > 0 && (!a.pos || !a.score)) return hipErrorInvalidValue;
  if (a.nchunks > 0) {
    if (a.s.label) hipLaunchKernelGGL((rows_beyond_kernel<true, false>), dim3((unsigned)a.nchunks), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL((rows_beyond_kernel<false, false>), dim3((unsigned)a.nchunks), dim3(64), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(rows_beyond_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.nchunks == 0 || a.capacity == 0) return e;
  if (a.s.label) hipLaunchKernelGGL((rows_beyond_kernel<true, true>), dim3((unsigned)a.nchunks), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL((rows_beyond_kernel<false, true>), dim3((unsigned)a.nchunks), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lck
