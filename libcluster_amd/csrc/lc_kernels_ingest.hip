// Device-resident data in, row results out.
//
// pack_rows_kernel / pack_cols_kernel build the context's padded image (NP x DP row-major, every group padded to RG rows,
// pad rows and pad columns +0.0) from J strided DEVICE sources in one launch, writing every byte of the image themselves,
// and leave the minimum over the valid entries and the number of NaNs among them (integer atomics on an order-preserving
// key: the same bits on every run).  unpack_qz_kernel / unpack_qz_cols_kernel copy rows of the column-major qZ into a
// strided device destination.  No kernel here reads or writes outside the rows and columns its launch names: every source
// address is n * rs + d * cs with n < N_j, d < D, every destination address lies inside the image / the (n, K) block.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lc_kernels.h"

namespace lck {
namespace {

constexpr int PK_THREADS = 256;
constexpr int PK_ROWS = 256;  // padded rows per block of pack_rows_kernel (64 per wave)
constexpr int TP_ROWS = 64;   // rows of a transposing tile (one per lane on the side that is contiguous along the rows)
constexpr int TP_COLS = 64;   // columns of a transposing tile
// LDS row stride (doubles) of a transposing tile [TP_COLS][stride]: filled with lane = row (consecutive doubles: no
// conflict), read with LPR lanes along the columns and 64 / LPR rows side by side.  ds_read_b64 is served in halves of 32
// lanes on 64 banks of 4 bytes: lane (sg, sl) of a half reads dword 2 (stride sl + sg) + const, so stride = 32 / LPR modulo 32
// (odd for LPR = 64 and 32, where a half holds one row) puts the 32 doubles of a half on 32 different bank pairs.
template <int LPR>
constexpr int tile_stride() { return TP_ROWS + (LPR >= 32 ? 1 : 32 / LPR); }

// the order of the doubles (-inf < ... < -0.0 < +0.0 < ... < +inf) as an order of unsigned keys; no number has the key ~0
__device__ __forceinline__ unsigned long long range_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the group of padded row p and its row inside the group: goff[j] <= p < goff[j + 1] (empty groups have no such p)
__device__ __forceinline__ int group_of(const int64_t* __restrict__ goff, int J, long long p) {
  int lo = 0, hi = J;  // goff[lo] <= p < goff[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (goff[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}
// source of padded row p (element d at + d * cs), nullptr for a pad row
__device__ __forceinline__ const double* row_source(const PackRowsLaunch& a, long long p) {
  if (p >= a.NP) return nullptr;
  const int j = a.J > 1 ? group_of(a.goff, a.J, p) : 0;
  const long long n = p - a.goff[j];
  return n < a.Nj[j] ? a.src[j] + n * a.rs : nullptr;
}

// the block's minimum key and NaN count -> a.range (one atomic of each kind per block at the most)
__device__ __forceinline__ void range_commit(unsigned long long key, unsigned int nan, unsigned long long* range) {
  __shared__ unsigned long long blk_key;
  __shared__ unsigned int blk_nan;
  if (threadIdx.x == 0) {
    blk_key = ~0ull;
    blk_nan = 0;
  }
  __syncthreads();
  if (key != ~0ull) atomicMin(&blk_key, key);
  if (nan) atomicAdd(&blk_nan, nan);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (blk_key != ~0ull) atomicMin(range, blk_key);
    if (blk_nan) atomicAdd(range + 1, (unsigned long long)blk_nan);
  }
}

// Sources whose rows are contiguous (cs == 1: LPR lanes read consecutive doubles of a row, 64 / LPR rows side by side) and
// any other positive strides (the same lanes gather).  The writes are the image's rows: coalesced either way.
// a.X == nullptr: nothing is stored (the reduction alone, Context::data_range over an image that is already there).
template <int LPR>
__global__ __launch_bounds__(PK_THREADS) void pack_rows_kernel(PackRowsLaunch a) {
  constexpr int SUB = 64 / LPR;
  __shared__ const double* srow[PK_ROWS];
  const long long p0 = (long long)blockIdx.x * PK_ROWS;
  srow[threadIdx.x] = row_source(a, p0 + threadIdx.x);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sg = lane / LPR, sl = lane % LPR;
  unsigned long long key = ~0ull;
  unsigned int nan = 0;
  for (int s = 0; s < PK_ROWS / 4; s += SUB) {
    const int r = wave * (PK_ROWS / 4) + s + sg;
    const long long p = p0 + r;
    if (p >= a.NP) break;
    const double* __restrict__ src = srow[r];
    double* __restrict__ dst = a.X ? a.X + (size_t)p * a.DP : nullptr;
    for (int c = sl; c < a.DP; c += LPR) {
      double v = 0.0;
      if (src && c < a.D) {
        v = src[(long long)c * a.cs];
        if (v != v) ++nan;
        else {
          const unsigned long long k = range_key(v);
          key = k < key ? k : key;
        }
      }
      if (dst) dst[c] = v;
    }
  }
  range_commit(key, nan, a.range);
}

// Sources whose columns are contiguous (rs == 1): a 64 x 64 tile goes through LDS, read with lane = row (consecutive doubles
// of a source column) and written with LPR lanes along the image's row.
template <int LPR>
__global__ __launch_bounds__(PK_THREADS) void pack_cols_kernel(PackRowsLaunch a) {
  constexpr int SUB = 64 / LPR, S = tile_stride<LPR>();
  __shared__ double tile[TP_COLS * S];
  const long long p0 = (long long)blockIdx.x * TP_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sg = lane / LPR, sl = lane % LPR;
  const double* __restrict__ src = row_source(a, p0 + lane);  // (element d at + d * cs)
  unsigned long long key = ~0ull;
  unsigned int nan = 0;
  for (int c0 = 0; c0 < a.DP; c0 += TP_COLS) {
    for (int dd = wave; dd < TP_COLS; dd += PK_THREADS / 64) {
      const int d = c0 + dd;
      if (d >= a.DP) break;
      double v = 0.0;
      if (src && d < a.D) {
        v = src[(long long)d * a.cs];
        if (v != v) ++nan;
        else {
          const unsigned long long k = range_key(v);
          key = k < key ? k : key;
        }
      }
      tile[dd * S + lane] = v;
    }
    __syncthreads();
    for (int s = 0; s < TP_ROWS / 4; s += SUB) {
      const int r = wave * (TP_ROWS / 4) + s + sg;
      const long long p = p0 + r;
      if (p < a.NP)
        for (int dd = sl; dd < TP_COLS && c0 + dd < a.DP; dd += LPR) a.X[(size_t)p * a.DP + c0 + dd] = tile[dd * S + r];
    }
    __syncthreads();
  }
  range_commit(key, nan, a.range);
}

// q[r * rs + k * cs] = col[k * ldq + r]: lane = row.  The reads are coalesced; so are the writes of a column-major
// destination (rs == 1: K contiguous copies), any other destination takes them as they fall.
__global__ __launch_bounds__(PK_THREADS) void unpack_qz_cols_kernel(UnpackQzLaunch a) {
  const long long r = (long long)blockIdx.x * PK_THREADS + threadIdx.x;
  if (r >= a.n) return;
  for (int k = blockIdx.y; k < a.K; k += gridDim.y) a.q[r * a.rs + (long long)k * a.cs] = a.col[(size_t)k * a.ldq + r];
}

// Row-major destinations (cs == 1): a 64-row x 64-column tile through LDS, read with lane = row, written with LPR lanes
// along the destination's row.
template <int LPR>
__global__ __launch_bounds__(PK_THREADS) void unpack_qz_kernel(UnpackQzLaunch a) {
  constexpr int SUB = 64 / LPR, S = tile_stride<LPR>();
  __shared__ double tile[TP_COLS * S];
  const long long r0 = (long long)blockIdx.x * TP_ROWS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sg = lane / LPR, sl = lane % LPR;
  for (int k0 = 0; k0 < a.K; k0 += TP_COLS) {
    for (int kk = wave; kk < TP_COLS && k0 + kk < a.K; kk += PK_THREADS / 64)
      if (r0 + lane < a.n) tile[kk * S + lane] = a.col[(size_t)(k0 + kk) * a.ldq + r0 + lane];
    __syncthreads();
    for (int s = 0; s < TP_ROWS / 4; s += SUB) {
      const int r = wave * (TP_ROWS / 4) + s + sg;
      if (r0 + r < a.n)
        for (int kk = sl; kk < TP_COLS && k0 + kk < a.K; kk += LPR) a.q[(r0 + r) * a.rs + k0 + kk] = tile[kk * S + r];
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_pack_rows(const PackRowsLaunch& a, hipStream_t stream) {
  if (a.J < 1 || a.D < 1 || a.DP < a.D || a.NP < 0 || a.NP % RG || a.rs < 1 || a.cs < 1 || !a.src || !a.Nj || !a.goff ||
      !a.range)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.range, 0xff, sizeof(unsigned long long), stream);  // (~0: no entry yet)
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.range + 1, 0, sizeof(unsigned long long), stream);
  if (e != hipSuccess) return e;
  if (a.NP == 0) return hipSuccess;
  const int lpr = a.DP <= 16 ? 16 : a.DP <= 32 ? 32 : 64;
  if (a.rs == 1 && a.cs != 1 && a.X) {
    const dim3 grid((unsigned)((a.NP + TP_ROWS - 1) / TP_ROWS));
    switch (lpr) {
      case 16: hipLaunchKernelGGL(pack_cols_kernel<16>, grid, dim3(PK_THREADS), 0, stream, a); break;
      case 32: hipLaunchKernelGGL(pack_cols_kernel<32>, grid, dim3(PK_THREADS), 0, stream, a); break;
      default: hipLaunchKernelGGL(pack_cols_kernel<64>, grid, dim3(PK_THREADS), 0, stream, a); break;
    }
  } else {
    const dim3 grid((unsigned)((a.NP + PK_ROWS - 1) / PK_ROWS));
    switch (lpr) {
      case 16: hipLaunchKernelGGL(pack_rows_kernel<16>, grid, dim3(PK_THREADS), 0, stream, a); break;
      case 32: hipLaunchKernelGGL(pack_rows_kernel<32>, grid, dim3(PK_THREADS), 0, stream, a); break;
      default: hipLaunchKernelGGL(pack_rows_kernel<64>, grid, dim3(PK_THREADS), 0, stream, a); break;
    }
  }
  return hipGetLastError();
}

void data_range_decode(const unsigned long long* range_h, double* min, int64_t* n_nan) {
  const unsigned long long k = range_h[0];
  if (min) {
    if (k == ~0ull) {
      *min = INFINITY;  // no valid entry that is a number
    } else {
      const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
      double v;
      __builtin_memcpy(&v, &b, sizeof v);
      *min = v;
    }
  }
  if (n_nan) *n_nan = (int64_t)range_h[1];
}

hipError_t launch_unpack_qz(const UnpackQzLaunch& a, hipStream_t stream) {
  if (a.n < 0 || a.K < 1 || a.ldq < a.n || a.rs < 1 || a.cs < 1 || !a.col || !a.q) return hipErrorInvalidValue;
  if (a.n == 0) return hipSuccess;
  if (a.cs == 1 && a.rs != 1) {
    const dim3 grid((unsigned)((a.n + TP_ROWS - 1) / TP_ROWS));
    const int lpr = a.K <= 16 ? 16 : a.K <= 32 ? 32 : 64;
    switch (lpr) {
      case 16: hipLaunchKernelGGL(unpack_qz_kernel<16>, grid, dim3(PK_THREADS), 0, stream, a); break;
      case 32: hipLaunchKernelGGL(unpack_qz_kernel<32>, grid, dim3(PK_THREADS), 0, stream, a); break;
      default: hipLaunchKernelGGL(unpack_qz_kernel<64>, grid, dim3(PK_THREADS), 0, stream, a); break;
    }
  } else {
    const dim3 grid((unsigned)((a.n + PK_THREADS - 1) / PK_THREADS), (unsigned)(a.K < 64 ? a.K : 64));
    hipLaunchKernelGGL(unpack_qz_cols_kernel, grid, dim3(PK_THREADS), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace lck
