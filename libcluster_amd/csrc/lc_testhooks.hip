// Test-hook entry points: libcluster_hip_testhooks.so ONLY (libcluster_amd/build.py, HOOK_ONLY_SOURCES) -- the shipped
// library exports no lc_test_* symbol (tests/test_host.py).  One wrapper per launcher of lc_kernels_aux.hip: host arrays in,
// one launch (or the launcher pair a Context method uses together), host arrays out; 0 on success, the HIP error code
// otherwise.  Everything a kernel would use as an address is checked on the host BEFORE anything is launched: a wrong
// test comes back as -1 and a failed assertion, never as a memory fault.  Buffers marked "io" are uploaded as the
// caller filled them (sentinels) and downloaded whole, so that a write outside the intended entries shows.
// Python side: tests/aux_hooks.py; cases: tests/test_gpu_aux_kernels.py, tests/test_gpu_predict_kernels.py for the
// launchers of lc_kernels_predict.hip and lc_kernels_topic.hip, tests/test_gpu_launch_plans.py for the two launch plans, and
// tests/test_gpu_hot_kernels.py for launch_estep, launch_suffstat (with launch_fold_extra) and launch_fused, and
// tests/test_gpu_diag_kernels.py for launch_estep_diag, launch_suffstat_diag and the host packer.  Hooks named lcx_test_* are
// bound by their own test files: lcx_test_loo_rows (tests/test_gpu_loo_kernels.py), the statistics list hooks
// (tests/test_gpu_stats_lists.py and its neighbours) and, at the end of this file, the six launchers of lc_kernels_holes.hip:
// lcx_test_holes_scan (launch_holes_scan, launch_holes_fill), lcx_test_predict_holes (launch_predict_holes / _var / _keep) and
// lcx_test_holes_draws (launch_predict_holes_keep, launch_holes_draws), cases in tests/test_gpu_holes_kernels.py (inputs:
// tests/holes_kernel_cases.py, held to their conditions without a device by tests/test_holes_kernels_refs_host.py).
// The hooks of lc_kernels_ingest.hip follow them: lcx_test_pack_rows, lcx_test_unpack_qz and lcx_test_ctx_image
// (tests/ingest_hooks.py; cases in tests/test_gpu_ingest_kernels.py and tests/test_gpu_device_io.py).  Last come the launchers
// of lc_kernels_sample.hip (lcx_test_sample, lcx_test_cond_draws; tests/test_gpu_sample_kernels.py), lc_kernels_rank.hip
// (lcx_test_top_rows) and lc_kernels_select.hip (lcx_test_score_select, lcx_test_score_counts, lcx_test_rows_beyond;
// tests/test_gpu_rank_select_kernels.py).
#include <algorithm>
#include <cstdio>
#include <exception>
#include <vector>

#include "lc_ctx.hpp"
#include "lc_device.hpp"
#include "lc_predict.hpp"

namespace {

using lck::RG;
typedef long long i64;  // (ctypes c_longlong; int64_t on the device side)

// device copies of the host arrays of one call; finish() waits, downloads the io buffers and frees everything
class Scope {
 public:
  ~Scope() {
    for (auto& b : bufs_)
      if (b.d) (void)hipFree(b.d);
  }
  template <typename T>
  T* in(const T* h, size_t n) { return static_cast<T*>(add(const_cast<T*>(h), n * sizeof(T), false, true)); }
  template <typename T>
  T* io(T* h, size_t n) { return static_cast<T*>(add(h, n * sizeof(T), true, true)); }
  template <typename T>
  T* out(T* h, size_t n) { return static_cast<T*>(add(h, n * sizeof(T), true, false)); }
  template <typename T>
  T* scratch(size_t n) { return static_cast<T*>(add(nullptr, n * sizeof(T), false, false)); }
  bool ok() const { return err_ == hipSuccess; }
  int finish(hipError_t launched) {
    if (err_ == hipSuccess) err_ = launched;
    if (err_ == hipSuccess) err_ = hipDeviceSynchronize();
    for (auto& b : bufs_)
      if (err_ == hipSuccess && b.back && b.bytes) err_ = hipMemcpy(b.h, b.d, b.bytes, hipMemcpyDeviceToHost);
    return (int)err_;
  }

 private:
  struct Buf {
    void *d, *h;
    size_t bytes;
    bool back;
  };
  void* add(void* h, size_t bytes, bool back, bool upload) {
    Buf b{nullptr, h, bytes, back};
    if (err_ == hipSuccess) err_ = hipMalloc(&b.d, bytes ? bytes : 16);  // (an empty array still gets an address)
    if (err_ == hipSuccess && upload && bytes) err_ = hipMemcpy(b.d, h, bytes, hipMemcpyHostToDevice);
    bufs_.push_back(b);
    return b.d;
  }
  std::vector<Buf> bufs_;
  hipError_t err_ = hipSuccess;
};

// rginfo words of nrg row groups: every group index inside [0, ngroups), every count inside 0 ... 16
bool rginfo_ok(const int* rginfo, i64 nrg, i64 ngroups) {
  for (i64 g = 0; g < nrg; ++g) {
    const int info = rginfo[g];
    if (info < 0 || (info >> 5) >= ngroups || (info & 31) > RG) return false;
  }
  return true;
}

// a selection as the gathers address it: M source rows inside [0, nsrc), J >= 1 groups whose starts ascend from 0 to M, every
// destination row goff_sub[j] + (p - starts[j]) inside [0, ndst)
bool selection_ok(const i64* idx, i64 M, i64 nsrc, const i64* starts, const i64* goff_sub, int J, i64 ndst) {
  if (!idx || !starts || !goff_sub || M < 0 || J < 1 || nsrc < 0 || ndst < 0) return false;
  for (i64 p = 0; p < M; ++p)
    if (idx[p] < 0 || idx[p] >= nsrc) return false;
  if (starts[0] != 0 || starts[J] != M) return false;
  for (int j = 0; j < J; ++j) {
    const i64 cnt = starts[j + 1] - starts[j];
    if (cnt < 0 || goff_sub[j] < 0 || goff_sub[j] > ndst || cnt > ndst - goff_sub[j]) return false;
  }
  return true;
}

__global__ void __launch_bounds__(256) exp_nonpos_probe_kernel(const double* __restrict__ x, i64 n, double* __restrict__ out) {
  __shared__ double etab[64];
  lck::fill_exp_table(etab, threadIdx.x, 256);
  __syncthreads();
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = lck::exp_nonpos(x[i], etab);
}
__global__ void __launch_bounds__(256) rcp_pos_probe_kernel(const double* __restrict__ x, i64 n, double* __restrict__ out) {
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = lck::rcp_pos(x[i]);
}
__global__ void __launch_bounds__(256) log1p_nonneg_probe_kernel(const double* __restrict__ x, i64 n, double* __restrict__ out) {
  __shared__ lck::LogEntry ltab[128];
  lck::fill_log_table(ltab, threadIdx.x, 256);
  __syncthreads();
  const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = lck::log1p_nonneg(x[i], ltab);
}

// the rows of a prediction launch: nrg >= 1 row groups inside ldq; rginfo words naming groups below J, or (null) nrows
bool pred_rows_ok(i64 nrg, i64 ldq, const int* rginfo, i64 nrows, int J) {
  if (nrg < 1 || nrg > ((i64)1 << 40) / RG || nrg * RG > ldq || J < 1) return false;
  return rginfo ? rginfo_ok(rginfo, nrg, J) : (nrows >= 0 && nrows <= nrg * RG);
}

}  // namespace

#define LC_HOOK extern "C" __attribute__((visibility("default"))) int

// the device-side rank-order sum of LIBCLUSTER_COMM=rccl-gather on host data (tests/test_gpu_comm.py): `world` blocks of
// `count` doubles in, `count` out
LC_HOOK lc_test_rank_order_sum(const double* in, int world, i64 count, double* out) {
  if (!in || !out || world < 1 || count < 1) return -1;
  Scope s;
  const double* din = s.in(in, (size_t)world * (size_t)count);
  double* dout = s.out(out, (size_t)count);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_rank_order_sum(din, world, count, dout, nullptr));
}

// ---- device math -------------------------------------------------------------------------------------------------
LC_HOOK lc_test_exp_nonpos(const double* x, i64 n, double* out) {
  if (!x || !out || n < 1) return -1;
  Scope s;
  const double* dx = s.in(x, (size_t)n);
  double* dout = s.out(out, (size_t)n);
  if (!s.ok()) return s.finish(hipSuccess);
  hipLaunchKernelGGL(exp_nonpos_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dx, n, dout);
  return s.finish(hipGetLastError());
}
LC_HOOK lc_test_rcp_pos(const double* x, i64 n, double* out) {
  if (!x || !out || n < 1) return -1;
  Scope s;
  const double* dx = s.in(x, (size_t)n);
  double* dout = s.out(out, (size_t)n);
  if (!s.ok()) return s.finish(hipSuccess);
  hipLaunchKernelGGL(rcp_pos_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dx, n, dout);
  return s.finish(hipGetLastError());
}
LC_HOOK lc_test_log1p_nonneg(const double* x, i64 n, double* out) {
  if (!x || !out || n < 1) return -1;
  Scope s;
  const double* dx = s.in(x, (size_t)n);
  double* dout = s.out(out, (size_t)n);
  if (!s.ok()) return s.finish(hipSuccess);
  hipLaunchKernelGGL(log1p_nonneg_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dx, n, dout);
  return s.finish(hipGetLastError());
}

// ---- reductions --------------------------------------------------------------------------------------------------
// partial [nparts x n] -> out [n]; use_tmp: hand the launcher its REDUCE_TMP_ELEMS * 64 doubles of scratch
LC_HOOK lc_test_reduce_partials(const double* partial, int nparts, i64 n, double* out, int use_tmp) {
  if (!partial || !out || nparts < 0 || n < 1) return -1;
  Scope s;
  const double* dp = s.in(partial, (size_t)nparts * (size_t)n);
  double* dout = s.io(out, (size_t)n);
  double* tmp = use_tmp ? s.scratch<double>((size_t)lck::REDUCE_TMP_ELEMS * 64) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_reduce_partials(dp, nparts, n, dout, nullptr, tmp));
}
// partial [nrec x n]; cluster k sums the records krec[kptr[k] .. kptr[k + 1]) -> out [K x n]
LC_HOOK lc_test_reduce_records(const double* partial, int nrec, i64 n, int K, const int* kptr, const int* krec, double* out) {
  if (!partial || !kptr || !krec || !out || nrec < 0 || n < 1 || K < 1 || kptr[0] < 0) return -1;
  for (int k = 0; k < K; ++k)
    if (kptr[k + 1] < kptr[k]) return -1;
  for (int c = kptr[0]; c < kptr[K]; ++c)
    if (krec[c] < 0 || krec[c] >= nrec) return -1;
  Scope s;
  const double* dp = s.in(partial, (size_t)nrec * (size_t)n);
  const int* dkptr = s.in(kptr, (size_t)K + 1);
  const int* dkrec = s.in(krec, (size_t)kptr[K]);
  double* dout = s.io(out, (size_t)K * (size_t)n);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_reduce_records(dp, n, K, dkptr, dkrec, dout, nullptr));
}
// qZ [K x ldq], goff [J + 1] -> out [J x K]; use_tmp / rows as launch_group_colsum takes them (`rows` is no address: it
// only steers the launcher's choice of path, every path reads goff's own row ranges)
LC_HOOK lc_test_group_colsum(const double* qZ, i64 ldq, int K, const i64* goff, int J, double* out, int use_tmp, i64 rows) {
  if (!qZ || !goff || !out || K < 1 || J < 1 || ldq < 1 || goff[0] < 0 || goff[J] > ldq) return -1;
  for (int j = 0; j < J; ++j)
    if (goff[j + 1] < goff[j]) return -1;
  Scope s;
  const double* dq = s.in(qZ, (size_t)K * (size_t)ldq);
  const int64_t* dg = reinterpret_cast<const int64_t*>(s.in(goff, (size_t)J + 1));
  double* dout = s.io(out, (size_t)J * (size_t)K);
  double* tmp = use_tmp ? s.scratch<double>((size_t)lck::REDUCE_TMP_ELEMS * 64) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_group_colsum(dq, ldq, K, dg, J, dout, nullptr, tmp, rows));
}
// qZ (io) [Kbuf x ldq]: columns 0 .. K of the nrg * 16 rows are filled; rginfo [nrg] or null (then nrows)
LC_HOOK lc_test_fill_qz(double* qZ, i64 ldq, int K, int Kbuf, const int* rginfo, i64 nrows, i64 nrg, double value) {
  if (!qZ || K < 1 || K > Kbuf || nrg < 1 || nrg * RG > ldq) return -1;
  if (rginfo ? !rginfo_ok(rginfo, nrg, 1 << 26) : (nrows < 0 || nrows > nrg * RG)) return -1;
  Scope s;
  double* dq = s.io(qZ, (size_t)Kbuf * (size_t)ldq);
  const int* drg = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_fill_qz(dq, ldq, K, drg, nrows, nrg, value, nullptr));
}

// ---- split search: row selection -----------------------------------------------------------------------------------
// select_count, the host's exclusive scan, select_compact and group_starts as Context::select_rows_col chains them.
// qcol [NP]; goff [J + 1] ascending; counts (out) [select_blocks(NP)]; idx (io) [cap]; starts (io) [J + 1]; *M (out).
// -1 when the arguments are unusable or the selection would not fit into idx -- then nothing behind select_count was
// launched and idx / starts are as the caller filled them (*M is the count found, or untouched); a HIP error code
// likewise leaves them alone.
LC_HOOK lc_test_select_rows(const double* qcol, i64 NP, double thresh, const i64* goff, int J, int* counts, i64* idx, i64 cap,
                            i64* starts, i64* M) {
  if (!qcol || !goff || !counts || !idx || !starts || !M || NP < 1 || J < 1 || cap < 1) return -1;
  for (int j = 0; j < J; ++j)
    if (goff[j + 1] < goff[j]) return -1;
  const int nb = lck::select_blocks(NP);
  Scope s;
  const double* dq = s.in(qcol, (size_t)NP);
  const int64_t* dg = reinterpret_cast<const int64_t*>(s.in(goff, (size_t)J + 1));
  int* dcnt = s.scratch<int>((size_t)nb);
  int64_t* doff = s.scratch<int64_t>((size_t)nb);
  int64_t* didx = reinterpret_cast<int64_t*>(s.io(idx, (size_t)cap));
  int64_t* dst = reinterpret_cast<int64_t*>(s.io(starts, (size_t)J + 1));
  if (!s.ok()) return s.finish(hipSuccess);
  hipError_t e = lck::launch_select_count(dq, NP, thresh, dcnt, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(counts, dcnt, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  std::vector<int64_t> off((size_t)nb);
  int64_t tot = 0;
  for (int b = 0; b < nb; ++b) {
    if (counts[b] < 0 || counts[b] > 1024) return -1;  // (what select_compact would use as an address)
    off[(size_t)b] = tot;
    tot += counts[b];
  }
  *M = tot;
  if (tot > cap) return -1;
  e = hipMemcpy(doff, off.data(), (size_t)nb * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = lck::launch_select_compact(dq, NP, thresh, doff, didx, nullptr);
  if (e == hipSuccess) e = lck::launch_group_starts(didx, tot, dg, J, dst, nullptr);
  return s.finish(e);
}

// ---- split search: gathers and the scatter ----------------------------------------------------------------------------
// X [nsrc x DP] -> Xdst (io) [ndst x DP]
LC_HOOK lc_test_gather_rows(const double* X, i64 nsrc, int DP, const i64* idx, i64 M, const i64* starts, const i64* goff_sub, int J,
                            double* Xdst, i64 ndst) {
  if (!X || !Xdst || DP < 2 || DP % 2 || !selection_ok(idx, M, nsrc, starts, goff_sub, J, ndst)) return -1;
  Scope s;
  const double* dX = s.in(X, (size_t)nsrc * DP);
  const int64_t* di = reinterpret_cast<const int64_t*>(s.in(idx, (size_t)M));
  const int64_t* ds = reinterpret_cast<const int64_t*>(s.in(starts, (size_t)J + 1));
  const int64_t* dg = reinterpret_cast<const int64_t*>(s.in(goff_sub, (size_t)J + 1));
  double* dD = s.io(Xdst, (size_t)ndst * DP);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_gather_rows(dX, DP, di, M, ds, dg, J, dD, nullptr));
}
// X [nsrc x DP] -> Xdst (io) [ndst x DP], row p from row idx[p]
LC_HOOK lc_test_gather_rows_plain(const double* X, i64 nsrc, int DP, const i64* idx, i64 M, double* Xdst, i64 ndst) {
  if (!X || !Xdst || !idx || DP < 2 || DP % 2 || M < 0 || M > ndst) return -1;
  for (i64 p = 0; p < M; ++p)
    if (idx[p] < 0 || idx[p] >= nsrc) return -1;
  Scope s;
  const double* dX = s.in(X, (size_t)nsrc * DP);
  const int64_t* di = reinterpret_cast<const int64_t*>(s.in(idx, (size_t)M));
  double* dD = s.io(Xdst, (size_t)ndst * DP);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_gather_rows_plain(dX, DP, di, M, dD, nullptr));
}
// column-major src [K x lds] (rows < nsrc <= lds) -> column-major dst (io) [K x ldd]
LC_HOOK lc_test_gather_cols(const double* src, i64 lds, i64 nsrc, int K, const i64* idx, i64 M, const i64* starts,
                            const i64* goff_sub, int J, double* dst, i64 ldd) {
  if (!src || !dst || K < 1 || nsrc > lds || !selection_ok(idx, M, nsrc, starts, goff_sub, J, ldd)) return -1;
  Scope s;
  const double* dS = s.in(src, (size_t)K * (size_t)lds);
  const int64_t* di = reinterpret_cast<const int64_t*>(s.in(idx, (size_t)M));
  const int64_t* ds = reinterpret_cast<const int64_t*>(s.in(starts, (size_t)J + 1));
  const int64_t* dg = reinterpret_cast<const int64_t*>(s.in(goff_sub, (size_t)J + 1));
  double* dD = s.io(dst, (size_t)K * (size_t)ldd);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_gather_cols(dS, lds, K, di, M, ds, dg, J, dD, ldd, nullptr));
}
// row-major src [nsrc x lds] (lds >= K) -> column-major dst (io) [K x ldd]
LC_HOOK lc_test_gather_rowmajor(const double* src, i64 lds, i64 nsrc, int K, const i64* idx, i64 M, const i64* starts,
                                const i64* goff_sub, int J, double* dst, i64 ldd) {
  if (!src || !dst || K < 1 || K > lds || !selection_ok(idx, M, nsrc, starts, goff_sub, J, ldd)) return -1;
  Scope s;
  const double* dS = s.in(src, (size_t)nsrc * (size_t)lds);
  const int64_t* di = reinterpret_cast<const int64_t*>(s.in(idx, (size_t)M));
  const int64_t* ds = reinterpret_cast<const int64_t*>(s.in(starts, (size_t)J + 1));
  const int64_t* dg = reinterpret_cast<const int64_t*>(s.in(goff_sub, (size_t)J + 1));
  double* dD = s.io(dst, (size_t)K * (size_t)ldd);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_gather_rowmajor(dS, lds, K, di, M, ds, dg, J, dD, ldd, nullptr));
}
// row-major src [nsrc x lds], columns cols[0 .. nc) (each inside [0, lds)) -> column-major dst (io) [nc x ldd]
LC_HOOK lc_test_gather_rowmajor_cols(const double* src, i64 lds, i64 nsrc, const int* cols, int nc, const i64* idx, i64 M,
                                     const i64* starts, const i64* goff_sub, int J, double* dst, i64 ldd) {
  if (!src || !dst || !cols || nc < 1 || lds < 1 || !selection_ok(idx, M, nsrc, starts, goff_sub, J, ldd)) return -1;
  for (int c = 0; c < nc; ++c)
    if (cols[c] < 0 || cols[c] >= lds) return -1;
  Scope s;
  const double* dS = s.in(src, (size_t)nsrc * (size_t)lds);
  const int* dc = s.in(cols, (size_t)nc);
  const int64_t* di = reinterpret_cast<const int64_t*>(s.in(idx, (size_t)M));
  const int64_t* ds = reinterpret_cast<const int64_t*>(s.in(starts, (size_t)J + 1));
  const int64_t* dg = reinterpret_cast<const int64_t*>(s.in(goff_sub, (size_t)J + 1));
  double* dD = s.io(dst, (size_t)nc * (size_t)ldd);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_gather_rowmajor_cols(dS, lds, dc, nc, di, M, ds, dg, J, dD, ldd, nullptr));
}
// src [ncol x lds] (lds >= M) -> dest (io) [ncol x ndst]: dest[t][idx[p]] = src[t][p].  ncol beyond the launcher's limit is
// handed to it as it is (its refusal is what a test asks for); nothing is launched then.
LC_HOOK lc_test_scatter_cols(const double* src, i64 lds, int ncol, double* dest, i64 ndst, const i64* idx, i64 M) {
  if (!src || !dest || !idx || ncol < 1 || ncol > 64 || M < 0 || M > lds || ndst < 1) return -1;
  for (i64 p = 0; p < M; ++p)
    if (idx[p] < 0 || idx[p] >= ndst) return -1;
  Scope s;
  const double* dS = s.in(src, (size_t)ncol * (size_t)lds);
  double* dD = s.io(dest, (size_t)ncol * (size_t)ndst);
  const int64_t* di = reinterpret_cast<const int64_t*>(s.in(idx, (size_t)M));
  if (!s.ok()) return s.finish(hipSuccess);
  std::vector<double*> dp((size_t)ncol);
  for (int t = 0; t < ncol; ++t) dp[(size_t)t] = dD + (size_t)t * (size_t)ndst;
  return s.finish(lck::launch_scatter_cols(dS, lds, ncol, dp.data(), di, M, nullptr));
}

// ---- split search: initial split, augmentation, transpose -----------------------------------------------------------
// X [NP x DP]; mv [2 DP]; q (io) [2 x ldq]; rginfo [NP / 16] or null (then nrows); thr [ngroups] (mode 2)
LC_HOOK lc_test_split_init(const double* X, int DP, int D, i64 NP, const int* rginfo, i64 nrows, int ngroups, const double* mv,
                           double* q, i64 ldq, int mode, const double* thr) {
  if (!X || !mv || !q || DP < 16 || DP % 16 || D < 1 || D > DP || NP < 1 || NP > ldq || mode < 0 || mode > 2 || ngroups < 1) return -1;
  if (rginfo ? (NP % RG || !rginfo_ok(rginfo, NP / RG, ngroups)) : (nrows < 0 || nrows > NP)) return -1;
  if (mode == 2 && !thr) return -1;
  Scope s;
  const double* dX = s.in(X, (size_t)NP * DP);
  const int* drg = rginfo ? s.in(rginfo, (size_t)(NP / RG)) : nullptr;
  const double* dmv = s.in(mv, (size_t)2 * DP);
  const double* dthr = thr ? s.in(thr, (size_t)ngroups) : nullptr;
  double* dq = s.io(q, (size_t)2 * (size_t)ldq);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_split_init(dX, DP, D, NP, drg, nrows, dmv, dq, ldq, mode, dthr, nullptr));
}
// q (io) [(K + 1) x ldq] (rows < NP <= ldq); qsub1 [nsub]; qhash (io) [NP] or null
LC_HOOK lc_test_aug_from_sub(double* q, i64 ldq, i64 NP, int k, int K, const i64* idx, i64 M, const i64* starts,
                             const i64* goff_sub, int J, const double* qsub1, i64 nsub, i64* qhash) {
  if (!q || !qsub1 || K < 1 || k < 0 || k >= K || NP > ldq || !selection_ok(idx, M, NP, starts, goff_sub, J, nsub)) return -1;
  Scope s;
  double* dq = s.io(q, (size_t)(K + 1) * (size_t)ldq);
  const int64_t* di = reinterpret_cast<const int64_t*>(s.in(idx, (size_t)M));
  const int64_t* ds = reinterpret_cast<const int64_t*>(s.in(starts, (size_t)J + 1));
  const int64_t* dg = reinterpret_cast<const int64_t*>(s.in(goff_sub, (size_t)J + 1));
  const double* dsub = s.in(qsub1, (size_t)nsub);
  int64_t* dh = qhash ? reinterpret_cast<int64_t*>(s.io(qhash, (size_t)NP)) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_aug_from_sub(dq, ldq, k, K, di, M, ds, dg, J, dsub, nullptr, dh));
}
// qZ [K x ldq] -> qT (io) [nqt >= NP * K]
LC_HOOK lc_test_transpose_qz(const double* qZ, i64 ldq, int K, i64 NP, double* qT, i64 nqt) {
  if (!qZ || !qT || K < 1 || NP < 1 || NP > ldq || nqt < NP * K) return -1;
  Scope s;
  const double* dq = s.in(qZ, (size_t)K * (size_t)ldq);
  double* dT = s.io(qT, (size_t)nqt);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_transpose_qz(dq, ldq, K, NP, dT, nullptr));
}

// ---- model selection: the normalisation sweep, fingerprints, the bounded pass ---------------------------------------------
// dcache [Kc x ldc]; fresh [nfresh x ldf] or null; colmap [K] or null; ctab [J x K]; rginfo [NP / 16] or null (then nrows);
// qZ (io) [Kq x ldq], Kq >= K; fz_part (io) [nblk]; optional, all io: ll_part [nblk x K], dq [NP x ldd], amax [NP],
// qhash [NP], rmax [NP], ramax [NP], colmask [2].  nblk must equal softmax_cached_grid(NP).
// K beyond the launcher's limit goes to the launcher as it is: it refuses and launches nothing.
LC_HOOK lc_test_softmax_cached(const double* dcache, int Kc, i64 ldc, const double* fresh, int nfresh, i64 ldf, const int* colmap,
                               const double* ctab, int J, int K, const int* rginfo, i64 nrows, i64 NP, double* qZ, int Kq, i64 ldq,
                               double* fz_part, i64 nblk, double* ll_part, double* dq, i64 ldd, double* amax, i64* qhash,
                               int qhash_in, double* rmax, int* ramax, unsigned long long* colmask) {
  if (!dcache || !ctab || !qZ || !fz_part || K < 1 || K > 4096 || Kc < 1 || J < 1 || NP < 1 || Kq < K) return -1;
  if (NP > ldc || NP > ldq || nblk != lck::softmax_cached_grid(NP)) return -1;
  if (fresh ? (nfresh < 1 || NP > ldf) : nfresh != 0) return -1;
  for (int j = 0; j < K; ++j) {
    const int cm = colmap ? colmap[j] : j;
    if (cm >= 0 ? cm >= Kc : -(i64)cm - 1 >= nfresh) return -1;
  }
  if (rginfo ? (NP % RG || !rginfo_ok(rginfo, NP / RG, J)) : (nrows < 0 || nrows > NP)) return -1;
  if (dq ? (!amax || ldd < K) : (amax || qhash || colmask)) return -1;
  if (!rmax != !ramax) return -1;
  Scope s;
  lck::CachedNormLaunch a{};
  a.dcache = s.in(dcache, (size_t)Kc * (size_t)ldc);
  a.ldc = ldc;
  a.fresh = fresh ? s.in(fresh, (size_t)nfresh * (size_t)ldf) : nullptr;
  a.ldf = ldf;
  a.colmap = colmap ? s.in(colmap, (size_t)K) : nullptr;
  a.ctab = s.in(ctab, (size_t)J * (size_t)K);
  a.K = K;
  a.rginfo = rginfo ? s.in(rginfo, (size_t)(NP / RG)) : nullptr;
  a.nrows = nrows;
  a.NP = NP;
  a.qZ = s.io(qZ, (size_t)Kq * (size_t)ldq);
  a.ldq = ldq;
  a.fz_part = s.io(fz_part, (size_t)nblk);
  a.ll_part = ll_part ? s.io(ll_part, (size_t)nblk * (size_t)K) : nullptr;
  a.dq = dq ? s.io(dq, (size_t)NP * (size_t)ldd) : nullptr;
  a.ldd = ldd;
  a.amax = amax ? s.io(amax, (size_t)NP) : nullptr;
  a.qhash = qhash ? reinterpret_cast<int64_t*>(s.io(qhash, (size_t)NP)) : nullptr;
  a.qhash_in = qhash_in;
  a.rmax = rmax ? s.io(rmax, (size_t)NP) : nullptr;
  a.ramax = ramax ? s.io(ramax, (size_t)NP) : nullptr;
  a.colmask = colmask ? s.io(colmask, (size_t)2) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_softmax_cached(a, nullptr));
}
// qZ [K x ldq], qhash [NP] -> *bad
LC_HOOK lc_test_qhash_verify(const double* qZ, i64 ldq, int K, i64 NP, const i64* qhash, unsigned long long* bad) {
  if (!qZ || !qhash || !bad || K < 1 || NP < 1 || NP > ldq) return -1;
  Scope s;
  const double* dq = s.in(qZ, (size_t)K * (size_t)ldq);
  const int64_t* dh = reinterpret_cast<const int64_t*>(s.in(qhash, (size_t)NP));
  *bad = 0;
  unsigned long long* db = s.io(bad, 1);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_qhash_verify(dq, ldq, K, NP, dh, db, nullptr));
}
// dst (io) [Kdst x ldq], src [K x ldq], dhash (io) [NP], shash [NP]
LC_HOOK lc_test_qz_resync(double* dst, const double* src, i64 ldq, int K, int Kdst, i64 NP, i64* dhash, const i64* shash) {
  if (!dst || !src || !dhash || !shash || K < 1 || Kdst < K || NP < 1 || NP > ldq) return -1;
  Scope s;
  double* dd = s.io(dst, (size_t)Kdst * (size_t)ldq);
  const double* ds = s.in(src, (size_t)K * (size_t)ldq);
  int64_t* dh = reinterpret_cast<int64_t*>(s.io(dhash, (size_t)NP));
  const int64_t* sh = reinterpret_cast<const int64_t*>(s.in(shash, (size_t)NP));
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_qz_resync(dd, ds, ldq, K, Kdst, NP, dh, sh, nullptr));
}
// ref [ncol x NP], dest (io) [ncol x NP], sigma / bnorm / cnew [ncol], rmax [NP], ramax [NP] (any value: the kernel treats
// an index outside [0, K) as "recompute"), usable [K], dcj [K], need (io) [NP].  ncol or K beyond the launcher's limits
// go to the launcher (with the first BOUND_MAX_COLS / BOUND_MAX_K entries of the tables): it refuses and launches nothing.
LC_HOOK lc_test_bound_select(int ncol, int K, i64 NP, const double* ref, double* dest, const double* sigma, const double* bnorm,
                             const double* cnew, const double* rmax, const int* ramax, double T, const unsigned char* usable,
                             const double* dcj, double* need) {
  if (!ref || !dest || !sigma || !bnorm || !cnew || !rmax || !ramax || !usable || !dcj || !need) return -1;
  if (ncol < 1 || ncol > 64 || K < 1 || K > 4096 || NP < 1) return -1;
  Scope s;
  lck::BoundSelectLaunch a{};
  a.ncol = ncol;
  a.K = K;
  a.NP = NP;
  const double* dref = s.in(ref, (size_t)ncol * (size_t)NP);
  double* ddest = s.io(dest, (size_t)ncol * (size_t)NP);
  for (int t = 0; t < ncol && t < lck::BOUND_MAX_COLS; ++t) {
    a.ref[t] = dref + (size_t)t * (size_t)NP;
    a.dest[t] = ddest + (size_t)t * (size_t)NP;
    a.sigma[t] = sigma[t];
    a.bnorm[t] = bnorm[t];
    a.cnew[t] = cnew[t];
  }
  for (int j = 0; j < K && j < lck::BOUND_MAX_K; ++j) {
    a.usable[j] = usable[j];
    a.dcj[j] = dcj[j];
  }
  a.rmax = s.in(rmax, (size_t)NP);
  a.ramax = s.in(ramax, (size_t)NP);
  a.T = T;
  a.need = s.io(need, (size_t)NP);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_bound_select(a, nullptr));
}

// ---- prediction (lc_kernels_predict.hip) ------------------------------------------------------------------------------------
// col (io; qcol == col) [ncols x ldq], ncols >= max(K, Kp); rginfo [nrg] or null (then nrows, J = 1); ctab [J x K];
// ptab [J x Kp], pscale / pexp [Kp] (null when Kp = 0); label / logZ / logp (io) [nrg * 16]
LC_HOOK lc_test_predict_rows(double* col, int ncols, i64 ldq, int K, int Kp, i64 nrg, const int* rginfo, i64 nrows, int J,
                             const double* ctab, const double* ptab, const double* pscale, const double* pexp, int keep_q,
                             int* label, double* logZ, double* logp) {
  if (!col || !ctab || !label || !logZ || !logp || K < 1 || Kp < 0 || ncols < K || ncols < Kp || ncols > 4096) return -1;
  if (Kp > 0 && (!ptab || !pscale || !pexp)) return -1;
  if (!pred_rows_ok(nrg, ldq, rginfo, nrows, J) || (!rginfo && J != 1)) return -1;
  const size_t NP = (size_t)(nrg * RG);
  Scope s;
  lck::PredictRowsLaunch a;
  double* dcol = s.io(col, (size_t)ncols * (size_t)ldq);
  a.col = dcol;
  a.qcol = dcol;
  a.ldq = ldq;
  a.K = K;
  a.Kp = Kp;
  a.nrg = nrg;
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.nrows = nrows;
  a.ctab = s.in(ctab, (size_t)J * K);
  a.ptab = Kp ? s.in(ptab, (size_t)J * Kp) : nullptr;
  a.pscale = Kp ? s.in(pscale, (size_t)Kp) : nullptr;
  a.pexp = Kp ? s.in(pexp, (size_t)Kp) : nullptr;
  a.keep_q = keep_q ? 1 : 0;
  a.label = s.io(label, NP);
  a.logZ = s.io(logZ, NP);
  a.logp = s.io(logp, NP);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_predict_rows(a, nullptr));
}
// X [nrg * 16 x DP]; a / w [Kp x DP]; ptab [J x Kp]; pexp [Kp]; logp (io) [nrg * 16]; flag (io) one int.  A DP that is no
// multiple of PRED_RENORM goes to the launcher as it is (its refusal is what a test asks for; nothing is launched then).
LC_HOOK lc_test_predict_diag(int mode, const double* X, int DP, i64 nrg, const int* rginfo, i64 nrows, int J, int Kp,
                             const double* a_, const double* w, const double* ptab, const double* pexp, double* logp, int* flag) {
  if (!X || !a_ || !w || !ptab || !pexp || !logp || !flag || (mode != 0 && mode != 1) || DP < 1 || DP > 4096 || Kp < 1) return -1;
  if (!pred_rows_ok(nrg, nrg * RG, rginfo, nrows, J) || (!rginfo && J != 1)) return -1;
  const size_t NP = (size_t)(nrg * RG);
  Scope s;
  lck::PredictDiagLaunch a;
  a.mode = mode;
  a.X = s.in(X, NP * DP);
  a.DP = DP;
  a.nrg = nrg;
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.nrows = nrows;
  a.Kp = Kp;
  a.a = s.in(a_, (size_t)Kp * DP);
  a.w = s.in(w, (size_t)Kp * DP);
  a.ptab = s.in(ptab, (size_t)J * Kp);
  a.pexp = s.in(pexp, (size_t)Kp);
  a.logp = s.io(logp, NP);
  a.flag = s.io(flag, 1);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_predict_diag(a, nullptr));
}
// X [nrg * 16 x DP]; col (io) [Kp x ldq]; ttab [J x Kp]; pscale / pexp [Kp]; mext [Kp x Dae]; T [Kp x Dae x Dbp]; mean (io)
// [nrg * 16 x Db]; logp (io) [nrg * 16].  A combination of widths that launch_predict_cond refuses (its own conditions,
// restated here) has no array sizes: it goes to the launcher with the numbers alone and no buffer, and nothing is launched.
LC_HOOK lc_test_predict_cond(const double* X, int DP, int Da, int Dae, int Db, int Dbp, int Kp, double* col, i64 ldq, i64 nrg,
                             const int* rginfo, i64 nrows, int J, const double* ttab, const double* pscale, const double* pexp,
                             const double* mext, const double* T, double* mean, double* logp) {
  if (!X || !col || !ttab || !pscale || !pexp || !mext || !T || !mean || !logp) return -1;
  if (!pred_rows_ok(nrg, ldq, rginfo, nrows, J) || (!rginfo && J != 1)) return -1;
  lck::PredictCondLaunch a;
  a.DP = DP;
  a.Da = Da;
  a.Dae = Dae;
  a.Db = Db;
  a.Dbp = Dbp;
  a.Kp = Kp;
  a.ldq = ldq;
  a.nrg = nrg;
  a.nrows = nrows;
  if (Kp < 1 || Da < 1 || Db < 1 || DP < Da || Dae < Da + 1 || Dae % 4 != 0 || Dbp < Db || Dbp % 4 != 0)
    return (int)lck::launch_predict_cond(a, nullptr);
  if (Kp > 4096 || DP > 4096 || Dae > 4096 || Dbp > 4096) return -1;
  const size_t NP = (size_t)(nrg * RG);
  Scope s;
  a.X = s.in(X, NP * DP);
  a.col = s.io(col, (size_t)Kp * (size_t)ldq);
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.ttab = s.in(ttab, (size_t)J * Kp);
  a.pscale = s.in(pscale, (size_t)Kp);
  a.pexp = s.in(pexp, (size_t)Kp);
  a.mext = s.in(mext, (size_t)Kp * Dae);
  a.T = s.in(T, (size_t)Kp * Dae * Dbp);
  a.mean = s.io(mean, NP * Db);
  a.logp = s.io(logp, NP);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_predict_cond(a, nullptr));
}

// (lcx_: tests/aux_hooks.py declares every lc_test_* export, and this one is bound by its own test file.)
// launch_loo_rows, then (worst and value given) launch_loo_worst on what it left (lc_kernels_loo.hip; tests/test_gpu_loo_kernels.py).
// X [nrg * 16 x DP]; col [Kp x ldq]; ttab [J x Kp]; pscale / pexp [Kp]; gnu [Kp] or null (no variance: var has to be null
// too); mean / hlogp / ipd [Kp x DP]; P [Kp x DP x DP]; logp [nrg * 16].  cond, cmean and var (io) are guard + nrg * 16 * DP +
// guard doubles, worst (io) guard + nrg * 16 + guard ints and value (io) as many doubles: the kernels see the middle part, the
// guards come back as they went in.
LC_HOOK lcx_test_loo_rows(const double* X, int DP, int D, int Kp, const double* col, i64 ldq, i64 nrg, const int* rginfo, i64 nrows,
                          int J, const double* ttab, const double* pscale, const double* pexp, const double* gnu,
                          const double* mean, const double* P, const double* hlogp, const double* ipd, const double* logp,
                          i64 guard, double* cond, double* cmean, double* var, int* worst, double* value) {
  if (!X || !col || !ttab || !pscale || !pexp || !mean || !P || !hlogp || !ipd || !logp || !cond || !cmean) return -1;
  if ((var != nullptr) != (gnu != nullptr) || (worst != nullptr) != (value != nullptr)) return -1;
  if (!pred_rows_ok(nrg, ldq, rginfo, nrows, J) || (!rginfo && J != 1)) return -1;
  if (Kp < 1 || Kp > 4096 || D < 1 || DP < D || DP > 4096 || DP % 16 != 0 || guard < 0 || guard > (1 << 20)) return -1;
  const size_t NP = (size_t)(nrg * RG), G = (size_t)guard;
  Scope s;
  lck::LooRowsLaunch a;
  a.X = s.in(X, NP * DP);
  a.DP = DP;
  a.D = D;
  a.Kp = Kp;
  a.col = s.in(col, (size_t)Kp * (size_t)ldq);
  a.ldq = ldq;
  a.nrg = nrg;
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.nrows = nrows;
  a.ttab = s.in(ttab, (size_t)J * Kp);
  a.pscale = s.in(pscale, (size_t)Kp);
  a.pexp = s.in(pexp, (size_t)Kp);
  a.gnu = gnu ? s.in(gnu, (size_t)Kp) : nullptr;
  a.mean = s.in(mean, (size_t)Kp * DP);
  a.P = s.in(P, (size_t)Kp * DP * DP);
  a.hlogp = s.in(hlogp, (size_t)Kp * DP);
  a.ipd = s.in(ipd, (size_t)Kp * DP);
  a.logp = s.in(logp, NP);
  double* dcond = s.io(cond, NP * DP + 2 * G);
  double* dmean = s.io(cmean, NP * DP + 2 * G);
  double* dvar = var ? s.io(var, NP * DP + 2 * G) : nullptr;
  int* dworst = worst ? s.io(worst, NP + 2 * G) : nullptr;
  double* dvalue = value ? s.io(value, NP + 2 * G) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  a.cond = dcond + G;
  a.cmean = dmean + G;
  a.var = dvar ? dvar + G : nullptr;
  hipError_t e = lck::launch_loo_rows(a, nullptr);
  if (e == hipSuccess && worst) {
    lck::LooWorstLaunch w;
    w.cond = a.cond;
    w.DP = DP;
    w.D = D;
    w.nrg = nrg;
    w.rginfo = a.rginfo;
    w.nrows = nrows;
    w.worst = dworst + G;
    w.value = dvalue + G;
    e = lck::launch_loo_worst(w, nullptr);
  }
  return s.finish(e);
}

// ---- document inference (lc_kernels_topic.hip) ----------------------------------------------------------------------------------
// topic_infer_lds itself: the bytes of dynamic LDS (0: K and T do not fit; *tile_cap and *e_lds are then untouched)
LC_HOOK lc_test_topic_plan(int K, int T, int threads, const i64* nrows, int docs, i64* tile_cap, int* e_lds) {
  if (!tile_cap || !e_lds || K < 1 || T < 1 || K > (1 << 20) || T > (1 << 20) || threads < 64 || threads > 1024 || docs < 0 ||
      (docs > 0 && !nrows))
    return -1;
  for (int i = 0; i < docs; ++i)
    if (nrows[i] < 0 || nrows[i] > ((i64)1 << 40)) return -1;
  int64_t cap = *tile_cap;
  const size_t lds = lck::topic_infer_lds(K, T, threads, reinterpret_cast<const int64_t*>(nrows), docs, &cap, e_lds);
  *tile_cap = cap;
  return (int)lds;
}
// col (io) [K x ldq]; goff / nrows [docs]: document i owns the rows goff[i] ... goff[i] + nrows[i], inside NP <= ldq and
// disjoint from every other document's; a [docs x T]; E [T x K]; label / logZ (io) [NP]; qY (io) [docs x T]; F / dint (io)
// [docs x 2].  threads = 0: chosen as Context::topic_infer does.  The plan (LDS bytes, tile_cap, e_lds) is topic_infer_lds';
// lds_request > 0 replaces the byte count and must exceed it (a test of the launcher's upper limit).  K, T, max_sweeps or
// threads that launch_topic_infer refuses go to it with the numbers alone and no buffer: nothing is launched.
LC_HOOK lc_test_topic_infer(double* col, i64 ldq, i64 NP, int K, int T, int docs, const i64* goff, const i64* nrows, const double* a_,
                            const double* E, int max_sweeps, double tol, int keep_q, int threads, i64 lds_request, int* label,
                            double* logZ, double* qY, double* F, int* dint) {
  if (!col || !E || !label || !logZ || docs < 0 || NP < 0 || NP > ldq) return -1;
  if (docs > 0 && (!goff || !nrows || !a_ || !qY || !F || !dint)) return -1;
  i64 maxN = 0;
  std::vector<std::pair<i64, i64>> span;
  for (int i = 0; i < docs; ++i) {
    if (nrows[i] < 0 || goff[i] < 0 || goff[i] > NP || nrows[i] > NP - goff[i]) return -1;
    maxN = std::max(maxN, nrows[i]);
    if (nrows[i]) span.emplace_back(goff[i], goff[i] + nrows[i]);
  }
  std::sort(span.begin(), span.end());
  for (size_t i = 1; i < span.size(); ++i)
    if (span[i].first < span[i - 1].second) return -1;
  lck::TopicInferLaunch l;
  l.threads = threads ? threads : maxN <= 64 ? 64 : maxN <= 128 ? 128 : 256;
  l.ldq = ldq;
  l.K = K;
  l.T = T;
  l.docs = docs;
  l.max_sweeps = max_sweeps;
  l.tol = tol;
  l.keep_q = keep_q ? 1 : 0;
  if (docs > 0 && (K < 1 || T < 1 || max_sweeps < 1 || (l.threads != 64 && l.threads != 128 && l.threads != 256)))
    return (int)lck::launch_topic_infer(l, 0, nullptr);
  if (K < 1 || T < 1 || K > 4096 || T > 4096) return -1;
  int64_t cap = 0;
  int el = 0;
  size_t lds = lck::topic_infer_lds(K, T, l.threads, reinterpret_cast<const int64_t*>(nrows), docs, &cap, &el);
  if (lds == 0) return -1;
  if (lds_request != 0) {
    if (lds_request <= (i64)lds) return -1;
    lds = (size_t)lds_request;
  }
  l.tile_cap = cap;
  l.e_lds = el;
  Scope s;
  l.col = s.io(col, (size_t)K * (size_t)ldq);
  l.goff = reinterpret_cast<const int64_t*>(s.in(goff, (size_t)docs));
  l.nrows = reinterpret_cast<const int64_t*>(s.in(nrows, (size_t)docs));
  l.a = s.in(a_, (size_t)docs * T);
  l.E = s.in(E, (size_t)T * K);
  l.label = s.io(label, (size_t)NP);
  l.logZ = s.io(logZ, (size_t)NP);
  l.qY = s.io(qY, (size_t)docs * T);
  l.F = s.io(F, (size_t)docs * 2);
  l.dint = s.io(dint, (size_t)docs * 2);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_topic_infer(l, lds, nullptr));
}

// ---- launch plans (lc_kernels.h: SuffstatPlan, EstepPlan) ----------------------------------------------------------------------
// suffstat_plan itself: out [7] = route, nchunks, chunk_rows, extra, klast0, KR, clusters per block; name [32]
LC_HOOK lc_test_suffstat_plan(int DP, int DC, i64 NP, int K, int mode, i64* out, char* name) {
  if (!out || !name || K < 1 || NP < 1 || mode < 0 || mode > 3) return -1;
  const lck::SuffstatPlan p = lck::suffstat_plan(DP, DC, NP, K, (lck::SuffstatMode)mode);
  out[0] = p.route, out[1] = p.nchunks, out[2] = p.chunk_rows, out[3] = p.extra, out[4] = p.klast0, out[5] = p.KR;
  out[6] = p.clusters_per_block;
  snprintf(name, 32, "%s", p.name);
  return 0;
}
// An E-step launch that no instance serves: *grid = estep_grid, the return value is launch_estep's.  The launch carries
// numbers alone and no buffer, so a launch that estep_plan accepts is not handed on (-1): nothing is ever launched here.
LC_HOOK lc_test_estep_refusal(int DP, int DC, int K, int raw, int sparse, i64 nrg, i64* grid) {
  if (!grid || K < 1 || nrg < 1) return -1;
  lck::EstepLaunch a{};
  a.DP = DP;
  a.DC = DC;
  a.K = K;
  a.raw = raw ? 1 : 0;
  a.sparse = sparse ? 1 : 0;
  a.nrg = nrg;
  if (lck::estep_plan(a).ok) return -1;
  *grid = lck::estep_grid(a);
  return (int)lck::launch_estep(a, nullptr);
}

// ---- the hot path: E-step, statistics pass, fused pass (tests/test_gpu_hot_kernels.py) ---------------------------------------------
namespace {

// widths a Gauss-Wishart launch can have: the padded layouts, and for the narrow ones the active widths with an instance
bool gw_width_ok(int DP, int DC) {
  if (DP > 128) return DP % 64 == 0 && DP <= lck::GW_MAX_DP && (DC == 0 || DC == DP);
  if (DP < 16 || lck::padded_dim(DP) != DP) return false;
  return DC == 0 || DC == DP || (DP >= 32 && DC == DP - 8) || ((DP == 32 || DP == 48) && (DC == DP - 4 || DC == DP - 12));
}
constexpr size_t HOT_LDS_LIMIT = 160 * 1024;  // gfx950: LDS a workgroup can be granted
constexpr i64 HOT_MAX_NRG = (i64)1 << 22;     // 64M rows: far beyond any test, keeps every product below 2^63

}  // namespace

// estep_plan itself: out [8] = ok, rows_per_block, grid, four_groups, DC, lq_lds, lds_bytes, estep_pstride(DP, DC) (-1 when !ok)
LC_HOOK lc_test_estep_plan(int DP, int DC, int K, int raw, int sparse, i64 nrg, i64* out) {
  if (!out || K < 1 || nrg < 1 || DP < 1 || DC < 0) return -1;
  lck::EstepLaunch a{};
  a.DP = DP;
  a.DC = DC;
  a.K = K;
  a.raw = raw ? 1 : 0;
  a.sparse = sparse ? 1 : 0;
  a.nrg = nrg;
  const lck::EstepPlan p = lck::estep_plan(a);
  out[0] = p.ok ? 1 : 0, out[1] = p.rows_per_block, out[2] = p.grid, out[3] = p.four_groups ? 1 : 0, out[4] = p.DC;
  out[5] = p.lq_lds, out[6] = (i64)p.lds_bytes;
  out[7] = p.ok ? (i64)lck::estep_pstride(DP, p.DC) : -1;
  return 0;
}
// X [nrg * 16 x DP]; params [K x estep_pstride(DP, DC)]; ctab [J x K]; rginfo [nrg] or null (then nrows, J = 1); qZ (io)
// [Kbuf x ldq], Kbuf >= K, ldq >= nrg * 16; fz_part (io) [nfz >= grid]; ll_part (io) [nll >= grid * K] or null.  A launch
// estep_plan refuses comes back as -1 (lc_test_estep_refusal hands those to the launcher, without buffers).
LC_HOOK lc_test_estep(const double* X, int DP, int DC, i64 nrg, const double* params, const double* ctab, int J, const int* rginfo,
                      i64 nrows, int K, int raw, int sparse, double* qZ, int Kbuf, i64 ldq, double* fz_part, i64 nfz, double* ll_part,
                      i64 nll) {
  if (!X || !params || !ctab || !qZ || !fz_part || K < 1 || K > 4096 || Kbuf < K || Kbuf > 8192 || J < 1 || J > (1 << 20)) return -1;
  if (nrg < 1 || nrg > HOT_MAX_NRG || ldq < nrg * RG || !gw_width_ok(DP, DC)) return -1;
  if (rginfo ? !rginfo_ok(rginfo, nrg, J) : (J != 1 || nrows < 0 || nrows > nrg * RG)) return -1;
  lck::EstepLaunch a{};
  a.DP = DP;
  a.DC = DC;
  a.K = K;
  a.raw = raw ? 1 : 0;
  a.sparse = sparse ? 1 : 0;
  a.nrg = nrg;
  a.nrows = nrows;
  a.ldq = ldq;
  const lck::EstepPlan p = lck::estep_plan(a);
  if (!p.ok || p.grid < 1 || p.lds_bytes > HOT_LDS_LIMIT) return -1;
  if (nfz < p.grid || (ll_part && nll < p.grid * K)) return -1;
  Scope s;
  a.X = s.in(X, (size_t)(nrg * RG) * DP);
  a.params = s.in(params, (size_t)K * (size_t)lck::estep_pstride(DP, p.DC));
  a.ctab = s.in(ctab, (size_t)J * K);
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.qZ = s.io(qZ, (size_t)Kbuf * (size_t)ldq);
  a.fz_part = s.io(fz_part, (size_t)nfz);
  a.ll_part = ll_part ? s.io(ll_part, (size_t)nll) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_estep(a, nullptr));
}

// rec (io) [nrec doubles >= (K + extra) * SS]: launch_fold_extra alone
LC_HOOK lc_test_fold_extra(double* rec, i64 nrec, i64 SS, int K, int klast0, int extra) {
  if (!rec || SS < 1 || SS > ((i64)1 << 24) || K < 1 || K > 4096 || klast0 < 0 || klast0 >= K || extra < 0 || extra > 4096) return -1;
  if (nrec < (i64)(K + extra) * SS) return -1;
  Scope s;
  double* d = s.io(rec, (size_t)nrec);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_fold_extra(d, SS, K, klast0, extra, nullptr));
}

// One statistics pass as Context::suffstat runs it.  X [NP x DP]; qZ [K x ldq]; mode = SuffstatMode; rginfo [NP / 16] and
// smask [J x K] with SS_MASKED_DENSE (optional with SS_ZERO_SKIP, absent otherwise); SS_WORK_LIST: nitems items as the
// parallel arrays r0 / r1 / kofs / kcnt / rec0, klist [nklist], nrec records in all -- checked against what
// Context::build_sparse_worklist produces and suffstat_kernel relies on: row ranges inside NP made of whole row groups,
// 1 ... clusters_per_block clusters per item taken from klist, every cluster below K, the items' records disjoint and
// inside the buffer.  partial (io) [npartial >= records * stat_stride(DP)].  plan_out [7] = suffstat_plan's numbers (route
// first), computed here.  fold: the reductions Context::suffstat chains behind the pass (launch_reduce_partials, or
// launch_reduce_records for a work list; launch_fold_extra when the plan has extra records) into folded (io) [nfolded >= K * SS].
// lcx_test_suffstat_speck: the same with SuffstatLaunch::speck_skip given explicitly (0 / 1 / 2; 1 or 2 on a route without a
// skipping instance is launch_suffstat's to refuse); lc_test_suffstat follows the context's default: on where the plan takes the
// feature GEMM.  (lcx_: tests/aux_hooks.py declares every lc_test_* export, and this one is bound by its own test file.)
static int test_suffstat(const double* X, int DP, int DC, i64 NP, const double* qZ, int K, i64 ldq, int mode, const int* rginfo,
                         const unsigned char* smask, int J, int nitems, const i64* r0, const i64* r1, const int* kofs, const int* kcnt,
                         const i64* rec0, const int* klist, int nklist, int nrec_listed, int skip_listed, double* partial, i64 npartial,
                         int fold, double* folded, i64 nfolded, i64* plan_out, int speck_skip) {
  if (!X || !qZ || !partial || !plan_out || K < 1 || K > 4096 || mode < 0 || mode > 3 || !gw_width_ok(DP, DC)) return -1;
  if (NP < RG || NP % RG || NP > HOT_MAX_NRG * RG || ldq < NP || ldq % 2) return -1;  // (the quad and feature kernels read q in 16-byte pieces)
  const lck::SuffstatMode m = (lck::SuffstatMode)mode;
  const bool listed = m == lck::SS_WORK_LIST;
  const bool masked = !listed && smask != nullptr;
  if (m == lck::SS_DENSE && smask) return -1;
  if (m == lck::SS_MASKED_DENSE && !smask) return -1;
  if (masked && (!rginfo || J < 1 || J > (1 << 20) || !rginfo_ok(rginfo, NP / RG, J))) return -1;
  if (fold && (!folded || nfolded < (i64)K * lck::stat_stride(DP))) return -1;
  const lck::SuffstatPlan p = lck::suffstat_plan(DP, DC, NP, K, m);
  plan_out[0] = p.route, plan_out[1] = p.nchunks, plan_out[2] = p.chunk_rows, plan_out[3] = p.extra, plan_out[4] = p.klast0;
  plan_out[5] = p.KR, plan_out[6] = p.clusters_per_block;
  if (p.nchunks < 1 || p.chunk_rows < lck::SS_BR || p.chunk_rows % lck::SS_BR || (i64)p.nchunks * p.chunk_rows < NP) return -1;
  const i64 SS = lck::stat_stride(DP);
  i64 nrec = (i64)p.nchunks * p.KR;
  std::vector<lck::SSItem> items;
  std::vector<int> kptr, krec;
  if (listed) {
    if (!r0 || !r1 || !kofs || !kcnt || !rec0 || !klist || nitems < 1 || nklist < 1 || nrec_listed < 1) return -1;
    nrec = nrec_listed;
    for (int t = 0; t < nklist; ++t)
      if (klist[t] < 0 || klist[t] >= K) return -1;
    std::vector<char> used((size_t)nrec, 0);
    std::vector<std::vector<int>> recs((size_t)K);
    for (int i = 0; i < nitems; ++i) {
      if (r0[i] < 0 || r0[i] > r1[i] || r1[i] > NP || r0[i] % RG || r1[i] % RG) return -1;
      if (kcnt[i] < 1 || kcnt[i] > p.clusters_per_block || kofs[i] < 0 || kofs[i] > nklist - kcnt[i]) return -1;
      if (rec0[i] < 0 || rec0[i] > nrec - kcnt[i]) return -1;
      for (int t = 0; t < kcnt[i]; ++t) {
        if (used[(size_t)(rec0[i] + t)]) return -1;
        used[(size_t)(rec0[i] + t)] = 1;
        recs[(size_t)klist[kofs[i] + t]].push_back((int)(rec0[i] + t));
      }
      items.push_back(lck::SSItem{r0[i], r1[i], kofs[i], kcnt[i], rec0[i]});
    }
    kptr.assign((size_t)K + 1, 0);
    for (int k = 0; k < K; ++k) {
      krec.insert(krec.end(), recs[(size_t)k].begin(), recs[(size_t)k].end());
      kptr[(size_t)k + 1] = (int)krec.size();
    }
  }
  if (npartial < nrec * SS) return -1;
  Scope s;
  lck::SuffstatLaunch a{};
  a.DP = DP;
  a.DC = DC;
  a.X = s.in(X, (size_t)NP * DP);
  a.NP = NP;
  a.qZ = s.in(qZ, (size_t)K * (size_t)ldq);
  a.ldq = ldq;
  a.K = K;
  a.mode = m;
  a.rginfo = masked ? s.in(rginfo, (size_t)(NP / RG)) : nullptr;
  a.smask = masked ? s.in(smask, (size_t)J * K) : nullptr;
  a.partial = s.io(partial, (size_t)npartial);
  a.nchunks = p.nchunks;
  a.KR = p.KR;
  a.chunk_rows = p.chunk_rows;
  a.speck_skip = speck_skip < 0 ? (p.route == lck::SS_FEAT ? lck::speck_skip_mode() : 0) : speck_skip;
  const int* dkptr = nullptr;
  const int* dkrec = nullptr;
  if (listed) {
    a.items = s.in(items.data(), items.size());
    a.klist = s.in(klist, (size_t)nklist);
    a.nitems = nitems;
    a.skip_listed = skip_listed ? 1 : 0;
    if (fold) {
      dkptr = s.in(kptr.data(), kptr.size());
      dkrec = s.in(krec.data(), krec.size());
    }
  }
  double* dfold = fold ? s.io(folded, (size_t)nfolded) : nullptr;
  double* ext = fold && !listed && p.extra > 0 ? s.scratch<double>((size_t)p.KR * (size_t)SS) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  hipError_t e = lck::launch_suffstat(a, p, nullptr);
  if (e == hipSuccess && fold) {
    if (listed) {
      e = lck::launch_reduce_records(a.partial, SS, K, dkptr, dkrec, dfold, nullptr);
    } else if (p.extra > 0) {
      e = lck::launch_reduce_partials(a.partial, p.nchunks, (i64)p.KR * SS, ext, nullptr);
      if (e == hipSuccess) e = lck::launch_fold_extra(ext, SS, K, p.klast0, p.extra, nullptr);
      if (e == hipSuccess) e = hipMemcpyAsync(dfold, ext, (size_t)K * (size_t)SS * sizeof(double), hipMemcpyDeviceToDevice, nullptr);
    } else {
      e = lck::launch_reduce_partials(a.partial, p.nchunks, (i64)K * SS, dfold, nullptr);
    }
  }
  return s.finish(e);
}
LC_HOOK lc_test_suffstat(const double* X, int DP, int DC, i64 NP, const double* qZ, int K, i64 ldq, int mode, const int* rginfo,
                         const unsigned char* smask, int J, int nitems, const i64* r0, const i64* r1, const int* kofs, const int* kcnt,
                         const i64* rec0, const int* klist, int nklist, int nrec_listed, int skip_listed, double* partial, i64 npartial,
                         int fold, double* folded, i64 nfolded, i64* plan_out) {
  return test_suffstat(X, DP, DC, NP, qZ, K, ldq, mode, rginfo, smask, J, nitems, r0, r1, kofs, kcnt, rec0, klist, nklist, nrec_listed,
                       skip_listed, partial, npartial, fold, folded, nfolded, plan_out, -1);
}
LC_HOOK lcx_test_suffstat_speck(const double* X, int DP, int DC, i64 NP, const double* qZ, int K, i64 ldq, int mode, const int* rginfo,
                                const unsigned char* smask, int J, int nitems, const i64* r0, const i64* r1, const int* kofs,
                                const int* kcnt, const i64* rec0, const int* klist, int nklist, int nrec_listed, int skip_listed,
                               double* partial, i64 npartial, int fold, double* folded, i64 nfolded, i64* plan_out, int speck_skip) {
  if (speck_skip < 0 || speck_skip > 2) return -1;
  return test_suffstat(X, DP, DC, NP, qZ, K, ldq, mode, rginfo, smask, J, nitems, r0, r1, kofs, kcnt, rec0, klist, nklist, nrec_listed,
                       skip_listed, partial, npartial, fold, folded, nfolded, plan_out, speck_skip);
}

// lcx_test_suffstat_lists: the list route of a skipping pass on a dense launch (launch_suffstat_list_build alone with sums = 0,
// launch_suffstat_lists otherwise; the launchers refuse what has no instance).  plan_out [7] as above.  The lists come back
// as lens_out (io) [nlens >= nchunks * quads] and ent_out (io) [nent >= nchunks * quads * chunk_rows]: segment (chunk, quad)
// starts at (chunk * quads + quad) * chunk_rows and only its first lens entries are written; -2: a length outside its segment.
// partial (io), fold / folded (io) as in lc_test_suffstat.  (lcx_: bound by its own test file, like the hook above.)
static int test_suffstat_lists(const double* X, int DP, int DC, i64 NP, const double* qZ, int K, i64 ldq, int sums, double* partial,
                               i64 npartial, int fold, double* folded, i64 nfolded, i64* plan_out, int* lens_out, i64 nlens, int* ent_out,
                               i64 nent, i64 chunk_rows) {
  if (!X || !qZ || !partial || !plan_out || !lens_out || !ent_out || K < 1 || K > 4096 || !gw_width_ok(DP, DC)) return -1;
  if (NP < RG || NP % RG || NP > HOT_MAX_NRG * RG || ldq < NP || ldq % 2 || chunk_rows < 0 || chunk_rows % lck::SS_BR) return -1;
  const i64 SS = lck::stat_stride(DP);
  if (fold && (!sums || !folded || nfolded < (i64)K * SS)) return -1;
  lck::SuffstatPlan p = lck::suffstat_plan(DP, DC, NP, K, lck::SS_DENSE);
  if (chunk_rows > 0) {  // (the caller's chunking in place of the plan's: chunks of more than 65536 rows have 32-bit entries)
    p.chunk_rows = chunk_rows;
    p.nchunks = (int)((NP + chunk_rows - 1) / chunk_rows);
  }
  plan_out[0] = p.route, plan_out[1] = p.nchunks, plan_out[2] = p.chunk_rows, plan_out[3] = p.extra, plan_out[4] = p.klast0;
  plan_out[5] = p.KR, plan_out[6] = p.clusters_per_block;
  if (p.nchunks < 1 || p.chunk_rows < lck::SS_BR || p.chunk_rows % lck::SS_BR || (i64)p.nchunks * p.chunk_rows < NP) return -1;
  const lck::SsListLayout lay = lck::ss_list_layout(p.nchunks, p.chunk_rows, K);
  const i64 nseg = (i64)p.nchunks * lay.nq;
  if (npartial < (i64)p.nchunks * p.KR * SS || nlens < nseg || nent < nseg * p.chunk_rows) return -1;
  Scope s;
  lck::SuffstatLaunch a{};
  a.DP = DP;
  a.DC = DC;
  a.X = s.in(X, (size_t)NP * DP);
  a.NP = NP;
  a.qZ = s.in(qZ, (size_t)K * (size_t)ldq);
  a.ldq = ldq;
  a.K = K;
  a.mode = lck::SS_DENSE;
  a.rginfo = nullptr;
  a.smask = nullptr;
  a.partial = s.io(partial, (size_t)npartial);
  a.nchunks = p.nchunks;
  a.KR = p.KR;
  a.chunk_rows = p.chunk_rows;
  unsigned char* lists = s.scratch<unsigned char>(lay.bytes);
  double* dfold = fold ? s.io(folded, (size_t)nfolded) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  hipError_t e = hipMemset(lists, 0xff, lay.bytes);
  if (e == hipSuccess)
    e = sums ? lck::launch_suffstat_lists(a, p, lists, lay.bytes, nullptr) : lck::launch_suffstat_list_build(a, p, lists, lay.bytes, nullptr);
  if (e == hipSuccess && fold) e = lck::launch_reduce_partials(a.partial, p.nchunks, (i64)K * SS, dfold, nullptr);
  const int rc = s.finish(e);
  if (rc != 0) return rc;
  std::vector<unsigned char> raw(lay.bytes);
  if (hipMemcpy(raw.data(), lists, lay.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const int* lens = reinterpret_cast<const int*>(raw.data());
  for (i64 g = 0; g < nseg; ++g)
    if (lens[g] < 0 || lens[g] > p.chunk_rows) return -2;
  for (i64 g = 0; g < nseg; ++g) {
    lens_out[g] = lens[g];
    for (int i = 0; i < lens[g]; ++i) {
      const size_t at = (size_t)g * (size_t)p.chunk_rows + (size_t)i;
      ent_out[at] = lay.wide ? (int)reinterpret_cast<const unsigned*>(raw.data() + lay.ent_off)[at]
                             : (int)reinterpret_cast<const unsigned short*>(raw.data() + lay.ent_off)[at];
    }
  }
  return 0;
}

LC_HOOK lcx_test_suffstat_lists(const double* X, int DP, int DC, i64 NP, const double* qZ, int K, i64 ldq, int sums, double* partial,
                                i64 npartial, int fold, double* folded, i64 nfolded, i64* plan_out, int* lens_out, i64 nlens, int* ent_out,
                                i64 nent) {
  return test_suffstat_lists(X, DP, DC, NP, qZ, K, ldq, sums, partial, npartial, fold, folded, nfolded, plan_out, lens_out, nlens, ent_out,
                             nent, 0);
}
// The same with the caller's rows per chunk (a multiple of the staging batch; as many chunks as cover NP) in place of the plan's:
// plan_out [1], [2] report them.  (tests/test_gpu_stats_owner_lists.py: a chunk of more than 65536 rows has 32-bit entries.)
LC_HOOK lcx_test_suffstat_lists_chunked(const double* X, int DP, int DC, i64 NP, const double* qZ, int K, i64 ldq, i64 chunk_rows,
                                        double* partial, i64 npartial, double* folded, i64 nfolded, i64* plan_out, int* lens_out, i64 nlens,
                                        int* ent_out, i64 nent) {
  if (chunk_rows < 1) return -1;
  return test_suffstat_lists(X, DP, DC, NP, qZ, K, ldq, 1, partial, npartial, 1, folded, nfolded, plan_out, lens_out, nlens, ent_out, nent,
                             chunk_rows);
}

// ---- kept-quad masks (EstepLaunch::qmask; tests/test_gpu_estep_masks.py binds these) -------------------------------------------
// lc_test_estep with a mask buffer: qmask (io) [nmask >= quads of K x nrg] or null -- the launcher refuses the pointer on a
// launch whose plan does not emit (hipErrorInvalidValue comes back as such).  Everything else as lc_test_estep.
LC_HOOK lcx_test_estep_masks(const double* X, int DP, int DC, i64 nrg, const double* params, const double* ctab, int J, const int* rginfo,
                             i64 nrows, int K, double* qZ, int Kbuf, i64 ldq, double* fz_part, i64 nfz, double* ll_part, i64 nll,
                             unsigned short* qmask, i64 nmask, int* emits) {
  if (!X || !params || !ctab || !qZ || !fz_part || !emits || K < 1 || K > 4096 || Kbuf < K || Kbuf > 8192 || J < 1 || J > (1 << 20)) return -1;
  if (nrg < 1 || nrg > HOT_MAX_NRG || ldq < nrg * RG || !gw_width_ok(DP, DC)) return -1;
  if (rginfo ? !rginfo_ok(rginfo, nrg, J) : (J != 1 || nrows < 0 || nrows > nrg * RG)) return -1;
  if (qmask && nmask < (i64)((K + 3) / 4) * nrg) return -1;
  lck::EstepLaunch a{};
  a.DP = DP;
  a.DC = DC;
  a.K = K;
  a.nrg = nrg;
  a.nrows = nrows;
  a.ldq = ldq;
  const lck::EstepPlan p = lck::estep_plan(a);
  if (!p.ok || p.grid < 1 || p.lds_bytes > HOT_LDS_LIMIT) return -1;
  if (nfz < p.grid || (ll_part && nll < p.grid * K)) return -1;
  *emits = p.emits ? 1 : 0;
  Scope s;
  a.X = s.in(X, (size_t)(nrg * RG) * DP);
  a.params = s.in(params, (size_t)K * (size_t)lck::estep_pstride(DP, p.DC));
  a.ctab = s.in(ctab, (size_t)J * K);
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.qZ = s.io(qZ, (size_t)Kbuf * (size_t)ldq);
  a.fz_part = s.io(fz_part, (size_t)nfz);
  a.ll_part = ll_part ? s.io(ll_part, (size_t)nll) : nullptr;
  a.qmask = qmask ? s.io(qmask, (size_t)nmask) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_estep(a, nullptr));
}

// The two list builders side by side.  qZ [K x ldq]; qmask [quads x NP / 16] (the masks of that qZ: the caller's business);
// chunk_rows > 0: that many rows per chunk (a multiple of 4) and as many chunks as cover NP, instead of the plan's.
// which = 0: launch_suffstat_list_build (reads qZ), 1: launch_suffstat_list_build_masks (reads qmask).  out [2] = nchunks,
// chunk_rows; lens_out / ent_out as lcx_test_suffstat_lists hands them back; -2: a length outside its segment.
LC_HOOK lcx_test_list_build(int which, const double* qZ, int DC, i64 NP, int K, i64 ldq, const unsigned short* qmask, i64 chunk_rows,
                            i64* out, int* lens_out, i64 nlens, int* ent_out, i64 nent) {
  const int DP = 64;
  if (!qZ || !qmask || !out || !lens_out || !ent_out || K < 1 || K > 4096 || !gw_width_ok(DP, DC)) return -1;
  if (NP < RG || NP % RG || NP > HOT_MAX_NRG * RG || ldq < NP || chunk_rows < 0 || chunk_rows % 4) return -1;
  lck::SuffstatPlan p = lck::suffstat_plan(DP, DC, NP, K, lck::SS_DENSE);
  if (chunk_rows > 0) {
    p.chunk_rows = chunk_rows;
    p.nchunks = (int)((NP + chunk_rows - 1) / chunk_rows);
  }
  if (p.nchunks < 1 || p.chunk_rows < 4 || (i64)p.nchunks * p.chunk_rows < NP) return -1;
  out[0] = p.nchunks, out[1] = p.chunk_rows;
  const lck::SsListLayout lay = lck::ss_list_layout(p.nchunks, p.chunk_rows, K);
  const i64 nseg = (i64)p.nchunks * lay.nq, nrg = NP / RG;
  if (nlens < nseg || nent < nseg * p.chunk_rows) return -1;
  Scope s;
  lck::SuffstatLaunch a{};
  a.DP = DP;
  a.DC = DC;
  a.X = s.scratch<double>(16);  // (the builders never read X; the launchers' checks want a pointer)
  a.NP = NP;
  a.qZ = s.in(qZ, (size_t)K * (size_t)ldq);
  a.ldq = ldq;
  a.K = K;
  a.mode = lck::SS_DENSE;
  a.nchunks = p.nchunks;
  a.KR = p.KR;
  a.chunk_rows = p.chunk_rows;
  const unsigned short* dmask = s.in(qmask, (size_t)lay.nq * (size_t)nrg);
  unsigned char* lists = s.scratch<unsigned char>(lay.bytes);
  if (!s.ok()) return s.finish(hipSuccess);
  hipError_t e = hipMemset(lists, 0xff, lay.bytes);
  if (e == hipSuccess)
    e = which ? lck::launch_suffstat_list_build_masks(a, p, dmask, nrg, lists, lay.bytes, nullptr)
              : lck::launch_suffstat_list_build(a, p, lists, lay.bytes, nullptr);
  const int rc = s.finish(e);
  if (rc != 0) return rc;
  std::vector<unsigned char> raw(lay.bytes);
  if (hipMemcpy(raw.data(), lists, lay.bytes, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const int* lens = reinterpret_cast<const int*>(raw.data());
  for (i64 g = 0; g < nseg; ++g)
    if (lens[g] < 0 || lens[g] > p.chunk_rows) return -2;
  for (i64 g = 0; g < nseg; ++g) {
    lens_out[g] = lens[g];
    for (int i = 0; i < lens[g]; ++i) {
      const size_t at = (size_t)g * (size_t)p.chunk_rows + (size_t)i;
      ent_out[at] = lay.wide ? (int)reinterpret_cast<const unsigned*>(raw.data() + lay.ent_off)[at]
                             : (int)reinterpret_cast<const unsigned short*>(raw.data() + lay.ent_off)[at];
    }
  }
  return 0;
}

// The two probes side by side: which = 0: launch_speck_probe on qZ [K x ldq], 1: launch_speck_probe_masks on qmask [quads x NP / 16].
// out [4] = kept pairs, one-quad rows, pairs looked at, rows looked at.
LC_HOOK lcx_test_speck_probe(int which, const double* qZ, i64 ldq, int K, i64 NP, const unsigned short* qmask, i64* out) {
  if (!qZ || !qmask || !out || K < 1 || K > 4096 || NP < RG || NP % RG || NP > HOT_MAX_NRG * RG || ldq < NP || ldq % 2) return -1;
  const i64 nrg = NP / RG;
  Scope s;
  const double* dq = s.in(qZ, (size_t)K * (size_t)ldq);
  const unsigned short* dm = s.in(qmask, (size_t)((K + 3) / 4) * (size_t)nrg);
  int* act = s.scratch<int>(2);
  if (!s.ok()) return s.finish(hipSuccess);
  int64_t pairs = 0, rows = 0;
  const hipError_t e = which ? lck::launch_speck_probe_masks(dm, nrg, K, NP, act, &pairs, nullptr, &rows)
                             : lck::launch_speck_probe(dq, ldq, K, NP, act, &pairs, nullptr, &rows);
  const int rc = s.finish(e);
  if (rc != 0) return rc;
  int h[2] = {0, 0};
  if (hipMemcpy(h, act, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  out[0] = h[0], out[1] = h[1], out[2] = pairs, out[3] = rows;
  return 0;
}

// lcx_test_suffstat_list_deal: the list kernel's tile map (lck::ftl_feature) evaluated on the host, no device involved.
// info [6] = shared deal at this width (0 / 1), waves, tiles per wave, ftl_paired, ftl_split, the ones-column; feat (io)
// [nfeat >= waves * tiles * 16 * 4]: u, w, kind (FtKind), shared of lane l16 of tile t of wave v at ((v * tiles + t) * 16 + l16) * 4.
// -1: a width without a list instance.  (lcx_: bound by its own test file.)
LC_HOOK lcx_test_suffstat_list_deal(int DP, int DC, i64* info, int* feat, i64 nfeat) {
  if (!info || !feat || !gw_width_ok(DP, DC) || !lck::suffstat_list_instance(DP, DC)) return -1;
  const int dc = DC ? DC : DP, waves = 8, tiles = lck::ftl_tpw(dc);
  if (nfeat < (i64)waves * tiles * 16 * 4) return -1;
  info[0] = lck::ftl_shared(dc) ? 1 : 0, info[1] = waves, info[2] = tiles, info[3] = lck::ftl_paired(dc), info[4] = lck::ftl_split(dc);
  info[5] = DP;
  for (int v = 0; v < waves; ++v)
    for (int t = 0; t < tiles; ++t)
      for (int l = 0; l < 16; ++l) {
        const lck::FtlFeature f = lck::ftl_feature(dc, DP, v, t, l);
        int* o = feat + ((size_t)(v * tiles + t) * 16 + l) * 4;
        o[0] = f.u, o[1] = f.w, o[2] = f.kind, o[3] = f.shared;
      }
  return 0;
}

// lcx_test_suffstat_owner_deal: the owner kernel's map (lck::fto_feature) evaluated on the host, no device involved.
// info [3] = diagonals (FTO_DIAGS), accumulators of a lane (FTO_ACCS), 1 if this build routes DC = 64 lists to the owner
// kernel; feat (io) [nfeat >= FTO_ACCS * 64 * 3]: u, w, kind (FtKind) of lane l of accumulator t at (t * 64 + l) * 3.
LC_HOOK lcx_test_suffstat_owner_deal(i64* info, int* feat, i64 nfeat) {
  if (!info || !feat || nfeat < (i64)lck::FTO_ACCS * 64 * 3) return -1;
  info[0] = lck::FTO_DIAGS, info[1] = lck::FTO_ACCS, info[2] = lck::suffstat_owner_instance(64, 64) ? 1 : 0;
  for (int t = 0; t < lck::FTO_ACCS; ++t)
    for (int l = 0; l < 64; ++l) {
      const lck::FtFeature f = lck::fto_feature(l, t);
      int* o = feat + ((size_t)t * 64 + l) * 3;
      o[0] = f.u, o[1] = f.w, o[2] = f.kind;
    }
  return 0;
}

// out [4] = fused_eligible, fused_plan's grid, compute units of the device, fused_record(DP, K)
LC_HOOK lc_test_fused_plan(int DP, i64 nrg, int K, i64* out) {
  if (!out || K < 1 || K > 4096 || nrg < 0 || nrg > HOT_MAX_NRG || DP < 1 || DP > 1024) return -1;
  out[0] = lck::fused_eligible(DP, K) ? 1 : 0;
  out[1] = lck::fused_plan(DP, nrg, K);
  out[2] = lck::current_device_cus();
  out[3] = (i64)lck::fused_record(DP, K);
  return 0;
}
// X [nrg * 16 x 16]; params [K x pstride(16)]; ctab [J x K]; rginfo [nrg] or null (then nrows, J = 1); grid: 0 = fused_plan's,
// otherwise 1 <= grid <= fused_plan's (which never exceeds the number of 256-row tiles); qZ (io) [Kbuf x ldq]; partial (io)
// [npartial >= grid x fused_record(16, K)]; *grid_used: the blocks launched
LC_HOOK lc_test_fused(const double* X, int D, i64 nrg, const double* params, const double* ctab, int J, const int* rginfo, i64 nrows,
                      int K, int want_ll, int grid, double* qZ, int Kbuf, i64 ldq, double* partial, i64 npartial, int* grid_used) {
  const int DP = 16;
  if (!X || !params || !ctab || !qZ || !partial || !grid_used || D < 1 || D > DP || K < 1 || Kbuf < K || Kbuf > 8192) return -1;
  if (nrg < 1 || nrg > HOT_MAX_NRG || ldq < nrg * RG || J < 1 || J > (1 << 20) || !lck::fused_eligible(DP, K)) return -1;
  if (rginfo ? !rginfo_ok(rginfo, nrg, J) : (J != 1 || nrows < 0 || nrows > nrg * RG)) return -1;
  const int plan = lck::fused_plan(DP, nrg, K);
  if (plan < 1 || grid < 0 || grid > plan) return -1;
  const int g = grid ? grid : plan;
  if (npartial < (i64)g * lck::fused_record(DP, K)) return -1;
  *grid_used = g;
  Scope s;
  lck::FusedLaunch a{};
  a.DP = DP;
  a.D = D;
  a.X = s.in(X, (size_t)(nrg * RG) * DP);
  a.nrg = nrg;
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.nrows = nrows;
  a.params = s.in(params, (size_t)K * (size_t)lck::pstride(DP));
  a.ctab = s.in(ctab, (size_t)J * K);
  a.K = K;
  a.qZ = s.io(qZ, (size_t)Kbuf * (size_t)ldq);
  a.ldq = ldq;
  a.partial = s.io(partial, (size_t)npartial);
  a.want_ll = want_ll != 0;
  a.grid = g;
  a.ngroups = J;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_fused(a, nullptr));
}

// ---- the separable families: E-step (both paths) and statistics pass (tests/test_gpu_diag_kernels.py) ------------------------------
namespace {

bool diag_width_ok(int DP) { return DP >= 16 && (DP <= 128 ? DP % 16 == 0 : (DP % 64 == 0 && DP <= 1024)); }

void diag_estep_plan_out(const lck::DiagEstepPlan& p, i64* out, char* name) {
  out[0] = p.ok ? 1 : 0, out[1] = p.mfma ? 1 : 0, out[2] = p.mode, out[3] = p.grid, out[4] = (i64)p.lds_bytes;
  out[5] = p.wide ? 1 : 0, out[6] = p.KT, out[7] = p.REG ? 1 : 0, out[8] = p.NT, out[9] = p.QUAD ? 1 : 0, out[10] = p.R;
  out[11] = p.KTM, out[12] = p.instance, out[13] = p.nslots, out[14] = p.per_cu, out[15] = p.block_cap;
  if (name) snprintf(name, 32, "%s", p.name ? p.name : "");
}
void diag_stat_plan_out(const lck::DiagStatPlan& p, i64* out, char* name) {
  out[0] = p.ok ? 1 : 0, out[1] = p.nslice, out[2] = p.rsplit, out[3] = p.second, out[4] = p.nblocks, out[5] = p.width;
  out[6] = p.last_width, out[7] = p.BR, out[8] = p.BR_last, out[9] = p.nstage ? 1 : 0, out[10] = p.nstage_last ? 1 : 0;
  out[11] = p.deep ? 1 : 0, out[12] = p.deep_last ? 1 : 0, out[13] = (i64)p.lds_bytes;
  if (name) snprintf(name, 32, "%s", p.name ? p.name : "");
}
constexpr int DIAG_SINK = 256, DIAG_SINK_GUARD = 64;

}  // namespace

// estep_diag_plan itself, of a launch described by numbers alone (mfma / want_ll / grouped: whether wt / ll_part / rginfo
// would be set): out [16] = ok, mfma, mode, grid, lds_bytes, wide, KT, REG, NT, QUAD, R, KTM, instance, nslots, per_cu,
// block_cap; name [32].  The matrix-pipe plan asks the device for its compute units.
LC_HOOK lc_test_estep_diag_plan(int DP, int K, int mode, i64 nrg, int mfma, int raw, int want_ll, int grouped, int ngroups,
                                i64* out, char* name) {
  if (!out || !name || K < 1 || K > 4096 || nrg < 0 || nrg > HOT_MAX_NRG || DP < 1 || DP > 1024 || mode < 0 || mode > 2 || ngroups < 1)
    return -1;
  static double some;
  static int somei;
  lck::DiagEstepLaunch a{};
  a.DP = DP, a.D = DP, a.K = K, a.mode = mode, a.nrg = nrg, a.raw = raw ? 1 : 0, a.ngroups = ngroups;
  a.wt = mfma ? &some : nullptr;
  a.ll_part = want_ll ? &some : nullptr;
  a.rginfo = grouped ? &somei : nullptr;
  diag_estep_plan_out(lck::estep_diag_plan(a), out, name);
  return 0;
}
// One launch_estep_diag.  X [nrg * 16 x DP]; params [3][K][DP] (a, w2, w1); ctab [J x K]; rginfo [nrg] or null (then nrows,
// J = 1); wt null: the difference-form kernels; otherwise wt [nwt = estep_diag_mfma_weights(DP, K, mode) > 0], mu [DP]
// (mode 2: may be null), constk [K] and sink (io) [256 + 64 guard doubles].  qZ (io) [Kbuf x ldq]; fz_part (io) [nfz >=
// estep_diag_grid(nrg)]; ll_part (io) [nll >= estep_diag_grid(nrg) x K] or null.  plan_out [16] / name [32] as
// lc_test_estep_diag_plan.  A launch whose dynamic LDS exceeds what a workgroup can be granted is refused here.
LC_HOOK lc_test_estep_diag(const double* X, int DP, i64 nrg, const double* params, int mode, const double* ctab, int J,
                           const int* rginfo, i64 nrows, int K, int raw, const double* wt, i64 nwt, const double* mu,
                           const double* constk, double* qZ, int Kbuf, i64 ldq, double* fz_part, i64 nfz, double* ll_part, i64 nll,
                           double* sink, i64* plan_out, char* name) {
  if (!X || !params || !ctab || !qZ || !fz_part || !plan_out || !name || K < 1 || K > 4096 || Kbuf < K || Kbuf > 8192) return -1;
  if (J < 1 || J > (1 << 20) || mode < 0 || mode > 2 || nrg < 1 || nrg > HOT_MAX_NRG || nrg * RG > ldq) return -1;
  if (!diag_width_ok(DP)) return -1;
  if (rginfo ? !rginfo_ok(rginfo, nrg, J) : (J != 1 || nrows < 0 || nrows > nrg * RG)) return -1;
  if (wt) {
    const i64 nw = lck::estep_diag_mfma_weights(DP, K, mode);
    if (nw <= 0 || nwt != nw || !constk || !sink || (mode != 2 && !mu)) return -1;
  } else if (nwt != 0 || mu || constk || sink) {
    return -1;
  }
  lck::DiagEstepLaunch a{};
  a.DP = DP, a.D = DP, a.K = K, a.mode = mode, a.nrg = nrg, a.nrows = nrows, a.raw = raw ? 1 : 0, a.ngroups = J, a.ldq = ldq;
  static double some;
  a.wt = wt ? &some : nullptr;
  a.ll_part = ll_part ? &some : nullptr;
  a.rginfo = rginfo;
  const lck::DiagEstepPlan p = lck::estep_diag_plan(a);
  diag_estep_plan_out(p, plan_out, name);
  if (!p.ok || p.grid < 1 || p.grid > p.nslots || p.lds_bytes > HOT_LDS_LIMIT) return -1;
  if (nfz < p.nslots || (ll_part && nll < p.nslots * K)) return -1;
  Scope s;
  a.X = s.in(X, (size_t)(nrg * RG) * DP);
  a.params = s.in(params, (size_t)3 * K * DP);
  a.ctab = s.in(ctab, (size_t)J * K);
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.qZ = s.io(qZ, (size_t)Kbuf * (size_t)ldq);
  a.fz_part = s.io(fz_part, (size_t)nfz);
  a.ll_part = ll_part ? s.io(ll_part, (size_t)nll) : nullptr;
  a.wt = nullptr;
  if (wt) {
    a.wt = s.in(wt, (size_t)nwt);
    std::vector<double> zero((size_t)DP, 0.0);
    a.mu = s.in(mu ? mu : zero.data(), (size_t)DP);
    a.constk = s.in(constk, (size_t)K);
    a.sink = s.io(sink, (size_t)(DIAG_SINK + DIAG_SINK_GUARD));
  }
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_estep_diag(a, nullptr));
}

// suffstat_diag_plan itself: out [14] = ok, nslice, rsplit, second, nblocks, width, last_width, BR, BR_last, nstage,
// nstage_last, deep, deep_last, lds_bytes; name [32]
LC_HOOK lc_test_suffstat_diag_plan(int DP, int K, int second, i64* out, char* name) {
  if (!out || !name) return -1;
  diag_stat_plan_out(lck::suffstat_diag_plan(DP, K, second), out, name);
  return 0;
}
// One launch_suffstat_diag.  X [NP x DP]; qZ [K x ldq]; rginfo [NP / 16] and smask [J x K] together or neither; partial (io)
// [npartial >= nchunks x rsplit x K x (1 + 2 DP)]; fold: the launch_reduce_partials Context::suffstat_diag chains behind
// it, into folded (io) [nfolded >= K x (1 + 2 DP)].  plan_out [14] as lc_test_suffstat_diag_plan.
LC_HOOK lc_test_suffstat_diag(const double* X, int DP, i64 NP, const double* qZ, int K, i64 ldq, const int* rginfo,
                              const unsigned char* smask, int J, int nchunks, i64 chunk_rows, int second, double* partial,
                              i64 npartial, int fold, double* folded, i64 nfolded, i64* plan_out) {
  if (!X || !qZ || !partial || !plan_out || K < 1 || K > 4096 || !diag_width_ok(DP)) return -1;
  if (NP < RG || NP % RG || NP > HOT_MAX_NRG * RG || ldq < NP) return -1;
  if (nchunks < 1 || chunk_rows < 32 || chunk_rows % 32 || chunk_rows > HOT_MAX_NRG * RG) return -1;
  if (!((i64)(nchunks - 1) * chunk_rows < NP && NP <= (i64)nchunks * chunk_rows)) return -1;
  if ((smask != nullptr) != (rginfo != nullptr)) return -1;
  if (smask && (J < 1 || J > (1 << 20) || !rginfo_ok(rginfo, NP / RG, J))) return -1;
  const lck::DiagStatPlan p = lck::suffstat_diag_plan(DP, K, second);
  diag_stat_plan_out(p, plan_out, nullptr);
  if (!p.ok || p.lds_bytes > HOT_LDS_LIMIT) return -1;
  const i64 SS = 1 + 2 * (i64)DP;
  const i64 nparts = (i64)nchunks * p.rsplit;
  if (npartial < nparts * K * SS || nparts > (1 << 24)) return -1;
  if (fold && (!folded || nfolded < (i64)K * SS)) return -1;
  Scope s;
  lck::DiagStatLaunch a{};
  a.DP = DP;
  a.X = s.in(X, (size_t)NP * DP);
  a.NP = NP;
  a.qZ = s.in(qZ, (size_t)K * (size_t)ldq);
  a.ldq = ldq;
  a.K = K;
  a.rginfo = smask ? s.in(rginfo, (size_t)(NP / RG)) : nullptr;
  a.smask = smask ? s.in(smask, (size_t)J * K) : nullptr;
  a.partial = s.io(partial, (size_t)npartial);
  a.nchunks = nchunks;
  a.chunk_rows = chunk_rows;
  a.second = second ? 1 : 0;
  double* dfold = fold ? s.io(folded, (size_t)nfolded) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  hipError_t e = lck::launch_suffstat_diag(a, nullptr);
  if (e == hipSuccess && fold) e = lck::launch_reduce_partials(a.partial, (int)nparts, (i64)K * SS, dfold, nullptr);
  return s.finish(e);
}

// The host packer of the matrix-pipe path (no device): a / w2 / w1 [K x D] -> mu [DP], constk [K + 1], wt [nwt =
// estep_diag_mfma_weights(DP, K, mode) > 0], *cond (estep_diag_centre's figure)
LC_HOOK lc_test_diag_pack(int D, int DP, int K, int mode, const double* a_, const double* w2, const double* w1, double* mu,
                          double* constk, double* wt, i64 nwt, double* cond) {
  if (!a_ || !w2 || !w1 || !mu || !constk || !wt || !cond || K < 1 || K > 4096 || mode < 0 || mode > 2) return -1;
  if (D < 1 || D > DP || DP > 128 || DP % 16) return -1;
  const i64 nw = lck::estep_diag_mfma_weights(DP, K, mode);
  if (nw <= 0 || nwt != nw) return -1;
  *cond = lck::estep_diag_centre(D, DP, K, mode, a_, w2, mu);
  lck::estep_diag_pack(D, DP, K, mode, a_, w2, w1, mu, constk, wt, nw);
  return 0;
}

// estep_diag_mfma_weights itself (no device)
LC_HOOK lc_test_diag_weights(int DP, int K, int mode) { return (int)lck::estep_diag_mfma_weights(DP, K, mode); }

// ---- rows with holes (lc_kernels_holes.hip; tests/test_gpu_holes_kernels.py binds these) -----------------------------------------
namespace {

// row_valid (lc_device.hpp) on the host
bool host_row_valid(i64 row, const int* rginfo, i64 nrows, int& j) {
  const i64 g = row / RG;
  const int r = (int)(row - g * RG);
  j = rginfo ? rginfo[g] >> 5 : 0;
  const i64 rem = nrows - g * RG;
  const int nv = rginfo ? rginfo[g] & 31 : rem >= RG ? RG : rem > 0 ? (int)rem : 0;
  return r < nv;
}

// the hole records as predict_holes_kernel and holes_draws_kernel address X, P and their tables with them: per valid row
// 0 <= count <= HOLES_MAX and count < D, cols[0 .. count) ascending inside [0, D)
bool hole_records_ok(const int* count, const int* cols, i64 nrg, const int* rginfo, i64 nrows, int D) {
  for (i64 row = 0; row < nrg * RG; ++row) {
    int j;
    if (!host_row_valid(row, rginfo, nrows, j)) continue;
    const int cnt = count[row];
    if (cnt < 0 || cnt > lck::HOLES_MAX || cnt >= D) return false;
    for (int i = 0; i < cnt; ++i) {
      const int c = cols[row * lck::HOLES_MAX + i];
      if (c < 0 || c >= D || (i > 0 && c <= cols[row * lck::HOLES_MAX + i - 1])) return false;
    }
  }
  return true;
}

// what the three prediction hooks share: the numbers of a launch over filled rows
bool holes_launch_ok(int DP, int D, int Kp, i64 ldq, i64 nrg, const int* rginfo, i64 nrows, int J, i64 guard) {
  if (!pred_rows_ok(nrg, ldq, rginfo, nrows, J) || (!rginfo && J != 1)) return false;
  return Kp >= 1 && Kp <= 4096 && D >= 1 && DP >= D && DP <= 4096 && DP % 16 == 0 && guard >= 0 && guard <= (1 << 20);
}

// the arguments predict_holes_kernel reads, uploaded; X, col and logp (io) are guard + payload + guard
void holes_upload(Scope& s, lck::PredictHolesLaunch& a, double* X, int DP, int Kp, double* col, i64 ldq, i64 nrg, const int* rginfo,
                  i64 nrows, int J, const int* count, const int* cols, const double* ttab, const double* pscale,
                  const double* pexp, const double* mean, const double* P, size_t G, double* logp) {
  const size_t NP = (size_t)(nrg * RG), NH = lck::HOLES_MAX + 1;
  a.X = s.io(X, NP * DP + 2 * G) + G;
  a.DP = DP;
  a.Kp = Kp;
  a.col = s.io(col, (size_t)Kp * (size_t)ldq + 2 * G) + G;
  a.ldq = ldq;
  a.nrg = nrg;
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.nrows = nrows;
  a.count = s.in(count, NP);
  a.cols = s.in(cols, NP * lck::HOLES_MAX);
  a.ttab = s.in(ttab, (size_t)J * NH * Kp);
  a.pscale = s.in(pscale, (size_t)Kp);
  a.pexp = s.in(pexp, NH * Kp);
  a.mean = s.in(mean, (size_t)Kp * DP);
  a.P = s.in(P, (size_t)Kp * DP * DP);
  a.logp = s.io(logp, NP + 2 * G) + G;
}

}  // namespace

// launch_holes_scan, then (fill given) launch_holes_fill on what it left.  X (io) is guard + nrg * 16 * DP + guard doubles,
// count (io) guard + nrg * 16 + guard ints, cols (io) guard + nrg * 16 * HOLES_MAX + guard ints: the kernels see the middle
// part.  rginfo [nrg] or null (then nrows, J = 1); fill [D] or null; out (io) [3].
LC_HOOK lcx_test_holes_scan(double* X, int DP, int D, i64 nrg, const int* rginfo, i64 nrows, int J, const double* fill, i64 guard,
                            int* count, int* cols, unsigned long long* out) {
  if (!X || !count || !cols || !out) return -1;
  if (nrg < 1 || nrg > ((i64)1 << 30) / RG || J < 1 || (!rginfo && J != 1)) return -1;
  if (rginfo ? !rginfo_ok(rginfo, nrg, J) : (nrows < 0 || nrows > nrg * RG)) return -1;
  if (D < 1 || DP < D || DP > 4096 || DP % 16 != 0 || guard < 0 || guard > (1 << 20)) return -1;
  const size_t NP = (size_t)(nrg * RG), G = (size_t)guard;
  Scope s;
  double* dX = s.io(X, NP * DP + 2 * G);
  int* dcount = s.io(count, NP + 2 * G);
  int* dcols = s.io(cols, NP * lck::HOLES_MAX + 2 * G);
  const int* drg = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  const double* dfill = fill ? s.in(fill, (size_t)D) : nullptr;
  unsigned long long* dout = s.io(out, 3);
  if (!s.ok()) return s.finish(hipSuccess);
  lck::HolesScanLaunch a;
  a.X = dX + G;
  a.DP = DP;
  a.D = D;
  a.nrg = nrg;
  a.rginfo = drg;
  a.nrows = nrows;
  a.count = dcount + G;
  a.cols = dcols + G;
  a.out = dout;
  hipError_t e = lck::launch_holes_scan(a, nullptr);
  if (e == hipSuccess && fill) {  // (the scan's own records: every recorded column is below D)
    lck::HolesFillLaunch f;
    f.X = dX + G;
    f.DP = DP;
    f.nrg = nrg;
    f.rginfo = drg;
    f.nrows = nrows;
    f.count = a.count;
    f.cols = a.cols;
    f.fill = dfill;
    e = lck::launch_holes_fill(f, nullptr);
  }
  return s.finish(e);
}

// mode 0 / 1 / 2: launch_predict_holes / launch_predict_holes_var / launch_predict_holes_keep.  X [nrg * 16 x DP] filled, col
// [Kp x ldq] (read in all modes, written in mode 2) and logp [nrg * 16] are io, guard + payload + guard doubles; count
// [nrg * 16], cols [nrg * 16 x HOLES_MAX]; ttab [J x (HOLES_MAX + 1) x Kp]; pscale [Kp]; pexp [(HOLES_MAX + 1) x Kp]; mean
// [Kp x DP]; P [Kp x DP x DP]; mode 1 only: gnu [(HOLES_MAX + 1) x Kp] and var (io) guard + nrg * 16 * HOLES_MAX + guard.
LC_HOOK lcx_test_predict_holes(int mode, double* X, int DP, int D, int Kp, double* col, i64 ldq, i64 nrg, const int* rginfo,
                               i64 nrows, int J, const int* count, const int* cols, const double* ttab, const double* pscale,
                               const double* pexp, const double* mean, const double* P, const double* gnu, i64 guard,
                               double* logp, double* var) {
  if (mode < 0 || mode > 2 || !X || !col || !count || !cols || !ttab || !pscale || !pexp || !mean || !P || !logp) return -1;
  if ((gnu != nullptr) != (mode == 1) || (var != nullptr) != (mode == 1)) return -1;
  if (!holes_launch_ok(DP, D, Kp, ldq, nrg, rginfo, nrows, J, guard)) return -1;
  if (!hole_records_ok(count, cols, nrg, rginfo, nrows, D)) return -1;
  const size_t NP = (size_t)(nrg * RG), G = (size_t)guard;
  Scope s;
  lck::PredictHolesLaunch a;
  holes_upload(s, a, X, DP, Kp, col, ldq, nrg, rginfo, nrows, J, count, cols, ttab, pscale, pexp, mean, P, G, logp);
  const double* dgnu = gnu ? s.in(gnu, (size_t)(lck::HOLES_MAX + 1) * Kp) : nullptr;
  double* dvar = var ? s.io(var, NP * lck::HOLES_MAX + 2 * G) : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  if (mode == 0) return s.finish(lck::launch_predict_holes(a, nullptr));
  if (mode == 1) {
    lck::PredictHolesVarLaunch v;
    v.h = a;
    v.gnu = dgnu;
    v.var = dvar + G;
    return s.finish(lck::launch_predict_holes_var(v, nullptr));
  }
  lck::PredictHolesKeepLaunch k;
  k.h = a;
  k.tcol = const_cast<double*>(a.col);
  return s.finish(lck::launch_predict_holes_keep(k, nullptr));
}

// launch_predict_holes_keep, then launch_holes_draws on what it left.  The arguments of lcx_test_predict_holes (mode 2), goff
// [J + 1] or null, cqnu [Kp], ndraws, seed; draws (io) guard + nrg * 16 * max(ndraws, 1) * HOLES_MAX + guard doubles and label
// (io) guard + nrg * 16 * max(ndraws, 1) + guard ints, pre-filled by the caller with 0 / -1.  An ndraws outside 1 ...
// DRAWS_MAX (at most 128) goes to launch_holes_draws alone, with all buffers: its refusal is what a test asks for.
LC_HOOK lcx_test_holes_draws(double* X, int DP, int D, int Kp, double* col, i64 ldq, i64 nrg, const int* rginfo, i64 nrows, int J,
                             const int* count, const int* cols, const double* ttab, const double* pscale, const double* pexp,
                             const double* mean, const double* P, const i64* goff, const double* cqnu, int ndraws,
                             unsigned long long seed, i64 guard, double* logp, double* draws, int* label) {
  if (!X || !col || !count || !cols || !ttab || !pscale || !pexp || !mean || !P || !logp || !cqnu || !draws || !label) return -1;
  if (!holes_launch_ok(DP, D, Kp, ldq, nrg, rginfo, nrows, J, guard) || ndraws < 0 || ndraws > 128) return -1;
  if (!hole_records_ok(count, cols, nrg, rginfo, nrows, D)) return -1;
  const size_t NP = (size_t)(nrg * RG), G = (size_t)guard, nd = (size_t)(ndraws > 1 ? ndraws : 1);
  Scope s;
  lck::HolesDrawsLaunch v;
  holes_upload(s, v.h, X, DP, Kp, col, ldq, nrg, rginfo, nrows, J, count, cols, ttab, pscale, pexp, mean, P, G, logp);
  v.goff = goff ? reinterpret_cast<const int64_t*>(s.in(goff, (size_t)J + 1)) : nullptr;
  v.cqnu = s.in(cqnu, (size_t)Kp);
  v.ndraws = ndraws;
  v.seed = seed;
  v.draws = s.io(draws, NP * nd * lck::HOLES_MAX + 2 * G) + G;
  v.label = s.io(label, NP * nd + 2 * G) + G;
  if (!s.ok()) return s.finish(hipSuccess);
  hipError_t e = hipSuccess;
  if (ndraws >= 1 && ndraws <= lck::DRAWS_MAX) {
    lck::PredictHolesKeepLaunch k;
    k.h = v.h;
    k.tcol = const_cast<double*>(v.h.col);
    e = lck::launch_predict_holes_keep(k, nullptr);
  }
  if (e == hipSuccess) e = lck::launch_holes_draws(v, nullptr);
  return s.finish(e);
}

// ---- device-resident data in, row results out (lc_kernels_ingest.hip; tests/ingest_hooks.py, tests/test_gpu_ingest_kernels.py) ----
// launch_pack_rows over J host sources: src[j] is a buffer of src_elems[j] doubles in which element (n, d) of group j sits at
// n * rs + d * cs (checked here for every group with rows).  image (io) is guard + NP * DP + guard doubles as the caller filled
// them (NaN: every byte the kernel owes shows), NP = the groups' rows padded to 16 each, DP = padded_dim_wide(D); image_elems
// must say exactly that.  range (out) [2]: the raw words; min / n_nan (out): what data_range_decode makes of them.
LC_HOOK lcx_test_pack_rows(const double* const* src, const i64* src_elems, int J, const i64* Nj, int D, i64 rs, i64 cs, i64 guard,
                           double* image, i64 image_elems, unsigned long long* range, double* min, i64* n_nan) {
  if (!src || !src_elems || !Nj || !image || !range || !min || !n_nan) return -1;
  if (J < 1 || J > (1 << 20) || D < 1 || D > 4096 || rs < 1 || cs < 1 || rs > ((i64)1 << 30) || cs > ((i64)1 << 30)) return -1;
  if (guard < 0 || guard > (1 << 20)) return -1;
  const int DP = lck::padded_dim_wide(D);
  std::vector<int64_t> goff((size_t)J + 1, 0), tab(2 * (size_t)J, 0);
  for (int j = 0; j < J; ++j) {
    if (Nj[j] < 0 || Nj[j] > ((i64)1 << 30)) return -1;
    if (Nj[j] > 0 && (!src[j] || (Nj[j] - 1) * rs + (i64)(D - 1) * cs >= src_elems[j])) return -1;
    goff[(size_t)j + 1] = goff[(size_t)j] + (Nj[j] + RG - 1) / RG * RG;
  }
  const i64 NP = goff[(size_t)J];
  const size_t G = (size_t)guard;
  if (image_elems != NP * DP + 2 * guard) return -1;
  Scope s;
  for (int j = 0; j < J; ++j) {
    tab[(size_t)j] = Nj[j] > 0 ? (int64_t)reinterpret_cast<intptr_t>(s.in(src[j], (size_t)src_elems[j])) : 0;
    tab[(size_t)J + j] = Nj[j];
  }
  const int64_t* dtab = s.in(tab.data(), tab.size());
  lck::PackRowsLaunch a;
  a.J = J;
  a.D = D;
  a.DP = DP;
  a.NP = NP;
  a.src = reinterpret_cast<const double* const*>(dtab);
  a.Nj = dtab + J;
  a.goff = s.in(goff.data(), goff.size());
  a.rs = rs;
  a.cs = cs;
  a.X = s.io(image, (size_t)image_elems) + G;
  a.range = s.out(range, 2);
  if (!s.ok()) return s.finish(hipSuccess);
  const int rc = s.finish(lck::launch_pack_rows(a, nullptr));
  if (rc == 0) {
    int64_t nn = 0;
    lck::data_range_decode(range, min, &nn);
    *n_nan = nn;
  }
  return rc;
}

// launch_unpack_qz: rows [off, off + n) of the K columns of col [K x ldq] into q (io: guard + q_elems + guard doubles as the
// caller filled them), entry (r, k) at guard + r * rs + k * cs, which must lie inside the q_elems for every r < n, k < K.
LC_HOOK lcx_test_unpack_qz(const double* col, i64 ldq, int K, i64 off, i64 n, double* q, i64 q_elems, i64 guard, i64 rs, i64 cs) {
  if (!col || !q) return -1;
  if (K < 1 || K > 4096 || ldq < 1 || ldq > ((i64)1 << 30) || off < 0 || n < 0 || off > ldq - n) return -1;
  if (rs < 1 || cs < 1 || rs > ((i64)1 << 30) || cs > ((i64)1 << 30) || guard < 0 || guard > (1 << 20) || q_elems < 0) return -1;
  if (n > 0 && (n - 1) * rs + (i64)(K - 1) * cs >= q_elems) return -1;
  Scope s;
  lck::UnpackQzLaunch a;
  a.col = s.in(col, (size_t)K * (size_t)ldq) + off;
  a.ldq = ldq;
  a.n = n;
  a.K = K;
  a.q = s.io(q, (size_t)(q_elems + 2 * guard)) + guard;
  a.rs = rs;
  a.cs = cs;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_unpack_qz(a, nullptr));
}

// the whole padded image of a context (an lc_ctx*: the handle holds its lcc::Context first) -> out [NP x DP]; out_elems must
// say exactly that (np / dp, when given, report the two sizes either way)
LC_HOOK lcx_test_ctx_image(void* ctx, double* out, i64 out_elems, i64* np, int* dp) {
  if (!ctx) return -1;
  const lcc::Context* c = reinterpret_cast<const lcc::Context*>(ctx);
  if (np) *np = c->NP();
  if (dp) *dp = c->DP();
  if (!out) return out_elems == 0 ? 0 : -1;
  if (c->J() < 1 || out_elems != c->NP() * c->DP()) return -1;
  try {
    c->test_image(out);
  } catch (const std::exception&) {
    return (int)hipErrorUnknown;
  }
  return 0;
}

// ---- the samplers, ranking and threshold queries (lc_kernels_sample.hip, lc_kernels_rank.hip, lc_kernels_select.hip) -----------
// Bound by tests/test_gpu_sample_kernels.py and tests/test_gpu_rank_select_kernels.py.  Every hook: host arrays in, ONE launcher,
// host arrays out.  Outputs are guard + payload + guard elements as the caller filled them (a canary): the kernels see the middle
// part.  A combination the launcher refuses by its own conditions (restated here) goes to the launcher with the caller's host
// pointers, none of which is then used: nothing is launched, and its refusal is what the test asks for.
namespace {

bool guard_ok(i64 guard) { return guard >= 0 && guard <= (1 << 20); }

// the score columns of a ranking or threshold launch as the kernels address them: C columns of ld >= NP elements, NP a multiple
// of 16, rginfo [NP / 16] with counts 0 ... 16 or (null) 0 <= nrows <= NP, label [NP] or null
bool score_columns_ok(const double* col, i64 ld, int C, i64 NP, const int* rginfo, i64 nrows) {
  if (C < 1 || C > 4096 || NP < 0 || NP % RG != 0 || NP > ((i64)1 << 24) || ld < NP || ld > ((i64)1 << 25)) return false;
  if ((i64)C * ld > ((i64)1 << 26) || (ld > 0 && !col)) return false;
  return rginfo ? rginfo_ok(rginfo, NP / RG, (i64)1 << 26) : (nrows >= 0 && nrows <= NP);
}
void score_columns_upload(Scope& s, lck::ScoreColumns& c, const double* col, i64 ld, int C, i64 NP, const int* rginfo, i64 nrows,
                          const int* label, int label0) {
  c.col = s.in(col, (size_t)C * (size_t)ld);
  c.ld = ld;
  c.C = C;
  c.NP = NP;
  c.rginfo = rginfo ? s.in(rginfo, (size_t)(NP / RG)) : nullptr;
  c.nrows = nrows;
  c.label = label ? s.in(label, (size_t)NP) : nullptr;
  c.label0 = label0;
}
void score_columns_numbers(lck::ScoreColumns& c, const double* col, i64 ld, int C, i64 NP, const int* rginfo, i64 nrows,
                           const int* label, int label0) {
  c.col = col;
  c.ld = ld;
  c.C = C;
  c.NP = NP;
  c.rginfo = rginfo;
  c.nrows = nrows;
  c.label = label;
  c.label0 = label0;
}
// columns_ok of lc_kernels_select.hip, restated
bool select_columns_refused(int C, i64 NP, i64 ld) { return C < 1 || C > 65535 || NP < 0 || NP % RG != 0 || ld < NP; }

}  // namespace

// launch_sample.  rginfo [ceil(NP / 16)] with goff [J + 1], or both null (J = 1, the first nrows rows valid); cdf [J x Kp]; klast
// [J]; loc [Kp x D] (null in mode 2); fac [Kp x D x D] (mode 0) or [Kp x D]; shape [Kp].  X (io) guard + NP * DP + guard doubles,
// label (io) guard + NP + guard ints.
LC_HOOK lcx_test_sample(int mode, int D, int DP, int Kp, i64 NP, i64 nrows, i64 row_offset, unsigned long long seed, const int* rginfo,
                        const i64* goff, int J, const double* cdf, const int* klast, const double* loc, const double* fac,
                        const double* shape, i64 guard, double* X, int* label) {
  if (!X || !label || !guard_ok(guard) || NP < 1 || NP > ((i64)1 << 24) || J < 1 || J > (1 << 20)) return -1;
  lck::SampleLaunch a;
  a.mode = mode;
  a.DP = DP;
  a.D = D;
  a.Kp = Kp;
  a.nrows = nrows;
  a.NP = NP;
  a.row_offset = row_offset;
  a.seed = seed;
  if (Kp < 1 || D < 1 || DP < D || DP % 2 != 0 || !cdf || !klast || !fac || !shape || mode < 0 || mode > 2 || (mode != 2 && !loc)) {
    a.X = X;
    a.label = label;
    a.cdf = cdf;
    a.klast = klast;
    a.loc = loc;
    a.fac = fac;
    a.shape = shape;
    return (int)lck::launch_sample(a, nullptr);
  }
  if (Kp > 4096 || D > 1024 || DP > 1024 || row_offset < 0 || row_offset > ((i64)1 << 39)) return -1;
  const i64 nrg = (NP + RG - 1) / RG;
  if ((rginfo != nullptr) != (goff != nullptr) || (!rginfo && J != 1)) return -1;
  if (rginfo ? !rginfo_ok(rginfo, nrg, J) : (nrows < 0 || nrows > NP)) return -1;
  for (int j = 0; j < J; ++j)
    if (klast[j] < 0 || klast[j] >= Kp) return -1;
  const size_t G = (size_t)guard, nfac = mode == 0 ? (size_t)Kp * D * D : (size_t)Kp * D;
  Scope s;
  a.X = s.io(X, (size_t)NP * DP + 2 * G) + G;
  a.label = s.io(label, (size_t)NP + 2 * G) + G;
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.goff = goff ? reinterpret_cast<const int64_t*>(s.in(goff, (size_t)J + 1)) : nullptr;
  a.cdf = s.in(cdf, (size_t)J * Kp);
  a.klast = s.in(klast, (size_t)J);
  a.loc = loc ? s.in(loc, (size_t)Kp * D) : nullptr;
  a.fac = s.in(fac, nfac);
  a.shape = s.in(shape, (size_t)Kp);
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_sample(a, nullptr));
}

// launch_predict_cond_draws alone, on what predict_cond_kernel would have left: col [Kp x ldq] holds t_k and logp [nrg * 16] the
// row's log density, both the caller's.  X [nrg * 16 x DP]; ttab [J x Kp]; pexp / cq [Kp]; mext [Kp x Dae]; T [Kp x Dae x Dbp];
// Lt [Kp x Dbp x Dbp]; goff [J + 1] or null.  draws (io) guard + nrg * 16 * ndraws * Db + guard doubles, label (io) guard +
// nrg * 16 * ndraws + guard ints (ndraws counted as at least 1).
LC_HOOK lcx_test_cond_draws(const double* X, int DP, int Da, int Dae, int Db, int Dbp, int Kp, const double* col, i64 ldq, i64 nrg,
                            const int* rginfo, i64 nrows, int J, const double* ttab, const double* pexp, const double* mext,
                            const double* T, const double* logp, const i64* goff, const double* Lt, const double* cq, int ndraws,
                            unsigned long long seed, i64 guard, double* draws, int* label) {
  if (!X || !col || !ttab || !pexp || !mext || !T || !logp || !Lt || !cq || !draws || !label || !guard_ok(guard)) return -1;
  if (!pred_rows_ok(nrg, ldq, rginfo, nrows, J) || (!rginfo && J != 1) || (goff && !rginfo) || nrg > (1 << 16)) return -1;
  lck::PredictCondDrawsLaunch v;
  lck::PredictCondLaunch& a = v.c;
  a.DP = DP;
  a.Da = Da;
  a.Dae = Dae;
  a.Db = Db;
  a.Dbp = Dbp;
  a.Kp = Kp;
  a.ldq = ldq;
  a.nrg = nrg;
  a.nrows = nrows;
  v.ndraws = ndraws;
  v.seed = seed;
  if (Kp < 1 || Da < 1 || Db < 1 || DP < Da || Dae < Da + 1 || Dae % 4 != 0 || Dbp < Db || Dbp % 4 != 0 || ndraws < 1 ||
      ndraws > lck::DRAWS_MAX) {
    v.Lt = Lt;
    v.cq = cq;
    v.draws = draws;
    v.label = label;
    return (int)lck::launch_predict_cond_draws(v, nullptr);
  }
  if (Kp > 4096 || DP > 4096 || Dae > 4096 || Dbp > 4096) return -1;
  const size_t NP = (size_t)(nrg * RG), G = (size_t)guard;
  Scope s;
  a.X = s.in(X, NP * DP);
  a.col = const_cast<double*>(s.in(col, (size_t)Kp * (size_t)ldq));
  a.rginfo = rginfo ? s.in(rginfo, (size_t)nrg) : nullptr;
  a.ttab = s.in(ttab, (size_t)J * Kp);
  a.pexp = s.in(pexp, (size_t)Kp);
  a.mext = s.in(mext, (size_t)Kp * Dae);
  a.T = s.in(T, (size_t)Kp * Dae * Dbp);
  a.logp = const_cast<double*>(s.in(logp, NP));
  v.goff = goff ? reinterpret_cast<const int64_t*>(s.in(goff, (size_t)J + 1)) : nullptr;
  v.Lt = s.in(Lt, (size_t)Kp * Dbp * Dbp);
  v.cq = s.in(cq, (size_t)Kp);
  v.draws = s.io(draws, NP * ndraws * Db + 2 * G) + G;
  v.label = s.io(label, NP * ndraws + 2 * G) + G;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_predict_cond_draws(v, nullptr));
}

// launch_top_rows.  col [C x ld]; rginfo [NP / 16] or null (then nrows); label [NP] or null.  pkey / ppos (io) guard +
// top_rows_chunks(NP) * C * m + guard, out_score / out_pos (io) guard + C * m + guard.
LC_HOOK lcx_test_top_rows(const double* col, i64 ld, int C, i64 NP, const int* rginfo, i64 nrows, const int* label, int m, int largest,
                          int nchunks, i64 guard, double* pkey, long long* ppos, double* out_score, long long* out_pos) {
  if (!pkey || !ppos || !out_score || !out_pos || !guard_ok(guard)) return -1;
  lck::TopRowsLaunch a;
  a.ld = ld;
  a.C = C;
  a.NP = NP;
  a.nrows = nrows;
  a.m = m;
  a.largest = largest;
  a.nchunks = nchunks;
  if (m < 1 || m > lck::TOP_MAX_M || C < 1 || C > 65535 || NP < 0 || NP % RG != 0 || ld < NP || nchunks != lck::top_rows_chunks(NP)) {
    a.col = col;
    a.rginfo = rginfo;
    a.label = label;
    a.pkey = pkey;
    a.ppos = ppos;
    a.out_score = out_score;
    a.out_pos = out_pos;
    return (int)lck::launch_top_rows(a, nullptr);
  }
  if (!score_columns_ok(col, ld, C, NP, rginfo, nrows)) return -1;
  const size_t G = (size_t)guard, np = (size_t)nchunks * C * m;
  Scope s;
  a.col = s.in(col, (size_t)C * (size_t)ld);
  a.rginfo = rginfo ? s.in(rginfo, (size_t)(NP / RG)) : nullptr;
  a.label = label ? s.in(label, (size_t)NP) : nullptr;
  a.pkey = s.io(pkey, np + 2 * G) + G;
  a.ppos = s.io(ppos, np + 2 * G) + G;
  a.out_score = s.io(out_score, (size_t)C * m + 2 * G) + G;
  a.out_pos = s.io(out_pos, (size_t)C * m + 2 * G) + G;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_top_rows(a, nullptr));
}

// launch_score_select.  The columns of lcx_test_top_rows with label0; probs [nprobs].  hist (io) [C x SEL_HIST_WORDS] and state
// (io) [C x SEL_STATE_WORDS] go up as the caller filled them and come back whole; out (io) guard + C + 2 C nprobs + guard.
LC_HOOK lcx_test_score_select(const double* col, i64 ld, int C, i64 NP, const int* rginfo, i64 nrows, const int* label, int label0,
                              int nprobs, const double* probs, i64 guard, unsigned long long* hist, long long* state,
                              long long* out) {
  if (!probs || !out || !guard_ok(guard) || nprobs < 0 || nprobs > 64) return -1;
  lck::ScoreSelectLaunch a;
  a.nprobs = nprobs;
  for (int i = 0; i < nprobs && i < lck::SEL_MAX; ++i) a.probs[i] = probs[i];
  if (select_columns_refused(C, NP, ld) || NP == 0 || nprobs < 1 || nprobs > lck::SEL_MAX || !hist || !state) {
    score_columns_numbers(a.s, col, ld, C, NP, rginfo, nrows, label, label0);
    a.hist = hist;
    a.state = state;
    a.out = out;
    return (int)lck::launch_score_select(a, nullptr);
  }
  if (!score_columns_ok(col, ld, C, NP, rginfo, nrows)) return -1;
  const size_t G = (size_t)guard;
  Scope s;
  score_columns_upload(s, a.s, col, ld, C, NP, rginfo, nrows, label, label0);
  a.hist = s.io(hist, (size_t)C * lck::SEL_HIST_WORDS);
  a.state = s.io(state, (size_t)C * lck::SEL_STATE_WORDS);
  a.out = s.io(out, (size_t)C + 2 * (size_t)C * nprobs + 2 * G) + G;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_score_select(a, nullptr));
}

// launch_score_counts.  thr [nthr]; out (io) guard + C * (1 + nthr) + guard raw words, as the caller filled them.
LC_HOOK lcx_test_score_counts(const double* col, i64 ld, int C, i64 NP, const int* rginfo, i64 nrows, const int* label, int label0,
                              int nthr, const double* thr, i64 guard, unsigned long long* out) {
  if (!thr || !out || !guard_ok(guard) || nthr < 0 || nthr > 64) return -1;
  lck::ScoreCountsLaunch a;
  a.nthr = nthr;
  for (int i = 0; i < nthr && i < lck::SEL_MAX; ++i) a.thr[i] = thr[i];
  if (select_columns_refused(C, NP, ld) || nthr < 1 || nthr > lck::SEL_MAX) {
    score_columns_numbers(a.s, col, ld, C, NP, rginfo, nrows, label, label0);
    a.out = out;
    return (int)lck::launch_score_counts(a, nullptr);
  }
  if (!score_columns_ok(col, ld, C, NP, rginfo, nrows)) return -1;
  const size_t G = (size_t)guard;
  Scope s;
  score_columns_upload(s, a.s, col, ld, C, NP, rginfo, nrows, label, label0);
  a.out = s.io(out, (size_t)C * (1 + (size_t)nthr) + 2 * G) + G;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_score_counts(a, nullptr));
}

// launch_rows_beyond.  One column [ld]; chunkoff (io) guard + top_rows_chunks(NP) + guard, total (io) [1], pos / score (io) guard
// + capacity + guard each (or null).
LC_HOOK lcx_test_rows_beyond(const double* col, i64 ld, int C, i64 NP, const int* rginfo, i64 nrows, const int* label, int label0,
                             double thr, int above, i64 capacity, int nchunks, i64 guard, long long* chunkoff, long long* total,
                             long long* pos, double* score) {
  if (!chunkoff || !total || !guard_ok(guard) || capacity < 0 || capacity > ((i64)1 << 24)) return -1;
  lck::RowsBeyondLaunch a;
  a.thr = thr;
  a.above = above;
  a.capacity = capacity;
  a.nchunks = nchunks;
  if (select_columns_refused(C, NP, ld) || C != 1 || nchunks != lck::top_rows_chunks(NP) || (capacity > 0 && (!pos || !score))) {
    score_columns_numbers(a.s, col, ld, C, NP, rginfo, nrows, label, label0);
    a.chunkoff = chunkoff;
    a.total = total;
    a.pos = pos;
    a.score = score;
    return (int)lck::launch_rows_beyond(a, nullptr);
  }
  if (!score_columns_ok(col, ld, C, NP, rginfo, nrows)) return -1;
  const size_t G = (size_t)guard;
  Scope s;
  score_columns_upload(s, a.s, col, ld, C, NP, rginfo, nrows, label, label0);
  a.chunkoff = s.io(chunkoff, (size_t)nchunks + 2 * G) + G;
  a.total = s.io(total, 1);
  a.pos = pos ? s.io(pos, (size_t)capacity + 2 * G) + G : nullptr;
  a.score = score ? s.io(score, (size_t)capacity + 2 * G) + G : nullptr;
  if (!s.ok()) return s.finish(hipSuccess);
  return s.finish(lck::launch_rows_beyond(a, nullptr));
}
