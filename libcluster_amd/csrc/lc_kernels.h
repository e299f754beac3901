// Internal launcher interface between the C-ABI layer and the gfx950 kernels.
// Everything here is plain pointers + sizes; all pointers are DEVICE pointers
// unless a name ends in _h.  Launchers enqueue on `stream` and do not sync.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lck {

// ---- data layout constants -------------------------------------------------
// X on device: row-major [NP x DP] doubles, DP = D rounded up to a multiple of 16 up to 128 (a multiple of 64 beyond that),
// pad columns zero.  Groups are padded to multiples of 16 rows (a "row-group"),
// pad rows zero.  qZ on device: column-major, qZ[k*ldq + row], ldq = NP.
constexpr int RG = 16;  // rows per row-group (one MFMA column block)

inline int padded_dim(int D) {
  return D <= 16 ? 16 : D <= 32 ? 32 : D <= 48 ? 48 : D <= 64 ? 64 : D <= 80 ? 80 : D <= 96 ? 96 : D <= 112 ? 112 : D <= 128 ? 128 : -1;
}
// LDS row stride (doubles) of a staged X batch in the statistics kernels: DP + 16 puts the two rows a ds_read_b64
// half-wave touches on disjoint banks when the stride is 16 mod 32; 48, 80 and 112 need 32 more for that (16 keeps
// the stride it was tuned with)
// (DP = 16: no padding at all -- 32 dwords per row put the two rows of a half-wave on the two halves of the 64 banks;
// the DP + 16 = 32 doubles of round 2 put them on the SAME banks: the bank conflicts of suffstat_kernel<16> in its profile)
__host__ __device__ constexpr int lds_row_stride(int DP) { return DP == 16 ? 16 : (DP + 16) % 32 != 16 ? DP + 32 : DP + 16; }
// wider observations are padded to a multiple of 64 columns: the separable (diagonal / exponential) families process
// them in 128-column blocks with a possible half block at the end (any D), the Gauss-Wishart kernels in 64-column
// panels / 64 x 64 whitener blocks
inline int padded_dim_wide(int D) { return D <= 128 ? padded_dim(D) : (D + 63) / 64 * 64; }
constexpr int GW_MAX_DP = 1024;  // Gauss-Wishart kernels: panel / chunk streaming beyond 128 (tested to 512)
inline int ntiles(int DP) { int nt = DP / 4; return nt * (nt + 1) / 2; }
// doubles per cluster in the packed E-step parameter stream
inline int pstride(int DP) { return ntiles(DP) * 16 + DP; }
// wide observations (DP > 128): the whitener streams as 64 x 64 blocks (I, J <= I), row-major; one chunk = 256 tiles
// of 16 doubles + the 64 entries of -b_I
constexpr int WIDE_CHUNK = 256 * 16 + 64;
inline int wide_chunks(int DP) { int np = DP / 64; return np * (np + 1) / 2; }
// doubles per cluster in the packed E-step parameter stream (the constant table c_jk follows K of these): the ONE
// place that knows both layouts -- every packer and every launch that places `ctab` asks here
// (narrow layouts: the stream holds the tiles of the ACTIVE width DC <= DP only -- estep_active_width)
inline int64_t estep_pstride(int DP, int DC) { return DP > 128 ? (int64_t)wide_chunks(DP) * WIDE_CHUNK : (int64_t)pstride(DC); }
inline int64_t estep_pstride(int DP) { return estep_pstride(DP, DP); }
// Active width of the Gauss-Wishart E-step and feature-GEMM statistics (round 6): the columns D ... DP - 1 of the padded
// layout are zero, and both kernels work in 4-column tiles / patches -- they walk the tiles of DC = D rounded up to a
// multiple of 8 (of 4 up to 48 columns) instead of those of DP (D = 23: 21 whitener tiles per cluster instead of 36, 24 feature tiles instead of
// 39).  Same X layout, same records (the entries of the idle columns are never written: zero), same results bit for bit
// (the skipped products are 0 * 0).  DP = 16 has the fused pass's own narrow instances (NTA).
// (granularity: 4 columns at the 32- and 48-column layouts, where the padding is the larger share -- D = 17 walks 20 columns,
//  not 24 --, 8 columns beyond: one more instance per layout there instead of three)
inline int estep_active_width(int D, int DP) {
  if (DP < 32 || DP > 128) return DP;
  const int g = DP <= 48 ? 4 : 8, lo = DP <= 48 ? DP - 12 : DP - 8;
  const int dc = (D + g - 1) / g * g;
  return dc < DP ? (dc < lo ? lo : dc) : DP;
}
// doubles per cluster in a stats record: [N_k, s_k[DP], S_k[DP*DP]]
inline int64_t stat_stride(int DP) { return 1 + (int64_t)DP + (int64_t)DP * DP; }

// Kernels that need more than 64 KB of dynamic LDS must be told so once per device (function attributes are per
// device; one process may hold contexts on several).  granted = a static per launcher instance.
struct LdsGrant {
  size_t granted[16] = {};
};
inline hipError_t grant_dynamic_lds(const void* fn, size_t bytes, LdsGrant& g) {
  if (bytes <= 64 * 1024) return hipSuccess;
  int dev = -1;
  const bool tracked = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16;
  if (tracked && bytes <= g.granted[dev]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess && tracked) g.granted[dev] = bytes;
  return e;
}

// rginfo word per row-group: (group << 5) | nvalid   (nvalid in 0..16)
inline int rginfo_pack(int group, int nvalid) { return (group << 5) | nvalid; }

struct EstepLaunch {
  int DP;
  int DC = 0;            // active width (estep_active_width; 0 = DP): tiles of the columns >= DC are neither packed nor walked
  const double* X;       // [NP x DP]
  int64_t nrg;           // number of row-groups (NP / 16)
  const int* rginfo;     // [nrg] or nullptr (single group; nvalid from nrows)
  int64_t nrows;         // valid rows when rginfo == nullptr
  const double* params;  // [K x estep_pstride(DP, DC)] packed tiles + b
  const double* ctab;    // [J x K] c_jk (may hold -inf for sparse-inactive)
  int K;
  double* qZ;            // [K x ldq]
  int64_t ldq;
  double* fz_part;       // [estep_grid(...)]
  double* ll_part;       // [estep_grid(...) x K], or nullptr: skip the split-ordering data term
  int raw = 0;           // 1: stop after writing log q~ (no log-sum-exp, fz/ll untouched)
  int sparse = 0;        // 1: ctab holds -inf entries; waves skip clusters inactive for all their rows
  int lq_lds = 0;        // filled in by launch_estep (EstepPlan::lq_lds)
  // Kept-quad masks of the responsibilities this launch stores, or nullptr: one 16-bit word per (cluster
  // quad c, 16-row group g) at qmask[c * nrg + g], bit i = "row 16 g + i keeps quad c" = !(q < SPECK_TAU) for any of the
  // quad's clusters < K, taken on the q that is stored (a NaN is kept, a pad row's 0.0 is not) -- ss_list_build_kernel's
  // rule to the letter.  [(K + 3) / 4 x nrg], every word written.  Only the instances with EstepPlan::emits take it
  // (launch_estep refuses the pointer on any other launch).
  unsigned short* qmask = nullptr;
};
// ONE decision per launch, read by estep_grid and by every launcher: a function of the WHOLE launch -- DP, DC, K, raw,
// sparse, nrg have to be set (D = 64 / 80 run four row groups per wave where the log q~ table fits in LDS: other rows per block)
struct EstepPlan {
  bool ok;              // false: no instance serves this launch (launch_estep returns hipErrorInvalidValue)
  int rows_per_block;
  int64_t grid;         // blocks of the launch (and partial sums the caller provides); -1 when !ok
  bool four_groups;     // the four-row-group instance of D = 64 / 80
  int DC, lq_lds;       // the active-width instance; log q~ waits in LDS (four row groups per wave, small K) instead of in qZ
  size_t lds_bytes;     // dynamic LDS of the launch
  bool emits = false;   // the instance can write EstepLaunch::qmask (dense, normalising, DP = 64 with DC 64 or 56; three or four row groups per wave)
};
EstepPlan estep_plan(const EstepLaunch& a);
int64_t estep_grid(const EstepLaunch& a);  // estep_plan(a).grid
hipError_t launch_estep(const EstepLaunch& a, hipStream_t stream);

// ---- small observations: E-step + the next iteration's statistics in one persistent pass (lc_kernels_fused.hip) ----
struct FusedLaunch {
  int DP;
  int D = 16;            // observation width before padding (D <= 8: the half-width instance)
  const double* X;       // [NP x DP]
  int64_t nrg;           // row groups (NP / 16)
  const int* rginfo;     // [nrg] or nullptr (single group)
  int64_t nrows;         // valid rows when rginfo == nullptr
  const double* params;  // [K x pstride(DP)] as for estep_kernel
  const double* ctab;    // [J x K]
  int K;
  double* qZ;            // [K x ldq]: written once (the new responsibilities)
  int64_t ldq;
  // ONE partial record per block, folded by a single reduce_partials launch:
  //   [K x stat_stride(DP) statistics of the NEW responsibilities | Fz | LL_k (K; zeros when !want_ll)]
  double* partial;       // [grid x fused_record(DP, K)]
  bool want_ll;          // also the split-ordering data term
  int grid;              // fused_plan(...)
  int ngroups = 1;       // J: rows of ctab (the table waits in LDS when J x K <= FUSED_CT_CAP)
  // share (per mille) of a CU's tiles that goes to the SECOND of its two blocks (blocks grid / 2 ... grid - 1); 0: every
  // block the same (launch_fused sets it; the kernel's tile deal is a function of (blockIdx, grid, nrg) alone)
  int yshare = 0;
};
constexpr int FUSED_CT_CAP = 1024;
inline int64_t fused_record(int DP, int K) { return (int64_t)K * (1 + DP + (int64_t)DP * DP) + 1 + K; }
bool fused_eligible(int DP, int K);          // a property of the shape alone (identical on every rank)
int fused_plan(int DP, int64_t nrg, int K);  // persistent blocks for nrg row groups (0 when there are none)
hipError_t launch_fused(const FusedLaunch& a, hipStream_t stream);

// sparse work item of suffstat_kernel: rows [r0, r1) of one group x clusters klist[kofs .. kofs + kcnt)
struct SSItem {
  int64_t r0, r1;
  int kofs, kcnt;
  int64_t rec0;  // partial record of the item's first cluster
};
// ---- the Gauss-Wishart statistics pass: ONE decision (suffstat_plan) for the caller's buffers, the launcher and the tests ----
constexpr int SS_BR = 32;  // rows staged per batch: a row chunk is a whole number of them
// The library's one "speck" threshold, 2^-300: responsibilities below it are flushed to zero by the moved-row
// sweeps of the split search, and a (4-row step, cluster quad) pair that holds nothing else is left out of the
// feature-GEMM statistics pass (SuffstatLaunch::speck_skip).
constexpr double SPECK_TAU = 0x1p-300;
// the kernel a pass runs: suffstat_kernel, suffstat_feat_kernel, suffstat_quad_kernel, suffstat_kernel's panel launches (DP > 128)
enum SuffstatRoute { SS_PER_CLUSTER = 0, SS_FEAT = 1, SS_QUAD = 2, SS_WIDE = 3 };
// what a pass does with the responsibilities: all of them (no mask); a [J x K] mask whose pairs are staged as zeros;
// the variant that skips (4-row step, cluster) pairs with all-zero q (exact; with or without a mask); a sparse work list
enum SuffstatMode { SS_DENSE = 0, SS_MASKED_DENSE = 1, SS_ZERO_SKIP = 2, SS_WORK_LIST = 3 };
struct SuffstatPlan {
  SuffstatRoute route;
  int nchunks;             // row chunks of the dense (chunk, slice) grid ...
  int64_t chunk_rows;      // ... of this many rows (a multiple of SS_BR)
  // Ragged K: when the last cluster slice of the per-cluster kernel fills only one or two of its four waves, the idle waves
  // take over part of the active waves' rows (2 or 4 row classes) and write `extra` more records per chunk after the K regular
  // ones ([row class - 1][cluster of the last slice]); klast0 = first cluster of that slice.  launch_fold_extra adds them in.
  int extra, klast0, KR;   // KR = K + extra records per chunk
  int clusters_per_block;  // of the per-cluster kernel (4 waves x clusters per wave): what a work-list item holds
  const char* name;        // the kernel a profiler will list
};
// a function of the shape and the mode alone (identical on every rank) -- and, from NP = 64 * 1024 on, of the device's
// CU count and the resident blocks per CU of the instance (asked once per instance).  K < 1 or NP < 1: nothing to run.
SuffstatPlan suffstat_plan(int DP, int DC, int64_t NP, int K, SuffstatMode mode);
struct SuffstatLaunch {
  int DP;
  int DC = 0;               // active width (estep_active_width; 0 = DP): the feature-GEMM and few-cluster kernels deal out its patches only
  const double* X;
  int64_t NP;               // padded rows (multiple of 16)
  const double* qZ;
  int64_t ldq;
  int K;
  SuffstatMode mode = SS_DENSE;
  const int* rginfo;        // needed only with smask
  const unsigned char* smask;  // [J x K] 1 = accumulate, or nullptr (SS_MASKED_DENSE: set; SS_ZERO_SKIP: optional; else nullptr)
  double* partial;          // [nchunks x KR x stat_stride(DP)]
  // the plan's, copied by the caller: launch_suffstat refuses a launch that contradicts the plan it is handed
  int nchunks = 0, KR = 0;
  int64_t chunk_rows = 0;
  // SS_WORK_LIST: the items (device) instead of the dense (chunk, slice) grid, the active cluster lists they point into
  const SSItem* items = nullptr;
  const int* klist = nullptr;
  int nitems = 0, skip_listed = 0;  // skip_listed: the listed pairs run the zero-skipping variant too
  // 1: leave out the (4-row step, cluster quad) pairs whose sixteen responsibilities are all below SPECK_TAU.  Only the
  // feature GEMM (SS_FEAT) has such an instance: launch_suffstat refuses the flag on every other route.
  // 2: the same, and a staged batch whose rows all have at most one kept quad is sorted by that quad first (stable; the
  // steps are then groups of four rows AS PLACED).  Other values are refused.
  int speck_skip = 0;
  // ---- written by the internal launchers, each for its own kernel (whatever the caller puts here is overwritten) ----
  int nslice = 1;                                  // blocks per row chunk
  int slice0 = 0, rs = 1, klast0 = 0, nklast = 0;  // suffstat_kernel: the row-split launch of the last slice; suffstat_feat_kernel: klast0 = first cluster of the range
  int64_t ldx = 0;                                 // wide observations (DP > 128), 64-column panels: row stride of X,
  int DPW = 0, colA = 0, colB = 0;                 // record width, first column of the A-side / B-side panel
};
// p = suffstat_plan(a.DP, a.DC, a.NP, a.K, a.mode), computed ONCE per pass by the caller (the fill searches are not free)
hipError_t launch_suffstat(const SuffstatLaunch& a, const SuffstatPlan& p, hipStream_t stream);

// The selector in front of a speck-skipping pass: up to SPECK_PROBE_STEPS 4-row steps of qZ, evenly strided
// over the rows, are looked at and the (step, cluster quad) pairs that would be KEPT are counted into *active (device, int,
// zeroed here); *pairs (host) = the pairs looked at.  The pass skips when at least a quarter of them could be skipped
// (speck_probe_says_skip): with fewer, the skipping instance's branches cost more than they save (a pass that can skip
// nothing is 10 % slower than the dense instance).  Integer counts of a fixed sample: a deterministic function of qZ.
constexpr int SPECK_PROBE_STEPS = 4096;
constexpr int64_t SPECK_PROBE_MIN_ROWS = 4096;  // below: no probe, the dense instance
// active[1] (zeroed here too) counts the sampled ROWS that keep a value of exactly one quad -- the rows a list pass (below)
// touches once; *rows (host, optional) = the rows looked at.  K > 256 (a step's quads no longer sit in one wave): not counted.
hipError_t launch_speck_probe(const double* qZ, int64_t ldq, int K, int64_t NP, int* active, int64_t* pairs, hipStream_t stream,
                              int64_t* rows = nullptr);
inline bool speck_probe_says_skip(int64_t active, int64_t pairs) { return pairs > 0 && 4 * (pairs - active) >= pairs; }
// Does a skipping pass take the list route (below)?  At least LC_FT_LIST_SHARE64 / 64 of the sampled rows have to keep exactly
// one quad (decided in lc_kernels_suffstat.hip, a device source: tools/variants.py can build another share).
bool speck_probe_says_lists(int64_t single, int64_t rows);

// ---- the list route of a skipping pass (suffstat_list_kernel) -------------------------------------------
// Every (row chunk, cluster quad) of the plan gets the ascending list of the chunk's rows that keep a value of the quad
// ("not (q < SPECK_TAU)" in any of its clusters: a NaN is kept, pad rows are in no list, a soft row is in several), and one
// block sums one list: at DC = 56 with the feature GEMM's arithmetic for a single quad (all four q of a listed row), at
// DC = 64 one wave per cluster on the VALU, a listed row going into a cluster only where speck_keeps(its own q)
// (suffstat_owner_kernel).  Same partial records as launch_suffstat.
// The buffer: [nchunks x nq] lengths (int), then [nchunks x nq] segments of chunk_rows chunk-local row offsets each -- a
// segment can hold every row of its chunk, so no list overflows whatever qZ holds -- as 16-bit values while a chunk has at
// most 65536 rows, 32-bit beyond.
struct SsListLayout {
  int nq;            // cluster quads of K
  bool wide;         // 32-bit offsets
  size_t ent_off;    // byte offset of the segments
  size_t bytes;      // of the whole buffer
};
inline SsListLayout ss_list_layout(int nchunks, int64_t chunk_rows, int K) {
  SsListLayout l{(K + 3) / 4, chunk_rows > 65536, 0, 0};
  l.ent_off = ((size_t)nchunks * l.nq * sizeof(int) + 15) / 16 * 16;
  l.bytes = l.ent_off + (size_t)nchunks * l.nq * (size_t)chunk_rows * (l.wide ? 4 : 2);
  return l;
}
bool suffstat_list_instance(int DP, int DC);  // a suffstat_list_kernel exists for this width (DC = 0: DP)
bool suffstat_owner_instance(int DP, int DC);  // its lists are summed by suffstat_owner_kernel (false with -DLC_FTL_OWNER=0)
bool speck_lists_enabled();                   // false in a build with -DLC_FT_SPECK_LISTS=0 (tools/variants.py)
// a (dense, SS_FEAT) launch as launch_suffstat takes it, with its plan; lists: ss_list_layout(...).bytes of device memory.
// Both refuse (hipErrorInvalidValue, nothing launched) a launch that is not the plan's, a route other than the feature
// GEMM's, a width without an instance and a buffer that is too small.  _build: the lists alone; the other: lists + sums.
hipError_t launch_suffstat_list_build(const SuffstatLaunch& a, const SuffstatPlan& p, void* lists, size_t bytes, hipStream_t stream);
hipError_t launch_suffstat_lists(const SuffstatLaunch& a, const SuffstatPlan& p, void* lists, size_t bytes, hipStream_t stream);
// The same lists and the same probe counts from the kept-quad masks an E-step left behind (EstepLaunch::qmask: [nq x nrg]
// 16-bit words, nrg = a.NP / 16) instead of from qZ, which is not read at all: one block per (row chunk, cluster quad)
// walks the chunk's bit range of the quad -- addressed by bit, a chunk need not start on a word --, popcounts give the
// places, no atomics.  Same layout, lengths and entries as launch_suffstat_list_build / the same two counts, *pairs and
// *rows as launch_speck_probe, whatever the masks hold.
hipError_t launch_suffstat_list_build_masks(const SuffstatLaunch& a, const SuffstatPlan& p, const unsigned short* qmask, int64_t nrg,
                                            void* lists, size_t bytes, hipStream_t stream);
hipError_t launch_suffstat_lists_masks(const SuffstatLaunch& a, const SuffstatPlan& p, const unsigned short* qmask, int64_t nrg,
                                       void* lists, size_t bytes, hipStream_t stream);
hipError_t launch_speck_probe_masks(const unsigned short* qmask, int64_t nrg, int K, int64_t NP, int* active, int64_t* pairs,
                                    hipStream_t stream, int64_t* rows = nullptr);
// the masks of a qZ buffer by the rule alone (tests: LC_TEST_VERIFY_QMASK recomputes what a pass is about to trust)
hipError_t launch_qmask_from_qz(const double* qZ, int64_t ldq, int K, int64_t nrg, unsigned short* qmask, hipStream_t stream);
// SuffstatLaunch::speck_skip of a pass that skips: 2 (sorted batches); 1 in a build with -DLC_FT_SPECK_SORT=0 (decided in
// lc_kernels_suffstat.hip, a device source, so that tools/variants.py can build the unsorted rule for a same-visit A/B)
int speck_skip_mode();

// ---- tile plan of the feature-GEMM statistics kernel (suffstat_feat_kernel, lc_kernels_suffstat.hip) ----------------
// Features of the active width DC, one per lane of a 16-feature tile (lane (lo2, blk) of tile T holds feature
// 16 T + lo2 + 4 blk), in this order:
//   the off-diagonal 4 x 4 patches (ia < ja, ja-major) whole: u = 4 ia + lo2, w = 4 ja + blk (same LDS reads as the
//     patch deal had);
//   the 10 distinct products x_i x_j (i <= j) of each diagonal 4 x 4 block, packed;
//   the DC linear features x_i * 1;
//   N_k = 1 * 1.
// Spare slots of the last tile read 1 * 1 and are not stored.  D = 64: 120 x 16 + 160 + 64 + 1 = 2145 features in 135
// tiles (the patch deal took 141: whole diagonal patches, whole 16-column s_k blocks, a tile of its own for N_k).
__host__ __device__ constexpr int ft_offdiag(int DC) { return (DC / 4) * (DC / 4 - 1) / 2; }
__host__ __device__ constexpr int ft_features(int DC) { return 16 * ft_offdiag(DC) + 10 * (DC / 4) + DC + 1; }
__host__ __device__ constexpr int ft_tiles(int DC) { return (ft_features(DC) + 15) / 16; }
enum FtKind { FT_PRODUCT = 0, FT_LINEAR = 1, FT_COUNT = 2, FT_SPARE = 3 };
struct FtFeature {
  int u, w, kind;  // staged columns of the two factors (`one`: the column of ones)
};
// (always inlined: behind the long unrolled step loops of the speck-skipping instances hipcc otherwise CALLS them from the
//  epilogue, with ft_deal's two results in scratch)
// the features behind the off-diagonal patches, g = 0 ...: diagonal products, linear features, N_k, spare slots
__host__ __device__ __attribute__((always_inline)) constexpr FtFeature ft_feature_rest(int DC, int one, int g) {
  const int ndiag = 10 * (DC / 4);
  if (g < ndiag) {  // (i, j) of a diagonal block: (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
    const int b = 4 * (g / 10), e = g % 10;
    const int i = e < 4 ? 0 : e < 7 ? 1 : e < 9 ? 2 : 3, i0 = e < 4 ? 0 : e < 7 ? 4 : e < 9 ? 7 : 9;
    return {b + i, b + i + (e - i0), FT_PRODUCT};
  }
  g -= ndiag;
  if (g < DC) return {g, one, FT_LINEAR};
  return {one, one, g == DC ? FT_COUNT : FT_SPARE};
}
__host__ __device__ __attribute__((always_inline)) constexpr FtFeature ft_feature(int DC, int one, int f) {
  const int noff = 16 * ft_offdiag(DC);
  if (f < noff) {
    const int p = f / 16, r = f % 16;
    int ja = 1;
    while ((ja + 1) * ja / 2 <= p) ++ja;
    return {4 * (p - ja * (ja - 1) / 2) + (r & 3), 4 * ja + (r >> 2), FT_PRODUCT};
  }
  return ft_feature_rest(DC, one, f - noff);
}
// Waves per block.  The waves of a block share one staged batch, so 8 waves (one block per CU, longer batches) halve
// the staging instructions and barriers per MFMA against 4 waves (two blocks per CU): D = 64, N = 10M, K = 32:
// 22.03 -> 21.70 ms.
// (round 5: D = 80, 96, 112 as 8-wave blocks too -- half the staging registers per thread, and with them every instance
//  but <80, 6> free of scratch, where the 4-wave instances spilled 64 ... 136 bytes into the step loop: the feature GEMM
//  now runs at these widths, N = 4M, K = 32: D = 96 22.9 -> 19.1 ms (0.67 -> 0.81 of the fp64 peak), D = 80 15.0 -> 13.7,
//  D = 112 (N = 3M) 21.9 -> 19.9)
#ifndef LC_FT_WAVES64
#define LC_FT_WAVES64 8
#endif
#ifndef LC_FT_WAVES128
#define LC_FT_WAVES128 8
#endif
__host__ __device__ constexpr int ft_waves(int DP) { return DP == 64 ? LC_FT_WAVES64 : DP == 128 ? LC_FT_WAVES128 : DP > 64 ? 8 : 4; }
// tiles per wave: as many as the accumulators allow (72 doubles; 64 for 8 quads at D = 80, 96, 112, where 72 spill) -- 9 tiles
// with 8 cluster quads, 12 with 6, 14 with 5: a launch with fewer quads keeps its MFMAs per step (and has fewer blocks
// re-staging the same rows)
__host__ __device__ constexpr int ft_tpw_max(int DP, int NQ) {
  const int t = (NQ >= 8 && DP > 64 && DP < 128 ? 64 : 72) / NQ;
  return t < 14 ? t : 14;  // (two address registers per tile)
}
__host__ __device__ constexpr int ft_nslice(int DP, int DC, int NQ) {  // blocks per row chunk
  return (ft_tiles(DC) + ft_waves(DP) * ft_tpw_max(DP, NQ) - 1) / (ft_waves(DP) * ft_tpw_max(DP, NQ));
}
__host__ __device__ constexpr int ft_tpw(int DP, int DC, int NQ) {  // tiles of the fuller waves
  return (ft_tiles(DC) + ft_waves(DP) * ft_nslice(DP, DC, NQ) - 1) / (ft_waves(DP) * ft_nslice(DP, DC, NQ));
}
// The tiles of wave `wave` of block `slice` of a chunk: [*t0, *t0 + *nt).
// 8 waves: dealt per SIMD.  A block's waves go to the four SIMDs of its CU in cyclic order, so waves w and w + 4 share
// one matrix pipe, and with one barrier per staged batch a block lasts as long as its busiest SIMD: the 4 x nslice SIMDs
// of a chunk take ceil or floor of TILES / (4 nslice) tiles each, split ceil / floor between the two waves (D = 64, 8
// quads: 17 17 17 17 | 17 17 17 16 = waves of 9 + 8, the last 8 + 8).  A per-wave deal (the first TILES % 16 waves of
// one tile more) put 9 + 9 on one SIMD or more of every block: 18 tile-streams where 17 do.
// 4 waves (two blocks per CU, the partners belong to different blocks): TPW everywhere, the last waves of a chunk carry
// idle tiles -- a second instance of the batch body costs more there than the idle tiles do (D = 128, 4 waves: 72.9 ->
// 77.2 ms with an uneven deal; both bodies compete for the instruction cache).
__host__ __device__ __attribute__((always_inline)) constexpr void ft_deal(int DP, int DC, int NQ, int slice, int wave, int* t0, int* nt) {
  const int tiles = ft_tiles(DC), nsl = ft_nslice(DP, DC, NQ);
  if (ft_waves(DP) == 8) {
    const int ns = 4 * nsl, s = slice * 4 + (wave & 3), l = tiles / ns, r = tiles % ns;
    const int load = l + (s < r ? 1 : 0), first = s * l + (s < r ? s : r);
    *t0 = first + (wave < 4 ? 0 : (load + 1) / 2);
    *nt = wave < 4 ? (load + 1) / 2 : load / 2;
  } else {
    const int tpw = ft_tpw(DP, DC, NQ), t = (slice * 4 + wave) * tpw;
    *t0 = t;
    *nt = tiles - t < tpw ? (tiles - t > 0 ? tiles - t : 0) : tpw;
  }
}
// The list kernel (one cluster quad per block): ALL tiles of the width in one 8-wave block, dealt per SIMD as above --
// D = 64: 135 tiles = 34 34 34 33 per SIMD = waves of 17 + 17, the last 17 + 16.  ftl_tpw: tiles of the fuller waves; a
// wave with one fewer runs an idle tile (1 * 1, not stored) on the one SIMD that has a slot to spare.
__host__ __device__ constexpr int ftl_tpw(int DC) { return ((ft_tiles(DC) + 3) / 4 + 1) / 2; }
__host__ __device__ __attribute__((always_inline)) constexpr void ft_deal_one(int DC, int wave, int* t0, int* nt) {
  const int tiles = ft_tiles(DC), s = wave & 3, l = tiles / 4, r = tiles % 4;
  const int load = l + (s < r ? 1 : 0), first = s * l + (s < r ? s : r);
  *t0 = first + (wave < 4 ? 0 : (load + 1) / 2);
  *nt = wave < 4 ? (load + 1) / 2 : load / 2;
}
// The list kernel's SHARED deal.  ft_deal_one hands a wave 17 consecutive tiles, and each reads both factors
// of its product from LDS -- 35 fragment reads per 17 MFMAs, most of them the same `w` fragment again.  Here a wave's
// off-diagonal tiles share a factor.  The DC / 4 = 16 column blocks are the vertices of K16 and the 120 off-diagonal 4 x 4
// patches its edges, oriented as a circulant: block a owns {a, a + 1 ... a + 7 (mod 16)}, and the eight diameters {a, a + 8}
// go to a < 8 -- blocks 0-7 own 8 edges, blocks 8-15 own 7, every edge once.  Wave v takes the stars of blocks v and v + 8:
//   tiles 0 ... S - 1  (S = ftl_split = 8): patch (v, v + 1 + t),               the SHARED factor column 4 v + blk
//   tiles S ... P - 1  (P = ftl_paired = 15): patch (v + 8, v + 8 + 1 + t - S), the shared factor column 4 (v + 8) + blk
//   tiles P, P + 1: "free" tiles 2 v and 2 v + 1 of ft_feature_rest (diagonal products, linear features, N_k; both factors
//     read as before); free tile 15 does not exist, so wave 7 runs the idle 1 * 1 tile there: 34 34 34 33 tiles per SIMD as
//     in ft_deal_one.
// A paired tile's other factor sits in the lo2 position (column 4 o + lo2): the two access patterns of ft_feature.  u * w
// commutes, so which block of a patch is the shared one changes no bit.  22 fragment reads per 17 MFMAs.
// -DLC_FTL_SHARED=0 (tools/variants.py) restores ft_deal_one's deal.  Widths other than 64 keep it: DC = 56 has 14 blocks,
// whose 7 + 6 stars fill seven waves of 13 tiles and leave the eighth with 13 free ones -- a second batch body.
#ifndef LC_FTL_SHARED
#define LC_FTL_SHARED 1
#endif
__host__ __device__ constexpr bool ftl_shared(int DC) { return LC_FTL_SHARED != 0 && DC == 64; }
__host__ __device__ constexpr int ftl_paired(int DC) { return ftl_shared(DC) ? DC / 4 - 1 : 0; }  // paired tiles of a wave
__host__ __device__ constexpr int ftl_split(int DC) { return ftl_shared(DC) ? DC / 8 : 0; }       // ... of its first star
struct FtlFeature {
  int u, w, kind;  // as FtFeature; a paired tile: u = the tile's own column (lo2 position), w = the shared one (blk position)
  int shared;      // which shared fragment of the wave the tile uses: 0, 1; -1: none (both factors read)
};
// lane (lo2, blk) = l16 of tile t of wave `wave`, either deal: THE map of the list kernel (addresses and epilogue)
__host__ __device__ __attribute__((always_inline)) constexpr FtlFeature ftl_feature(int DC, int one, int wave, int t, int l16) {
  if (!ftl_shared(DC)) {
    int t0 = 0, nt = 0;
    ft_deal_one(DC, wave, &t0, &nt);
    if (t >= nt) return {one, one, FT_SPARE, -1};
    const FtFeature f = ft_feature(DC, one, 16 * (t0 + t) + l16);
    return {f.u, f.w, f.kind, -1};
  }
  const int nb = DC / 4, S = ftl_split(DC), P = ftl_paired(DC);
  if (t < P) {
    const int second = t >= S ? 1 : 0, a = wave + second * S, o = (a + 1 + t - second * S) % nb;
    return {4 * o + (l16 & 3), 4 * a + (l16 >> 2), FT_PRODUCT, second};
  }
  const FtFeature f = ft_feature_rest(DC, one, 16 * (2 * wave + t - P) + l16);
  return {f.u, f.w, f.kind, -1};
}
// the wave's factor registers: paired tiles use register `shared`, the others one of their own behind the two
__host__ __device__ constexpr int ftl_nw(int DC) { return ftl_shared(DC) ? 2 + ftl_tpw(DC) - ftl_paired(DC) : ftl_tpw(DC); }
__host__ __device__ constexpr int ftl_wi(int DC, int t) {
  return !ftl_shared(DC) ? t : t < ftl_split(DC) ? 0 : t < ftl_paired(DC) ? 1 : 2 + t - ftl_paired(DC);
}
static_assert(!ftl_shared(64) || (ftl_tpw(64) == ftl_paired(64) + 2 && 16 * 2 * 8 >= ft_features(64) - 16 * ft_offdiag(64)),
              "shared deal: 8 waves of two stars and two free tiles");

// The owner kernel (suffstat_owner_kernel, DC = DP = 64): one WAVE per cluster, lane w owns column w, and the
// wave's accumulator t holds, in lane w,
//   t = 0 ... 32 ("diagonals"): the product x_w x_((w + t) mod 64) -- every unordered pair once; at t = 32 lanes w and w + 32
//     hold the same product (summed in the same order), and only the lower one is stored: the upper is FT_SPARE
//   t = 33: the linear feature x_w,  t = 34: N_k (every lane holds it, lane 0 stores it)
// fto_feature: THE map of that kernel's epilogue, (u, w) as in FtFeature with `one` = 64 for the column of ones.
constexpr int FTO_DIAGS = 33, FTO_ACCS = 35;
__host__ __device__ __attribute__((always_inline)) constexpr FtFeature fto_feature(int lane, int t) {
  if (t < FTO_DIAGS) return {lane, (lane + t) & 63, t == 32 && lane >= 32 ? FT_SPARE : FT_PRODUCT};
  if (t == FTO_DIAGS) return {lane, 64, FT_LINEAR};
  return {64, 64, lane == 0 ? FT_COUNT : FT_SPARE};
}

// the smallest tile count of any wave (the 8-wave deal: ft_tpw or one fewer)
__host__ __device__ constexpr int ft_nt_min(int DP, int DC, int NQ) {
  int m = ft_tpw(DP, DC, NQ);
  for (int sl = 0; sl < ft_nslice(DP, DC, NQ); ++sl)
    for (int w = 0; w < ft_waves(DP); ++w) {
      int t0 = 0, nt = 0;
      ft_deal(DP, DC, NQ, sl, w, &t0, &nt);
      m = nt < m ? nt : m;
    }
  return m;
}

hipError_t launch_fold_extra(double* rec, int64_t SS, int K, int klast0, int extra, hipStream_t stream);
hipError_t launch_reduce_records(const double* partial, int64_t n, int K, const int* kptr, const int* krec, double* out,
                                 hipStream_t stream);

// out[e] = sum_c partial[c*n + e]  (fixed order => deterministic)
// tmp (optional): REDUCE_TMP_ELEMS * 64 doubles of scratch, enables the two-stage path for very many records
constexpr int REDUCE_TMP_ELEMS = 512;
hipError_t launch_reduce_partials(const double* partial, int nparts, int64_t n, double* out, hipStream_t stream,
                                  double* tmp = nullptr);
// out[j*K+k] = sum over rows of group j of qZ[k*ldq + row]; goff = padded row offsets [J+1]
// tmp (optional, REDUCE_TMP_ELEMS * 64 doubles) and rows (total padded rows) enable the sliced path for few large groups
hipError_t launch_group_colsum(const double* qZ, int64_t ldq, int K, const int64_t* goff, int J, double* out,
                               hipStream_t stream, double* tmp = nullptr, int64_t rows = 0);
// qZ[:, 0..K) = value on valid rows, 0 on pad rows
hipError_t launch_fill_qz(double* qZ, int64_t ldq, int K, const int* rginfo, int64_t nrows, int64_t nrg, double value,
                          hipStream_t stream);
// ---- diagonal Gaussian / exponential families (NormGamma, ExpGamma) --------------------------
struct DiagEstepLaunch {
  int DP, D;
  const double* X;
  int64_t nrg;
  const int* rginfo;
  int64_t nrows;
  const double* params;  // [3][K][DP]: a, w2, w1 (padding columns zero)
  int mode = 0;          // 0: general, 1: w1 == 0 (NormGamma), 2: a == w2 == 0 (ExpGamma)
  const double* ctab;    // [J x K]
  int K;
  double* qZ;
  int64_t ldq;
  double* fz_part;       // [ceil(NP/64)]
  double* ll_part;       // [ceil(NP/64) x K] or nullptr
  int raw = 0;
  // matrix-pipe path (estep_diag_mfma_kernel), chosen by lc_ctx.cpp when the expansion around `mu` is well conditioned:
  const double* wt = nullptr;      // packed weight tiles [ceil(K/4)][NTF][16]; nullptr: the difference-form VALU kernel
  const double* mu = nullptr;      // [DP] centre (unused in mode 2)
  const double* constk = nullptr;  // [K] sum_d (w2 a'^2 + w1 mu)
  int ngroups = 1;                 // J: rows of ctab (with several groups the plain instance keeps the table in LDS when J x K <= EDM_CT_CAP)
  double* sink = nullptr;          // [256] scratch: where the lanes of padding clusters / missing row groups store (see the kernel)
};
constexpr int EDM_CT_CAP = 1024;
inline int64_t estep_diag_grid(int64_t nrg) { return (nrg * RG + 63) / 64; }
int64_t estep_diag_mfma_weights(int DP, int K, int mode);
// ONE decision per launch, taken by estep_diag_plan and switched on by launch_estep_diag: a function of DP, K, mode, nrg,
// raw, ngroups and of which of wt / rginfo / ll_part are set (the pointers themselves are not followed).
// instance of estep_diag_mfma_kernel: generic (raw or LL_k, or K > 32), plain (the VBEM iterations', the table c_jk read
// from global memory), tabled (the table waits in LDS), one-group (no row-group table at all)
enum DiagEstepInstance { EDI_NONE = 0, EDI_GENERIC = 1, EDI_PLAIN = 2, EDI_TABLED = 3, EDI_ONEGROUP = 4 };
struct DiagEstepPlan {
  bool ok;           // false: no instance serves this launch (launch_estep_diag returns hipErrorInvalidValue)
  bool mfma;         // the matrix-pipe kernel (wt set)
  int mode;          // 0 / 1 / 2 as the kernels see it
  int64_t grid;      // blocks launched (0: nothing to run)
  size_t lds_bytes;  // dynamic LDS of the launch
  const char* name;  // the kernel a profiler will list
  // difference-form VALU kernels
  bool wide;         // estep_diag_wide_kernel (DP > 128)
  int KT;            // clusters per tile
  bool REG;          // log q~ stays in registers
  // matrix-pipe kernel
  int NT;            // 4-column feature tiles per half (DP / 4)
  bool QUAD;         // the quadratic half of the features too (mode != 2)
  int R, KTM;        // row groups per wave; cluster tiles kept in registers (0: per-lane LDS slots, any K)
  int instance;      // DiagEstepInstance
  int64_t nslots;    // partial slots the kernel fills or zeroes (estep_diag_grid)
  int per_cu;        // resident blocks per compute unit the grid is sized by
  int64_t block_cap; // compute units x per_cu: the most blocks a launch gets (more tiles: several tiles per block)
};
DiagEstepPlan estep_diag_plan(const DiagEstepLaunch& a);
hipError_t launch_estep_diag(const DiagEstepLaunch& a, hipStream_t stream);
// The packed operands of the matrix-pipe path (host; Context::estep_diag).  a / w2 / w1: [K x D].
// estep_diag_centre: mu [DP] = the mean of the cluster centres (pad columns and mode 2: zero); returns the conditioning
// figure max_d max_k |w2_kd| reach_d^2 (0 in mode 2) that decides between the two paths.
// estep_diag_pack: constk [K + 1] and the weight tiles wt [estep_diag_mfma_weights(DP, K, mode)] around that centre.
double estep_diag_centre(int D, int DP, int K, int mode, const double* a, const double* w2, double* mu);
void estep_diag_pack(int D, int DP, int K, int mode, const double* a, const double* w2, const double* w1, const double* mu,
                     double* constk, double* wt, int64_t nw);

struct DiagStatLaunch {
  int DP;
  const double* X;
  int64_t NP;
  const double* qZ;
  int64_t ldq;
  int K;
  const int* rginfo;
  const unsigned char* smask;
  double* partial;       // [nchunks * rsplit x K x (1 + 2 DP)], rsplit = suffstat_diag_rsplit(K)
  int nchunks;
  int64_t chunk_rows;    // multiple of 32
  int second = 1;        // 0: skip the second moments (ExpGamma)
  int nslice = 0, rsplit = 0;  // filled in by launch_suffstat_diag
  int ldx = 0, col0 = 0, DPT = 0;  // ditto: row stride of X, first column and total padded width (wide D)
};
int suffstat_diag_rsplit(int K);
// ONE decision per statistics pass of the separable families (launch_suffstat_diag switches on it)
struct DiagStatPlan {
  bool ok;             // false: no instance for this width
  int nslice, rsplit;  // blocks per row chunk (64 clusters each); row classes = partial records per chunk
  int second;
  int nblocks;         // launches: 1, or (DP > 128) one per block of 128 columns ...
  int width, last_width;  // ... of `width` columns each, the last one of `last_width` (128 or 64)
  // of the launch that owns the first column (the one that writes N_k) / of the last column block
  int BR, BR_last;           // rows staged per batch
  bool nstage, nstage_last;  // N_k summed where q is staged: the records of the row classes >= 1 carry N_k = 0
  bool deep, deep_last;      // two batches in flight
  size_t lds_bytes;          // of the first launch
  const char* name;
};
DiagStatPlan suffstat_diag_plan(int DP, int K, int second);
hipError_t launch_suffstat_diag(const DiagStatLaunch& a, hipStream_t stream);

// ---- split-search data passes (partobs / splitobs / auglabels on the device) ----
int select_blocks(int64_t NP);  // number of per-block counts select_count produces
hipError_t launch_select_count(const double* qcol, int64_t NP, double thresh, int* counts, hipStream_t stream);
hipError_t launch_select_compact(const double* qcol, int64_t NP, double thresh, const int64_t* offsets, int64_t* idx,
                                 hipStream_t stream);
hipError_t launch_group_starts(const int64_t* idx, int64_t M, const int64_t* goff, int J, int64_t* starts,
                               hipStream_t stream);
// qT[row * K + k] = qZ[k * ldq + row]
hipError_t launch_transpose_qz(const double* qZ, int64_t ldq, int K, int64_t NP, double* qT, hipStream_t stream);
// dst[c, gathered row of p] = src[c, idx[p]] for K columns (column-major, leading dimensions lds / ldd)
hipError_t launch_gather_cols(const double* src, int64_t lds, int K, const int64_t* idx, int64_t M, const int64_t* starts,
                              const int64_t* goff_sub, int J, double* dst, int64_t ldd, hipStream_t stream);
hipError_t launch_gather_rowmajor(const double* src, int64_t lds, int K, const int64_t* idx, int64_t M,
                                  const int64_t* starts, const int64_t* goff_sub, int J, double* dst, int64_t ldd,
                                  hipStream_t stream);
// the same for the nc source columns cols[0 .. nc) (device array): dst[c, gathered row of p] = src[idx[p], cols[c]]
hipError_t launch_gather_rowmajor_cols(const double* src, int64_t lds, const int* cols, int nc, const int64_t* idx, int64_t M,
                                       const int64_t* starts, const int64_t* goff_sub, int J, double* dst, int64_t ldd,
                                       hipStream_t stream);
hipError_t launch_gather_rows(const double* X, int DP, const int64_t* idx, int64_t M, const int64_t* starts,
                              const int64_t* goff_sub, int J, double* Xdst, hipStream_t stream);
hipError_t launch_split_init(const double* X, int DP, int D, int64_t NP, const int* rginfo, int64_t nrows,
                             const double* mv, double* q, int64_t ldq, int mode, const double* thr,
                             hipStream_t stream);
// qhash (or nullptr): the rows it rewrites lose their fingerprint (CachedNormLaunch::qhash)
hipError_t launch_aug_from_sub(double* q, int64_t ldq, int k, int K, const int64_t* idx, int64_t M,
                               const int64_t* starts, const int64_t* goff_sub, int J, const double* qsub1,
                               hipStream_t stream, int64_t* qhash = nullptr);

// split search: normalise K columns of log q~ = c_jk + (cached | freshly computed) -0.5 d^2 (softmax_cached_kernel)
struct CachedNormLaunch {
  const double* dcache;  // [Kc x ldc] cached -0.5 d^2 of the round's clusters
  int64_t ldc;
  const double* fresh;   // [nfresh x ldf] the recomputed columns
  int64_t ldf;
  const int* colmap;     // [K] device: >= 0 cache column, < 0 fresh column -(v + 1); nullptr: cache column j for cluster j
  const double* ctab;    // [J x K]
  int K;
  const int* rginfo;     // or nullptr (single group)
  int64_t nrows, NP;
  double* qZ;
  int64_t ldq;
  double* fz_part;       // [softmax_cached_grid(NP)]
  // optional (both or neither): how far this E-step moved the responsibilities it overwrites
  double* ll_part = nullptr;  // [softmax_cached_grid(NP) x K] or nullptr: sum_n q_nk (log q~_nk - c_jk) partials
  double* dq = nullptr;    // [NP x ldd], ROW-major (ldd >= K): q_new - q_old, written for the rows with amax > dq_tol only
  double dq_tol = 0.0;
  int64_t ldd = 0;
  double* amax = nullptr;  // [NP] max_j |q_new - q_old| of the row
  // optional, with dq: a 64-bit fingerprint of every row of qZ (QHASH_NONE: unknown).  The sweep writes the fingerprint of
  // what it leaves in a row; with qhash_in it first compares: a row whose new values have the fingerprint of the old
  // ones is unchanged and its K old values are not even read (between the candidates of a split round that is almost
  // every row: half of the sweep's traffic)
  int64_t* qhash = nullptr;  // [NP]
  int qhash_in = 0;          // the fingerprints describe the responsibilities being overwritten
  // optional (both or neither): every row's largest log q~ and the cluster it belongs to -- what the NEXT recomputation of
  // a few columns needs to tell which rows those columns cannot reach (BoundSelectLaunch)
  double* rmax = nullptr;  // [NP]
  int* ramax = nullptr;    // [NP]
  // optional, with dq: bit j of colmask[j / 64] is set when any row's q_new - q_old is non-zero in column j (two words,
  // zeroed by the caller): delta_suffstat forms the moved rows' statistics for those clusters only
  unsigned long long* colmask = nullptr;
};
// Model selection: which rows does a recomputed column of -0.5 d^2 matter for?  (Context::estep_cache, round 5.)
// A split candidate changes two columns and the raw pass that recomputes them reads ALL of X for them (1.7 ms at N = 10M,
// D = 64: X-bound) -- although, for all but the candidate's own rows and their neighbours, the new responsibilities are
// exactly 0.0.  For a reference cluster `ref` (the column's own previous version, or the parent of a split) whose column
// is still in the slab,
//     d^2_new(x) = |B y + b|^2 >= (sigma_min(B) |y| - |b|)^2,   y = A_ref (x - m_ref), B = A_new A_ref^-1, b = A_new (m_ref - m_new)
// bounds the new column from ABOVE by a function of the old one:  log q~_new <= c_new - 0.5 (sigma sqrt(d^2_ref) - |b|)_+^2.
// A row whose largest log q~ over the UNCHANGED columns (rmax + the change of that cluster's constant) exceeds that bound
// by more than T gets -inf in the new column instead of its true value -- the same bits out of the normalisation sweep:
// with T > 745.2 exp(log q~ - max) underflows to 0.0 either way; in the moved-row sweeps, which store q < 2^-300 as zero,
// T > 208 suffices (an addend below 2^-54 of a sum that contains the row's exp(0) = 1 never changes it).  The other rows
// are flagged in `need` (1.0 / 0.0), gathered, and recomputed by the ordinary raw E-step.
constexpr int BOUND_MAX_COLS = 8, BOUND_MAX_K = 72;
struct BoundSelectLaunch {
  int ncol = 0, K = 0;
  int64_t NP = 0;
  const double* ref[BOUND_MAX_COLS];  // [NP] -0.5 d^2 of column t's reference cluster
  double* dest[BOUND_MAX_COLS];       // [NP] where column t goes: -inf is written for the rows that need no value
  double sigma[BOUND_MAX_COLS], bnorm[BOUND_MAX_COLS], cnew[BOUND_MAX_COLS];
  const double* rmax;
  const int* ramax;
  double T;
  unsigned char usable[BOUND_MAX_K];  // cluster j's column (and so rmax of its rows) is what it was when rmax was written
  double dcj[BOUND_MAX_K];            // change of c_j since then
  double* need;                       // [NP] out: 1.0 = recompute this row's columns
};
hipError_t launch_bound_select(const BoundSelectLaunch& a, hipStream_t stream);
// Xdst[p] = X[idx[p]] (rows of DP doubles), p < M
hipError_t launch_gather_rows_plain(const double* X, int DP, const int64_t* idx, int64_t M, double* Xdst, hipStream_t stream);
// dest[t][idx[p]] = src[t * lds + p], t < ncol, p < M
hipError_t launch_scatter_cols(const double* src, int64_t lds, int ncol, double* const* dest_host, const int64_t* idx, int64_t M,
                               hipStream_t stream);
// Switches of the test suite (the literal schedule of the split search, kernel instances forced on or off): read from
// the environment by libcluster_hip_testhooks.so ONLY -- in the shipped library this returns nullptr for every name, so
// no environment variable can change which kernel runs or what a learner returns (defined in lc_ctx.cpp).
const char* test_switch(const char* name);
constexpr int64_t QHASH_NONE = (int64_t)0x8000000000000000ull;
// out[i] = ((in[0][i] + in[1][i]) + in[2][i]) + ... over `world` blocks of `count` doubles, rank 0 first: the additions of
// the host transport (lc_comm.cpp, HostComm::allreduce_sum), on the device, behind ncclAllGather (LIBCLUSTER_COMM=rccl-gather)
hipError_t launch_rank_order_sum(const double* gathered, int world, int64_t count, double* out, hipStream_t stream);
// tests: rows whose stored fingerprint is neither QHASH_NONE nor that of the K values in the buffer are counted in *bad
hipError_t launch_qhash_verify(const double* qZ, int64_t ldq, int K, int64_t NP, const int64_t* qhash,
                               unsigned long long* bad, hipStream_t stream);
// dst row := src row (K values, zeros in dst's columns K .. Kdst-1, the fingerprint) wherever the rows' fingerprints differ
hipError_t launch_qz_resync(double* dst, const double* src, int64_t ldq, int K, int Kdst, int64_t NP, int64_t* dhash,
                            const int64_t* shash, hipStream_t stream);
int64_t softmax_cached_grid(int64_t NP);
int softmax_cached_max_k();  // widest K the sweep is built for
hipError_t launch_softmax_cached(const CachedNormLaunch& a, hipStream_t stream);

// ---- ranking (lc_kernels_rank.hip): the m best rows of each of C columns -----------------------------------
// Entry a is better than b when its score is larger (`largest`; smaller otherwise), or the scores compare equal and its
// position is lower: a total order, so the result does not depend on the chunking.  NaN scores and pad rows are never
// selected; with `label`, column c only sees the rows with label[row] == c.
constexpr int TOP_CHUNK_ROWS = 8192;  // rows per wave of the first stage: N = 10M gives a single column 1 221 waves, more than the chip has SIMDs
constexpr int TOP_MAX_M = 64;         // one list entry per lane
struct TopRowsLaunch {
  const double* col = nullptr;  // [C x ld]
  int64_t ld = 0;
  int C = 0;
  int64_t NP = 0;               // padded rows (multiple of 16)
  const int* rginfo = nullptr;  // [NP / 16] or nullptr (single group; the valid rows are the first nrows)
  int64_t nrows = 0;
  const int* label = nullptr;   // [NP] or nullptr: no filter
  int m = 0;                    // 1 ... TOP_MAX_M
  int largest = 1;
  int nchunks = 0;              // top_rows_chunks(NP)
  double* pkey = nullptr;       // [nchunks x C x m] partial lists of the first stage (keys: the score, negated for smallest)
  long long* ppos = nullptr;    // [nchunks x C x m]
  double* out_score = nullptr;  // [C x m] best first; NaN / -1 in the slots past the column's candidates
  long long* out_pos = nullptr; // [C x m] padded row
};
int top_rows_chunks(int64_t NP);
hipError_t launch_top_rows(const TopRowsLaunch& a, hipStream_t stream);

// ---- order and threshold queries (lc_kernels_select.hip) over the same columns ---------------------------------
// The columns and filters of TopRowsLaunch; `label`: column c only sees the rows with label[row] == label0 + c.  NaN scores and
// pad rows take part in nothing.
constexpr int SEL_MAX = 16;             // LC_QUANTILES_MAX: ranks / thresholds per call
constexpr int SEL_STATE_WORDS = 58;     // 8-byte words of the per-column state between the passes of the radix select
constexpr int SEL_HIST_WORDS = SEL_MAX * 256;  // ... and of its global histograms (one of 256 bins per active prefix)
constexpr int SEL_GRID_BLOCKS = 2048;   // blocks of 256 threads the histogram / counts kernels spread over all columns (8 per CU)
struct ScoreColumns {
  const double* col = nullptr;  // [C x ld]
  int64_t ld = 0;
  int C = 0;
  int64_t NP = 0;               // padded rows (multiple of 16)
  const int* rginfo = nullptr;  // [NP / 16] or nullptr (single group; the valid rows are the first nrows)
  int64_t nrows = 0;
  const int* label = nullptr;   // [NP] or nullptr: no filter
  int label0 = 0;
};
// Order statistics: rank r_i = min(n - 1, max(0, ceil(probs[i] n) - 1)) of the column's n participating scores in the total
// order -inf < ... < -0.0 < +0.0 < ... < +inf.  out: [C] n | [C x nprobs] r_i (-1: n = 0) | [C x nprobs] the bits of the value
// (0 where the rank is -1).  NP > 0.  The launcher zeroes hist; state needs no initial value.
struct ScoreSelectLaunch {
  ScoreColumns s;
  int nprobs = 0;                       // 1 ... SEL_MAX
  double probs[SEL_MAX] = {};
  unsigned long long* hist = nullptr;   // [C x SEL_HIST_WORDS]
  long long* state = nullptr;           // [C x SEL_STATE_WORDS]
  long long* out = nullptr;             // [C + 2 C nprobs]
};
hipError_t launch_score_select(const ScoreSelectLaunch& a, hipStream_t stream);
// out[c][0] = n, out[c][1 + i] = the participating scores <= thr[i] (IEEE comparison); the launcher zeroes out
struct ScoreCountsLaunch {
  ScoreColumns s;
  int nthr = 0;                         // 1 ... SEL_MAX
  double thr[SEL_MAX] = {};
  unsigned long long* out = nullptr;    // [C x (1 + nthr)]
};
hipError_t launch_score_counts(const ScoreCountsLaunch& a, hipStream_t stream);
// The participating rows of ONE column (s.C = 1) with score <= thr (above = 0) or >= thr, in row order: *total = how many,
// pos / score = the first min(total, capacity) of them (padded rows).
struct RowsBeyondLaunch {
  ScoreColumns s;
  double thr = 0.0;
  int above = 0;
  int64_t capacity = 0;
  int nchunks = 0;                      // top_rows_chunks(NP)
  long long* chunkoff = nullptr;        // [nchunks] scratch: the chunk counts, then their exclusive scan
  long long* total = nullptr;           // [1]
  long long* pos = nullptr;             // [capacity]
  double* score = nullptr;              // [capacity]
};
hipError_t launch_rows_beyond(const RowsBeyondLaunch& a, hipStream_t stream);

// synthetic mixture generator (bench): Philox4x32-10, counter = global row.
struct SynthLaunch {
  int DP, D, K;
  double* X;               // [NP x DP]
  double* qZ;              // [K x ldq] initial responsibilities, or nullptr
  int64_t ldq;
  int64_t nrows;           // valid rows
  int64_t NP;
  int64_t row_offset;      // global index of row 0 (rank sharding)
  uint64_t seed;
  const double* mu;        // [K x D]
  const double* L;         // [K x D x D] lower Cholesky factors, row-major
  double hard;             // q on the true label (0.9); rest (1-hard)/(K-1)
  // grouped data (all null / 0 for a single group): row-group info, padded group offsets, per-group
  // cumulative mixing proportions [J x K] (null = uniform labels), global id of local group 0
  const int* rginfo = nullptr;
  const int64_t* goff = nullptr;
  const double* cdf = nullptr;
  const int64_t* gids = nullptr;  // [J] global group ids (Philox counters), or null: group_base + local index
  int64_t group_base = 0;
};
hipError_t launch_synth(const SynthLaunch& a, hipStream_t stream);

// topic_infer_kernel (lc_kernels_topic.hip): the class of every document and the segments of its rows
// under a learned SCM / MCM model, one workgroup per document.  col holds L_nk = Eloglike_k(x_n) (a raw E-step with the
// clusters' constants); per document the kernel iterates vbeZ / vbeY (scluster.cpp:50-124) with the model fixed until
// its own qY moves by <= tol (tol < 0: exactly max_sweeps sweeps), then runs one last vbeZ for the per-row outputs.
struct TopicInferLaunch {
  double* col = nullptr;  // [K columns x ldq]; with keep_q the documents' rows become q
  int64_t ldq = 0;
  int K = 0, T = 0, docs = 0;
  const int64_t* goff = nullptr;   // [docs] first (padded) row of every document
  const int64_t* nrows = nullptr;  // [docs] rows of every document
  const double* a = nullptr;       // [docs x T] E[log pi_gt] (+ Eloglike_t(w_i), MCM)
  const double* E = nullptr;       // [T x K] E[log pi_tk]
  int max_sweeps = 1;
  double tol = 0.0;
  int keep_q = 0;
  int threads = 64;       // workgroup size (64, 128 or 256), from the largest document
  int64_t tile_cap = 0;   // doubles of LDS for a document's L tile (N_i K <= tile_cap: the sweeps never leave the CU)
  int e_lds = 0;          // E lives in LDS (T K <= TOPIC_E_LDS)
  int* label = nullptr;   // [NP] per row
  double* logZ = nullptr; // [NP]
  double* qY = nullptr;   // [docs x T]
  double* F = nullptr;    // [docs x 2] Fyz, Fz
  int* dint = nullptr;    // [docs x 2] label_t, sweeps
};
constexpr int TOPIC_E_LDS = 128;            // doubles: the largest E table kept in LDS
constexpr int TOPIC_LDS_BYTES = 40 * 1024;  // per workgroup at most: four workgroups per CU whatever the documents' size
// dynamic LDS of a launch over documents of nrows[docs] (host array) rows: the small vectors, the E table when it fits
// and the largest L tile among the documents that fit the budget (*tile_cap); 0: K and T are too large for the budget
size_t topic_infer_lds(int K, int T, int threads, const int64_t* nrows, int docs, int64_t* tile_cap, int* e_lds);
hipError_t launch_topic_infer(const TopicInferLaunch& a, size_t lds_bytes, hipStream_t stream);

// ---- device-resident data in, row results out (lc_kernels_ingest.hip) -----------------------------------------
// The padded image X [NP x DP] of J groups from strided DEVICE sources, one launch for all groups: element (n, d) of group j
// is src[j][n * rs + d * cs] (n < Nj[j], d < D), the columns D ... DP - 1 and every pad row become +0.0; every byte of the
// image is written.  rs == 1 (column-major sources) goes through an LDS tile, everything else reads along the rows
// (coalesced for cs == 1).  range[0] is left holding the key of the minimum over the valid entries that are numbers
// (data_range_decode), range[1] the number of NaNs among them: integer atomics, the same bits on every run; the launcher
// initialises both.  X == nullptr: the two values alone (over an image that exists: src[j] = image row goff[j], rs = DP, cs = 1).
struct PackRowsLaunch {
  int J = 0, D = 0, DP = 0;
  int64_t NP = 0;                       // padded rows of the image (goff[J])
  const double* const* src = nullptr;   // [J] device array of device pointers (a group without rows: never read)
  const int64_t* Nj = nullptr;          // [J]
  const int64_t* goff = nullptr;        // [J + 1] padded row offsets
  int64_t rs = 0, cs = 0;               // >= 1
  double* X = nullptr;
  unsigned long long* range = nullptr;  // [2]
};
hipError_t launch_pack_rows(const PackRowsLaunch& a, hipStream_t stream);
// host: the two words of PackRowsLaunch::range -> minimum (+inf: no valid entry is a number) and NaN count
void data_range_decode(const unsigned long long* range_h, double* min, int64_t* n_nan);
// q[r * rs + k * cs] = col[k * ldq + r], r < n, k < K: n rows of the column-major qZ (col points at the first of them) into a
// strided device destination.  Row-major destinations (cs == 1) go through an LDS tile; nothing outside the n x K entries
// is written.
struct UnpackQzLaunch {
  const double* col = nullptr;
  int64_t ldq = 0, n = 0;
  int K = 0;
  double* q = nullptr;
  int64_t rs = 0, cs = 0;  // >= 1
};
hipError_t launch_unpack_qz(const UnpackQzLaunch& a, hipStream_t stream);

}  // namespace lck
