// Device-side helpers shared by the kernel translation units.
//
// Matrix instruction: v_mfma_f64_4x4x4_4b_f64 (four independent 4x4x4 blocks, 512 flop, 16 cycles/SIMD = 32
// flop/clk/SIMD; measured 73-77 TFLOP/s on MI355X, vs 47-49 for v_mfma_f64_16x16x4_f64 --
// profiles/r01_mfma_f64_probe.log).  Lane layout (probed, tools/mfma_f64_4x4_layout.hip),
// lane = lo2 + 4*blk + 16*hi:
//   A[i][k] of block blk : i = lo2, k = hi
//   B[k][j] of block blk : j = lo2, k = hi
//   D[i][j] of block blk : j = lo2, i = hi
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "lc_kernels.h"

namespace lck {

// Compute units of the CURRENT device (a process may hold contexts on several, and learn_sharded drives its shards from
// concurrent threads: one relaxed atomic slot per device, filled by whoever asks first -- every writer stores the same
// value).  256 when the query fails.
inline int current_device_cus() {
  static std::atomic<int> cus_of[32];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) dev = -1;
  int cus = dev >= 0 ? cus_of[dev].load(std::memory_order_relaxed) : 0;
  if (cus <= 0) {
    hipDeviceProp_t p;
    if (dev >= 0 && hipGetDeviceProperties(&p, dev) == hipSuccess) cus = p.multiProcessorCount;
    if (cus <= 0) cus = 256;
    if (dev >= 0) cus_of[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

__device__ __forceinline__ double mfma4(double a, double b, double c) {
  return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// The list route's rule for one responsibility: kept unless it is below the speck threshold -- a NaN is kept,
// the 0.0 of a pad row is not.  ss_list_build_kernel reads it off qZ, the E-step's sweep off the value it is about to store
// (EstepLaunch::qmask); both have to agree to the bit, so both ask here.
__device__ __forceinline__ bool speck_keeps(double q) { return !(q < SPECK_TAU); }

// max without the canonicalising self-max hipcc puts in front of fmax (three v_max_f64 per call where one does;
// the operands here are never signalling NaNs).  NOT for an operand that an MFMA has just written: the hazard recogniser
// does not look inside inline asm, so the wait states an MFMA result needs before a VALU read are not inserted in front
// of it -- use fmax there (seen as NaN rows out of the half-width fused instance, whose last chain link sits right in
// front of the max).
__device__ __forceinline__ double max_raw(double a, double b) {
  // ("+v": the result goes into the register that holds `a` -- with a separate "=v" output the allocator may hand the asm a
  //  freshly freed register that an in-flight MFMA still reads as SrcC or is about to write, and no wait states are
  //  inserted for asm in that direction either; tools/check_isa.py looks at both directions)
  asm("v_max_f64 %0, %0, %1" : "+v"(a) : "v"(b));
  return a;
}

// exp(x) for x <= 0 (log q~ - max in the normalisation sweeps; -inf allowed), 1 ulp: 2^(n / 64) from a 64-entry table the
// kernel keeps in LDS (fill_exp_table) times a degree-5 polynomial on |r| <= ln 2 / 128 -- 16 VALU instructions and one
// LDS read against the 26 of the library exp, in kernels whose normalisation is bound by fp64 issue (one exponential per
// responsibility: K of them per row).  Reference: probutils::logsumexp / vbexpectation's exp() calls
// (src/probutils.cpp:146, src/cluster.cpp:130-131); the result differs from libm's by at most one unit in the last place.
static __constant__ double LC_EXP2_TAB[64] = {
    0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
    0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
    0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
    0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
    0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
    0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
    0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
    0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
    0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
    0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
    0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
    0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
    0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
    0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0};
__device__ __forceinline__ void fill_exp_table(double* etab, int tid, int nthreads) {
  for (int i = tid; i < 64; i += nthreads) etab[i] = LC_EXP2_TAB[i];
}
__device__ __forceinline__ double exp_nonpos(double x, const double* etab) {
  // (exp(-750) = 0; keeps n finite for x = -inf.  fmax, not the asm max_raw: the argument is the result of a subtraction,
  //  which hipcc knows to be canonical -- one v_max_f64 -- and inline asm counts as convergent, which keeps the sweeps'
  //  run-time loops from being unrolled)
  x = fmax(x, -750.0);
  const double n = __builtin_rint(x * 0x1.71547652b82fep+6);      // 64 / ln 2
  double r = fma(n, -0x1.62e42fef00000p-7, x);                    // ln 2 / 64, 33 significant bits: n * C1 is exact
  r = fma(n, -0x1.473de6af278edp-40, r);
  double q = fma(r, 1.0 / 120.0, 1.0 / 24.0);
  q = fma(q, r, 1.0 / 6.0);
  q = fma(q, r, 0.5);
  const double p = fma(q, r * r, r);                               // e^r - 1
  const int ni = (int)n;
  const double T = etab[ni & 63];
  return ldexp(fma(T, p, T), ni >> 6);
}
// 1 / s for s > 0, finite (a row's sum of exponentials, >= 1): hardware estimate + two Newton steps, < 1 ulp off the
// correctly rounded quotient -- 5 instructions against the 12 of an IEEE division
__device__ __forceinline__ double rcp_pos(double s) {
  double y = __builtin_amdgcn_rcp(s);
  double e = fma(-s, y, 1.0);
  y = fma(y, e, y);
  e = fma(-s, y, 1.0);
  return fma(y, e, y);
}

// log1p(z) for z >= 0 within about 2 ulp, one table read and a degree-8 polynomial (the library's log1p works in
// double-double arithmetic: several times the instructions, in a kernel with one log1p per entry).  u = 1 + z = 2^e f,
// f in [1, 2); t_i ~ 1 / (1 + i / 128) for the top seven bits i of f, r = f t_i - 1 in [0, 2^-7) (one fma, correctly
// rounded), log u = e ln 2 - log t_i + log1p(r) with -log t_i as a double-double of the rounded t_i; the rounding error of
// 1 + z (exact: c = z - (u - 1)) adds c / u.
struct LogEntry {
  double t, hi, lo;
};
static __constant__ LogEntry LC_LOG_TAB[128] = {
    {0x1.0000000000000p+0, 0x0.0p+0, 0x0.0p+0},
    {0x1.fc07f01fc07f0p-1, 0x1.fe02a6b106799p-8, -0x1.e44b7e3711e7fp-67},
    {0x1.f81f81f81f820p-1, 0x1.fc0a8b0fc03c4p-7, -0x1.83092c5964281p-62},
    {0x1.f44659e4a4271p-1, 0x1.7b91b07d5b126p-6, -0x1.6d80ab38e9430p-62},
    {0x1.f07c1f07c1f08p-1, 0x1.f829b0e7832f8p-6, 0x1.33e3f04f1ef25p-60},
    {0x1.ecc07b301ecc0p-1, 0x1.39e87b9febd68p-5, -0x1.5bfa937f551b7p-59},
    {0x1.e9131abf0b767p-1, 0x1.77458f632dcffp-5, 0x1.8d3ca87b92968p-63},
    {0x1.e573ac901e574p-1, 0x1.b42dd711971b9p-5, 0x1.0a34531f67db5p-59},
    {0x1.e1e1e1e1e1e1ep-1, 0x1.f0a30c01162a8p-5, 0x1.85f325c5bbacdp-59},
    {0x1.de5d6e3f8868ap-1, 0x1.16536eea37ae3p-4, 0x1.2189705cf74cap-58},
    {0x1.dae6076b981dbp-1, 0x1.341d7961bd1d0p-4, -0x1.3599f227becbbp-58},
    {0x1.d77b654b82c34p-1, 0x1.51b073f06183cp-4, -0x1.5b61c65e5741ap-58},
    {0x1.d41d41d41d41dp-1, 0x1.6f0d28ae56b4ep-4, -0x1.20db323097324p-59},
    {0x1.d0cb58f6ec074p-1, 0x1.8c345d6319b23p-4, -0x1.294d2f5668495p-58},
    {0x1.cd85689039b0bp-1, 0x1.a926d3a4ad562p-4, -0x1.d7a16eab1e2adp-59},
    {0x1.ca4b3055ee191p-1, 0x1.c5e548f5bc743p-4, 0x1.2eb0bf7c0b0d9p-59},
    {0x1.c71c71c71c71cp-1, 0x1.e27076e2af2eap-4, -0x1.61578001e015ap-60},
    {0x1.c3f8f01c3f8f0p-1, 0x1.fec9131dbeabcp-4, -0x1.5746b9981b36cp-58},
    {0x1.c0e070381c0e0p-1, 0x1.0d77e7cd08e5bp-3, 0x1.9a5dc5e9030adp-57},
    {0x1.bdd2b899406f7p-1, 0x1.1b72ad52f67a2p-3, -0x1.fbe7ee5c69946p-57},
    {0x1.bacf914c1bad0p-1, 0x1.29552f81ff521p-3, 0x1.301771c407dc0p-57},
    {0x1.b7d6c3dda338bp-1, 0x1.371fc201e8f75p-3, 0x1.e6cb62af18a02p-62},
    {0x1.b4e81b4e81b4fp-1, 0x1.44d2b6ccb7d1cp-3, 0x1.7d3d950f87e23p-59},
    {0x1.b2036406c80d9p-1, 0x1.526e5e3a1b438p-3, -0x1.546ff8a470d3ap-57},
    {0x1.af286bca1af28p-1, 0x1.5ff3070a793d6p-3, -0x1.bc60efafc6f6cp-58},
    {0x1.ac5701ac5701bp-1, 0x1.6d60fe719d21bp-3, 0x1.d551d97132e87p-57},
    {0x1.a98ef606a63bep-1, 0x1.7ab890210d907p-3, -0x1.1072534a57e7dp-57},
    {0x1.a6d01a6d01a6dp-1, 0x1.87fa06520c911p-3, -0x1.9f7fdbfa08d9ap-57},
    {0x1.a41a41a41a41ap-1, 0x1.9525a9cf456b6p-3, -0x1.26fb3e2b1d1dap-57},
    {0x1.a16d3f97a4b02p-1, 0x1.a23bc1fe2b561p-3, 0x1.24dc46c1ea664p-57},
    {0x1.9ec8e951033d9p-1, 0x1.af3c94e80bff3p-3, 0x1.a3398064df33ep-57},
    {0x1.9c2d14ee4a102p-1, 0x1.bc286742d8cd4p-3, 0x1.cfce744870f57p-58},
    {0x1.999999999999ap-1, 0x1.c8ff7c79a9a20p-3, -0x1.4f689f8434011p-57},
    {0x1.970e4f80cb872p-1, 0x1.d5c216b4fbb94p-3, -0x1.a37794d03657dp-58},
    {0x1.948b0fcd6e9e0p-1, 0x1.e27076e2af2e8p-3, -0x1.61578001e015ep-59},
    {0x1.920fb49d0e229p-1, 0x1.ef0adcbdc5935p-3, 0x1.e8637950dc20dp-57},
    {0x1.8f9c18f9c18fap-1, 0x1.fb9186d5e3e29p-3, 0x1.355519b0de535p-57},
    {0x1.8d3018d3018d3p-1, 0x1.0402594b4d041p-2, -0x1.08ec217a5022dp-57},
    {0x1.8acb90f6bf3aap-1, 0x1.0a324e27390e2p-2, 0x1.bdcfde8061c03p-56},
    {0x1.886e5f0abb04ap-1, 0x1.1058bf9ae4ad4p-2, 0x1.3f415699663ecp-63},
    {0x1.8618618618618p-1, 0x1.1675cababa60fp-2, 0x1.ce63eab883727p-61},
    {0x1.83c977ab2beddp-1, 0x1.1c898c16999fbp-2, 0x1.9f1a39d500e3cp-56},
    {0x1.8181818181818p-1, 0x1.22941fbcf7966p-2, -0x1.dbd7ac258a2bdp-58},
    {0x1.7f405fd017f40p-1, 0x1.2895a13de86a4p-2, 0x1.7ad24c13f040fp-56},
    {0x1.7d05f417d05f4p-1, 0x1.2e8e2bae11d31p-2, -0x1.1e99b72bd7bf2p-57},
    {0x1.7ad2208e0ecc3p-1, 0x1.347dd9a987d56p-2, -0x1.16ea62c048cfbp-56},
    {0x1.78a4c8178a4c8p-1, 0x1.3a64c556945eap-2, 0x1.cbcd735d03424p-60},
    {0x1.767dce434a9b1p-1, 0x1.404308686a7e4p-2, -0x1.f79f6c1059cdbp-57},
    {0x1.745d1745d1746p-1, 0x1.4618bc21c5ec2p-2, -0x1.7a42642661c62p-61},
    {0x1.724287f46debcp-1, 0x1.4be5f957778a1p-2, -0x1.4b366b609027ap-58},
    {0x1.702e05c0b8170p-1, 0x1.51aad872df82ep-2, -0x1.d8db0a7cc1543p-56},
    {0x1.6e1f76b4337c7p-1, 0x1.5767717455a6cp-2, -0x1.fb2a49af933e8p-57},
    {0x1.6c16c16c16c17p-1, 0x1.5d1bdbf5809cap-2, -0x1.7dc9c7c23801fp-56},
    {0x1.6a13cd1537290p-1, 0x1.62c82f2b9c796p-2, -0x1.090a0dd59fe35p-58},
    {0x1.6816816816817p-1, 0x1.686c81e9b14adp-2, 0x1.710af840538e3p-56},
    {0x1.661ec6a5122f9p-1, 0x1.6e08eaa2ba1e4p-2, -0x1.bfb1b39ca3a0fp-56},
    {0x1.642c8590b2164p-1, 0x1.739d7f6bbd007p-2, 0x1.ce24c53fad3f0p-58},
    {0x1.623fa77016240p-1, 0x1.792a55fdd47a1p-2, 0x1.f057691fe9ed7p-56},
    {0x1.6058160581606p-1, 0x1.7eaf83b82afc2p-2, -0x1.698b43096b576p-59},
    {0x1.5e75bb8d015e7p-1, 0x1.842d1da1e8b18p-2, 0x1.54ec519784677p-56},
    {0x1.5c9882b931057p-1, 0x1.89a3386c1425bp-2, 0x1.2d38c40881e0bp-57},
    {0x1.5ac056b015ac0p-1, 0x1.8f11e873662c8p-2, 0x1.f85da755a61a3p-56},
    {0x1.58ed2308158edp-1, 0x1.947941c2116fbp-2, 0x1.1266e8a3e8838p-57},
    {0x1.571ed3c506b3ap-1, 0x1.99d958117e08ap-2, -0x1.315b444ee1f38p-56},
    {0x1.5555555555555p-1, 0x1.9f323ecbf984dp-2, -0x1.a92e513217f58p-59},
    {0x1.5390948f40febp-1, 0x1.a484090e5bb09p-2, 0x1.fff29adc3ad3bp-56},
    {0x1.51d07eae2f815p-1, 0x1.a9cec9a9a084ap-2, -0x1.ab7b00ad0dabcp-58},
    {0x1.5015015015015p-1, 0x1.af1293247786bp-2, 0x1.533844a15dc28p-58},
    {0x1.4e5e0a72f0539p-1, 0x1.b44f77bcc8f64p-2, -0x1.a0892a8b38eedp-61},
    {0x1.4cab88725af6ep-1, 0x1.b9858969310fdp-2, -0x1.f3827583b8877p-57},
    {0x1.4afd6a052bf5bp-1, 0x1.beb4d9da71b7ap-2, 0x1.be1874deaef08p-56},
    {0x1.49539e3b2d067p-1, 0x1.c3dd7a7cdad4dp-2, 0x1.7d9e0a5bd4d37p-57},
    {0x1.47ae147ae147bp-1, 0x1.c8ff7c79a9a21p-2, 0x1.3097607bcbfeep-56},
    {0x1.460cbc7f5cf9ap-1, 0x1.ce1af0b85f3ecp-2, -0x1.6416a1aa97b31p-57},
    {0x1.446f86562d9fbp-1, 0x1.d32fe7e00ebd5p-2, 0x1.4ef6465f5f46ep-57},
    {0x1.42d6625d51f87p-1, 0x1.d83e7258a2f3ep-2, 0x1.c515ba2ec9444p-58},
    {0x1.4141414141414p-1, 0x1.dd46a04c1c4a1p-2, -0x1.19d95b62e2476p-62},
    {0x1.3fb013fb013fbp-1, 0x1.e24881a7c6c26p-2, 0x1.05ec7a2caa523p-57},
    {0x1.3e22cbce4a902p-1, 0x1.e744261d68789p-2, 0x1.cdf68dbcf2ed3p-56},
    {0x1.3c995a47babe7p-1, 0x1.ec399d2468cc1p-2, -0x1.94623581958cfp-59},
    {0x1.3b13b13b13b14p-1, 0x1.f128f5faf06ecp-2, -0x1.328df13bb38c2p-56},
    {0x1.3991c2c187f63p-1, 0x1.f6123fa7028adp-2, 0x1.5456c3cb6cd06p-58},
    {0x1.3813813813814p-1, 0x1.faf588f78f31dp-2, 0x1.cd7d9f2754362p-57},
    {0x1.3698df3de0748p-1, 0x1.ffd2e0857f497p-2, -0x1.4d05f9366f27fp-59},
    {0x1.3521cfb2b78c1p-1, 0x1.02552a5a5d0ffp-1, 0x1.e9c695d7ee800p-57},
    {0x1.33ae45b57bcb2p-1, 0x1.04bdf9da926d2p-1, 0x1.8fe60804593bfp-56},
    {0x1.323e34a2b10bfp-1, 0x1.0723e5c1cdf41p-1, -0x1.6a1a71dbba44ep-59},
    {0x1.30d190130d190p-1, 0x1.0986f4f573521p-1, -0x1.37012b5805e02p-56},
    {0x1.2f684bda12f68p-1, 0x1.0be72e4252a83p-1, 0x1.b4c4bdd99efffp-56},
    {0x1.2e025c04b8097p-1, 0x1.0e44985d1cc8cp-1, -0x1.c546885a5a707p-59},
    {0x1.2c9fb4d812ca0p-1, 0x1.109f39e2d4c96p-1, 0x1.f78fb26c2de46p-55},
    {0x1.2b404ad012b40p-1, 0x1.12f719593efbdp-1, -0x1.67f6e731c1795p-56},
    {0x1.29e4129e4129ep-1, 0x1.154c3d2f4d5eap-1, 0x1.98f33a3965e29p-57},
    {0x1.288b01288b013p-1, 0x1.179eabbd899a0p-1, -0x1.c73e320bf059fp-58},
    {0x1.27350b8812735p-1, 0x1.19ee6b467c96fp-1, -0x1.fa3422887e218p-57},
    {0x1.25e22708092f1p-1, 0x1.1c3b81f713c25p-1, -0x1.0b583899021d1p-56},
    {0x1.2492492492492p-1, 0x1.1e85f5e7040d1p-1, -0x1.084e99683070ep-55},
    {0x1.23456789abcdfp-1, 0x1.20cdcd192ab6ep-1, -0x1.aabf0bc229014p-55},
    {0x1.21fb78121fb78p-1, 0x1.23130d7bebf43p-1, -0x1.748725e374d6ep-55},
    {0x1.20b470c67c0d9p-1, 0x1.2555bce98f7cap-1, 0x1.9810eb6b440f4p-55},
    {0x1.1f7047dc11f70p-1, 0x1.2795e1289b11bp-1, 0x1.ade0fcf6e5a1dp-55},
    {0x1.1e2ef3b3fb874p-1, 0x1.29d37fec2b08bp-1, 0x1.01735b2e9733fp-55},
    {0x1.1cf06ada2811dp-1, 0x1.2c0e9ed448e8cp-1, -0x1.8a158f3917586p-55},
    {0x1.1bb4a4046ed29p-1, 0x1.2e47436e40268p-1, 0x1.0950861a4886bp-55},
    {0x1.1a7b9611a7b96p-1, 0x1.307d7334f10bep-1, 0x1.fdac850fab36dp-56},
    {0x1.19453808ca29cp-1, 0x1.32b1339121d71p-1, 0x1.d02ab5b3d916bp-56},
    {0x1.1811811811812p-1, 0x1.34e289d9ce1d2p-1, 0x1.775c96c42e729p-56},
    {0x1.16e0689427379p-1, 0x1.37117b54747b6p-1, -0x1.808bf6deec882p-55},
    {0x1.15b1e5f75270dp-1, 0x1.393e0d3562a1ap-1, -0x1.38eef67f2483ap-55},
    {0x1.1485f0e0acd3bp-1, 0x1.3b68449fffc23p-1, 0x1.c63b7b06164dap-55},
    {0x1.135c81135c811p-1, 0x1.3d9026a7156fbp-1, 0x1.0084c7a15a4f5p-58},
    {0x1.12358e75d3033p-1, 0x1.3fb5b84d16f43p-1, 0x1.0a74ea82e55dfp-56},
    {0x1.1111111111111p-1, 0x1.41d8fe84672afp-1, -0x1.ee6d0cf42e7fap-55},
    {0x1.0fef010fef011p-1, 0x1.43f9fe2f9ce67p-1, 0x1.e1c9ee6d83b86p-55},
    {0x1.0ecf56be69c90p-1, 0x1.4618bc21c5ec2p-1, 0x1.e85bd9bd99e3ap-56},
    {0x1.0db20a88f4696p-1, 0x1.48353d1ea88dfp-1, -0x1.40a85d133f80bp-55},
    {0x1.0c9714fbcda3bp-1, 0x1.4a4f85db03ebbp-1, -0x1.d76102e1644f2p-55},
    {0x1.0b7e6ec259dc8p-1, 0x1.4c679afccee39p-1, -0x1.e971322ce7900p-57},
    {0x1.0a6810a6810a7p-1, 0x1.4e7d811b75bb0p-1, -0x1.5d3d9ea6e9ea8p-55},
    {0x1.0953f39010954p-1, 0x1.50913cc01686bp-1, 0x1.9e59d2d85ab62p-56},
    {0x1.0842108421084p-1, 0x1.52a2d265bc5abp-1, 0x1.73be4578ad97bp-56},
    {0x1.073260a47f7c6p-1, 0x1.54b2467999498p-1, 0x1.f4550a2d0f60cp-55},
    {0x1.0624dd2f1a9fcp-1, 0x1.56bf9d5b3f399p-1, 0x1.11c6217363fcbp-57},
    {0x1.05197f7d73404p-1, 0x1.58cadb5cd7989p-1, 0x1.624bc9764c22cp-55},
    {0x1.0410410410410p-1, 0x1.5ad404c359f2dp-1, 0x1.eca6aa97c08e7p-55},
    {0x1.03091b51f5e1ap-1, 0x1.5cdb1dc6c1765p-1, 0x1.47b71e2eb8419p-56},
    {0x1.0204081020408p-1, 0x1.5ee02a9241676p-1, -0x1.bca7da80b6f7ep-55},
    {0x1.0101010101010p-1, 0x1.60e32f44788d9p-1, -0x1.58376a5f4b135p-57}};
__device__ __forceinline__ void fill_log_table(LogEntry* lt, int tid, int nthreads) {
  for (int i = tid; i < 128; i += nthreads) lt[i] = LC_LOG_TAB[i];
}
__device__ __forceinline__ double log1p_nonneg(double z, const LogEntry* lt) {
  const double u = 1.0 + z;
  const double c = z - (u - 1.0);
  const int hi = __double2hiint(u);
  const LogEntry& L = lt[(hi >> 13) & 127];
  const double f = __hiloint2double((hi & 0x000fffff) | 0x3ff00000, __double2loint(u));
  const double e = (double)((hi >> 20) - 1023);
  const double r = fma(f, L.t, -1.0);
  double p = fma(-0.125, r, 1.0 / 7.0);  // log1p(r) = r + r^2 (-1/2 + r/3 - ... - r^6/8)
  p = fma(p, r, -1.0 / 6.0);
  p = fma(p, r, 0.2);
  p = fma(p, r, -0.25);
  p = fma(p, r, 1.0 / 3.0);
  p = fma(p, r, -0.5);
  const double lr = fma(r * r, p, r);
  const double head = fma(e, 0x1.62e42fefa3800p-1, L.hi);  // (ln 2's leading part times e is exact)
  const double tail = fma(e, 0x1.ef35793c76730p-45, L.lo) + c * __builtin_amdgcn_rcp(u);
  const double res = head + (lr + tail);
  return u < __builtin_huge_val() ? res : u;
}

// Fingerprint of one row of responsibilities (softmax_cached_kernel writes and compares them; qhash_verify_kernel
// recomputes them in the tests): a multiplicative chain over the NON-ZERO entries,
//   h <- (h ^ (bits(q_j) + C (j + 1))) * G;  h ^= h >> 32      (mod 2^64, G odd)
// A zero entry leaves h as it is, so K columns and K + 1 columns with q_K = 0 agree; every other entry is mixed in
// together with its column, so a label that moves from one column to another changes the fingerprint.  (Round 4 summed
// bits(q_j) * G (2 j + 1): LINEAR in the bit patterns -- two rows collided whenever sum_j (2 j + 1) dbits_j = 0, e.g.
// column 0 up by 3 ulp and column 1 down by 1, which few-ulp moves between the sweeps of a split round do produce.
// In the chain a change of any entry reaches every later step through a product and an xor: no small integer relation
// between the entries' moves survives.)
constexpr uint64_t QHASH_SEED = 0x243F6A8885A308D3ull;
__device__ __forceinline__ uint64_t qhash_step(uint64_t acc, double q, int j) {
  const uint64_t b = (uint64_t)__double_as_longlong(q);  // (q >= +0: a zero is the all-zero pattern)
  uint64_t t = (acc ^ (b + 0xD6E8FEB86659FD93ull * (uint64_t)(j + 1))) * 0x9E3779B97F4A7C15ull;
  t ^= t >> 32;
  return b ? t : acc;
}
__device__ __forceinline__ int64_t qhash_finish(uint64_t acc) {
  const int64_t h = (int64_t)acc;
  return h == QHASH_NONE ? 1 : h;
}

// n-th read of a cluster's parameter stream (for it: -b[it], tile(it,0), ..., tile(it,it)):
// .jt < 0: element of the -b vector (offset in doubles from Pb), else of tile (it,jt) (from Pt)
struct RdInfo {
  int it, jt, off;
};
__host__ __device__ constexpr RdInfo rd_info(int n) {
  int it = 0;
  while (n >= it + 2) {
    n -= it + 2;
    ++it;
  }
  return n == 0 ? RdInfo{it, -1, 4 * it} : RdInfo{it, n - 1, (it * (it + 1) / 2 + (n - 1)) * 16};
}

// compile-time loop: f(std::integral_constant<int, 0>{}), ..., f(<N-1>)
template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

// sum over the 4 lanes {l, l^16, l^32, l^48}
__device__ __forceinline__ double sum_over_hi(double v) {
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
// sum over the 16 lanes of a DPP row (same hi)
__device__ __forceinline__ double sum_over_lo4(double v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
  v = sum_over_lo4(v);
  return sum_over_hi(v);
}
// largest value of the wave, in every lane
__device__ __forceinline__ double wave_max(double v) {
  for (int d = 1; d < 64; d <<= 1) v = fmax(v, __shfl_xor(v, d));
  return v;
}

// lane `src` (wave-uniform) of a double, through the scalar unit
__device__ __forceinline__ double readlane_f64(double v, int src) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// group of a padded row and whether it holds an observation (rginfo: lck::rginfo_pack per row group, or null for a single
// group of nrows rows)
__device__ __forceinline__ bool row_valid(int64_t row, const int* rginfo, int64_t nrows, int& j) {
  const int64_t g = row / RG;
  const int r = (int)(row - g * RG);
  int nv;
  if (rginfo) {
    const int w = rginfo[g];
    j = w >> 5;
    nv = w & 31;
  } else {
    j = 0;
    const int64_t rem = nrows - g * RG;
    nv = rem >= RG ? RG : rem > 0 ? (int)rem : 0;
  }
  return r < nv;
}

// online log-sum-exp: the terms pushed so far sum to s * exp(m); one exponential per term.  -inf terms add nothing
// (with m = -inf too, d is NaN: not `up`, and exp_nonpos clamps NaN to exp(-750) = 0).
__device__ __forceinline__ void lse_push(double v, double& m, double& s, const double* etab) {
  const double d = v - m;
  const bool up = d > 0.0;
  const double e = exp_nonpos(up ? -d : d, etab);
  s = up ? fma(s, e, 1.0) : s + e;
  m = up ? v : m;
}

}  // namespace lck
