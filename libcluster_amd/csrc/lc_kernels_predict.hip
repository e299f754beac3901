// Prediction kernels: what a learned mixture says about observations that were not in the training set.
//
// predict_rows_kernel finishes the raw E-step (estep_kernel / estep_wide_kernel / estep_diag_kernel with zero
// constants) the way vbexpectation does (cluster.cpp:91-138) -- E[log pi_jk] + Eloglike_k(x_n), log-sum-exp over
// Kful, q = exp(. - logZ) -- and, for Gauss-Wishart clusters, turns the same distances into the posterior predictive
// (multivariate Student-t per cluster, mixed with E[pi_jk]).  predict_diag_kernel forms the predictive of the separable
// families (product of Student-t / Lomax densities per dimension), which has no GEMM form.
#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "lc_device.hpp"
#include "lc_predict.hpp"

namespace lck {
namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_COLS = 8;  // predict_rows_kernel: columns loaded per batch

// group of a padded row and whether it holds an observation
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

__global__ __launch_bounds__(PR_THREADS) void predict_rows_kernel(PredictRowsLaunch a) {
  __shared__ double etab[64];
  __shared__ LogEntry ltab[128];
  fill_exp_table(etab, threadIdx.x, PR_THREADS);
  fill_log_table(ltab, threadIdx.x, PR_THREADS);
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  int j = 0;
  if (row >= a.nrg * RG || !row_valid(row, a.rginfo, a.nrows, j)) return;
  const double* __restrict__ ct = a.ctab + (size_t)j * a.K;
  const double* __restrict__ pt = a.ptab + (size_t)j * a.Kp;
  const double* __restrict__ col = a.col + row;
  constexpr double NINF = -std::numeric_limits<double>::infinity();
  double m = NINF, s = 0.0, best = NINF, mp = NINF, sp = 0.0;
  int lab = 0;
  const int Kmax = a.K > a.Kp ? a.K : a.Kp;
  for (int k0 = 0; k0 < Kmax; k0 += PR_COLS) {  // the one read of the row's columns
    // PR_COLS independent loads in flight per lane before the arithmetic that consumes them (one at a time left the
    // kernel waiting on memory latency)
    double r[PR_COLS];
#pragma unroll
    for (int i = 0; i < PR_COLS; ++i) r[i] = k0 + i < Kmax ? col[(size_t)(k0 + i) * a.ldq] : 0.0;
#pragma unroll
    for (int i = 0; i < PR_COLS; ++i) {
      const int k = k0 + i;
      if (k < a.K) {
        const double v = ct[k] + r[i];
        if (v > best) {  // first maximum: the lowest k on ties
          best = v;
          lab = k;
        }
        lse_push(v, m, s, etab);
      }
      if (k < a.Kp) lse_push(pt[k] - a.pexp[k] * log1p_nonneg(a.pscale[k] * (-2.0 * r[i]), ltab), mp, sp, etab);
    }
  }
  const double lz = m + log(s);
  a.label[row] = lab;
  a.logZ[row] = lz;
  if (a.Kp > 0) a.logp[row] = mp + log(sp);
  if (a.keep_q) {
    double* q = a.qcol + row;
    for (int k = 0; k < a.K; ++k) q[(size_t)k * a.ldq] = exp_nonpos(ct[k] + q[(size_t)k * a.ldq] - lz, etab);
  }
}

// log of a product of factors >= 1 taken PRED_RENORM at a time, the binary exponent moved out after every group
__device__ __forceinline__ double log_scaled(double p, int ex) {
  return fma((double)ex, 0x1.62e42fefa39efp-1, log(p)) + (double)ex * 0x1.abc9e3b39803fp-56;
}

template <int MODE>
__device__ __forceinline__ double pred_factor(double x, double ad, double wd) {
  if constexpr (MODE == 0) {
    const double t = x - ad;
    return fma(wd * t, t, 1.0);
  } else {
    return fma(wd, x, 1.0);
  }
}

// DPT > 0: the padded width is DPT and the row's x lives in registers; DPT = 0: any DP, x re-read from the cache
template <int MODE, int DPT>
__global__ __launch_bounds__(PR_THREADS) void predict_diag_kernel(PredictDiagLaunch a) {
  __shared__ double etab[64];
  fill_exp_table(etab, threadIdx.x, PR_THREADS);
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  int j = 0;
  if (row >= a.nrg * RG || !row_valid(row, a.rginfo, a.nrows, j)) return;
  const int DP = DPT > 0 ? DPT : a.DP;
  const double* __restrict__ xr = a.X + (size_t)row * DP;
  double xv[DPT > 0 ? DPT : 1];
  bool neg = false;
  if constexpr (DPT > 0) {
#pragma unroll
    for (int d = 0; d < DPT; d += 2) {
      const double2 v = *reinterpret_cast<const double2*>(xr + d);
      xv[d] = v.x;
      xv[d + 1] = v.y;
      neg = neg || v.x < 0.0 || v.y < 0.0;
    }
  } else {
    for (int d = 0; d < DP; ++d) neg = neg || xr[d] < 0.0;
  }
  if (MODE == 1 && neg) *a.flag = 1;  // (ExpGamma's domain, cluster.cpp:742; every writer stores the same value)
  const double* __restrict__ pt = a.ptab + (size_t)j * a.Kp;
  double m = -std::numeric_limits<double>::infinity(), s = 0.0;
  for (int k = 0; k < a.Kp; ++k) {  // wave-uniform: the cluster's parameters are the same for every lane
    const double* __restrict__ ak = a.a + (size_t)k * DP;
    const double* __restrict__ wk = a.w + (size_t)k * DP;
    // two running products over alternate groups of PRED_RENORM factors, each group multiplied as a tree: the chain of
    // dependent fp64 operations is a third of the serial product's (the kernel runs at 2-3 waves per SIMD)
    double p[2] = {1.0, 1.0};
    int ex[2] = {0, 0};
    auto group = [&](int h, double f0, double f1, double f2, double f3) {
      int e;
      p[h] = frexp(p[h] * ((f0 * f1) * (f2 * f3)), &e);
      ex[h] += e;
    };
    static_assert(PRED_RENORM == 4, "group() takes four factors");
    if constexpr (DPT > 0) {
      static_for<DPT / PRED_RENORM>([&](auto c) {
        const int d = c * PRED_RENORM;
        group(c & 1, pred_factor<MODE>(xv[d], MODE == 0 ? ak[d] : 0.0, wk[d]),
              pred_factor<MODE>(xv[d + 1], MODE == 0 ? ak[d + 1] : 0.0, wk[d + 1]),
              pred_factor<MODE>(xv[d + 2], MODE == 0 ? ak[d + 2] : 0.0, wk[d + 2]),
              pred_factor<MODE>(xv[d + 3], MODE == 0 ? ak[d + 3] : 0.0, wk[d + 3]));
      });
    } else {
      for (int d = 0; d < DP; d += PRED_RENORM)
        group((d / PRED_RENORM) & 1, pred_factor<MODE>(xr[d], MODE == 0 ? ak[d] : 0.0, wk[d]),
              pred_factor<MODE>(xr[d + 1], MODE == 0 ? ak[d + 1] : 0.0, wk[d + 1]),
              pred_factor<MODE>(xr[d + 2], MODE == 0 ? ak[d + 2] : 0.0, wk[d + 2]),
              pred_factor<MODE>(xr[d + 3], MODE == 0 ? ak[d + 3] : 0.0, wk[d + 3]));
    }
    lse_push(pt[k] - a.pexp[k] * log_scaled(p[0] * p[1], ex[0] + ex[1]), m, s, etab);
  }
  a.logp[row] = m + log(s);
}

// Conditional mean.  Lane = lo2 + 4 blk + 16 hi of v_mfma_f64_4x4x4_4b (lc_device.hpp): MFMA block blk of
// row group g multiplies the rows 16 g + 4 blk + {0..3} of the wave (A: row lo2, column hi of the k-step) with a 4 x 4 piece
// of the table (B: given column hi, target lo2 -- the same in all four blocks) into D (row hi, target lo2).  In the first
// part lane l scores row l of the wave, which is row 4 blk + lo2 of row group hi: the r_k of row group g sit in the lanes
// with hi = g, and one __shfl per row group hands them to the lanes that build the A operands.
__global__ __launch_bounds__(PC_THREADS) void predict_cond_kernel(PredictCondLaunch a) {
  __shared__ double etab[64];
  __shared__ LogEntry ltab[128];
  fill_exp_table(etab, threadIdx.x, PC_THREADS);
  fill_log_table(ltab, threadIdx.x, PC_THREADS);
  __syncthreads();  // (the only barrier: from here on the waves do not meet)
  constexpr int NG = PC_WAVE_ROWS / RG, NS = PC_CHUNK / 4, NQ = PC_PANEL / 4;
  static_assert(RG == 16 && NG == 4, "one MFMA block per quad of rows, one shuffle source per row group");
  const int lane = threadIdx.x & 63, lo2 = lane & 3, blk = (lane >> 2) & 3, hi = lane >> 4;
  const int64_t NP = a.nrg * RG;
  const int64_t wrow0 = ((int64_t)blockIdx.x * (PC_THREADS / 64) + (threadIdx.x >> 6)) * PC_WAVE_ROWS;
  if (wrow0 >= NP) return;
  // NP is a multiple of 16, not of 64: rows past the end are clamped for reading and never written
  const int64_t row = wrow0 + lane, rrow = row < NP ? row : NP - 1;
  int j = 0;
  const bool valid = row_valid(rrow, a.rginfo, a.nrows, j) && row < NP;
  if (!valid) j = 0;  // (a pad row is scored like any other, so that the wave stays whole, and nothing of it is written)
  constexpr double NINF = -std::numeric_limits<double>::infinity();
  double* __restrict__ col = a.col + rrow;
  double logp;
  {  // log p(x_a) as predict_rows_kernel forms logp; t_k replaces the raw column
    const double* __restrict__ tt = a.ttab + (size_t)j * a.Kp;
    double m = NINF, s = 0.0;
    for (int k0 = 0; k0 < a.Kp; k0 += PR_COLS) {
      double r[PR_COLS];
#pragma unroll
      for (int i = 0; i < PR_COLS; ++i) r[i] = k0 + i < a.Kp ? col[(size_t)(k0 + i) * a.ldq] : 0.0;
#pragma unroll
      for (int i = 0; i < PR_COLS; ++i) {
        const int k = k0 + i;
        if (k < a.Kp) {
          const double t = tt[k] - a.pexp[k] * log1p_nonneg(a.pscale[k] * (-2.0 * r[i]), ltab);
          lse_push(t, m, s, etab);
          if (valid) col[(size_t)k * a.ldq] = t;
        }
      }
    }
    logp = m + log(s);
    if (valid) a.logp[row] = logp;
  }
  // rows of the A operands (row lo2 of block blk) and of the results (row hi of block blk), per row group
  int64_t xrow[NG];
  bool ovalid[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int64_t ra = wrow0 + g * RG + 4 * blk + lo2, ro = wrow0 + g * RG + 4 * blk + hi;
    xrow[g] = ra < NP ? ra : NP - 1;
    int jo;
    ovalid[g] = ro < NP && row_valid(ro < NP ? ro : NP - 1, a.rginfo, a.nrows, jo);
  }
  for (int t0 = 0; t0 < a.Db; t0 += PC_PANEL) {  // the accumulators of one panel of targets are resident
    const int nq = (a.Dbp - t0) / 4 < NQ ? (a.Dbp - t0) / 4 : NQ;
    double acc[NG][NQ];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int q = 0; q < NQ; ++q) acc[g][q] = 0.0;
    for (int c0 = 0; c0 < a.Dae; c0 += PC_CHUNK) {  // the x of one chunk of given columns is resident
      const int ns = (a.Dae - c0) / 4 < NS ? (a.Dae - c0) / 4 : NS;
      double x[NG][NS];
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          const int c = c0 + 4 * s + hi;
          x[g][s] = c < a.Da ? a.X[(size_t)xrow[g] * a.DP + c] : c == a.Da ? 1.0 : 0.0;  // (the ones column carries m_b)
        }
      for (int k = 0; k < a.Kp; ++k) {
        // the tables stream from the cache cluster by cluster: Kp (Da + 1) Db doubles do not fit the LDS
        const double t = valid ? col[(size_t)k * a.ldq] : NINF;
        const double r = valid ? exp_nonpos(t - logp, etab) : 0.0;
        double rg[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) rg[g] = __shfl(r, g * RG + 4 * blk + lo2);
        const double* __restrict__ mk = a.mext + (size_t)k * a.Dae + c0 + hi;
        const double* __restrict__ Tk = a.T + ((size_t)k * a.Dae + c0 + hi) * a.Dbp + t0 + lo2;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          if (s < ns) {
            // the four scaled, centred operands of a k-step first, then its MFMAs in one run (a VALU
            // instruction between MFMAs is paid per switch)
            const double mv = mk[4 * s];
            double av[NG], bv[NQ];
#pragma unroll
            for (int g = 0; g < NG; ++g) av[g] = rg[g] * (x[g][s] - mv);
#pragma unroll
            for (int q = 0; q < NQ; ++q) bv[q] = q < nq ? Tk[(size_t)(4 * s) * a.Dbp + 4 * q] : 0.0;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
              if (q < nq) {
#pragma unroll
                for (int g = 0; g < NG; ++g) acc[g][q] = mfma4(av[g], bv[q], acc[g][q]);
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int64_t ro = wrow0 + g * RG + 4 * blk + hi;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int tcol = t0 + 4 * q + lo2;
        if (ovalid[g] && tcol < a.Db) a.mean[(size_t)ro * a.Db + tcol] = acc[g][q];
      }
    }
  }
}

template <int MODE>
hipError_t launch_diag_mode(const PredictDiagLaunch& a, dim3 grid, hipStream_t stream) {
  switch (a.DP) {
    case 16: hipLaunchKernelGGL((predict_diag_kernel<MODE, 16>), grid, dim3(PR_THREADS), 0, stream, a); break;
    case 32: hipLaunchKernelGGL((predict_diag_kernel<MODE, 32>), grid, dim3(PR_THREADS), 0, stream, a); break;
    case 48: hipLaunchKernelGGL((predict_diag_kernel<MODE, 48>), grid, dim3(PR_THREADS), 0, stream, a); break;
    case 64: hipLaunchKernelGGL((predict_diag_kernel<MODE, 64>), grid, dim3(PR_THREADS), 0, stream, a); break;
    default: hipLaunchKernelGGL((predict_diag_kernel<MODE, 0>), grid, dim3(PR_THREADS), 0, stream, a); break;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_predict_rows(const PredictRowsLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  const dim3 grid((unsigned)((rows + PR_THREADS - 1) / PR_THREADS));
  hipLaunchKernelGGL(predict_rows_kernel, grid, dim3(PR_THREADS), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_predict_diag(const PredictDiagLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0 || a.DP % PRED_RENORM != 0) return rows == 0 ? hipSuccess : hipErrorInvalidValue;
  const dim3 grid((unsigned)((rows + PR_THREADS - 1) / PR_THREADS));
  return a.mode == 0 ? launch_diag_mode<0>(a, grid, stream) : launch_diag_mode<1>(a, grid, stream);
}

hipError_t launch_predict_cond(const PredictCondLaunch& a, hipStream_t stream) {
  const int64_t rows = a.nrg * RG;
  if (rows == 0) return hipSuccess;
  if (a.Kp < 1 || a.Da < 1 || a.Db < 1 || a.DP < a.Da || a.Dae < a.Da + 1 || a.Dae % 4 != 0 || a.Dbp < a.Db || a.Dbp % 4 != 0)
    return hipErrorInvalidValue;
  const int64_t per = (int64_t)(PC_THREADS / 64) * PC_WAVE_ROWS;
  hipLaunchKernelGGL(predict_cond_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(PC_THREADS), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lck
