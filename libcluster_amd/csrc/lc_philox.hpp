// Counter-based random numbers on the device: Philox-4x32-10, 53-bit uniforms, a Box-Muller pair and a
// Marsaglia-Tsang gamma draw.  Shared by the synthetic-data generator (lc_kernels_aux.hip) and the model samplers
// (lc_kernels_sample.hip; holes_draws_kernel in lc_kernels_holes.hip).  Every value is a function of its counter and the key alone: nothing here depends on the launch
// shape or on what other lanes do.  The counter table is in the header comment of include/libcluster_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lck {

// stream tags (c3 & 0xff); bits 8 .. 31 of c3 hold the stream's sub-index (normal pair or gamma attempt)
constexpr uint32_t RNG_TAG_SYNTH_NORMAL = 0x01;  // lc_ctx_synth: c2 = pair
constexpr uint32_t RNG_TAG_SYNTH_LABEL = 0x02;   // lc_ctx_synth: c2 = 0
constexpr uint32_t RNG_TAG_CHOICE = 0x10;        // component choice: c2 = draw
constexpr uint32_t RNG_TAG_NORMAL = 0x11;        // normals: c2 = draw, sub = pair p -> z[2p], z[2p + 1]
constexpr uint32_t RNG_TAG_GAMMA_N = 0x12;       // gamma attempt's normal: c2 = draw or slot, sub = attempt
constexpr uint32_t RNG_TAG_GAMMA_U = 0x13;       // gamma attempt's uniform: c2 = draw or slot, sub = attempt
constexpr uint32_t RNG_TAG_GAMMA_B = 0x14;       // the uniform of the shape < 1 boost: c2 = draw or slot, sub = 0
constexpr uint32_t RNG_TAG_LOMAX = 0x15;         // Lomax uniforms: c2 = column pair p -> columns 2p, 2p + 1
constexpr int RNG_GAMMA_ATTEMPTS = 64;           // a rejection run this long has probability < 1e-80

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
    const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += W0; k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ double u01(uint32_t a, uint32_t b) {
  // 53-bit uniform in (0,1)
  const uint64_t v = (((uint64_t)a << 32) | b) >> 11;
  return ((double)v + 0.5) * (1.0 / 9007199254740992.0);
}

// the two normals of one Philox block: u1 = u01(o[0], o[1]), u2 = u01(o[2], o[3])
__device__ __forceinline__ void box_muller(const uint32_t o[4], double& z0, double& z1) {
  const double u1 = u01(o[0], o[1]), u2 = u01(o[2], o[3]);
  const double rad = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincos(6.283185307179586476925 * u2, &sn, &cs);
  z0 = rad * cs;
  z1 = rad * sn;
}

// One stream of a row: the 64-bit row counter g, the key and c2 (draw or slot).
struct RngStream {
  uint32_t c0, c1, c2, k0, k1;
  __device__ __forceinline__ void block(uint32_t tag, uint32_t sub, uint32_t o[4]) const {
    philox4x32_10(c0, c1, c2, tag | (sub << 8), k0, k1, o);
  }
};
__device__ __forceinline__ RngStream rng_stream(uint64_t g, uint64_t seed, uint32_t c2) {
  return RngStream{(uint32_t)g, (uint32_t)(g >> 32), c2, (uint32_t)seed, (uint32_t)(seed >> 32)};
}

// Gamma(shape, 1) for any shape > 0 (Marsaglia and Tsang 2000): attempt t takes its normal from block (GAMMA_N, t) and its
// uniform from block (GAMMA_U, t); shape < 1 draws Gamma(shape + 1) U^(1 / shape) with U from block (GAMMA_B, 0).
__device__ __forceinline__ double gamma_draw(const RngStream& s, double shape) {
  const double a = shape < 1.0 ? shape + 1.0 : shape;
  const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  double g = d;
  for (int t = 0; t < RNG_GAMMA_ATTEMPTS; ++t) {
    uint32_t o[4];
    s.block(RNG_TAG_GAMMA_N, (uint32_t)t, o);
    double x, unused;
    box_muller(o, x, unused);
    const double w = 1.0 + c * x;
    if (!(w > 0.0)) continue;
    const double v = w * w * w;
    s.block(RNG_TAG_GAMMA_U, (uint32_t)t, o);
    const double u = u01(o[0], o[1]);
    g = d * v;
    if (log(u) < 0.5 * x * x + d - d * v + d * log(v)) break;
  }
  if (shape < 1.0) {
    uint32_t o[4];
    s.block(RNG_TAG_GAMMA_B, 0u, o);
    g *= exp(log(u01(o[0], o[1])) / shape);
  }
  return g > 1e-300 ? g : 1e-300;  // (a scale divides by it)
}

}  // namespace lck
