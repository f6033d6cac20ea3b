// The generator of sdeint's Brownian increments (include/xde_hip_sde.h spells the mapping out): ONE statement of Philox4x32-10, the
// uniform mapping and Box-Muller, shared by the step kernels of xde_sde.hip and the fused step + KL kernels of xde_kl.hip.  The normals
// of a Philox call are those of elements W j .. W j + W - 1 of the FLAT array, whatever launch shape asks for them.
#pragma once

#include "xde_common.hpp"

namespace xde {

constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;  // Philox4x32 round multipliers
constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;  // Weyl key increments

struct Words {
  uint32_t w[4];
};

// Philox4x32-10 at counter (j_lo, j_hi, k, draw) under key (key0, key1)
__device__ __forceinline__ Words philox(uint64_t j, uint32_t k, uint32_t key0, uint32_t key1, uint32_t draw) {
  uint32_t c0 = uint32_t(j), c1 = uint32_t(j >> 32), c2 = k, c3 = draw;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) {
      key0 += kW0;
      key1 += kW1;
    }
    const uint32_t hi0 = __umulhi(kM0, c0), lo0 = kM0 * c0;
    const uint32_t hi1 = __umulhi(kM1, c2), lo1 = kM1 * c2;
    c0 = hi1 ^ c1 ^ key0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ key1;
    c3 = lo0;
  }
  return Words{{c0, c1, c2, c3}};
}

template <typename T> struct Block;  // normals per Philox call = elements per 16-byte vector
template <> struct Block<float> { static constexpr int W = 4; };
template <> struct Block<double> { static constexpr int W = 2; };

__device__ __forceinline__ void box_muller(float u1, float u2, float& z0, float& z1) {
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * u2, &sn, &cs);  // cos / sin of 2 pi u2 without rounding 2 pi
  z0 = r * cs;
  z1 = r * sn;
}

__device__ __forceinline__ void box_muller(double u1, double u2, double& z0, double& z1) {
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
}

// the normals of elements W j .. W j + W - 1 at step k (include/xde_hip_sde.h spells the mapping out): draw 0 is Z, draw 1 is V
__device__ __forceinline__ void normals(uint64_t j, uint32_t k, uint32_t key0, uint32_t key1, uint32_t draw, float (&z)[4]) {
  const Words x = philox(j, k, key0, key1, draw);
  float u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = float((x.w[i] >> 8) + 1u) * 0x1p-24f;
  box_muller(u[0], u[1], z[0], z[1]);
  box_muller(u[2], u[3], z[2], z[3]);
}

__device__ __forceinline__ void normals(uint64_t j, uint32_t k, uint32_t key0, uint32_t key1, uint32_t draw, double (&z)[2]) {
  const Words x = philox(j, k, key0, key1, draw);
  const uint64_t a = ((uint64_t(x.w[1]) << 32) | x.w[0]) >> 11;
  const uint64_t b = ((uint64_t(x.w[3]) << 32) | x.w[2]) >> 11;
  box_muller(double(a + 1u) * 0x1p-53, double(b + 1u) * 0x1p-53, z[0], z[1]);
}

}  // namespace xde
