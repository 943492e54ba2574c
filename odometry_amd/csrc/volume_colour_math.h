// volume_colour_math.h — the colour update of the TSDF volume's colour grid (include/odometry_hip.h, odo_volume_integrate_colour_dev /
// DESIGN.md section 9.6), host + device like odo_math.h: the kernel of volume_colour_kernels.hip and the g++ harness of
// tests/volume_colour_math_harness.cpp compile these same lines.
//
// The rule, per channel, in unsigned integers with floor division:  c' = (c * wc + s + ((wc + 1) >> 1)) / (wc + 1).
// The device has no integer divider; the divisor d = wc + 1 (1 .. 256) is shared by the three channels, so one reciprocal
// M = floor((2^32 - 1) / d) + 1 is formed per voxel and every quotient is the high word of n * M:
//   d no power of two: M = floor(2^32 / d) + 1, M d = 2^32 + e with 0 < e <= d, and n M / 2^32 = n / d + n e / (d 2^32); the second term
//     is below 2^17 * 256 / (d 2^32) = 2^-7 / d < 1 / d, the fraction of n / d is at most (d - 1) / d: the floor is that of n / d;
//   d a power of two (>= 2): M = 2^32 / d exactly;
//   d == 1 (wc == 0, the first sample) needs M = 2^32: taken out, c' = s.
// n = c * wc + s + (d >> 1) <= 255 * 255 + 255 + 128 < 2^17.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ODO_COLOUR_HD __host__ __device__ __forceinline__
#else
#define ODO_COLOUR_HD static inline
#endif

namespace odo {

// The reciprocal of d = 2 .. 256.
ODO_COLOUR_HD uint32_t colour_reciprocal(uint32_t d) { return 0xffffffffu / d + 1u; }

// One channel: c the stored value, wc = 1 .. 255 its weight, s the sample, M = colour_reciprocal(wc + 1).
ODO_COLOUR_HD uint32_t colour_channel(uint32_t c, uint32_t wc, uint32_t s, uint32_t M) {
  const uint32_t n = c * wc + s + ((wc + 1u) >> 1);
  return (uint32_t)(((uint64_t)n * M) >> 32);
}

// The whole word {R, G, B, wc} (bytes 0 .. 3) after one sample (r, g, b); max_weight = 1 .. 255.
ODO_COLOUR_HD uint32_t colour_update(uint32_t word, uint32_t r, uint32_t g, uint32_t b, uint32_t max_weight) {
  const uint32_t wc = word >> 24;
  if (wc != 0u) {
    const uint32_t M = colour_reciprocal(wc + 1u);
    r = colour_channel(word & 0xffu, wc, r, M);
    g = colour_channel((word >> 8) & 0xffu, wc, g, M);
    b = colour_channel((word >> 16) & 0xffu, wc, b, M);
  }
  const uint32_t wn = wc + 1u < max_weight ? wc + 1u : max_weight;
  return r | (g << 8) | (b << 16) | (wn << 24);
}

// The colour of a point on the edge (a, b) at alpha in [0, 1]: {R, G, B, A} of include/odometry_hip.h. fp32, the product rounded,
// then the sum (the unit is built with -ffp-contract=off; the host harness with -ffp-contract=off as well).
ODO_COLOUR_HD uint32_t colour_interpolate(uint32_t ca, uint32_t cb, float alpha) {
  const bool has_a = (ca >> 24) != 0u, has_b = (cb >> 24) != 0u;
  if (!has_a && !has_b) return 0u;
  if (!has_b) return (ca & 0xffffffu) | 0xff000000u;
  if (!has_a) return (cb & 0xffffffu) | 0xff000000u;
  uint32_t out = 0xff000000u;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int ch = 0; ch < 3; ch++) {
    const float fa = (float)((ca >> (8 * ch)) & 0xffu), fb = (float)((cb >> (8 * ch)) & 0xffu);
    const float prod = alpha * (fb - fa);
    const float v = __builtin_rintf(fa + prod);
    out |= ((uint32_t)(int)v & 0xffu) << (8 * ch);
  }
  return out;
}

}  // namespace odo
