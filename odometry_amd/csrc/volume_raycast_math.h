// volume_raycast_math.h — the arithmetic of the TSDF volume's ray-cast (include/odometry_hip.h, odo_volume_raycast_dev / DESIGN.md
// section 9.7), host + device like volume_colour_math.h: the kernel of volume_raycast_kernels.hip and the g++ harness of
// tests/volume_raycast_math_harness.cpp compile these same lines. The sample, the interpolation, the gradient, the hit and the march
// over the samples are each written once, here.
//
// fp32, one rounding per operation: both builds use -ffp-contract=off, the device build correctly rounded divide and sqrt. Every
// comparison that decides validity is made on floats before any conversion to an integer, so NaN and inf fail it.
//
// Voxel memory is reached through a loader `load(word)` that returns the two 32-bit voxel words at `word` and `word + 1` (two
// x-adjacent voxels) as one 64-bit value, the first in the low half: the eight corners of a cell are four such pairs.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "volume_math.h"

#if defined(__HIPCC__)
#define ODO_RC_HD __host__ __device__ __forceinline__
#else
#define ODO_RC_HD static inline
#endif

namespace odo {

// What a ray needs of the grid and the camera: the dimensions, the camera centre e in voxel-index coordinates and the ray's direction
// g in voxel-index units per metre of depth along the optical axis.
struct RcRay {
  int nx, ny, nz;
  float ex, ey, ez;
  float gx, gy, gz;
};

// One cell evaluation: the corners c[dx + 2 dy + 4 dz] as floats, the fractions, the cell's first voxel and the smallest weight.
struct RcCell {
  float c[8];
  float frx, fry, frz;
  float px, py, pz;
  uint32_t word;    // voxel (bx, by, bz)
  uint32_t wmin;
};

ODO_RC_HD float rc_pixel(int x, float c, float f) { return ((float)x - c) / f; }
ODO_RC_HD float rc_dir(float G0, float G1, float G2, float dx, float dy) { return (G0 * dx + G1 * dy) + G2; }
ODO_RC_HD float rc_t(float t_min, int n, float step) { return t_min + (float)n * step; }
ODO_RC_HD bool rc_in(float b, int dim) { return b >= 0.0f && b <= (float)(dim - 2); }
ODO_RC_HD float rc_q(uint32_t v) { return (float)vox_q(v); }   // (the voxel word: volume_math.h)
ODO_RC_HD uint32_t rc_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// The sample at depth t: false = invalid (outside the cells of the grid, or a corner that was never observed). A sample that fails
// the first test loads nothing.
template <class Load2>
ODO_RC_HD bool rc_cell(const Load2& load, const RcRay& r, float t, RcCell* o) {
  const float px = r.ex + t * r.gx, py = r.ey + t * r.gy, pz = r.ez + t * r.gz;
  const float bx = __builtin_floorf(px), by = __builtin_floorf(py), bz = __builtin_floorf(pz);
  if (!(rc_in(bx, r.nx) && rc_in(by, r.ny) && rc_in(bz, r.nz))) return false;
  const uint32_t sy = (uint32_t)r.nx, sz = (uint32_t)r.nx * (uint32_t)r.ny;   // (a grid has at most 2^30 voxels: odo_volume_create)
  const uint32_t word = ((uint32_t)(int)bz * (uint32_t)r.ny + (uint32_t)(int)by) * sy + (uint32_t)(int)bx;
  const uint64_t p00 = load(word), p10 = load(word + sy), p01 = load(word + sz), p11 = load(word + sz + sy);
  const uint32_t v[8] = {(uint32_t)p00, (uint32_t)(p00 >> 32), (uint32_t)p10, (uint32_t)(p10 >> 32),
                         (uint32_t)p01, (uint32_t)(p01 >> 32), (uint32_t)p11, (uint32_t)(p11 >> 32)};
  uint32_t wmin = v[0] >> 16;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 1; i < 8; i++) wmin = rc_min(wmin, v[i] >> 16);
  if (wmin == 0u) return false;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) o->c[i] = rc_q(v[i]);
  o->frx = px - bx; o->fry = py - by; o->frz = pz - bz;
  o->px = px; o->py = py; o->pz = pz;
  o->word = word;
  o->wmin = wmin;
  return true;
}

ODO_RC_HD float rc_lerp(float a, float b, float fr) { return a + fr * (b - a); }

// F: along x, then y, then z.
ODO_RC_HD float rc_interp(const RcCell& o) {
  const float l00 = rc_lerp(o.c[0], o.c[1], o.frx), l10 = rc_lerp(o.c[2], o.c[3], o.frx);
  const float l01 = rc_lerp(o.c[4], o.c[5], o.frx), l11 = rc_lerp(o.c[6], o.c[7], o.frx);
  const float m0 = rc_lerp(l00, l10, o.fry), m1 = rc_lerp(l01, l11, o.fry);
  return rc_lerp(m0, m1, o.frz);
}

// The gradient of the interpolant in the cell, normalised; false = it has no length.
ODO_RC_HD bool rc_normal(const RcCell& o, float* nx, float* ny, float* nz) {
  const float d00 = o.c[1] - o.c[0], d10 = o.c[3] - o.c[2], d01 = o.c[5] - o.c[4], d11 = o.c[7] - o.c[6];
  const float gx0 = rc_lerp(d00, d10, o.fry), gx1 = rc_lerp(d01, d11, o.fry);
  const float gx = rc_lerp(gx0, gx1, o.frz);
  const float l00 = rc_lerp(o.c[0], o.c[1], o.frx), l10 = rc_lerp(o.c[2], o.c[3], o.frx);
  const float l01 = rc_lerp(o.c[4], o.c[5], o.frx), l11 = rc_lerp(o.c[6], o.c[7], o.frx);
  const float gy0 = l10 - l00, gy1 = l11 - l01;
  const float gy = rc_lerp(gy0, gy1, o.frz);
  const float m0 = rc_lerp(l00, l10, o.fry), m1 = rc_lerp(l01, l11, o.fry);
  const float gz = m1 - m0;
  const float len = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz);
  if (!(len > 0.0f)) return false;
  *nx = gx / len; *ny = gy / len; *nz = gz / len;
  return true;
}

// The crossing between the last positive sample and the first non-positive one.
ODO_RC_HD float rc_hit(float t_prev, float F_prev, float t, float F) { return t_prev + (F_prev / (F_prev - F)) * (t - t_prev); }

ODO_RC_HD uint16_t rc_raw(float z, float depth_scale) { return (uint16_t)__builtin_fminf(65535.0f, __builtin_rintf(z * depth_scale)); }

// The voxel nearest to the cell evaluation's point; it is one of the cell's corners (p in [b, b + 1) gives floorf(p + 0.5f) in
// {b, b + 1}).
ODO_RC_HD uint32_t rc_nearest(const RcCell& o, const RcRay& r) {
  const int ix = (int)__builtin_floorf(o.px + 0.5f), iy = (int)__builtin_floorf(o.py + 0.5f), iz = (int)__builtin_floorf(o.pz + 0.5f);
  return ((uint32_t)iz * (uint32_t)r.ny + (uint32_t)iy) * (uint32_t)r.nx + (uint32_t)ix;
}

// The colour of the cell evaluation's point as the trilinear average of the cell's coloured corners. cp: the
// colour words {R, G, B, wc} of the eight corners as four x-adjacent pairs, in the order of rc_cell's loads (the corner order of
// RcCell::c). A corner counts with m = 1 if its wc > 0, else 0; the coverage M and per channel the sum P are rc_interp itself over m
// and over m * (float)C with the cell's fractions, so eight coloured corners give M == 1.0f exactly. (R, G, B, 255) with
// (uint8)fminf(255.0f, rintf(P / M)) per channel if M > 0.0f, else four zeros.
ODO_RC_HD uint32_t rc_colour_interp(const RcCell& o, const uint64_t cp[4]) {
  const uint32_t cw[8] = {(uint32_t)cp[0], (uint32_t)(cp[0] >> 32), (uint32_t)cp[1], (uint32_t)(cp[1] >> 32),
                          (uint32_t)cp[2], (uint32_t)(cp[2] >> 32), (uint32_t)cp[3], (uint32_t)(cp[3] >> 32)};
  RcCell m = o, p = o;   // (the fractions)
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int d = 0; d < 8; d++) m.c[d] = (cw[d] >> 24) ? 1.0f : 0.0f;
  const float M = rc_interp(m);
  if (!(M > 0.0f)) return 0u;
  uint32_t out = 0xff000000u;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 3; k++) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int d = 0; d < 8; d++) p.c[d] = m.c[d] * (float)((cw[d] >> (8 * k)) & 0xffu);
    out |= (uint32_t)__builtin_fminf(255.0f, __builtin_rintf(rc_interp(p) / M)) << (8 * k);
  }
  return out;
}

// The march: the ray ends at its first valid sample with F <= 0 and is a hit iff the sample before exists, is valid and is positive.
// Lanes of a wave leave the loop one by one; the wave leaves it when the last has.
template <class Load2>
ODO_RC_HD bool rc_march(const Load2& load, const RcRay& r, float t_min, float step, int n_steps, float* z) {
  bool have_prev = false;
  float t_prev = 0.0f, F_prev = 0.0f;
  RcCell cell;
  for (int n = 0; n < n_steps; n++) {
    const float t = rc_t(t_min, n, step);
    if (!rc_cell(load, r, t, &cell)) { have_prev = false; continue; }
    const float F = rc_interp(cell);
    if (F <= 0.0f) {
      if (!have_prev) return false;
      *z = rc_hit(t_prev, F_prev, t, F);
      return true;
    }
    have_prev = true; t_prev = t; F_prev = F;
  }
  return false;
}

}  // namespace odo
