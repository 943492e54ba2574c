// camera_math.h — the per-pixel arithmetic of the camera model, host + device like volume_raycast_math.h:
// the kernels of camera.hip.h and the g++ harness of tests/camera_math_harness.cpp compile these same lines. The map entry, the
// remapped pixel and the host-side coefficients ((P[:, :3] * R)^-1 by cofactors) are each written once, here.
//
//   map:   [x y w]^T = (P[:, :3] * R)^-1 * [u v 1]^T; x' = x/w, y' = y/w; r2 = x'^2 + y'^2;
//          kr = 1 + (k2*r2 + k1)*r2; xd = x'*kr + p1*2x'y' + p2*(r2 + 2x'^2); yd = y'*kr + p1*(r2 + 2y'^2) + p2*2x'y';
//          map_x = fx*xd + cx, map_y = fy*yd + cy   — fp64, stored as fp32 (CV_32FC1 maps).
//   remap: INTER_LINEAR with OpenCV's 5-bit fixed-point coordinates (INTER_BITS = 5): sx = rint(map_x * 32),
//          ix = sx >> 5, ax = sx & 31, weights (1 - ay/32)(1 - ax/32) ... as fp32 products, value =
//          ((S00*w00 + S01*w01) + S10*w10) + S11*w11; BORDER_CONSTANT: a tap outside the source reads border_value.
//
// Coordinates that do not fit. If, for either coordinate c of a pixel, !(fabsf(c * 32.0f) < 2147483648.0f) — NaN, +-inf, or a
// product that a 32-bit integer cannot hold — the pixel is border_value itself: stored as it is, no weights applied, no source
// element read. The test is made on floats before any conversion, so no build of these lines converts a value that an int cannot
// represent (undefined in C; x86 gives INT_MIN, gfx950's v_cvt_i32_f32 saturates and gives 0 for NaN).
//
// fp32 / fp64 with one rounding per operation: both builds use -ffp-contract=off. Source memory is reached through a loader
// `load(index)` that returns element `index` of the dense source (row * scols + column); only taps inside the source are loaded.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifndef ODO_HD
#if defined(__HIPCC__)
#define ODO_HD __host__ __device__ __forceinline__
#else
#define ODO_HD static inline
#endif
#endif

namespace odo {

struct CamCoef {     // everything the map kernel needs, fp64
  double iR[9];      // (P[:, :3] * R)^-1, row-major
  double fx, fy, cx, cy;  // raw camera matrix (skew is ignored, as cv::initUndistortRectifyMap does)
  double k1, k2, p1, p2;  // radial k1, k2 and tangential p1, p2 (the reference's "r1", "r2")
};

// One map entry.
ODO_HD void undistort_map_entry(const CamCoef& c, int u, int v, float* mx, float* my) {
  const double du = (double)u, dv = (double)v;
  const double _x = (c.iR[0] * du + c.iR[1] * dv) + c.iR[2];
  const double _y = (c.iR[3] * du + c.iR[4] * dv) + c.iR[5];
  const double _w = (c.iR[6] * du + c.iR[7] * dv) + c.iR[8];
  const double w = 1.0 / _w;
  const double x = _x * w, y = _y * w;
  const double x2 = x * x, y2 = y * y;
  const double r2 = x2 + y2, _2xy = (2.0 * x) * y;
  const double kr = 1.0 + (c.k2 * r2 + c.k1) * r2;
  const double xd = (x * kr + c.p1 * _2xy) + c.p2 * (r2 + 2.0 * x2);
  const double yd = (y * kr + c.p1 * (r2 + 2.0 * y2)) + c.p2 * _2xy;
  *mx = (float)(c.fx * xd + c.cx);
  *my = (float)(c.fy * yd + c.cy);
}

// Whether rint(c * 32) is a value of int: false for NaN, +-inf and |c * 32| >= 2^31.
ODO_HD bool remap_coord_fits(float c32) { return fabsf(c32) < 2147483648.0f; }

// One remapped pixel of a srows x scols source at map entry (mx, my).
template <class Load>
ODO_HD float remap_bilinear_pixel(const Load& load, int srows, int scols, float mx, float my, float border_value) {
  const float fx = mx * 32.0f, fy = my * 32.0f;
  if (!(remap_coord_fits(fx) && remap_coord_fits(fy))) return border_value;
  const int sx = (int)rintf(fx), sy = (int)rintf(fy);
  const int ix = sx >> 5, iy = sy >> 5;
  const float ax = (float)(sx & 31) * (1.0f / 32.0f), ay = (float)(sy & 31) * (1.0f / 32.0f);
  const float w00 = (1.0f - ay) * (1.0f - ax), w01 = (1.0f - ay) * ax, w10 = ay * (1.0f - ax), w11 = ay * ax;
  const bool x0 = (unsigned)ix < (unsigned)scols, x1 = (unsigned)(ix + 1) < (unsigned)scols;
  const bool y0 = (unsigned)iy < (unsigned)srows, y1 = (unsigned)(iy + 1) < (unsigned)srows;
  const float s00 = (x0 && y0) ? load((size_t)iy * scols + ix) : border_value;
  const float s01 = (x1 && y0) ? load((size_t)iy * scols + ix + 1) : border_value;
  const float s10 = (x0 && y1) ? load((size_t)(iy + 1) * scols + ix) : border_value;
  const float s11 = (x1 && y1) ? load((size_t)(iy + 1) * scols + ix + 1) : border_value;
  return ((s00 * w00 + s01 * w01) + s10 * w10) + s11 * w11;
}

// 3x3 inverse by cofactors in fp64, fixed operation order (part of the arithmetic contract: the CPU checker repeats it).
static inline bool cam_inv3(const double m[9], double out[9]) {
  const double c00 = m[4] * m[8] - m[5] * m[7];
  const double c01 = m[5] * m[6] - m[3] * m[8];
  const double c02 = m[3] * m[7] - m[4] * m[6];
  const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
  if (!(fabs(det) > 0.0)) return false;
  const double id = 1.0 / det;
  out[0] = c00 * id; out[1] = (m[2] * m[7] - m[1] * m[8]) * id; out[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  out[3] = c01 * id; out[4] = (m[0] * m[8] - m[2] * m[6]) * id; out[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  out[6] = c02 * id; out[7] = (m[1] * m[6] - m[0] * m[7]) * id; out[8] = (m[0] * m[4] - m[1] * m[3]) * id;
  return true;
}

// The map kernel's coefficients from the raw calibration {fx, fy, f_theta, cx, cy}, the distortion {k1, k2, p1, p2}, the 3x3
// rectifying rotation and the 3x4 projection (row-major): false when P[:, :3] * R is singular.
static inline bool cam_coef(const double raw[5], const double dist[4], const double R[9], const double P[12], CamCoef* k) {
  double PR[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      PR[i * 3 + j] = (P[i * 4 + 0] * R[0 * 3 + j] + P[i * 4 + 1] * R[1 * 3 + j]) + P[i * 4 + 2] * R[2 * 3 + j];
  if (!cam_inv3(PR, k->iR)) return false;
  k->fx = raw[0]; k->fy = raw[1]; k->cx = raw[3]; k->cy = raw[4];
  k->k1 = dist[0]; k->k2 = dist[1]; k->p1 = dist[2]; k->p2 = dist[3];
  return true;
}

}  // namespace odo
