// volume_icp_photo_math.h — the photometric row of the TSDF volume's frame-to-model alignment (include/odometry_hip.h,
// odo_volume_icp_photo_align_dev / DESIGN.md section 9.10), host + device over volume_icp_math.h: the kernels of
// volume_icp_photo_kernels.hip and the g++ harness of tests/volume_icp_photo_math_harness.cpp compile these same lines. The
// geometric row of a pixel stays icp_row, called as it is; this header adds the row that compares the sensor's grey value with
// the grey of the model's colour frame at the pixel's projection, and the 31 sums that both kinds of row share.
//
// fp32, one rounding per operation (-ffp-contract=off, correctly rounded divide and sqrt on the device). Every comparison that
// decides validity is made on floats before any conversion to an integer, so NaN and inf fail it.
#pragma once
#include "volume_icp_math.h"

namespace odo {

constexpr int kIcpPhotoAcc = 31;   // accumulate_row's 28 over both kinds of row, geometric pairs, photometric pairs, photometric cost

struct IcpPhotoView {
  float weight;        // lambda: metres per grey level
  float huber_delta;   // grey levels; 0: no robust weight
};

// The grey value of one word of the model's colour frame (bytes R, G, B, A in memory order): the front end's integer rule.
ODO_HD float icp_photo_grey(uint32_t c) {
  const uint32_t R = c & 255u, G = (c >> 8) & 255u, B = (c >> 16) & 255u;
  return (float)((R * 4899u + G * 9617u + B * 1868u + 8192u) >> 14);
}

// The photometric row of sensor pixel (x, y). grey: rows x cols float, the sensor's grey frame; rgba_m: rows x cols words of the
// model's colour frame; the rest as icp_row. false = no pair (J, res, w untouched). The model frames are read only at pixels that
// have passed the bounds test as floats.
ODO_HD bool icp_photo_row(const IcpView& a, const IcpPhotoView& ph, const float* C, const uint16_t* raw, const float* grey,
                          const float* depth_m, const uint32_t* rgba_m, int x, int y, float J[6], float* res, float* w) {
  const unsigned r = raw[(size_t)y * a.cols + x];
  const float gs = grey[(size_t)y * a.cols + x];   // (read beside raw, not behind the model's frames: it depends on nothing)
  if (r == 0u) return false;
  const float D = (float)r / a.depth_scale;
  if (D > a.max_depth) return false;
  const float dx = icp_pixel(x, a.cx, a.f), dy = icp_pixel(y, a.cy, a.f);
  const float px = dx * D, py = dy * D, pz = D;
  const float pmx = ((C[0] * px + C[4] * py) + C[8] * pz) + C[12];
  const float pmy = ((C[1] * px + C[5] * py) + C[9] * pz) + C[13];
  const float pmz = ((C[2] * px + C[6] * py) + C[10] * pz) + C[14];
  if (!(pmz > 0.0f)) return false;
  const float u = a.f * (pmx / pmz) + a.cx, v = a.f * (pmy / pmz) + a.cy;
  const float x0 = floorf(u), y0 = floorf(v);
  if (!(x0 >= 0.0f && x0 < (float)(a.cols - 1) && y0 >= 0.0f && y0 < (float)(a.rows - 1))) return false;
  const float xi = floorf(u + 0.5f), yi = floorf(v + 0.5f);   // x0 or x0 + 1: in range
  const size_t o = (size_t)(int)y0 * a.cols + (size_t)(int)x0;
  const float zm = depth_m[(size_t)(int)yi * a.cols + (size_t)(int)xi];   // (the five reads of the model together: none waits for another)
  const uint32_t c00 = rgba_m[o], c01 = rgba_m[o + 1], c10 = rgba_m[o + a.cols], c11 = rgba_m[o + a.cols + 1];
  if (!(zm > 0.0f && fabsf(pmz - zm) <= a.dist_max)) return false;
  if ((c00 >> 24) == 0u || (c01 >> 24) == 0u || (c10 >> 24) == 0u || (c11 >> 24) == 0u) return false;
  const float g00 = icp_photo_grey(c00), g01 = icp_photo_grey(c01), g10 = icp_photo_grey(c10), g11 = icp_photo_grey(c11);
  const float ax = u - x0, ay = v - y0;
  const float dt = g01 - g00, db = g11 - g10;
  const float top = g00 + ax * dt, bot = g10 + ax * db;
  const float val = top + ay * (bot - top);
  const float gx = dt + ay * (db - dt);
  const float gy = bot - top;
  const float e = ph.weight * (val - gs);
  const float s = (ph.weight * a.f) / pmz;
  const float jx = s * gx, jy = s * gy;
  const float jz = -((jx * pmx + jy * pmy) / pmz);
  J[0] = jx; J[1] = jy; J[2] = jz;
  J[3] = pmy * jz - pmz * jy;
  J[4] = pmz * jx - pmx * jz;
  J[5] = pmx * jy - pmy * jx;
  *res = e;
  *w = (ph.huber_delta > 0.0f) ? robust_weight(e, 1, ph.weight * ph.huber_delta, 1.0f) : 1.0f;
  return true;
}

// acc += one row {J0 .. J5, res, w} of either kind: the 28 terms as icp_term forms them (exact fp64 products, so adding one is what
// accumulate_row's fma does), then the row's own count and, for a photometric row, its share of the cost.
ODO_HD void icp_photo_accumulate(double acc[kIcpPhotoAcc], const float row[8], bool photometric) {
  for (int q = 0; q < ODO_NACC - 1; q++) {
    int ia, ib;
    icp_term_operands(q, &ia, &ib);
    acc[q] += icp_term(row, ia, ib);
  }
  if (photometric) {
    acc[29] += 1.0;
    acc[30] += icp_term(row, 6, 6);
  } else {
    acc[28] += 1.0;
  }
}

}  // namespace odo
