// stereo_depth_math.h — the rule of the dense stereo matcher (include/odometry_hip.h, odo_stereo_depth_create; DESIGN.md section
// 9.16), host + device like depth_filter_math.h: the kernels of stereo_depth_kernels.hip, the host object (stereo_depth_api.hip.h,
// the bounds it validates) and the g++ harness of tests/stereo_depth_math_harness.cpp compile these same lines. The census bit, the
// candidate walk, the uniqueness test, the sub-pixel step and the rounded division are each written once, here. Integers only but for
// the one fp32 division per pixel: nothing depends on the order in which a window is walked.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ODO_SD_HD __host__ __device__ __forceinline__
#else
#define ODO_SD_HD static inline
#endif

namespace odo {

constexpr int kSdCensusRx = 4;                      // the census window is 9 wide ...
constexpr int kSdCensusRy = 3;                      // ... by 7 high: 62 neighbours, one 64-bit word
constexpr int kSdMaxAgg = 3;                        // the aggregation radius A = 0 .. 3
constexpr int kSdMaxDisp = 255;                     // dmax <= 255: dr fits a byte
constexpr int kSdNoRight = 255;                     // dr of a right pixel without a candidate
constexpr int kSdNone = 1 << 30;                    // "no such cost": above every C <= 62 * 49 = 3038
constexpr int kSdMaxSize = 8192;                    // rows, cols
constexpr int kSdStatWords = 8;                     // interior, matched, rej_unique, rej_lr, rej_range, sum_q low, sum_q high, 0
static_assert(62 * (2 * kSdMaxAgg + 1) * (2 * kSdMaxAgg + 1) * 100 < kSdNone, "the uniqueness products fit int32");

// What happened to a pixel, in the order in which the reasons are counted (the first one only).
enum SdOutcome { kSdNotInterior = 0, kSdMatched = 1, kSdRejUnique = 2, kSdRejLr = 3, kSdRejRange = 4 };

struct SdRule {
  int dmin, dmax, A, uniq, lr_max, max_raw;
  float k;                                          // (float)(16 fx baseline depth_scale)
};

// The bounds odo_stereo_depth_create validates, in the order of the specification. 0: fine; otherwise the number of the bound that
// fails (1 size, 2 dmin, 3 dmax, 4 agg_radius, 5 uniqueness, 6 lr_max, 7 max_raw, 8 fx * baseline * depth_scale).
ODO_SD_HD int sd_check_params(int rows, int cols, int dmin, int dmax, int A, int uniq, int lr_max, int max_raw, double fx,
                              double baseline, double depth_scale) {
  if (rows < 1 || cols < 1 || rows > kSdMaxSize || cols > kSdMaxSize) return 1;
  if (dmin < 1) return 2;
  if (dmax > kSdMaxDisp || dmax < dmin + 2) return 3;
  if (A < 0 || A > kSdMaxAgg) return 4;
  if (uniq < 0 || uniq > 99) return 5;
  if (lr_max < -1) return 6;
  if (max_raw < 1 || max_raw > 65535) return 7;
  const float k = (float)(16.0 * fx * baseline * depth_scale);
  if (!(k > 0.0f) || !(k <= 3.0e38f)) return 8;
  return 0;
}
ODO_SD_HD float sd_k(double fx, double baseline, double depth_scale) { return (float)(16.0 * fx * baseline * depth_scale); }

// The census word of the pixel at img[0] (row stride `stride` floats); its whole window must be readable. Bit = neighbour < centre as
// fp32 (a NaN on either side: 0), the 62 neighbours row by row, the centre left out.
ODO_SD_HD uint64_t sd_census(const float* img, int stride) {
  const float c = img[0];
  uint32_t w[2] = {0u, 0u};
  int bit = 0;
#pragma unroll
  for (int dy = -kSdCensusRy; dy <= kSdCensusRy; dy++)
#pragma unroll
    for (int dx = -kSdCensusRx; dx <= kSdCensusRx; dx++) {
      if (dy == 0 && dx == 0) continue;
      w[bit / 31] |= (uint32_t)(img[dy * stride + dx] < c) << (bit % 31);
      bit++;
    }
  return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
}

ODO_SD_HD int sd_hamming(uint64_t a, uint64_t b) { return __builtin_popcountll(a ^ b); }

// The interior of the left image and the admissible candidates of a left pixel.
ODO_SD_HD bool sd_interior_row(int y, int rows, int A) { return y >= A + kSdCensusRy && y < rows - A - kSdCensusRy; }
ODO_SD_HD bool sd_interior_col(int x, int cols, int A) { return x >= A + kSdCensusRx && x < cols - A - kSdCensusRx; }
// The largest admissible candidate of left pixel x (below dmin: none).
ODO_SD_HD int sd_left_last(int x, int dmax, int A) { const int m = x - A - kSdCensusRx; return m < dmax ? m : dmax; }
// The largest admissible candidate of right pixel x (left pixel x + d must be interior; x >= A + 4 is the caller's test).
ODO_SD_HD int sd_right_last(int x, int cols, int dmax, int A) { const int m = cols - A - kSdCensusRx - 1 - x; return m < dmax ? m : dmax; }

// The walk over a pixel's candidates in ascending order, one step per candidate d with its cost c: afterwards c0 / dl are the smallest
// d of minimal cost, cm / cp the costs at dl - 1 / dl + 1 (-1: not walked), c2 the minimal cost over the walked d with |d - dl| > 1
// (kSdNone: there is none). m2 = the minimum over the candidates up to d - 2: what c2 becomes when d takes the lead.
struct SdWalk { int c0, dl, cm, cp, c2, last, m2; };
ODO_SD_HD void sd_walk_init(SdWalk* w) {
  w->c0 = kSdNone; w->dl = -2; w->cm = -1; w->cp = -1; w->c2 = kSdNone; w->last = -1; w->m2 = kSdNone;
}
ODO_SD_HD void sd_walk_step(SdWalk* w, int d, int c) {
  const int m1 = w->c0;
  if (c < w->c0) { w->c2 = w->m2; w->c0 = c; w->dl = d; w->cm = w->last; w->cp = -1; }
  else if (d == w->dl + 1) w->cp = c;
  else w->c2 = c < w->c2 ? c : w->c2;
  w->m2 = m1;
  w->last = c;
}

// Uniqueness: true = the winner stands.
ODO_SD_HD bool sd_unique(int c0, int c2, int uniq) { return c2 != kSdNone && c2 * (100 - uniq) > c0 * 100; }

// The sub-pixel step f in sixteenths, -8 .. 8; cm or cp < 0: a neighbour that was not walked (the winner at dmin, at dmax, or beside
// an inadmissible candidate).
ODO_SD_HD int sd_subpixel(int cm, int c0, int cp) {
  if (cm < 0 || cp < 0) return 0;
  const int den = cm - 2 * c0 + cp, num = cm - cp;
  if (den <= 0) return 0;
  const int a = num < 0 ? -num : num;
  const int f = (16 * a + den) / (2 * den);
  return num < 0 ? -f : f;
}

// raw = rintf(k / q): one correctly rounded fp32 division, then round half to even.
ODO_SD_HD float sd_raw(float k, int q) { return rintf(k / (float)q); }

// The end of a left pixel's rule, after its walk: `dr` is read only if the winner passes uniqueness (dr_row[x - dl], the right
// winners of the pixel's row). Returns the outcome; *depth and *q are what the frames get.
ODO_SD_HD int sd_finish(const SdWalk& w, const SdRule& r, const uint8_t* dr_row, int x, uint16_t* depth, uint16_t* q) {
  *depth = 0; *q = 0;
  if (w.c0 == kSdNone) return kSdNotInterior;
  if (!sd_unique(w.c0, w.c2, r.uniq)) return kSdRejUnique;
  if (r.lr_max >= 0) {
    const int e = (int)dr_row[x - w.dl] - w.dl;
    if ((e < 0 ? -e : e) > r.lr_max) return kSdRejLr;
  }
  const int qq = 16 * w.dl + sd_subpixel(w.cm, w.c0, w.cp);
  const float raw = sd_raw(r.k, qq);
  if (raw > (float)r.max_raw) return kSdRejRange;
  *depth = (uint16_t)raw;
  *q = (uint16_t)qq;
  return kSdMatched;
}

// ---- the reference walk over dense rows x cols planes of census words (the kernels walk tiles out of LDS instead) -------------------
// C(x, y, d) of the left pixel (x, y): every tap must have both descriptors.
ODO_SD_HD int sd_cost(const uint64_t* cl, const uint64_t* cr, int cols, int y, int x, int d, int A) {
  int c = 0;
  for (int j = -A; j <= A; j++)
    for (int i = -A; i <= A; i++) c += sd_hamming(cl[(long)(y + j) * cols + x + i], cr[(long)(y + j) * cols + x + i - d]);
  return c;
}

// dr of the right pixel (x, y): the smallest admissible d of minimal CR(x, y, d) = C(x + d, y, d); kSdNoRight where there is none.
ODO_SD_HD uint8_t sd_right_pixel(const uint64_t* cl, const uint64_t* cr, int rows, int cols, int y, int x, const SdRule& r) {
  if (!sd_interior_row(y, rows, r.A) || x < r.A + kSdCensusRx) return (uint8_t)kSdNoRight;
  const int last = sd_right_last(x, cols, r.dmax, r.A);
  SdWalk w;
  sd_walk_init(&w);
  for (int d = r.dmin; d <= last; d++) sd_walk_step(&w, d, sd_cost(cl, cr, cols, y, x + d, d, r.A));
  return w.c0 == kSdNone ? (uint8_t)kSdNoRight : (uint8_t)w.dl;
}

// The whole rule for the left pixel (x, y); dr is the rows x cols plane of right winners (not read when lr_max < 0).
ODO_SD_HD int sd_left_pixel(const uint64_t* cl, const uint64_t* cr, const uint8_t* dr, int rows, int cols, int y, int x,
                            const SdRule& r, uint16_t* depth, uint16_t* q) {
  SdWalk w;
  sd_walk_init(&w);
  if (sd_interior_row(y, rows, r.A) && sd_interior_col(x, cols, r.A)) {
    const int last = sd_left_last(x, r.dmax, r.A);
    for (int d = r.dmin; d <= last; d++) sd_walk_step(&w, d, sd_cost(cl, cr, cols, y, x, d, r.A));
  }
  return sd_finish(w, r, dr + (long)y * cols, x, depth, q);
}

}  // namespace odo
