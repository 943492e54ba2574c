// stereo_sgm_math.h — the rule of the dense stereo matcher's semi-global mode (include/odometry_hip.h, odo_stereo_depth_enable_sgm;
// DESIGN.md section 9.18), host + device over stereo_depth_math.h: the kernels of stereo_sgm_kernels.hip, the host object
// (stereo_depth_api.hip.h, the bounds it validates) and the g++ harness of tests/stereo_sgm_math_harness.cpp compile these same lines.
// The bounds, the active rectangle, the eight directions, the lines a direction is walked along and the one step of a path cost are
// each written once, here; the selection over the aggregate S is stereo_depth_math.h's walk, untouched. Integers only: S is a sum of
// integers and does not depend on the order of the paths.
#pragma once
#include "stereo_depth_math.h"

namespace odo {

constexpr int kSgmNone = 65535;                     // an entry of the C or S volume that is not admissible
constexpr int kSgmMaxSum = 65534;                   // paths * (Cmax + P2) at the most: an aggregate fits uint16 below kSgmNone
constexpr int kSgmMaxVolume = 1 << 30;              // rows * cols * D at the most
constexpr int kSgmMaxPaths = 8;
constexpr int kSgmInf = 1 << 28;                    // a path cost that is not there: kSgmInf - M + P1 > P2 whatever M <= 65534 is

// The bounds odo_stereo_depth_enable_sgm validates, in the order of the specification. 0: fine; otherwise the number of the bound that
// fails (1 the penalties 1 <= P1 <= P2, 2 paths, 3 the aggregate's range, 4 the volume's size).
ODO_SD_HD int sgm_check_params(int rows, int cols, int dmin, int dmax, int A, int p1, int p2, int paths) {
  if (p1 < 1 || p1 > p2) return 1;
  if (paths != 4 && paths != 8) return 2;
  const long long n = 2 * A + 1;
  if ((long long)paths * (62 * n * n + (long long)p2) > kSgmMaxSum) return 3;
  if ((long long)rows * cols * (dmax - dmin + 1) > kSgmMaxVolume) return 4;
  return 0;
}

// The active pixels: x0 <= x < x1 and y0 <= y < y1, the interior pixels with at least one admissible candidate. Empty when x1 <= x0 or
// y1 <= y0.
struct SgmRect { int x0, x1, y0, y1; };
ODO_SD_HD SgmRect sgm_rect(int rows, int cols, int dmin, int A) {
  SgmRect r;
  r.x0 = A + kSdCensusRx + dmin; r.x1 = cols - A - kSdCensusRx; r.y0 = A + kSdCensusRy; r.y1 = rows - A - kSdCensusRy;
  return r;
}
ODO_SD_HD bool sgm_empty(const SgmRect& r) { return r.x1 <= r.x0 || r.y1 <= r.y0; }
ODO_SD_HD bool sgm_active(const SgmRect& r, int x, int y) { return x >= r.x0 && x < r.x1 && y >= r.y0 && y < r.y1; }
// The number of admissible candidates of an active pixel in column x: dmin .. min(dmax, x - A - 4), at least one.
ODO_SD_HD int sgm_count(int x, int dmin, int dmax, int A) { return sd_left_last(x, dmax, A) - dmin + 1; }

// Direction r of `paths`: the first four are the 4-path set.
ODO_SD_HD void sgm_direction(int r, int* dx, int* dy) {
  const int tx[kSgmMaxPaths] = {1, -1, 0, 0, 1, -1, 1, -1};
  const int ty[kSgmMaxPaths] = {0, 0, 1, -1, 1, -1, -1, 1};
  *dx = tx[r]; *dy = ty[r];
}

// The lines of direction (dx, dy): every active pixel lies on exactly one. A line enters the rectangle through the side it moves away
// from; a diagonal enters through two sides, the row side first (lines 0 .. width - 1), then the column side without its corner.
ODO_SD_HD int sgm_lines(const SgmRect& r, int dx, int dy) {
  if (sgm_empty(r)) return 0;
  const int w = r.x1 - r.x0, h = r.y1 - r.y0;
  return dx != 0 && dy != 0 ? w + h - 1 : dx != 0 ? h : w;
}
// Line i starts at (*xs, *ys) and has *len pixels, each (dx, dy) from the one before.
ODO_SD_HD void sgm_line(const SgmRect& r, int dx, int dy, int i, int* xs, int* ys, int* len) {
  const int w = r.x1 - r.x0, h = r.y1 - r.y0;
  const int xin = dx > 0 ? r.x0 : r.x1 - 1, yin = dy > 0 ? r.y0 : r.y1 - 1;    // the entry column / row
  int x, y;
  if (dy == 0) { x = xin; y = r.y0 + i; }
  else if (dx == 0 || i < w) { x = r.x0 + i; y = yin; }
  else { x = xin; y = dy > 0 ? r.y0 + (i - w + 1) : r.y1 - 1 - (i - w + 1); }
  const int nx = dx > 0 ? r.x1 - x : dx < 0 ? x - r.x0 + 1 : w + h;
  const int ny = dy > 0 ? r.y1 - y : dy < 0 ? y - r.y0 + 1 : w + h;
  *xs = x; *ys = y; *len = nx < ny ? nx : ny;
}

// One candidate of one step of a path: c = C(p, d); l0, lm, lp = L_r(q, d), L_r(q, d - 1), L_r(q, d + 1), kSgmInf where the
// candidate is not admissible at q; m = the minimum of L_r(q, .). 0 <= the result - c <= P2.
ODO_SD_HD int sgm_step(int c, int l0, int lm, int lp, int m, int p1, int p2) {
  int a = p2, t = l0 - m;
  a = t < a ? t : a;
  t = lm - m + p1;
  a = t < a ? t : a;
  t = lp - m + p1;
  a = t < a ? t : a;
  return c + a;
}

// ---- the reference walk over dense [rows][cols][D] volumes (the kernels walk a line per wave instead) ------------------------------
// C of every pixel and candidate from the census planes, kSgmNone where the candidate is not admissible.
static inline void sgm_cost_volume(const uint64_t* cl, const uint64_t* cr, int rows, int cols, const SdRule& r, uint16_t* C) {
  const int D = r.dmax - r.dmin + 1;
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) {
      const bool in = sd_interior_row(y, rows, r.A) && sd_interior_col(x, cols, r.A);
      const int last = in ? sd_left_last(x, r.dmax, r.A) : r.dmin - 1;
      for (int d = r.dmin; d <= r.dmax; d++)
        C[((long)y * cols + x) * D + d - r.dmin] = (uint16_t)(d <= last ? sd_cost(cl, cr, cols, y, x, d, r.A) : kSgmNone);
    }
}

// S from C: kSgmNone where C is, the sum of the paths' costs elsewhere, direction by direction and line by line.
static inline void sgm_aggregate(const uint16_t* C, int rows, int cols, const SdRule& r, int p1, int p2, int paths, uint16_t* S) {
  const int D = r.dmax - r.dmin + 1;
  const SgmRect rc = sgm_rect(rows, cols, r.dmin, r.A);
  for (long i = 0; i < (long)rows * cols * D; i++) S[i] = (uint16_t)(C[i] == kSgmNone ? kSgmNone : 0);
  int prev[kSdMaxDisp + 2], cur[kSdMaxDisp + 2];                  // one more either side: L_r(q, d -+ 1) of the first and the last d
  for (int k = 0; k < paths; k++) {
    int dx, dy;
    sgm_direction(k, &dx, &dy);
    for (int line = 0; line < sgm_lines(rc, dx, dy); line++) {
      int x, y, len;
      sgm_line(rc, dx, dy, line, &x, &y, &len);
      for (int i = 0; i <= D + 1; i++) prev[i] = kSgmInf;
      for (int step = 0; step < len; step++, x += dx, y += dy) {
        const int n = sgm_count(x, r.dmin, r.dmax, r.A);
        const long base = ((long)y * cols + x) * D;
        int m = kSgmInf;
        for (int i = 1; i <= D; i++) m = prev[i] < m ? prev[i] : m;
        for (int i = 1; i <= n; i++) {
          const int c = C[base + i - 1];
          cur[i] = step == 0 ? c : sgm_step(c, prev[i], prev[i - 1], prev[i + 1], m, p1, p2);
          S[base + i - 1] = (uint16_t)(S[base + i - 1] + cur[i]);
        }
        for (int i = 0; i <= D + 1; i++) prev[i] = i >= 1 && i <= n ? cur[i] : kSgmInf;
      }
    }
  }
}

// dr of the right pixel (x, y) over the aggregate: the smallest admissible d of minimal S(x + d, y, d); kSdNoRight where there is none.
static inline uint8_t sgm_right_pixel(const uint16_t* S, int rows, int cols, int y, int x, const SdRule& r) {
  if (!sd_interior_row(y, rows, r.A) || x < r.A + kSdCensusRx) return (uint8_t)kSdNoRight;
  const int D = r.dmax - r.dmin + 1, last = sd_right_last(x, cols, r.dmax, r.A);
  SdWalk w;
  sd_walk_init(&w);
  for (int d = r.dmin; d <= last; d++) sd_walk_step(&w, d, S[((long)y * cols + x + d) * D + d - r.dmin]);
  return w.c0 == kSdNone ? (uint8_t)kSdNoRight : (uint8_t)w.dl;
}

// The whole selection for the left pixel (x, y) over the aggregate; dr is the rows x cols plane of right winners.
static inline int sgm_left_pixel(const uint16_t* S, const uint8_t* dr, int rows, int cols, int y, int x, const SdRule& r,
                                 uint16_t* depth, uint16_t* q) {
  SdWalk w;
  sd_walk_init(&w);
  if (sd_interior_row(y, rows, r.A) && sd_interior_col(x, cols, r.A)) {
    const int D = r.dmax - r.dmin + 1, last = sd_left_last(x, r.dmax, r.A);
    for (int d = r.dmin; d <= last; d++) sd_walk_step(&w, d, S[((long)y * cols + x) * D + d - r.dmin]);
  }
  return sd_finish(w, r, dr + (long)y * cols, x, depth, q);
}

}  // namespace odo
