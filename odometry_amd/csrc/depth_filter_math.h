// depth_filter_math.h — the rule of the bilateral depth filter (include/odometry_hip.h, odo_depth_filter_create; DESIGN.md section
// 9.12), host + device like volume_math.h: the kernel of depth_filter_kernels.hip, the host object (depth_filter_api.hip.h, the bounds
// it validates) and the g++ harness of tests/depth_filter_harness.cpp compile these same lines. The tap rule and the rounded division
// are each written once, here. Integers only: the sums do not depend on the order in which a window is walked.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ODO_DF_HD __host__ __device__ __forceinline__
#else
#define ODO_DF_HD static inline
#endif

namespace odo {

constexpr int kDfMaxRadius = 4;                                           // the window is (2R + 1)^2, R = 1 .. 4
constexpr int kDfMaxTaps = (2 * kDfMaxRadius + 1) * (2 * kDfMaxRadius + 1);   // 81: odo_depth_filter_params::ws
constexpr int kDfWsMax = 16;                                              // every spatial weight 0 .. 16, the centre's >= 1
constexpr int kDfRange = 256;                                             // wr[k], k = |delta| >> s; a tap with k >= 256 does not count
constexpr int kDfShiftMax = 4;                                            // shift[c >> 8] = 0 .. 4
// The sums fit int32: a counted tap has |delta| < 256 << 4, its weight is at most 16 * 255, and a window has at most 81 taps but its
// centre contributes delta = 0: |S| <= 4080 * 4095 * 80 = 1 336 608 000, and |S| + W / 2 <= that + 81 * 4080 / 2 < 2^31.
static_assert(4080LL * 4095 * 80 + 81LL * 4080 / 2 < (1LL << 31), "S + W / 2 fits int32");

// The range table as the tap rule reads it: wr's 256 entries and a 257th that is 0, the weight of a tap that does not count.
constexpr int kDfRangePadded = kDfRange + 1;
ODO_DF_HD void df_pad_range(const uint8_t* wr, uint8_t* wr0) {
  for (int i = 0; i < kDfRange; i++) wr0[i] = wr[i];
  wr0[kDfRange] = 0;
}

// One tap t of the window around the centre c != 0 with s = shift[c >> 8]: added to S and W iff it counts. `ws` is the tap's spatial
// weight, wr0 the padded range table. Branch-free: a tap that does not count (no reading, or k >= 256) reads the table's zero. The
// choice is made on the INDEX, in front of the lookup: with a select behind it (`counts ? ws * wr[k] : 0`) the device compiler puts a
// branch round every tap's load and waits for each in turn (R = 4 at 480 x 640: 24 us for a launch).
ODO_DF_HD void df_tap(int t, int c, int s, int ws, const uint8_t* wr0, int* S, int* W) {
  const int d = t - c;
  const int a = d < 0 ? -d : d;
  const int k = a >> s;
  const int w = ws * (int)wr0[((t != 0) & (k < kDfRange)) ? k : kDfRange];
  *S += w * d;
  *W += w;
}

// q = S / W rounded to nearest, ties away from zero, with C's truncating division; W >= 1.
ODO_DF_HD int df_round_div(int S, int W) {
  const uint32_t w = (uint32_t)W, h = w >> 1;
  return S >= 0 ? (int)(((uint32_t)S + h) / w) : -(int)(((uint32_t)(-S) + h) / w);
}

// The output of a pixel from its sums: c == 0 stays 0 (nothing is filled in).
ODO_DF_HD uint16_t df_output(int c, int S, int W) {
  return c == 0 ? (uint16_t)0 : (uint16_t)(c + df_round_div(S, W < 1 ? 1 : W));
}

// The whole rule for one pixel of a dense rows x cols frame: the reference walk (the kernel walks its window out of LDS instead).
// wr0: the padded range table (df_pad_range).
ODO_DF_HD uint16_t df_pixel(const uint16_t* raw, int rows, int cols, int y, int x, int R, const uint8_t* ws, const uint8_t* wr0,
                            const uint8_t* shift) {
  const int c = raw[(long)y * cols + x];
  if (c == 0) return 0;
  const int s = shift[c >> 8], n = 2 * R + 1;
  int S = 0, W = 0;
  for (int dy = -R; dy <= R; dy++) {
    for (int dx = -R; dx <= R; dx++) {
      const int yy = y + dy, xx = x + dx;
      if (yy < 0 || yy >= rows || xx < 0 || xx >= cols) continue;
      df_tap(raw[(long)yy * cols + xx], c, s, ws[(dy + R) * n + (dx + R)], wr0, &S, &W);
    }
  }
  return df_output(c, S, W);
}

// The bounds odo_depth_filter_create validates, in the order of the specification. 0: fine; otherwise the number of the bound that
// fails (1 radius, 2 a spatial weight above 16, 3 the centre weight 0, 4 wr[0] == 0, 5 a shift above 4).
ODO_DF_HD int df_check_tables(int R, const uint8_t* ws, const uint8_t* wr, const uint8_t* shift) {
  if (R < 1 || R > kDfMaxRadius) return 1;
  const int n = 2 * R + 1;
  for (int i = 0; i < n * n; i++) if (ws[i] > kDfWsMax) return 2;
  if (ws[R * n + R] < 1) return 3;
  if (wr[0] < 1) return 4;
  for (int i = 0; i < kDfRange; i++) if (shift[i] > kDfShiftMax) return 5;
  return 0;
}

}  // namespace odo
