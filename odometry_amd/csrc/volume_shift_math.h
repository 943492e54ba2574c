// volume_shift_math.h — the rules of the moving TSDF volume (include/odometry_hip.h, odo_volume_shift / odo_volume_follow; DESIGN.md
// section 9.9), host + device like volume_math.h: the kernels of volume_shift_kernels.hip, the host object (volume_shift_api.hip.h)
// and the g++ harness of tests/volume_shift_harness.cpp compile these same lines. Where a shifted voxel comes from, which voxels a
// shift destroys, how far the window may travel and the shift that follows a pose are each written once, here. The window's origin
// is host_fp.h's (hostfp::window_origin).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ODO_SHIFT_HD __host__ __device__ __forceinline__
#else
#define ODO_SHIFT_HD static inline
#endif

namespace odo {

constexpr int kShiftMaxOff = 1 << 24;   // |off_c| stays at or below it: (float)off_c is exact

// A shift by d voxels moves the origin by +d: new voxel i on an axis of n voxels is old voxel i + d. False: that lies outside the old
// grid and the new voxel is 0. (64-bit: every int d is legal.)
ODO_SHIFT_HD bool shift_source(int i, int d, int n, int* src) {
  const long long s = (long long)i + d;
  *src = (int)s;   // (only read when inside: then it fits)
  return s >= 0 && s < n;
}

// Old voxel i leaves under d iff no new voxel takes its value: i - d is outside [0, n).
ODO_SHIFT_HD bool shift_leaves(int i, int d, int n) {
  const long long t = (long long)i - d;
  return t < 0 || t >= n;
}

// The cumulative shift off + d on one axis, refused (false) beyond +-kShiftMaxOff.
ODO_SHIFT_HD bool shift_offset(int off, int d, int* out) {
  const long long s = (long long)off + d;
  if (s > kShiftMaxOff || s < -(long long)kShiftMaxOff) return false;
  *out = (int)s;
  return true;
}

// The shift that brings the window's centre to the point `focus` metres in front of the camera (column-major camera-to-world pose A):
// fp64 from the fp32 entries; p = t + focus * R[:, 2]; e_c = (p_c - (origin_c + 0.5 n_c vs)) / vs; d = 0 while max |e_c| < threshold,
// else d_c = nearbyint(e_c) (ties to even) clamped to +-n_c. False: one of the pose's 16 entries is not finite (d untouched). With
// a finite pose every e_c is finite: fp32 values cannot overflow fp64 here.
ODO_SHIFT_HD bool follow_shift(const float* A, const float* origin, const int* n, float vs, float focus, int threshold, int* d) {
  for (int i = 0; i < 16; i++) if (!(A[i] - A[i] == 0.0f)) return false;   // NaN or inf
  double e[3], big = 0.0;
  for (int c = 0; c < 3; c++) {
    const double p = (double)A[12 + c] + (double)focus * (double)A[8 + c];
    e[c] = (p - ((double)origin[c] + 0.5 * (double)n[c] * (double)vs)) / (double)vs;
    if (__builtin_fabs(e[c]) > big) big = __builtin_fabs(e[c]);
  }
  for (int c = 0; c < 3; c++) {
    d[c] = 0;
    if (big < (double)threshold) continue;
    const double r = __builtin_nearbyint(e[c]);
    d[c] = r > (double)n[c] ? n[c] : r < -(double)n[c] ? -n[c] : (int)r;
  }
  return true;
}

}  // namespace odo
