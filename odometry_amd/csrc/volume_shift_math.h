// volume_shift_math.h — the rules of the moving TSDF volume (include/odometry_hip.h, odo_volume_shift / odo_volume_follow; DESIGN.md
// section 9.9), host + device like volume_math.h: the kernels of volume_shift_kernels.hip, the host object (volume_shift_api.hip.h)
// and the g++ harness of tests/volume_shift_harness.cpp compile these same lines. Where a shifted voxel comes from, which voxels a
// shift destroys, how far the window may travel, the shift that follows a pose, and which cells and edges of the mesh a shift spills
// (tests/volume_spill_mesh_harness.cpp), and the key of the re-entry store (DESIGN.md section 9.14;
// volume_reentry_kernels.hip, tests/volume_reentry_harness.cpp) are each written once, here. The window's origin is host_fp.h's
// (hostfp::window_origin).
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

// ---- the mesh spill ---------------------------------------------------------------------------------------
// The old voxels that stay under d form the box [lo, hi] on every axis, empty (lo > hi) when |d| >= n. (64-bit: every int d is legal.)
ODO_SHIFT_HD void shift_stay_box(int d, int n, long long* lo, long long* hi) {
  *lo = d > 0 ? (long long)d : 0;
  *hi = d < 0 ? (long long)n - 1 + d : (long long)n - 1;
}

// On one axis: the cell with low corner c (0 <= c <= n - 2) has a corner that leaves, c < lo or c + 1 > hi.
ODO_SHIFT_HD bool shift_cell_axis(int c, int d, int n) {
  long long lo, hi;
  shift_stay_box(d, n, &lo, &hi);
  return c < lo || (long long)c + 1 > hi;
}

// The cell with low corner (i, j, k), all eight corners inside the grid, is spilled iff at least one of its corners leaves.
ODO_SHIFT_HD bool shift_cell_spilled(int i, int j, int k, int dx, int dy, int dz, int nx, int ny, int nz) {
  return shift_cell_axis(i, dx, nx) || shift_cell_axis(j, dy, ny) || shift_cell_axis(k, dz, nz);
}

// On one axis: the edge from a to a + step (step 0 or 1, both inside the grid, n >= 2) is an edge of cells whose low corner is a when
// step = 1, else one of {a - 1, a} within [0, n - 2]; true iff one of those has a leaving corner on this axis.
ODO_SHIFT_HD bool shift_edge_axis(int a, int step, int d, int n) {
  if (step) return shift_cell_axis(a, d, n);
  return (a >= 1 && shift_cell_axis(a - 1, d, n)) || (a <= n - 2 && shift_cell_axis(a, d, n));
}

// The edge from voxel (i, j, k) in direction c (= dx + 2 dy + 4 dz, 1 .. 7, the far end inside the grid) is spilled iff it is an edge of
// at least one spilled cell of the grid. The candidate cells are a product over the axes, so one axis with a spilling candidate is enough.
ODO_SHIFT_HD bool shift_edge_spilled(int i, int j, int k, int c, int dx, int dy, int dz, int nx, int ny, int nz) {
  return shift_edge_axis(i, c & 1, dx, nx) || shift_edge_axis(j, (c >> 1) & 1, dy, ny) || shift_edge_axis(k, (c >> 2) & 1, dz, nz);
}

// On one axis: voxel v is within one voxel of a leaving one, so one of its edges or its cell may be spilled. A voxel for which this is
// false on every axis owns no spilled edge and no spilled cell: the mesh spill's threads load nothing for it.
ODO_SHIFT_HD bool shift_near_axis(int v, int d, int n) {
  long long lo, hi;
  shift_stay_box(d, n, &lo, &hi);
  return (lo > 0 && v <= lo) || (hi < (long long)n - 1 && v >= hi);
}

ODO_SHIFT_HD bool shift_near(int i, int j, int k, int dx, int dy, int dz, int nx, int ny, int nz) {
  return shift_near_axis(i, dx, nx) || shift_near_axis(j, dy, ny) || shift_near_axis(k, dz, nz);
}

// The cumulative shift off + d on one axis, refused (false) beyond +-kShiftMaxOff.
ODO_SHIFT_HD bool shift_offset(int off, int d, int* out) {
  const long long s = (long long)off + d;
  if (s > kShiftMaxOff || s < -(long long)kShiftMaxOff) return false;
  *out = (int)s;
  return true;
}

// ---- re-entry -----------------------------------------------------------------------------------------------
// A voxel's global index on one axis: the window's cumulative shift plus its index in the window. The same physical voxel has the
// same g whenever it is in the window. (64-bit: every int is legal; with |off| <= kShiftMaxOff and i < 2^30 it fits an int32.)
ODO_SHIFT_HD long long reentry_global(int off, int i) {
  return (long long)off + i;
}

// The stored voxel g lies inside the window `off` voxels from where it was created, n voxels wide: *t is its index there (only read
// when inside: then it fits).
ODO_SHIFT_HD bool reentry_inside(int g, int off, int n, int* t) {
  const long long s = (long long)g - off;
  *t = (int)s;
  return s >= 0 && s < n;
}

// All three axes, and the word of the window's grid the voxel comes back to.
ODO_SHIFT_HD bool reentry_dest(const int g[3], const int off[3], int nx, int ny, int nz, long long* word) {
  int i, j, k;
  const bool in = reentry_inside(g[0], off[0], nx, &i) & reentry_inside(g[1], off[1], ny, &j) & reentry_inside(g[2], off[2], nz, &k);
  *word = ((long long)k * ny + j) * nx + i;
  return in;
}

// A leaving voxel is saved iff it has a non-zero bit: an all-zero voxel equals what an entering voxel holds anyway.
ODO_SHIFT_HD bool reentry_saved(uint32_t word, uint32_t colour) {
  return (word | colour) != 0u;
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
