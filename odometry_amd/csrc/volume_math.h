// volume_math.h — the voxel arithmetic of the TSDF volume (include/odometry_hip.h, odo_volume_integrate_dev / odo_volume_extract /
// odo_volume_mesh; DESIGN.md sections 9.4 and 9.5), host + device like volume_raycast_math.h: the kernels of volume_kernels.hip,
// volume_mesh_kernels.hip and volume_colour_kernels.hip and the g++ harness of tests/volume_math_harness.cpp compile these same
// lines. The voxel word, the index arithmetic, the gradient, the point of an edge and the integration of one voxel are each written
// once, here.
//
// fp32, one rounding per operation: both builds use -ffp-contract=off, the device build correctly rounded divide and sqrt. Every
// comparison that decides validity is made on floats before any conversion to an integer, so NaN and inf fail it.
//
// A voxel is 4 bytes, {int16 q, uint16 w} = one 32-bit word (q in the low half): q = truncated signed distance * 32767, w = weight,
// 0 = never observed. Voxel (i, j, k) is word (k * ny + j) * nx + i.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ODO_VOL_HD __host__ __device__ __forceinline__
#else
#define ODO_VOL_HD static inline
#endif

namespace odo {

struct VolGrid {
  uint32_t* vox;   // [nx * ny * nz]
  int nx, ny, nz;
  float vs, ox, oy, oz;
};

// What an integration needs of the depth frame and its camera.
struct VolFrame {
  int rows, cols;
  float f0, cx0, cy0;
  float depth_scale, max_depth, mu;
  int max_weight;
  float m0, m1, m2, m4, m5, m6, m8, m9, m10, m12, m13, m14;   // world-to-camera, column-major indices
  float zc_far;   // the early-out: 1.001 (max_depth + mu)
};

// ---- the voxel word and its place ------------------------------------------------------------------------------------------------
ODO_VOL_HD int vox_q(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }
ODO_VOL_HD int vox_w(uint32_t v) { return (int)(v >> 16); }
ODO_VOL_HD uint32_t vox_pack(int q, int w) { return ((uint32_t)w << 16) | ((uint32_t)q & 0xffffu); }
ODO_VOL_HD float vox_centre(float o, int i, float vs) { return o + ((float)i + 0.5f) * vs; }

ODO_VOL_HD void vox_ijk(const VolGrid& g, int v, int* i, int* j, int* k) {
  const int row = v / g.nx;
  *i = v - row * g.nx;
  *k = row / g.ny;
  *j = row - *k * g.ny;
}

// Word of the voxel at corner c (= dx + 2 dy + 4 dz) of the cell whose corner 0 is word v.
ODO_VOL_HD long long vox_corner_word(const VolGrid& g, int v, int c) {
  return (long long)v + (c & 1) + (long long)((c >> 1) & 1) * g.nx + (long long)((c >> 2) & 1) * g.nx * g.ny;
}

// An edge a -> b carries a point iff both voxels were observed and exactly one of them has q > 0.
ODO_VOL_HD bool vox_edge(uint32_t va, uint32_t vb) { return vox_w(va) > 0 && vox_w(vb) > 0 && (vox_q(va) > 0) != (vox_q(vb) > 0); }

// ---- the gradient ----------------------------------------------------------------------------------------------------------------
enum VoxDifference { kVoxBoth = 0, kVoxPlus, kVoxMinus, kVoxNeither };

// One axis: the central difference over the neighbours vp / vm when both were observed, else twice the one-sided difference towards
// the one that was (Q = this voxel's value), else nothing. A neighbour outside the grid is passed as 0: w = 0, not usable.
ODO_VOL_HD VoxDifference vox_difference(float Q, uint32_t vp, uint32_t vm, float* d) {
  const bool up = vox_w(vp) > 0, um = vox_w(vm) > 0;
  const float Qp = (float)vox_q(vp), Qm = (float)vox_q(vm);
  VoxDifference which = kVoxNeither;
  float diff = 0.0f;
  if (up && um) { diff = Qp - Qm; which = kVoxBoth; }
  else if (up) { diff = 2.0f * (Qp - Q); which = kVoxPlus; }
  else if (um) { diff = 2.0f * (Q - Qm); which = kVoxMinus; }
  *d = diff;
  return which;
}

// The gradient of Q = (float)q at voxel (i, j, k) = word v, whose own word is vc; false when an axis has neither neighbour.
ODO_VOL_HD bool vox_gradient(const VolGrid& g, long long v, int i, int j, int k, uint32_t vc, float* grad) {
  const float Q = (float)vox_q(vc);
  const int pos[3] = {i, j, k}, dim[3] = {g.nx, g.ny, g.nz};
  const long long stride[3] = {1, g.nx, (long long)g.nx * g.ny};
  bool ok = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int c = 0; c < 3; c++) {
    uint32_t vp = 0, vm = 0;
    if (pos[c] + 1 < dim[c]) vp = g.vox[v + stride[c]];
    if (pos[c] > 0) vm = g.vox[v - stride[c]];
    if (vox_difference(Q, vp, vm, &grad[c]) == kVoxNeither) ok = false;
  }
  return ok;
}

// ---- the point of an edge --------------------------------------------------------------------------------------------------------
ODO_VOL_HD float vox_alpha(uint32_t va, uint32_t vb) {
  const float qa = (float)vox_q(va);
  return qa / (qa - (float)vox_q(vb));
}

struct VoxEdgePoint {
  float alpha;
  float x, y, z;      // the centre of a moved by alpha * vs along the axes of the edge
  float nx, ny, nz;   // the interpolated gradient, normalised; 0 when either end has none or it has no length
  float w;            // the smaller weight
};

// The edge from voxel a (word va, centre (cx, cy, cz), gradient ga when has_a) to voxel b = a + (dx, dy, dz), each 0 or 1.
ODO_VOL_HD VoxEdgePoint vox_edge_point(uint32_t va, uint32_t vb, bool has_a, const float* ga, bool has_b, const float* gb, float cx,
                                       float cy, float cz, float vs, int dx, int dy, int dz) {
  VoxEdgePoint o;
  o.alpha = vox_alpha(va, vb);
  const float step = o.alpha * vs;
  o.x = dx ? cx + step : cx;
  o.y = dy ? cy + step : cy;
  o.z = dz ? cz + step : cz;
  o.nx = o.ny = o.nz = 0.0f;
  if (has_a && has_b) {
    const float mx = ga[0] + o.alpha * (gb[0] - ga[0]), my = ga[1] + o.alpha * (gb[1] - ga[1]), mz = ga[2] + o.alpha * (gb[2] - ga[2]);
    const float len = __builtin_sqrtf((mx * mx + my * my) + mz * mz);
    if (len > 0.0f) { o.nx = mx / len; o.ny = my / len; o.nz = mz / len; }
  }
  const int wa = vox_w(va), wb = vox_w(vb);
  o.w = (float)(wa < wb ? wa : wb);
  return o;
}

// ---- the integration of one voxel --------------------------------------------------------------------------------------------------
// Two parts, so that the depth pixel is loaded before the voxel and no voxel that fails a test is touched: vox_visit decides which
// pixel, if any, and hands the reading to the caller's keep(pixel, sdf, s), which loads the voxel and stores vox_update's new word.
// (The tests as functions of their own that return to an `if (...) continue` of the kernel were measured: their merged exits cost the
// integration 4 VGPRs, 21 instructions (exec-mask traffic in the loop) and 4.6 % on the large grid. DESIGN.md 9.4.)
enum VoxSkip { kVoxKept = 0, kVoxBehind, kVoxPast, kVoxOutside, kVoxHole, kVoxFar, kVoxBeyond };   // the test that ended a visit

// Voxel (i, j, k) against one depth frame: the projection of its centre and the tests in the specification's order, then
// keep(pixel, sdf, s) with s = the truncated distance in units of q.
template <class Keep>
ODO_VOL_HD VoxSkip vox_visit(const VolGrid& g, const VolFrame& f, const uint16_t* depth, int i, int j, int k, const Keep& keep) {
  const float X = vox_centre(g.ox, i, g.vs), Y = vox_centre(g.oy, j, g.vs), Z = vox_centre(g.oz, k, g.vs);
  const float zc = ((f.m2 * X + f.m6 * Y) + f.m10 * Z) + f.m14;
  if (!(zc > 0.0f)) return kVoxBehind;
  // Early-out in front of the two divides and the depth pixel; it only ever skips what the tests below skip: a reading that passes
  // D <= max_depth has D - zc <= max_depth - zc (fp32 subtraction is monotonic), and beyond zc_far = 1.001 (max_depth + mu) that is
  // below -mu by 0.1 %, ten thousand roundings. (The same for the four sides of the image was measured and dropped)
  if (zc > f.zc_far) return kVoxPast;
  const float xc = ((f.m0 * X + f.m4 * Y) + f.m8 * Z) + f.m12;
  const float yc = ((f.m1 * X + f.m5 * Y) + f.m9 * Z) + f.m13;
  const float u = f.f0 * (xc / zc) + f.cx0, v = f.f0 * (yc / zc) + f.cy0;
  const float xf = __builtin_floorf(u + 0.5f), yf = __builtin_floorf(v + 0.5f);
  if (!(xf >= 0.0f && xf < (float)f.cols && yf >= 0.0f && yf < (float)f.rows)) return kVoxOutside;   // (NaN fails too)
  const int pixel = (int)yf * f.cols + (int)xf;   // (< rows * cols <= 2^28)
  const unsigned raw = depth[pixel];
  if (raw == 0) return kVoxHole;
  const float D = (float)raw / f.depth_scale;
  if (D > f.max_depth) return kVoxFar;
  const float sdf = D - zc;
  if (sdf < -f.mu) return kVoxBeyond;
  keep(pixel, sdf, __builtin_fminf(1.0f, sdf / f.mu) * 32767.0f);
  return kVoxKept;
}

ODO_VOL_HD bool vox_in_band(float sdf, float mu) { return __builtin_fabsf(sdf) <= mu; }

// The running average F = (q W + s) / (W + 1), rounded to nearest even; the weight counts up to max_weight.
ODO_VOL_HD uint32_t vox_update(uint32_t old, float s, int max_weight) {
  const int wo = vox_w(old);
  const float W = (float)wo;
  const float F = ((float)vox_q(old) * W + s) / (W + 1.0f);
  const int qn = (int)__builtin_rintf(F);
  const int wn = wo + 1 < max_weight ? wo + 1 : max_weight;
  return vox_pack(qn, wn);
}

}  // namespace odo
