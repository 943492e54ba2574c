// volume_icp_math.h — the arithmetic of the TSDF volume's frame-to-model alignment (include/odometry_hip.h, odo_volume_icp_align_dev /
// DESIGN.md section 9.8), host + device like volume_raycast_math.h: the kernels of volume_icp_kernels.hip and the g++ harness of
// tests/volume_icp_math_harness.cpp compile these same lines. The row of one sensor pixel (association, gates, residual, Jacobian,
// weight), the step taken from the 29 sums and the eigenvalues that judge the sums' conditioning are each written once, here, over
// the LM arithmetic of odo_math.h (robust_weight, accumulate_row, solve_damped, se3_exp, se3_left_update_mat).
//
// fp32, one rounding per operation: both builds use -ffp-contract=off, the device build correctly rounded divide and sqrt. Every
// comparison that decides validity is made on floats before any conversion to an integer, so NaN and inf fail it.
#pragma once
#include "odo_math.h"

namespace odo {

// What a row needs of the two frames and the pose. C: sensor camera -> model camera, column-major. m: the rotation of the model
// camera's world-to-camera transform, row r column c at m[3 r + c] (it turns the ray-cast's world normals into the model camera).
struct IcpView {
  int rows, cols;
  float f, cx, cy;
  float depth_scale, max_depth;
  float dist_max, huber_delta;
  float m[9];
};

ODO_HD float icp_pixel(int x, float c, float f) { return ((float)x - c) / f; }

// One sensor pixel (x, y) (on the stride: the caller's business). raw: rows x cols uint16; depth_m: rows x cols float; nrmw_m: rows x
// cols x 4 float. false = no pair (J, res, w untouched). The model frame is read at (xi, yi) only after both have passed the bounds
// test as floats.
ODO_HD bool icp_row(const IcpView& a, const float* C, const uint16_t* raw, const float* depth_m, const float* nrmw_m, int x, int y,
                    float J[6], float* res, float* w) {
  const unsigned r = raw[(size_t)y * a.cols + x];
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
  const float xi = floorf(u + 0.5f), yi = floorf(v + 0.5f);
  if (!(xi >= 0.0f && xi < (float)a.cols && yi >= 0.0f && yi < (float)a.rows)) return false;
  const size_t o = (size_t)(int)yi * a.cols + (size_t)(int)xi;
  const float zm = depth_m[o];
  if (!(zm > 0.0f)) return false;
  const float nwx = nrmw_m[4 * o + 0], nwy = nrmw_m[4 * o + 1], nwz = nrmw_m[4 * o + 2];
  if (nwx == 0.0f && nwy == 0.0f && nwz == 0.0f) return false;
  const float nx = (a.m[0] * nwx + a.m[1] * nwy) + a.m[2] * nwz;
  const float ny = (a.m[3] * nwx + a.m[4] * nwy) + a.m[5] * nwz;
  const float nz = (a.m[6] * nwx + a.m[7] * nwy) + a.m[8] * nwz;
  const float vx = ((xi - a.cx) / a.f) * zm, vy = ((yi - a.cy) / a.f) * zm;
  const float ddx = pmx - vx, ddy = pmy - vy, ddz = pmz - zm;
  const float dd = (ddx * ddx + ddy * ddy) + ddz * ddz;
  if (!(dd <= a.dist_max * a.dist_max)) return false;
  const float e = (nx * ddx + ny * ddy) + nz * ddz;
  J[0] = nx; J[1] = ny; J[2] = nz;
  J[3] = pmy * nz - pmz * ny;
  J[4] = pmz * nx - pmx * nz;
  J[5] = pmx * ny - pmy * nx;
  *res = e;
  *w = (a.huber_delta > 0.0f) ? robust_weight(e, 1, a.huber_delta, 1.0f) : 1.0f;
  return true;
}

// A row as eight floats {J0 .. J5, res, w} (the layout of the debug output rows_dev). Term q < 28 of accumulate_row's 29 for one row
// is the exact fp64 product (double)(row[ia] * row[7]) * (double)row[ib], the first factor rounded to fp32 as accumulate_row does:
// q < 21 the upper triangle of J^T w J in row-major order (ia = a, ib = b), 21 .. 26 J^T w res (ia = q - 21, ib = 6), 27 w res^2
// (ia = ib = 6). Term 28 is the count.
ODO_HD void icp_term_operands(int q, int* ia, int* ib) {
  if (q >= 27) { *ia = 6; *ib = 6; return; }
  if (q >= 21) { *ia = q - 21; *ib = 6; return; }
  int a = 0, first = 0;
  while (q >= first + (6 - a)) { first += 6 - a; a++; }
  *ia = a; *ib = a + (q - first);
}
ODO_HD double icp_term(const float* row, int ia, int ib) { return (double)(row[ia] * row[7]) * (double)row[ib]; }

ODO_HD bool icp_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and inf

// One step from the sums of one evaluation at C. Returns 0 and moves C, or 1 (fewer than min_pairs pairs, or a sum that is not
// finite) and leaves C alone with delta = 0. *converged: both halves of the step are below their thresholds.
ODO_HD int icp_step(const double acc[ODO_NACC], int min_pairs, float eps_t, float eps_r, float C[16], float delta[6], int* converged) {
  bool ok = acc[28] >= (double)min_pairs;
  for (int i = 0; i < ODO_NACC; i++) ok = ok && icp_finite(acc[i]);
  *converged = 0;
  if (!ok) {
    for (int i = 0; i < 6; i++) delta[i] = 0.0f;
    return 1;
  }
  solve_damped(acc, 0.0f, delta);
  Se3 d, moved;
  se3_exp(delta, &d);
  se3_left_update_mat(d, C, &moved);
  se3_to_colmajor(moved, C);
  const float nt = sqrtf((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]);
  const float nr = sqrtf((delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5]);
  *converged = (nt < eps_t && nr < eps_r) ? 1 : 0;
  return 0;
}

// The eigenvalues of the undamped 6 x 6 of acc (fp64, ascending) by cyclic Jacobi: sweeps over the 15 pairs (p, q) in row-major
// order, each rotation chosen to zero a_pq (Golub & Van Loan's symmetric Schur step), until a sweep meets no off-diagonal entry
// that still changes a diagonal one (|a_pq| <= 2^-60 sqrt(|a_pp a_qq|) is skipped) or after 30 sweeps. Host only.
ODO_HD void icp_eigenvalues(const double acc[ODO_NACC], double ev[6]) {
  double A[6][6];
  int k = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) { A[a][b] = acc[k]; A[b][a] = acc[k]; k++; }
  for (int sweep = 0; sweep < 30; sweep++) {
    int rotated = 0;
    for (int p = 0; p < 5; p++)
      for (int q = p + 1; q < 6; q++) {
        const double apq = A[p][q];
        if (!(fabs(apq) > 8.673617379884035e-19 * sqrt(fabs(A[p][p] * A[q][q])))) {   // (a NaN entry is skipped too and stays)
          if (apq == apq) A[p][q] = A[q][p] = 0.0;
          continue;
        }
        rotated = 1;
        const double tau = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
        for (int i = 0; i < 6; i++) {   // A <- A G
          const double aip = A[i][p], aiq = A[i][q];
          A[i][p] = c * aip - s * aiq;
          A[i][q] = s * aip + c * aiq;
        }
        for (int i = 0; i < 6; i++) {   // A <- G^T A
          const double api = A[p][i], aqi = A[q][i];
          A[p][i] = c * api - s * aqi;
          A[q][i] = s * api + c * aqi;
        }
      }
    if (!rotated) break;
  }
  for (int i = 0; i < 6; i++) ev[i] = A[i][i];
  for (int i = 1; i < 6; i++)   // insertion sort, ascending
    for (int j = i; j > 0 && ev[j] < ev[j - 1]; j--) { const double t = ev[j]; ev[j] = ev[j - 1]; ev[j - 1] = t; }
}

}  // namespace odo
