// tests/devmath_ops.h — TEST INFRASTRUCTURE. One case of every odo_math.h operation the device-math harness calls, written once
// and compiled twice: by g++ into tests/hostemu.cpp (the host build the CPU tests hold to the oracle) and by hipcc into
// tests/devmath_harness.hip (the gfx950 build the GPU tests hold to that host build). A case reads element i of its input arrays
// and writes element i of its output arrays; nothing here is linked into the product.
#pragma once
#include "../odometry_amd/csrc/odo_math.h"

#include <string.h>

namespace dm {
using namespace odo;

ODO_HD void put_se3(const Se3& s, float* q) {
  q[0] = s.qx; q[1] = s.qy; q[2] = s.qz; q[3] = s.qw; q[4] = s.tx; q[5] = s.ty; q[6] = s.tz;
}

// cx_level + make_level_k: fl[i], cxy[3 i] = {k.cx, k.cy, cx_level(cx0, level)}
ODO_HD void op_level_k(int i, const float* f0, const float* cx0, const float* cy0, const int* level, double* fl, float* cxy) {
  const LevelK k = make_level_k(f0[i], cx0[i], cy0[i], level[i]);
  fl[i] = k.fl;
  cxy[3 * i + 0] = k.cx; cxy[3 * i + 1] = k.cy; cxy[3 * i + 2] = cx_level(cx0[i], level[i]);
}
ODO_HD void op_sincos(int i, const float* x, float* s, float* c) { sincos_f(x[i], &s[i], &c[i]); }
// se3_exp: the seven stored floats and the matrix
ODO_HD void op_se3_exp(int i, const float* a, float* q, float* M) {
  Se3 s;
  se3_exp(a + 6 * i, &s);
  put_se3(s, q + 7 * i);
  se3_to_colmajor(s, M + 16 * i);
}
// se3_from_colmajor -> se3_to_colmajor
ODO_HD void op_se3_roundtrip(int i, const float* Min, float* q, float* M) {
  Se3 s;
  se3_from_colmajor(Min + 16 * i, &s);
  put_se3(s, q + 7 * i);
  se3_to_colmajor(s, M + 16 * i);
}
// variant 0: se3_left_update(exp(d6), SE3(cur)); variant 1: se3_left_update_mat(exp(d6), matrix(SE3(cur)))
ODO_HD void op_se3_left_update(int i, const float* d6, const float* cur, int variant, float* q, float* M) {
  Se3 d, c, o;
  se3_exp(d6 + 6 * i, &d);
  se3_from_colmajor(cur + 16 * i, &c);
  if (variant) {
    float C[16];
    se3_to_colmajor(c, C);
    se3_left_update_mat(d, C, &o);
  } else {
    se3_left_update(d, c, &o);
  }
  put_se3(o, q + 7 * i);
  se3_to_colmajor(o, M + 16 * i);
}
ODO_HD void op_solve_damped(int i, const double* acc, const float* lambda, float* delta) {
  solve_damped(acc + ODO_NACC * i, lambda[i], delta + 6 * i);
}
ODO_HD void op_robust_weight(int i, const float* r, const int* robust, const float* huber, const float* scale, float* w) {
  w[i] = robust_weight(r[i], robust[i], huber[i], scale[i]);
}
ODO_HD void op_apply_step(int i, const LmState* in, LmState* out) {
  LmState s = in[i];
  lm_apply_step(&s, s.max_iters);
  out[i] = s;
}

// depth_lm_begin / depth_lm_decide / depth_lm_advance over a scripted error list (the replay of emu_depth_lm_schedule): script i
// reads errs[i * cap .. + n_errs[i]) and writes 5 ints per evaluation {lambda bits, err_last bits, current tag, pre tag, broke} and
// fin[3 i] = {evaluations, final current tag, iter}.
ODO_HD void op_depth_schedule(int i, int cap, const float* errs, const int* n_errs, const float* lambda0, const float* precision,
                              const int* max_iters, int* rec, int* fin) {
  DepthLmState st;
  depth_lm_begin(&st, lambda0[i], max_iters[i]);
  int cur = 0, pre = -1, tmp = 0, k = 0;
  int* R = rec + (size_t)i * cap * 5;
  while (!st.done && k < n_errs[i] && k < cap) {
    const int mode = depth_lm_decide(&st, errs[(size_t)i * cap + k], precision[i]);
    if (mode == 0) cur = pre;
    else if (mode == 1 || mode == 3) { cur = tmp; pre = cur; }
    memcpy(&R[5 * k + 0], &st.lambda, sizeof(int));
    memcpy(&R[5 * k + 1], &st.err_last, sizeof(int));
    R[5 * k + 2] = cur; R[5 * k + 3] = pre; R[5 * k + 4] = (mode >= 2) ? 1 : 0;
    k++;
    depth_lm_advance(&st, mode, max_iters[i]);
    if (mode >= 2) break;
    tmp = k;
  }
  fin[3 * i + 0] = k; fin[3 * i + 1] = cur; fin[3 * i + 2] = st.iter;
}

// ---------------------------------------------------------------------------------------------
// LM scripts: one Solve driven by a given list of accumulator sets instead of by images.
// The state starts as the fused kernels' prologue leaves it (lm_begin_solve and the five fields it does not set), the pyramid is
// walked as lm_state_machine walks it, and every evaluation is lm_consume. 64 dwords of state are written out after every evaluation.
// ---------------------------------------------------------------------------------------------
struct LmScript {
  int n_levels, stop_level, n_evals, acc_first;   // acc_first: index of the script's first accumulator set / output state
  float lambda0, precision;
  int max_iters[8];
  float init[16];
};
ODO_HD void script_begin(LmState* s, const float init[16]) {
  lm_begin_solve(s, init);
  s->level = -1; s->iter = 0; s->lambda = 0.0f; s->err_last = 1e+10f;
  for (int i = 0; i < 16; i++) s->T[i] = init[i];
}
ODO_HD void script_walk(LmState* s, const LmScript& sc) {
  while (!s->active && s->status == 0 && !s->finished) {
    const int next = (s->level < 0) ? sc.n_levels - 1 : s->level - 1;
    if (next < sc.stop_level) { s->finished = 1; break; }
    s->stop_reason = 0;
    lm_begin_level(s, next, sc.lambda0, sc.max_iters[next]);
  }
  if (s->status != 0) s->finished = 1;
}
ODO_HD bool script_live(const LmState& s) { return s.active != 0 && s.status == 0 && s.finished == 0; }
// Returns the number of evaluations consumed; out[acc_first + e] = the state after evaluation e.
ODO_HD int script_run(const LmScript& sc, const double* acc, LmState* out) {
  LmState s;
  script_begin(&s, sc.init);
  script_walk(&s, sc);
  int e = 0;
  for (; e < sc.n_evals; e++) {
    if (!script_live(s)) break;
    lm_consume(&s, acc + (size_t)(sc.acc_first + e) * ODO_NACC, sc.precision, s.max_iters);
    s.pending = 0;
    script_walk(&s, sc);
    out[sc.acc_first + e] = s;
  }
  return e;
}

// ---------------------------------------------------------------------------------------------
// One pixel of a level: hit, r, w, J[6] at index y * cols + x.
// mode 0: make_point + point_residual<true> (the level's sampling mode), 1: point_residual<false>, 3: point_residual_only (J stays 0).
// (mode 2, point_residual_g, and the dense stages exist on the device only: tests/devmath_harness.hip.)
// ---------------------------------------------------------------------------------------------
struct PixLevel {
  const float *I1, *I2, *D1;
  int rows, cols;
  LevelK k;
  float T[16];
  int robust;
  float huber_delta, scale_sqr;
};
ODO_HD void pix_store(const PixLevel& L, int o, bool hit, float r, const float J[6], int* hit_out, float* r_out, float* w_out, float* J_out) {
  hit_out[o] = hit ? 1 : 0;
  r_out[o] = hit ? r : 0.0f;
  w_out[o] = hit ? robust_weight(r, L.robust, L.huber_delta, L.scale_sqr) : 0.0f;
  for (int a = 0; a < 6; a++) J_out[(size_t)o * 6 + a] = hit ? J[a] : 0.0f;
}
ODO_HD void op_pixel(const PixLevel& L, int mode, int x, int y, int* hit_out, float* r_out, float* w_out, float* J_out) {
  const int o = y * L.cols + x;
  float r = 0.0f, J[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bool hit = false;
  const float d = L.D1[o];
  if (depth_valid(d)) {
    const PointK p = make_point(x, y, d, L.I1[o], L.k);
    if (mode == 0) hit = point_residual<true>(p, L.T, L.k, L.I2, L.rows, L.cols, &r, J);
    else if (mode == 1) hit = point_residual<false>(p, L.T, L.k, L.I2, L.rows, L.cols, &r, J);
    else hit = point_residual_only(p, L.T, L.k, L.I2, L.rows, L.cols, &r);
  }
  pix_store(L, o, hit, r, J, hit_out, r_out, w_out, J_out);
}

// make_point of pixel i of a level (x = i % cols, y = i / cols; every pixel, whatever its depth), the level's intrinsics from
// make_level_k as kf_fill_kernel_body derives them: the thirteen floats of a list entry in PointList's order — a = X, Y, Z, i1;
// b = fx_z, jw02, jw03, jw04; c = jw05, jw12, jw13, jw14; d = jw15.
ODO_HD void op_make_point(int i, const float* I1, const float* D1, int cols, float f0, float cx0, float cy0, int level, float* out13) {
  const LevelK k = make_level_k(f0, cx0, cy0, level);
  const PointK p = make_point(i % cols, i / cols, D1[i], I1[i], k);
  float* o = out13 + (size_t)i * 13;
  o[0] = p.X; o[1] = p.Y; o[2] = p.Z; o[3] = p.i1;
  o[4] = p.fx_z; o[5] = p.jw02; o[6] = p.jw03; o[7] = p.jw04;
  o[8] = p.jw05; o[9] = p.jw12; o[10] = p.jw13; o[11] = p.jw14;
  o[12] = p.jw15;
}

}  // namespace dm
