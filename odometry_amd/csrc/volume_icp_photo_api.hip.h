// volume_icp_photo_api.hip.h — frame-to-model tracking with a photometric term (odo_volume_icp_photo_eval_dev,
// odo_volume_icp_photo_align_dev, odo_volume_track_photo_dev, odo_volume_icp_photo_time_dev): the host side over the kernels of
// volume_icp_photo_kernels.hip. Included by odometry_hip.hip behind volume_icp_api.hip.h, whose helpers (the ordering, the parameter
// checks, the block count) it uses and does not change.
//
// As there, the alignment's device memory (the state, one partial per block of the finest grid, the trace) lives for one call.
#pragma once
#include "volume_icp_photo.hip.h"

static_assert(sizeof(odo_icp_photo_trace_row) == sizeof(IcpPhotoTraceRow) && offsetof(odo_icp_photo_trace_row, acc) == offsetof(IcpPhotoTraceRow, acc) &&
              offsetof(odo_icp_photo_trace_row, delta) == offsetof(IcpPhotoTraceRow, delta) &&
              offsetof(odo_icp_photo_trace_row, C) == offsetof(IcpPhotoTraceRow, C), "odo_icp_photo_trace_row is the device's IcpPhotoTraceRow");

struct IcpPhotoScratch {
  IcpPhotoState* state = nullptr;
  double* partials = nullptr;
  IcpPhotoTraceRow* trace = nullptr;
  ~IcpPhotoScratch() {
    if (state) (void)hipFree(state);
    if (partials) (void)hipFree(partials);
    if (trace) (void)hipFree(trace);
  }
};

static int icp_photo_alloc(IcpPhotoScratch* sc, int max_blocks, int trace_rows) {
  if (hipMalloc((void**)&sc->state, sizeof(IcpPhotoState)) != hipSuccess ||
      hipMalloc((void**)&sc->partials, sizeof(double) * kIcpPhotoAcc * (size_t)max_blocks) != hipSuccess ||
      (trace_rows > 0 && hipMalloc((void**)&sc->trace, sizeof(IcpPhotoTraceRow) * (size_t)trace_rows) != hipSuccess)) {
    (void)hipGetLastError();
    return fail("odo_volume_icp_photo: device allocation failed (%d partials, %d trace rows)", max_blocks, trace_rows);
  }
  return 0;
}

static int icp_photo_check(const char* who, const odo_icp_photo_params* ph) {
  if (!icp_float_ok(ph->weight, true)) return fail("%s: the photometric weight must be finite and > 0", who);
  if (!icp_float_ok(ph->huber_delta, false)) return fail("%s: the photometric huber_delta must be finite and >= 0", who);
  return 0;
}

// The frames of one call: the model's three and the sensor's two.
struct IcpPhotoFrames {
  const float* depth_m;
  const float* nrmw_m;
  const uint8_t* rgba_m;
  const uint16_t* raw;
  const float* grey;
};

static int icp_photo_frames_check(const char* who, const IcpPhotoFrames& f, const float* rows_dev) {
  if (!f.depth_m || !f.nrmw_m || !f.rgba_m || !f.raw || !f.grey) return fail("%s: NULL arg", who);
  if (((uintptr_t)f.depth_m & 3) || ((uintptr_t)f.nrmw_m & 15) || ((uintptr_t)f.rgba_m & 3) || ((uintptr_t)f.raw & 1) ||
      ((uintptr_t)f.grey & 3) || ((uintptr_t)rows_dev & 15))
    return fail("%s: misaligned frame (grey 4, rgba 4, depth 4, nrmw 16, raw 2, rows 16 bytes)", who);
  return 0;
}

static VolIcpPhotoRowsArgs icp_photo_rows_args(const odo_volume* v, const IcpPhotoFrames& f, const float* M, int stride, int level, float dist_max,
                                               float huber_delta, const odo_icp_photo_params* ph, const IcpPhotoScratch& sc, float* rows_dev) {
  VolIcpPhotoRowsArgs a;
  memset(&a, 0, sizeof(a));
  a.raw = f.raw; a.grey = f.grey; a.depth_m = f.depth_m; a.nrmw_m = f.nrmw_m; a.rgba_m = (const uint32_t*)f.rgba_m;
  a.rows = v->p.rows; a.cols = v->p.cols;
  a.f = v->p.K.f0; a.cx = v->p.K.cx0; a.cy = v->p.K.cy0;
  a.depth_scale = v->p.depth_scale; a.max_depth = v->p.max_depth;
  a.dist_max = dist_max; a.huber_delta = huber_delta;
  a.photo_weight = ph->weight; a.photo_huber = ph->huber_delta;
  a.m0 = M[0]; a.m1 = M[4]; a.m2 = M[8]; a.m3 = M[1]; a.m4 = M[5]; a.m5 = M[9]; a.m6 = M[2]; a.m7 = M[6]; a.m8 = M[10];
  a.stride = stride; a.level = level;
  a.state = sc.state; a.partials = sc.partials; a.rows_dev = rows_dev;
  return a;
}

// What odo_volume_icp_photo_eval_dev and odo_volume_icp_photo_time_dev check alike.
static int icp_photo_eval_check(const char* who, const odo_volume* v, const IcpPhotoFrames& f, const float* P_m, const float* Cm, int stride,
                                float dist_max, float huber_delta, const odo_icp_photo_params* ph, const float* rows_dev) {
  if (!v || !P_m || !Cm || !ph) return fail("%s: NULL arg", who);
  if (icp_photo_frames_check(who, f, rows_dev)) return -1;
  if (stride < 1 || stride > 16) return fail("%s: stride %d out of range (1 .. 16)", who, stride);
  if (!icp_float_ok(dist_max, true)) return fail("%s: dist_max must be finite and > 0", who);
  if (!icp_float_ok(huber_delta, false)) return fail("%s: huber_delta must be finite and >= 0", who);
  if (icp_photo_check(who, ph)) return -1;
  if (!pose_finite(P_m) || !pose_finite(Cm)) return fail("%s: a pose has a non-finite entry", who);
  return 0;
}

extern "C" int odo_volume_icp_photo_eval_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const uint8_t* rgba_m_dev,
                                             const float model_pose_colmajor[16], const uint16_t* raw_dev, const float* grey_dev,
                                             const float C_colmajor[16], int stride, float dist_max, float huber_delta,
                                             const odo_icp_photo_params* photo, double acc[31], float* rows_dev) {
  const char* who = "odo_volume_icp_photo_eval_dev";
  const IcpPhotoFrames f = {depth_m_dev, nrmw_m_dev, rgba_m_dev, raw_dev, grey_dev};
  if (!acc) return fail("%s: NULL arg", who);
  if (icp_photo_eval_check(who, v, f, model_pose_colmajor, C_colmajor, stride, dist_max, huber_delta, photo, rows_dev)) return -1;
  HIP_OK(hipSetDevice(v->device));
  IcpPhotoScratch sc;
  const int nblk = icp_blocks(v, stride);
  if (icp_photo_alloc(&sc, nblk, 0)) return -1;
  if (icp_order(v)) return -1;
  float M[16];
  hostfp::invert_rigid(model_pose_colmajor, M);
  IcpInit init;
  memcpy(init.C, C_colmajor, sizeof(init.C));
  launch_volume_icp_photo_init(sc.state, init, v->own);
  launch_volume_icp_photo_rows(icp_photo_rows_args(v, f, M, stride, 0, dist_max, huber_delta, photo, sc, rows_dev), v->own);
  VolIcpPhotoStepArgs s;
  memset(&s, 0, sizeof(s));
  s.partials = sc.partials; s.nblk = nblk; s.state = sc.state;
  launch_volume_icp_photo_step(s, v->own);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(acc, (const char*)sc.state + offsetof(IcpPhotoState, acc), sizeof(double) * kIcpPhotoAcc, hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  return 0;
}

// Event timing of the two kernels (tools/volume_cost.py icp --photo), as odo_volume_icp_time_dev.
extern "C" int odo_volume_icp_photo_time_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const uint8_t* rgba_m_dev,
                                             const float model_pose_colmajor[16], const uint16_t* raw_dev, const float* grey_dev,
                                             const float C_colmajor[16], int stride, float dist_max, float huber_delta,
                                             const odo_icp_photo_params* photo, int reps, float us[2]) {
  const char* who = "odo_volume_icp_photo_time_dev";
  const IcpPhotoFrames f = {depth_m_dev, nrmw_m_dev, rgba_m_dev, raw_dev, grey_dev};
  if (!us) return fail("%s: NULL arg", who);
  if (icp_photo_eval_check(who, v, f, model_pose_colmajor, C_colmajor, stride, dist_max, huber_delta, photo, nullptr)) return -1;
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  HIP_OK(hipSetDevice(v->device));
  IcpPhotoScratch sc;
  const int nblk = icp_blocks(v, stride);
  if (icp_photo_alloc(&sc, nblk, 0)) return -1;
  if (icp_order(v)) return -1;
  float M[16];
  hostfp::invert_rigid(model_pose_colmajor, M);
  IcpInit init;
  memcpy(init.C, C_colmajor, sizeof(init.C));
  const VolIcpPhotoRowsArgs ra = icp_photo_rows_args(v, f, M, stride, 0, dist_max, huber_delta, photo, sc, nullptr);
  VolIcpPhotoStepArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.partials = sc.partials; sa.nblk = nblk; sa.state = sc.state;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool ok = true;
  for (auto& e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  if (ok) {
    launch_volume_icp_photo_init(sc.state, init, v->own);
    launch_volume_icp_photo_rows(ra, v->own);   // (warm)
    launch_volume_icp_photo_step(sa, v->own);
    ok = hipEventRecord(ev[0], v->own) == hipSuccess;
    for (int i = 0; i < reps; i++) launch_volume_icp_photo_rows(ra, v->own);
    ok = ok && hipEventRecord(ev[1], v->own) == hipSuccess;
    for (int i = 0; i < reps; i++) launch_volume_icp_photo_step(sa, v->own);
    ok = ok && hipEventRecord(ev[2], v->own) == hipSuccess && hipGetLastError() == hipSuccess && hipStreamSynchronize(v->own) == hipSuccess;
    float ms0 = 0.0f, ms1 = 0.0f;
    ok = ok && hipEventElapsedTime(&ms0, ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&ms1, ev[1], ev[2]) == hipSuccess;
    us[0] = 1e3f * ms0 / (float)reps;
    us[1] = 1e3f * ms1 / (float)reps;
  }
  for (auto& e : ev) if (e) (void)hipEventDestroy(e);
  if (!ok) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(v->own);
    return fail("%s: timing failed", who);
  }
  return 0;
}

// The launches and the single wait of one alignment, every argument checked by the caller.
static int icp_photo_align(odo_volume* v, const odo_icp_params* p, const odo_icp_photo_params* ph, const IcpPhotoFrames& f, const float* P_m,
                           const float* P_init, float* abs_pose, odo_icp_photo_result* out, odo_icp_photo_trace_row* trace, int trace_capacity,
                           int* trace_n) {
  int total = 0, max_blocks = 1;
  for (int l = 0; l < p->levels; l++) {
    total += p->iters[l];
    max_blocks = std::max(max_blocks, icp_blocks(v, p->stride[l]));
  }
  const int trace_rows = trace ? std::min(trace_capacity, total) : 0;
  IcpPhotoScratch sc;
  if (icp_photo_alloc(&sc, max_blocks, trace_rows)) return -1;
  if (icp_order(v)) return -1;
  float M[16];
  IcpInit init;
  hostfp::icp_frame(P_m, P_init, M, init.C);
  launch_volume_icp_photo_init(sc.state, init, v->own);
  for (int l = 0; l < p->levels; l++) {
    const VolIcpPhotoRowsArgs ra = icp_photo_rows_args(v, f, M, p->stride[l], l, p->dist_max, p->huber_delta, ph, sc, nullptr);
    VolIcpPhotoStepArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.partials = sc.partials; sa.nblk = icp_blocks(v, p->stride[l]); sa.level = l;
    sa.min_pairs = p->min_pairs; sa.eps_t = p->eps_t; sa.eps_r = p->eps_r; sa.take_step = 1;
    sa.state = sc.state; sa.trace = sc.trace; sa.trace_capacity = trace_rows;
    for (int it = 0; it < p->iters[l]; it++) {
      launch_volume_icp_photo_rows(ra, v->own);
      launch_volume_icp_photo_step(sa, v->own);
    }
  }
  HIP_OK(hipGetLastError());
  IcpPhotoState st;
  HIP_OK(hipMemcpyAsync(&st, sc.state, sizeof(st), hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  const int n_rows = std::min(st.trace_n, trace_rows);
  if (n_rows > 0) {
    HIP_OK(hipMemcpyAsync(trace, sc.trace, sizeof(IcpPhotoTraceRow) * (size_t)n_rows, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipStreamSynchronize(v->own));
  }
  if (trace_n) *trace_n = n_rows;
  memset(out, 0, sizeof(*out));
  odo_icp_result* res = &out->icp;
  res->status = st.status;
  res->iterations = st.iterations;
  memcpy(res->C, st.C, sizeof(res->C));
  if (st.evaluated) {
    res->pairs = st.acc[28];
    res->cost = st.acc[27];
    out->photo_pairs = st.acc[29];
    out->photo_cost = st.acc[30];
    double ev[6];
    icp_eigenvalues(st.acc, ev);
    res->eig_min = ev[0];
    res->eig_max = ev[5];
  }
  if (res->status == 0 && !pose_finite(st.C)) res->status = 1;
  if (res->status == 0 && (!st.evaluated || res->eig_min < (double)p->min_eig_ratio * res->eig_max)) res->status = st.evaluated ? 2 : 1;
  if (res->status == 0) hostfp::mul4(P_m, st.C, abs_pose);
  else icp_nan_pose(abs_pose);
  return 0;
}

extern "C" int odo_volume_icp_photo_align_dev(odo_volume* v, const odo_icp_params* p, const odo_icp_photo_params* photo, const float* depth_m_dev,
                                              const float* nrmw_m_dev, const uint8_t* rgba_m_dev, const float model_pose_colmajor[16],
                                              const uint16_t* raw_dev, const float* grey_dev, const float init_pose_colmajor[16],
                                              float abs_pose_colmajor[16], odo_icp_photo_result* result, odo_icp_photo_trace_row* trace,
                                              int trace_capacity, int* trace_n) {
  const char* who = "odo_volume_icp_photo_align_dev";
  if (trace_n) *trace_n = 0;
  const IcpPhotoFrames f = {depth_m_dev, nrmw_m_dev, rgba_m_dev, raw_dev, grey_dev};
  if (!v || !p || !photo || !model_pose_colmajor || !init_pose_colmajor || !abs_pose_colmajor || !result) return fail("%s: NULL arg", who);
  if (trace_capacity < 0 || (trace && trace_capacity < 1)) return fail("%s: a trace buffer needs a capacity >= 1", who);
  if (icp_photo_frames_check(who, f, nullptr)) return -1;
  if (icp_check_params(who, p) || icp_photo_check(who, photo)) return -1;
  if (!pose_finite(model_pose_colmajor) || !pose_finite(init_pose_colmajor)) return fail("%s: a pose has a non-finite entry", who);
  HIP_OK(hipSetDevice(v->device));
  return icp_photo_align(v, p, photo, f, model_pose_colmajor, init_pose_colmajor, abs_pose_colmajor, result, trace, trace_capacity, trace_n);
}

extern "C" int odo_volume_track_photo_dev(odo_volume* v, const odo_icp_params* p, const odo_icp_photo_params* photo, const uint16_t* raw_dev,
                                          const float* grey_dev, const float prev_pose_colmajor[16], float abs_pose_colmajor[16],
                                          odo_icp_photo_result* result) {
  const char* who = "odo_volume_track_photo_dev";
  if (!v || !p || !photo || !raw_dev || !grey_dev || !prev_pose_colmajor || !abs_pose_colmajor || !result) return fail("%s: NULL arg", who);
  if (((uintptr_t)raw_dev & 1) || ((uintptr_t)grey_dev & 3)) return fail("%s: misaligned frame (raw 2, grey 4 bytes)", who);
  if (icp_check_params(who, p) || icp_photo_check(who, photo)) return -1;
  if (!pose_finite(prev_pose_colmajor)) return fail("%s: the pose has a non-finite entry (a frame whose Solve failed?)", who);
  if (!v->colour) return fail("%s: the volume has no colour grid (odo_volume_enable_colour first)", who);
  odo_raycast_params rp;
  rp.rows = v->p.rows; rp.cols = v->p.cols;
  rp.f = v->p.K.f0; rp.cx = v->p.K.cx0; rp.cy = v->p.K.cy0;
  const double step = (double)v->p.mu / 2;
  rp.t_min = 0.0f; rp.step = (float)step;
  rp.n_steps = (int)std::min(4096.0, std::max(1.0, std::ceil(((double)v->p.max_depth + (double)v->p.mu) / step) + 1.0));
  if (raycast_check(who, &rp, prev_pose_colmajor)) return -1;
  HIP_OK(hipSetDevice(v->device));
  if (volume_ray_frames(who, v, (long)rp.rows * rp.cols, true)) return -1;
  if (volume_raycast_launch(v, &rp, prev_pose_colmajor, v->d_ray_depth, nullptr, v->d_ray_nrmw, v->d_ray_rgba)) return -1;
  const IcpPhotoFrames f = {v->d_ray_depth, (const float*)v->d_ray_nrmw, (const uint8_t*)v->d_ray_rgba, raw_dev, grey_dev};
  return icp_photo_align(v, p, photo, f, prev_pose_colmajor, prev_pose_colmajor, abs_pose_colmajor, result, nullptr, 0, nullptr);
}
