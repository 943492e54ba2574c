// volume_icp_api.hip.h — frame-to-model tracking on the TSDF volume, geometric (odo_volume_icp_eval_dev, odo_volume_icp_align_dev,
// odo_volume_track_dev, odo_volume_icp_time_dev) and with the photometric term (odo_volume_icp_photo_eval_dev,
// odo_volume_icp_photo_align_dev, odo_volume_track_photo_dev, odo_volume_icp_photo_time_dev): the host side over the kernels of
// volume_icp_kernels.hip. Included by odometry_hip.hip behind volume_api.hip.h, whose object and helpers it uses and does not change.
//
// An entry point is its argument checks and a call into a body written once over the number of sums N (volume_icp.hip.h): the
// geometric path is N = ODO_NACC with no grey frame, no colour frame and no photometric parameters.
//
// The alignment's device memory (the state, one partial per block of the finest grid, the trace) lives for one call: allocated on
// entry, released after the call's single wait. A call costs three allocations beside its launches; the volume object stays as it is.
#pragma once
#include <cstddef>
#include <limits>
#include "volume_icp.hip.h"

static_assert(sizeof(odo_icp_trace_row) == sizeof(IcpTraceRow) && offsetof(odo_icp_trace_row, acc) == offsetof(IcpTraceRow, acc) &&
              offsetof(odo_icp_trace_row, delta) == offsetof(IcpTraceRow, delta) && offsetof(odo_icp_trace_row, C) == offsetof(IcpTraceRow, C),
              "odo_icp_trace_row is the device's IcpTraceRow");
static_assert(sizeof(odo_icp_photo_trace_row) == sizeof(IcpPhotoTraceRow) && offsetof(odo_icp_photo_trace_row, acc) == offsetof(IcpPhotoTraceRow, acc) &&
              offsetof(odo_icp_photo_trace_row, delta) == offsetof(IcpPhotoTraceRow, delta) &&
              offsetof(odo_icp_photo_trace_row, C) == offsetof(IcpPhotoTraceRow, C), "odo_icp_photo_trace_row is the device's IcpPhotoTraceRow");

template <int N>
struct IcpScratch {
  IcpStateT<N>* state = nullptr;
  double* partials = nullptr;
  IcpTraceRowT<N>* trace = nullptr;
  ~IcpScratch() {
    if (state) (void)hipFree(state);
    if (partials) (void)hipFree(partials);
    if (trace) (void)hipFree(trace);
  }
};

template <int N>
static int icp_alloc(IcpScratch<N>* sc, int max_blocks, int trace_rows) {
  if (hipMalloc((void**)&sc->state, sizeof(IcpStateT<N>)) != hipSuccess ||
      hipMalloc((void**)&sc->partials, sizeof(double) * N * (size_t)max_blocks) != hipSuccess ||
      (trace_rows > 0 && hipMalloc((void**)&sc->trace, sizeof(IcpTraceRowT<N>) * (size_t)trace_rows) != hipSuccess)) {
    (void)hipGetLastError();
    return fail("%s: device allocation failed (%d partials, %d trace rows)", N == ODO_NACC ? "odo_volume_icp" : "odo_volume_icp_photo", max_blocks,
                trace_rows);
  }
  return 0;
}

// The volume's own stream behind everything enqueued so far on the context's stream (the upload of the sensor frame) and behind
// everything that changed the volume.
static int icp_order(odo_volume* v) {
  hipEvent_t ev = nullptr;
  HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  const bool ok = hipEventRecord(ev, v->ctx->stream) == hipSuccess && hipStreamWaitEvent(v->own, ev, 0) == hipSuccess;
  (void)hipEventDestroy(ev);   // (released once it has completed)
  if (!ok) return fail("odo_volume_icp: ordering behind the context's stream failed");
  return volume_order_on(v, v->own);
}

static int icp_blocks(const odo_volume* v, int stride) {
  const dim3 g = volume_icp_grid(v->p.rows, v->p.cols, stride);
  return (int)(g.x * g.y);
}

static bool icp_float_ok(float x, bool positive) { return std::isfinite(x) && (positive ? x > 0.0f : x >= 0.0f); }

static int icp_check_params(const char* who, const odo_icp_params* p) {
  if (p->levels < 1 || p->levels > kIcpMaxLevels) return fail("%s: levels %d out of range (1 .. 3)", who, p->levels);
  long total = 0;
  for (int l = 0; l < p->levels; l++) {
    if (p->stride[l] < 1 || p->stride[l] > 16) return fail("%s: stride[%d] = %d out of range (1 .. 16)", who, l, p->stride[l]);
    if (p->iters[l] < 0 || p->iters[l] > 64) return fail("%s: iters[%d] = %d out of range (0 .. 64)", who, l, p->iters[l]);
    total += p->iters[l];
  }
  if (total < 1 || total > 64) return fail("%s: the iterations sum to %ld (1 .. 64)", who, total);
  if (!icp_float_ok(p->dist_max, true)) return fail("%s: dist_max must be finite and > 0", who);
  if (!icp_float_ok(p->huber_delta, false)) return fail("%s: huber_delta must be finite and >= 0", who);
  if (!icp_float_ok(p->eps_t, false) || !icp_float_ok(p->eps_r, false)) return fail("%s: eps_t and eps_r must be finite and >= 0", who);
  if (p->min_pairs < 6) return fail("%s: min_pairs %d (at least 6)", who, p->min_pairs);
  if (!(p->min_eig_ratio >= 0.0f && p->min_eig_ratio <= 1.0f)) return fail("%s: min_eig_ratio must lie in 0 .. 1", who);
  return 0;
}

static int icp_photo_check(const char* who, const odo_icp_photo_params* ph) {
  if (!icp_float_ok(ph->weight, true)) return fail("%s: the photometric weight must be finite and > 0", who);
  if (!icp_float_ok(ph->huber_delta, false)) return fail("%s: the photometric huber_delta must be finite and >= 0", who);
  return 0;
}

// The frames of one call: the model's three and the sensor's two. The geometric path has no rgba_m and no grey (nullptr).
struct IcpFrames {
  const float* depth_m;
  const float* nrmw_m;
  const uint8_t* rgba_m;
  const uint16_t* raw;
  const float* grey;
};

static int icp_photo_frames_check(const char* who, const IcpFrames& f, const float* rows_dev) {
  if (!f.depth_m || !f.nrmw_m || !f.rgba_m || !f.raw || !f.grey) return fail("%s: NULL arg", who);
  if (((uintptr_t)f.depth_m & 3) || ((uintptr_t)f.nrmw_m & 15) || ((uintptr_t)f.rgba_m & 3) || ((uintptr_t)f.raw & 1) ||
      ((uintptr_t)f.grey & 3) || ((uintptr_t)rows_dev & 15))
    return fail("%s: misaligned frame (grey 4, rgba 4, depth 4, nrmw 16, raw 2, rows 16 bytes)", who);
  return 0;
}

// What odo_volume_icp_photo_eval_dev and odo_volume_icp_photo_time_dev check alike.
static int icp_photo_eval_check(const char* who, const odo_volume* v, const IcpFrames& f, const float* P_m, const float* Cm, int stride,
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

// ph: the photometric parameters, nullptr for the geometric path.
template <int N>
static VolIcpRowsArgs<N> icp_rows_args(const odo_volume* v, const IcpFrames& f, const float* M, int stride, int level, float dist_max,
                                       float huber_delta, const odo_icp_photo_params* ph, const IcpScratch<N>& sc, float* rows_dev) {
  VolIcpRowsArgs<N> a;
  memset(&a, 0, sizeof(a));
  a.raw = f.raw; a.depth_m = f.depth_m; a.nrmw_m = f.nrmw_m;
  if constexpr (N == kIcpPhotoAcc) {
    a.grey = f.grey; a.rgba_m = (const uint32_t*)f.rgba_m;
    a.photo_weight = ph->weight; a.photo_huber = ph->huber_delta;
  }
  a.rows = v->p.rows; a.cols = v->p.cols;
  a.f = v->p.K.f0; a.cx = v->p.K.cx0; a.cy = v->p.K.cy0;
  a.depth_scale = v->p.depth_scale; a.max_depth = v->p.max_depth;
  a.dist_max = dist_max; a.huber_delta = huber_delta;
  a.m0 = M[0]; a.m1 = M[4]; a.m2 = M[8]; a.m3 = M[1]; a.m4 = M[5]; a.m5 = M[9]; a.m6 = M[2]; a.m7 = M[6]; a.m8 = M[10];
  a.stride = stride; a.level = level;
  a.state = sc.state; a.partials = sc.partials; a.rows_dev = rows_dev;
  return a;
}

// What one evaluation at C and its timing share: the scratch, the state's first value and the arguments of the rows kernel at the
// stride and of the step kernel's fold (take_step == 0: the state keeps its C). Every argument checked by the caller.
template <int N>
struct IcpEval {
  IcpScratch<N> sc;
  IcpInit init;
  VolIcpRowsArgs<N> rows;
  VolIcpStepArgs<N> fold;
};

template <int N>
static int icp_eval_prepare(IcpEval<N>* e, odo_volume* v, const IcpFrames& f, const float* P_m, const float* Cm, int stride, float dist_max,
                            float huber_delta, const odo_icp_photo_params* ph, float* rows_dev) {
  HIP_OK(hipSetDevice(v->device));
  const int nblk = icp_blocks(v, stride);
  if (icp_alloc(&e->sc, nblk, 0)) return -1;
  if (icp_order(v)) return -1;
  float M[16];
  hostfp::invert_rigid(P_m, M);
  memcpy(e->init.C, Cm, sizeof(e->init.C));
  e->rows = icp_rows_args(v, f, M, stride, 0, dist_max, huber_delta, ph, e->sc, rows_dev);
  memset(&e->fold, 0, sizeof(e->fold));
  e->fold.partials = e->sc.partials; e->fold.nblk = nblk; e->fold.state = e->sc.state;
  return 0;
}

template <int N>
static int icp_eval(odo_volume* v, const IcpFrames& f, const float* P_m, const float* Cm, int stride, float dist_max, float huber_delta,
                    const odo_icp_photo_params* ph, double* acc, float* rows_dev) {
  IcpEval<N> e;
  if (icp_eval_prepare(&e, v, f, P_m, Cm, stride, dist_max, huber_delta, ph, rows_dev)) return -1;
  launch_volume_icp_init(e.sc.state, e.init, v->own);
  launch_volume_icp_rows(e.rows, v->own);
  launch_volume_icp_step(e.fold, v->own);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(acc, (const char*)e.sc.state + offsetof(IcpStateT<N>, acc), sizeof(double) * N, hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  return 0;
}

// Event timing of the two kernels (tools/volume_cost.py icp [--photo]): `reps` launches of the rows kernel at C between two events
// on the volume's own stream, then `reps` launches of the step kernel's fold. us[0], us[1]: the mean time of one launch of either,
// microseconds.
template <int N>
static int icp_time(const char* who, odo_volume* v, const IcpFrames& f, const float* P_m, const float* Cm, int stride, float dist_max,
                    float huber_delta, const odo_icp_photo_params* ph, int reps, float us[2]) {
  IcpEval<N> e;
  if (icp_eval_prepare(&e, v, f, P_m, Cm, stride, dist_max, huber_delta, ph, nullptr)) return -1;
  const auto warm = [&]() {
    launch_volume_icp_init(e.sc.state, e.init, v->own);
    launch_volume_icp_rows(e.rows, v->own);
    launch_volume_icp_step(e.fold, v->own);
    return true;
  };
  const auto stage = [&](int q) {
    if (q == 0) launch_volume_icp_rows(e.rows, v->own);
    else launch_volume_icp_step(e.fold, v->own);
    return true;
  };
  return time_stages(who, v->own, reps, 2, us, warm, stage);
}

static void icp_nan_pose(float* A) {
  for (int i = 0; i < 16; i++) A[i] = std::numeric_limits<float>::quiet_NaN();
}

static odo_icp_result* icp_result_of(odo_icp_result* out) { return out; }
static odo_icp_result* icp_result_of(odo_icp_photo_result* out) { return &out->icp; }

// The launches and the single wait (two with a trace) of one alignment, every argument checked by the caller. Result and Trace are
// the public structs of the path: odo_icp_result / odo_icp_trace_row, or odo_icp_photo_result / odo_icp_photo_trace_row.
template <int N, class Result, class Trace>
static int icp_align(odo_volume* v, const odo_icp_params* p, const odo_icp_photo_params* ph, const IcpFrames& f, const float* P_m,
                     const float* P_init, float* abs_pose, Result* out, Trace* trace, int trace_capacity, int* trace_n) {
  static_assert(sizeof(Trace) == sizeof(IcpTraceRowT<N>), "the trace row of the path");
  int total = 0, max_blocks = 1;
  for (int l = 0; l < p->levels; l++) {
    total += p->iters[l];
    max_blocks = std::max(max_blocks, icp_blocks(v, p->stride[l]));
  }
  const int trace_rows = trace ? std::min(trace_capacity, total) : 0;
  IcpScratch<N> sc;
  if (icp_alloc(&sc, max_blocks, trace_rows)) return -1;
  if (icp_order(v)) return -1;
  float M[16];
  IcpInit init;
  hostfp::icp_frame(P_m, P_init, M, init.C);
  launch_volume_icp_init(sc.state, init, v->own);
  for (int l = 0; l < p->levels; l++) {
    const VolIcpRowsArgs<N> ra = icp_rows_args(v, f, M, p->stride[l], l, p->dist_max, p->huber_delta, ph, sc, nullptr);
    VolIcpStepArgs<N> sa;
    memset(&sa, 0, sizeof(sa));
    sa.partials = sc.partials; sa.nblk = icp_blocks(v, p->stride[l]); sa.level = l;
    sa.min_pairs = p->min_pairs; sa.eps_t = p->eps_t; sa.eps_r = p->eps_r; sa.take_step = 1;
    sa.state = sc.state; sa.trace = sc.trace; sa.trace_capacity = trace_rows;
    for (int it = 0; it < p->iters[l]; it++) {
      launch_volume_icp_rows(ra, v->own);
      launch_volume_icp_step(sa, v->own);
    }
  }
  HIP_OK(hipGetLastError());
  IcpStateT<N> st;
  HIP_OK(hipMemcpyAsync(&st, sc.state, sizeof(st), hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  const int n_rows = std::min(st.trace_n, trace_rows);
  if (n_rows > 0) {
    HIP_OK(hipMemcpyAsync(trace, sc.trace, sizeof(Trace) * (size_t)n_rows, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipStreamSynchronize(v->own));
  }
  if (trace_n) *trace_n = n_rows;
  memset(out, 0, sizeof(*out));
  odo_icp_result* res = icp_result_of(out);
  res->status = st.status;
  res->iterations = st.iterations;
  memcpy(res->C, st.C, sizeof(res->C));
  if (st.evaluated) {
    res->pairs = st.acc[28];
    res->cost = st.acc[27];
    if constexpr (N == kIcpPhotoAcc) {
      out->photo_pairs = st.acc[29];
      out->photo_cost = st.acc[30];
    }
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

// The model frames of a track: the ray-cast from the previous pose into the frames that the volume owns, with its colours if asked.
static int icp_track_raycast(const char* who, odo_volume* v, const float* prev_pose, bool colour) {
  odo_raycast_params rp;
  rp.rows = v->p.rows; rp.cols = v->p.cols;
  rp.f = v->p.K.f0; rp.cx = v->p.K.cx0; rp.cy = v->p.K.cy0;
  const double step = (double)v->p.mu / 2;
  rp.t_min = 0.0f; rp.step = (float)step;
  rp.n_steps = (int)std::min(4096.0, std::max(1.0, std::ceil(((double)v->p.max_depth + (double)v->p.mu) / step) + 1.0));
  if (raycast_check(who, &rp, prev_pose)) return -1;
  HIP_OK(hipSetDevice(v->device));
  if (volume_ray_frames(who, v, (long)rp.rows * rp.cols, colour)) return -1;
  return volume_raycast_launch(v, &rp, prev_pose, v->d_ray_depth, nullptr, v->d_ray_nrmw, colour ? v->d_ray_rgba : nullptr);
}

// ---- the geometric path -----------------------------------------------------------------------------------------------------------
extern "C" int odo_volume_icp_eval_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const float model_pose_colmajor[16],
                                       const uint16_t* raw_dev, const float C_colmajor[16], int stride, float dist_max, float huber_delta,
                                       double acc[29], float* rows_dev) {
  const char* who = "odo_volume_icp_eval_dev";
  if (!v || !depth_m_dev || !nrmw_m_dev || !model_pose_colmajor || !raw_dev || !C_colmajor || !acc) return fail("%s: NULL arg", who);
  if (((uintptr_t)depth_m_dev & 3) || ((uintptr_t)nrmw_m_dev & 15) || ((uintptr_t)raw_dev & 1) || ((uintptr_t)rows_dev & 15))
    return fail("%s: misaligned frame (depth 4, nrmw 16, raw 2, rows 16 bytes)", who);
  if (stride < 1 || stride > 16) return fail("%s: stride %d out of range (1 .. 16)", who, stride);
  if (!icp_float_ok(dist_max, true)) return fail("%s: dist_max must be finite and > 0", who);
  if (!icp_float_ok(huber_delta, false)) return fail("%s: huber_delta must be finite and >= 0", who);
  if (!pose_finite(model_pose_colmajor) || !pose_finite(C_colmajor)) return fail("%s: a pose has a non-finite entry", who);
  const IcpFrames f = {depth_m_dev, nrmw_m_dev, nullptr, raw_dev, nullptr};
  return icp_eval<ODO_NACC>(v, f, model_pose_colmajor, C_colmajor, stride, dist_max, huber_delta, nullptr, acc, rows_dev);
}

extern "C" int odo_volume_icp_time_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const float model_pose_colmajor[16],
                                       const uint16_t* raw_dev, const float C_colmajor[16], int stride, float dist_max, float huber_delta,
                                       int reps, float us[2]) {
  const char* who = "odo_volume_icp_time_dev";
  if (!v || !depth_m_dev || !nrmw_m_dev || !model_pose_colmajor || !raw_dev || !C_colmajor || !us) return fail("%s: NULL arg", who);
  if (((uintptr_t)depth_m_dev & 3) || ((uintptr_t)nrmw_m_dev & 15) || ((uintptr_t)raw_dev & 1))
    return fail("%s: misaligned frame (depth 4, nrmw 16, raw 2 bytes)", who);
  if (stride < 1 || stride > 16 || reps < 1 || reps > 10000) return fail("%s: stride 1 .. 16, reps 1 .. 10000", who);
  if (!icp_float_ok(dist_max, true) || !icp_float_ok(huber_delta, false)) return fail("%s: dist_max finite > 0, huber_delta finite >= 0", who);
  if (!pose_finite(model_pose_colmajor) || !pose_finite(C_colmajor)) return fail("%s: a pose has a non-finite entry", who);
  const IcpFrames f = {depth_m_dev, nrmw_m_dev, nullptr, raw_dev, nullptr};
  return icp_time<ODO_NACC>(who, v, f, model_pose_colmajor, C_colmajor, stride, dist_max, huber_delta, nullptr, reps, us);
}

extern "C" int odo_volume_icp_align_dev(odo_volume* v, const odo_icp_params* p, const float* depth_m_dev, const float* nrmw_m_dev,
                                        const float model_pose_colmajor[16], const uint16_t* raw_dev, const float init_pose_colmajor[16],
                                        float abs_pose_colmajor[16], odo_icp_result* result, odo_icp_trace_row* trace, int trace_capacity,
                                        int* trace_n) {
  const char* who = "odo_volume_icp_align_dev";
  if (trace_n) *trace_n = 0;
  if (!v || !p || !depth_m_dev || !nrmw_m_dev || !model_pose_colmajor || !raw_dev || !init_pose_colmajor || !abs_pose_colmajor || !result)
    return fail("%s: NULL arg", who);
  if (trace_capacity < 0 || (trace && trace_capacity < 1)) return fail("%s: a trace buffer needs a capacity >= 1", who);
  if (((uintptr_t)depth_m_dev & 3) || ((uintptr_t)nrmw_m_dev & 15) || ((uintptr_t)raw_dev & 1))
    return fail("%s: misaligned frame (depth 4, nrmw 16, raw 2 bytes)", who);
  if (icp_check_params(who, p)) return -1;
  if (!pose_finite(model_pose_colmajor) || !pose_finite(init_pose_colmajor)) return fail("%s: a pose has a non-finite entry", who);
  HIP_OK(hipSetDevice(v->device));
  const IcpFrames f = {depth_m_dev, nrmw_m_dev, nullptr, raw_dev, nullptr};
  return icp_align<ODO_NACC>(v, p, nullptr, f, model_pose_colmajor, init_pose_colmajor, abs_pose_colmajor, result, trace, trace_capacity, trace_n);
}

extern "C" int odo_volume_track_dev(odo_volume* v, const odo_icp_params* p, const uint16_t* raw_dev, const float prev_pose_colmajor[16],
                                    float abs_pose_colmajor[16], odo_icp_result* result) {
  const char* who = "odo_volume_track_dev";
  if (!v || !p || !raw_dev || !prev_pose_colmajor || !abs_pose_colmajor || !result) return fail("%s: NULL arg", who);
  if ((uintptr_t)raw_dev & 1) return fail("%s: misaligned frame (raw 2 bytes)", who);
  if (icp_check_params(who, p)) return -1;
  if (icp_track_raycast(who, v, prev_pose_colmajor, false)) return -1;
  const IcpFrames f = {v->d_ray_depth, (const float*)v->d_ray_nrmw, nullptr, raw_dev, nullptr};
  return icp_align<ODO_NACC>(v, p, nullptr, f, prev_pose_colmajor, prev_pose_colmajor, abs_pose_colmajor, result, (odo_icp_trace_row*)nullptr, 0,
                             nullptr);
}

// ---- with the photometric term ----------------------------------------------------------------------------------------------------
extern "C" int odo_volume_icp_photo_eval_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const uint8_t* rgba_m_dev,
                                             const float model_pose_colmajor[16], const uint16_t* raw_dev, const float* grey_dev,
                                             const float C_colmajor[16], int stride, float dist_max, float huber_delta,
                                             const odo_icp_photo_params* photo, double acc[31], float* rows_dev) {
  const char* who = "odo_volume_icp_photo_eval_dev";
  const IcpFrames f = {depth_m_dev, nrmw_m_dev, rgba_m_dev, raw_dev, grey_dev};
  if (!acc) return fail("%s: NULL arg", who);
  if (icp_photo_eval_check(who, v, f, model_pose_colmajor, C_colmajor, stride, dist_max, huber_delta, photo, rows_dev)) return -1;
  return icp_eval<kIcpPhotoAcc>(v, f, model_pose_colmajor, C_colmajor, stride, dist_max, huber_delta, photo, acc, rows_dev);
}

extern "C" int odo_volume_icp_photo_time_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const uint8_t* rgba_m_dev,
                                             const float model_pose_colmajor[16], const uint16_t* raw_dev, const float* grey_dev,
                                             const float C_colmajor[16], int stride, float dist_max, float huber_delta,
                                             const odo_icp_photo_params* photo, int reps, float us[2]) {
  const char* who = "odo_volume_icp_photo_time_dev";
  const IcpFrames f = {depth_m_dev, nrmw_m_dev, rgba_m_dev, raw_dev, grey_dev};
  if (!us) return fail("%s: NULL arg", who);
  if (icp_photo_eval_check(who, v, f, model_pose_colmajor, C_colmajor, stride, dist_max, huber_delta, photo, nullptr)) return -1;
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  return icp_time<kIcpPhotoAcc>(who, v, f, model_pose_colmajor, C_colmajor, stride, dist_max, huber_delta, photo, reps, us);
}

extern "C" int odo_volume_icp_photo_align_dev(odo_volume* v, const odo_icp_params* p, const odo_icp_photo_params* photo, const float* depth_m_dev,
                                              const float* nrmw_m_dev, const uint8_t* rgba_m_dev, const float model_pose_colmajor[16],
                                              const uint16_t* raw_dev, const float* grey_dev, const float init_pose_colmajor[16],
                                              float abs_pose_colmajor[16], odo_icp_photo_result* result, odo_icp_photo_trace_row* trace,
                                              int trace_capacity, int* trace_n) {
  const char* who = "odo_volume_icp_photo_align_dev";
  if (trace_n) *trace_n = 0;
  const IcpFrames f = {depth_m_dev, nrmw_m_dev, rgba_m_dev, raw_dev, grey_dev};
  if (!v || !p || !photo || !model_pose_colmajor || !init_pose_colmajor || !abs_pose_colmajor || !result) return fail("%s: NULL arg", who);
  if (trace_capacity < 0 || (trace && trace_capacity < 1)) return fail("%s: a trace buffer needs a capacity >= 1", who);
  if (icp_photo_frames_check(who, f, nullptr)) return -1;
  if (icp_check_params(who, p) || icp_photo_check(who, photo)) return -1;
  if (!pose_finite(model_pose_colmajor) || !pose_finite(init_pose_colmajor)) return fail("%s: a pose has a non-finite entry", who);
  HIP_OK(hipSetDevice(v->device));
  return icp_align<kIcpPhotoAcc>(v, p, photo, f, model_pose_colmajor, init_pose_colmajor, abs_pose_colmajor, result, trace, trace_capacity, trace_n);
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
  if (icp_track_raycast(who, v, prev_pose_colmajor, true)) return -1;
  const IcpFrames f = {v->d_ray_depth, (const float*)v->d_ray_nrmw, (const uint8_t*)v->d_ray_rgba, raw_dev, grey_dev};
  return icp_align<kIcpPhotoAcc>(v, p, photo, f, prev_pose_colmajor, prev_pose_colmajor, abs_pose_colmajor, result,
                                 (odo_icp_photo_trace_row*)nullptr, 0, nullptr);
}
