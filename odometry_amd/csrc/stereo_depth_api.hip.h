// stereo_depth_api.hip.h — the dense stereo matcher (odo_stereo_depth_*): the host object over the kernels of
// stereo_depth_kernels.hip. A rectified pair of fp32 grey frames on the device in, a uint16 depth frame out, three launches on the
// CONTEXT's stream: whatever the caller enqueues on that stream afterwards (odo_dev_download, odo_volume_integrate_dev of a volume
// created on the same context) is ordered behind them without a host wait; a tracker reads its depth frame on a stream of its own and
// is not. With the semi-global mode on (odo_stereo_depth_enable_sgm; stereo_sgm.hip.h) a run is census, cost, one launch per path
// and two selections instead, on the same stream and with the same outputs. Included by odometry_hip.hip.
#pragma once
#include "stereo_depth.hip.h"
#include "stereo_sgm.hip.h"

struct odo_stereo_depth {
  odo_ctx* ctx;
  int device;
  odo_stereo_depth_params p;
  int blocks;              // workgroups of the left match launch = rows of `d_partials`
  uint64_t* d_census;      // the left plane, then the right one: rows * cols words each
  uint8_t* d_dr;           // rows * cols
  uint16_t* d_q;           // rows * cols, zero until the first run
  uint16_t* d_depth;       // the internal depth frame, zero until the first run that uses it
  uint32_t* d_partials;    // [blocks][kSdStatWords], zero until the first run
  odo_speckle* speckle;    // odo_stereo_depth_enable_speckle: the filter every run enqueues behind the left match, or NULL
  int sgm_paths, sgm_p1, sgm_p2;   // odo_stereo_depth_enable_sgm: 4 or 8 paths and the penalties; 0 = the box matcher
  uint16_t* d_sgm_c;       // [rows][cols][D] while the semi-global mode is on, else NULL
  uint16_t* d_sgm_s;
};

static SdArgs sd_args(const odo_stereo_depth* s, const float* left, const float* right, uint16_t* out) {
  SdArgs a;
  memset(&a, 0, sizeof(a));
  const size_t n = (size_t)s->p.rows * s->p.cols;
  a.left = left; a.right = right; a.cl = s->d_census; a.cr = s->d_census + n; a.dr = s->d_dr;
  a.depth = out ? out : s->d_depth; a.q = s->d_q; a.partials = s->d_partials;
  a.rows = s->p.rows; a.cols = s->p.cols;
  a.r.dmin = s->p.dmin; a.r.dmax = s->p.dmax; a.r.A = s->p.agg_radius; a.r.uniq = s->p.uniqueness; a.r.lr_max = s->p.lr_max;
  a.r.max_raw = s->p.max_raw; a.r.k = sd_k(s->p.fx, s->p.baseline, s->p.depth_scale);
  return a;
}

static void sd_free(odo_stereo_depth* s) {
  if (s->d_census) (void)hipFree(s->d_census);
  if (s->d_dr) (void)hipFree(s->d_dr);
  if (s->d_q) (void)hipFree(s->d_q);
  if (s->d_depth) (void)hipFree(s->d_depth);
  if (s->d_partials) (void)hipFree(s->d_partials);
  if (s->d_sgm_c) (void)hipFree(s->d_sgm_c);
  if (s->d_sgm_s) (void)hipFree(s->d_sgm_s);
}

static SgmArgs sgm_args(const odo_stereo_depth* s, const SdArgs& a) {
  SgmArgs g;
  g.sd = a; g.C = s->d_sgm_c; g.S = s->d_sgm_s; g.p1 = s->sgm_p1; g.p2 = s->sgm_p2; g.paths = s->sgm_paths;
  return g;
}

// The semi-global mode's run in five groups, each enqueued on st: 0 census, 1 cost, 2 every path launch, 3 right selection, 4 left
// selection and outputs.
static void sgm_launch_group(const SgmArgs& g, int group, hipStream_t st) {
  switch (group) {
    case 0: launch_stereo_depth_stage(g.sd, 0, st); break;
    case 1: launch_sgm_cost(g, st); break;
    case 2: launch_sgm_paths(g, st); break;
    case 3: launch_sgm_select(g, true, st); break;
    default: launch_sgm_select(g, false, st); break;
  }
}
constexpr int kSgmGroups = 5;

extern "C" int odo_stereo_depth_create(odo_ctx* ctx, const odo_stereo_depth_params* p, odo_stereo_depth** out) {
  const char* who = "odo_stereo_depth_create";
  if (!ctx || !p || !out) return fail("%s: NULL arg", who);
  switch (sd_check_params(p->rows, p->cols, p->dmin, p->dmax, p->agg_radius, p->uniqueness, p->lr_max, p->max_raw, p->fx, p->baseline,
                          p->depth_scale)) {
    case 0: break;
    case 1: return fail("%s: bad size %dx%d (1 .. %d each)", who, p->cols, p->rows, kSdMaxSize);
    case 2: return fail("%s: dmin %d must be at least 1", who, p->dmin);
    case 3: return fail("%s: dmax %d out of range (dmin + 2 .. %d)", who, p->dmax, kSdMaxDisp);
    case 4: return fail("%s: agg_radius %d out of range (0 .. %d)", who, p->agg_radius, kSdMaxAgg);
    case 5: return fail("%s: uniqueness %d out of range (0 .. 99 percent)", who, p->uniqueness);
    case 6: return fail("%s: lr_max %d must be >= 0, or -1 for no left-right check", who, p->lr_max);
    case 7: return fail("%s: max_raw %d out of range (1 .. 65535)", who, p->max_raw);
    default: return fail("%s: 16 * fx * baseline * depth_scale must be a finite positive float", who);
  }
  HIP_OK(hipSetDevice(ctx->device));
  odo_stereo_depth* s = new (std::nothrow) odo_stereo_depth();
  if (!s) return fail("out of memory");
  memset((void*)s, 0, sizeof(*s));
  s->ctx = ctx; s->device = ctx->device; s->p = *p;
  s->blocks = sd_blocks_x(p->cols) * sd_blocks_y(p->rows);
  const size_t n = (size_t)p->rows * p->cols, pbytes = sizeof(uint32_t) * kSdStatWords * (size_t)s->blocks;
  const bool ok = hipMalloc((void**)&s->d_census, 2 * sizeof(uint64_t) * n) == hipSuccess && hipMalloc((void**)&s->d_dr, n) == hipSuccess &&
                  hipMalloc((void**)&s->d_q, sizeof(uint16_t) * n) == hipSuccess &&
                  hipMalloc((void**)&s->d_depth, sizeof(uint16_t) * n) == hipSuccess &&
                  hipMalloc((void**)&s->d_partials, pbytes) == hipSuccess &&
                  hipMemsetAsync(s->d_q, 0, sizeof(uint16_t) * n, ctx->stream) == hipSuccess &&
                  hipMemsetAsync(s->d_depth, 0, sizeof(uint16_t) * n, ctx->stream) == hipSuccess &&
                  hipMemsetAsync(s->d_partials, 0, pbytes, ctx->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(ctx->stream);
    sd_free(s);
    delete s;
    return fail("%s: device allocation failed (%dx%d)", who, p->cols, p->rows);
  }
  *out = s;
  return 0;
}

// NULL or misaligned frames, or an output that shares a byte with an input: -1 and nothing enqueued.
static int sd_check_frames(const char* who, const odo_stereo_depth* s, const float* left, const float* right, const uint16_t* out) {
  if (!s || !left || !right) return fail("%s: NULL arg", who);
  if ((((uintptr_t)left | (uintptr_t)right) & 3) || ((uintptr_t)out & 1)) return fail("%s: misaligned frame", who);
  if (out) {
    const uintptr_t n = (uintptr_t)s->p.rows * s->p.cols, o0 = (uintptr_t)out;
    const float* ins[2] = {left, right};
    for (const float* in : ins) {
      const uintptr_t i0 = (uintptr_t)in;
      if (i0 < o0 + sizeof(uint16_t) * n && o0 < i0 + sizeof(float) * n) return fail("%s: the output overlaps an input frame", who);
    }
  }
  return 0;
}

extern "C" int odo_stereo_depth_run_dev(odo_stereo_depth* s, const float* left_dev, const float* right_dev, uint16_t* out_depth_dev) {
  if (sd_check_frames("odo_stereo_depth_run_dev", s, left_dev, right_dev, out_depth_dev)) return -1;
  HIP_OK(hipSetDevice(s->device));
  const SdArgs a = sd_args(s, left_dev, right_dev, out_depth_dev);
  if (s->sgm_paths) {
    const SgmArgs g = sgm_args(s, a);
    for (int group = 0; group < kSgmGroups; group++) sgm_launch_group(g, group, s->ctx->stream);
  } else {
    for (int stage = 0; stage < 3; stage++) launch_stereo_depth_stage(a, stage, s->ctx->stream);
  }
  HIP_OK(hipGetLastError());
  if (s->speckle) return sp_enqueue(s->speckle, sp_args(s->speckle, a.q, a.q, a.depth));
  return 0;
}

// The speckle filter behind every later run: the key is the q frame, the targets are the q frame and the run's depth output.
// min_size == 0 takes it off again. The bounds are odo_speckle_create's.
extern "C" int odo_stereo_depth_enable_speckle(odo_stereo_depth* s, int max_diff, int min_size) {
  if (!s) return fail("odo_stereo_depth_enable_speckle: NULL arg");
  odo_speckle* f = nullptr;
  if (min_size != 0) {
    odo_speckle_params p;
    p.rows = s->p.rows; p.cols = s->p.cols; p.max_diff = max_diff; p.min_size = min_size;
    if (odo_speckle_create(s->ctx, &p, &f)) return -1;
  }
  if (s->speckle) (void)odo_speckle_destroy(s->speckle);   // (waits for the runs that use it)
  s->speckle = f;
  return 0;
}

extern "C" int odo_stereo_depth_speckle_stats(odo_stereo_depth* s, long out[8]) {
  if (!s || !out) return fail("odo_stereo_depth_speckle_stats: NULL arg");
  if (!s->speckle) return fail("odo_stereo_depth_speckle_stats: no speckle filter is enabled (odo_stereo_depth_enable_speckle)");
  return odo_speckle_stats(s->speckle, out);
}

extern "C" int odo_stereo_depth_disparity_dev(odo_stereo_depth* s, const uint16_t** q_dev) {
  if (!s || !q_dev) return fail("odo_stereo_depth_disparity_dev: NULL arg");
  *q_dev = s->d_q;
  return 0;
}

extern "C" int odo_stereo_depth_depth_dev(odo_stereo_depth* s, const uint16_t** depth_dev) {
  if (!s || !depth_dev) return fail("odo_stereo_depth_depth_dev: NULL arg");
  *depth_dev = s->d_depth;
  return 0;
}

extern "C" int odo_stereo_depth_stats(odo_stereo_depth* s, long out[8]) {
  if (!s || !out) return fail("odo_stereo_depth_stats: NULL arg");
  HIP_OK(hipSetDevice(s->device));
  std::vector<uint32_t> rows;
  try { rows.resize((size_t)kSdStatWords * s->blocks); } catch (...) { return fail("out of memory"); }
  HIP_OK(hipMemcpyAsync(rows.data(), s->d_partials, sizeof(uint32_t) * rows.size(), hipMemcpyDeviceToHost, s->ctx->stream));
  HIP_OK(hipStreamSynchronize(s->ctx->stream));
  unsigned long long sum[6] = {0, 0, 0, 0, 0, 0};
  for (int b = 0; b < s->blocks; b++)   // in block order
    for (int k = 0; k < 6; k++) sum[k] += rows[(size_t)kSdStatWords * b + k];
  for (int k = 0; k < 5; k++) out[k] = (long)sum[k];
  out[5] = (long)(sum[5] & 0xffffffffull);
  out[6] = (long)(sum[5] >> 32);
  out[7] = 0;
  return 0;
}

// Event timing (tools/stereo_depth_cost.py): one run to warm, then for each of the three kernels `reps` launches between two events on
// the context's stream; us[0 .. 2] the mean time of one census / right match / left match launch in microseconds. The outputs and the
// statistics hold the result of one run afterwards.
extern "C" int odo_stereo_depth_time_dev(odo_stereo_depth* s, const float* left_dev, const float* right_dev, uint16_t* out_depth_dev,
                                         int reps, float us[3]) {
  const char* who = "odo_stereo_depth_time_dev";
  if (!us) return fail("%s: NULL arg", who);
  if (sd_check_frames(who, s, left_dev, right_dev, out_depth_dev)) return -1;
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  if (s->sgm_paths) return fail("%s: the semi-global mode is on; its launches are timed by odo_stereo_depth_sgm_time_dev", who);
  HIP_OK(hipSetDevice(s->device));
  const SdArgs a = sd_args(s, left_dev, right_dev, out_depth_dev);
  hipStream_t st = s->ctx->stream;
  const auto warm = [&]() { for (int q = 0; q < 3; q++) launch_stereo_depth_stage(a, q, st); return true; };
  float t[3] = {0.0f, 0.0f, 0.0f};
  if (time_stages(who, st, reps, 3, t, warm, [&](int q) { launch_stereo_depth_stage(a, q, st); return true; })) return -1;
  for (int q = 0; q < 3; q++) us[q] = t[q];
  if (s->speckle) return sp_enqueue(s->speckle, sp_args(s->speckle, a.q, a.q, a.depth));
  return 0;
}

// ---- the semi-global mode (stereo_sgm_math.h) ------------------------------------------------------------
static int sgm_refuse(const char* who, int bound, int p1, int p2, int paths, int A) {
  switch (bound) {
    case 1: return fail("%s: penalties P1 %d, P2 %d must satisfy 1 <= P1 <= P2", who, p1, p2);
    case 2: return fail("%s: paths %d must be 4 or 8 (0 takes the mode off)", who, paths);
    case 3: return fail("%s: paths * (62 * (2 A + 1)^2 + P2) = %lld exceeds %d at agg_radius %d: an aggregate must fit uint16", who,
                        (long long)paths * (62LL * (2 * A + 1) * (2 * A + 1) + p2), kSgmMaxSum, A);
    default: return fail("%s: rows * cols * (dmax - dmin + 1) exceeds 2^30 entries a volume", who);
  }
}

extern "C" int odo_stereo_depth_enable_sgm(odo_stereo_depth* s, int p1, int p2, int paths) {
  const char* who = "odo_stereo_depth_enable_sgm";
  if (!s) return fail("%s: NULL arg", who);
  if (paths != 0) {   // what the arguments alone decide (the weakest case of each bound), before the matcher is read
    const int bound = sgm_check_params(1, 1, 1, 3, 0, p1, p2, paths);
    if (bound) return sgm_refuse(who, bound, p1, p2, paths, 0);
    const int full = sgm_check_params(s->p.rows, s->p.cols, s->p.dmin, s->p.dmax, s->p.agg_radius, p1, p2, paths);
    if (full) return sgm_refuse(who, full, p1, p2, paths, s->p.agg_radius);
  }
  HIP_OK(hipSetDevice(s->device));
  if (paths == 0) {
    if (s->d_sgm_c || s->d_sgm_s) {
      HIP_OK(hipStreamSynchronize(s->ctx->stream));   // a run in flight reads and writes the volumes
      (void)hipFree(s->d_sgm_c);
      (void)hipFree(s->d_sgm_s);
    }
    s->d_sgm_c = s->d_sgm_s = nullptr;
    s->sgm_paths = s->sgm_p1 = s->sgm_p2 = 0;
    return 0;
  }
  if (!s->d_sgm_c) {   // (the volumes' size is the matcher's: a change of penalties or paths keeps them)
    const size_t bytes = sizeof(uint16_t) * (size_t)s->p.rows * s->p.cols * (size_t)(s->p.dmax - s->p.dmin + 1);
    uint16_t *c = nullptr, *v = nullptr;
    if (hipMalloc((void**)&c, bytes) != hipSuccess || hipMalloc((void**)&v, bytes) != hipSuccess ||
        hipMemsetAsync(v, 0xFF, bytes, s->ctx->stream) != hipSuccess) {   // (S reads "inadmissible" until the first run)
      (void)hipGetLastError();
      if (c) (void)hipFree(c);
      if (v) (void)hipFree(v);
      return fail("%s: device allocation failed (two volumes of %zu bytes)", who, bytes);
    }
    s->d_sgm_c = c; s->d_sgm_s = v;
  }
  s->sgm_paths = paths; s->sgm_p1 = p1; s->sgm_p2 = p2;
  return 0;
}

// Event timing of the semi-global run (tools/stereo_sgm_cost.py): one run to warm, then each of the five groups `reps` times between
// two events; us[0 .. 4] the mean time of census / cost / all path launches / right selection / left selection in microseconds.
extern "C" int odo_stereo_depth_sgm_time_dev(odo_stereo_depth* s, const float* left_dev, const float* right_dev, uint16_t* out_depth_dev,
                                             int reps, float us[5]) {
  const char* who = "odo_stereo_depth_sgm_time_dev";
  if (!us) return fail("%s: NULL arg", who);
  if (sd_check_frames(who, s, left_dev, right_dev, out_depth_dev)) return -1;
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  if (!s->sgm_paths) return fail("%s: the semi-global mode is off (odo_stereo_depth_enable_sgm)", who);
  HIP_OK(hipSetDevice(s->device));
  const SgmArgs g = sgm_args(s, sd_args(s, left_dev, right_dev, out_depth_dev));
  hipStream_t st = s->ctx->stream;
  const auto warm = [&]() { for (int q = 0; q < kSgmGroups; q++) sgm_launch_group(g, q, st); return true; };
  float t[kSgmGroups] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (time_stages(who, st, reps, kSgmGroups, t, warm, [&](int q) { sgm_launch_group(g, q, st); return true; })) return -1;
  for (int q = 0; q < kSgmGroups; q++) us[q] = t[q];
  if (s->speckle) return sp_enqueue(s->speckle, sp_args(s->speckle, g.sd.q, g.sd.q, g.sd.depth));
  return 0;
}

extern "C" int odo_debug_sgm_volume(odo_stereo_depth* s, uint16_t* host_out) {
  const char* who = "odo_debug_sgm_volume";
  if (!s || !host_out) return fail("%s: NULL arg", who);
  if (!s->sgm_paths) return fail("%s: the semi-global mode is off (odo_stereo_depth_enable_sgm)", who);
  HIP_OK(hipSetDevice(s->device));
  const size_t bytes = sizeof(uint16_t) * (size_t)s->p.rows * s->p.cols * (size_t)(s->p.dmax - s->p.dmin + 1);
  HIP_OK(hipMemcpyAsync(host_out, s->d_sgm_s, bytes, hipMemcpyDeviceToHost, s->ctx->stream));
  HIP_OK(hipStreamSynchronize(s->ctx->stream));
  return 0;
}

extern "C" int odo_stereo_depth_destroy(odo_stereo_depth* s) {
  if (!s) return 0;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->ctx->stream);   // a run in flight reads and writes every block below
  if (s->speckle) (void)odo_speckle_destroy(s->speckle);
  sd_free(s);
  delete s;
  return 0;
}
