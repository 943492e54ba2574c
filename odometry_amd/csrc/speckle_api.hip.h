// speckle_api.hip.h — the speckle filter (odo_speckle_*): the host object over the kernels of speckle_kernels.hip. A uint16 key frame
// on the device in, up to two uint16 target frames filtered in place, four launches on the CONTEXT's stream and no host wait: the
// ordering rules are those of the depth filter and the stereo matcher (depth_filter_api.hip.h). Included by odometry_hip.hip in
// front of stereo_depth_api.hip.h, whose matcher can own one (odo_stereo_depth_enable_speckle).
#pragma once
#include "speckle.hip.h"

struct odo_speckle {
  odo_ctx* ctx;
  int device;
  odo_speckle_params p;
  int blocks;              // workgroups of the label and apply launches = rows of `d_partials`
  int32_t* d_parent;       // rows * cols
  int32_t* d_size;         // rows * cols
  uint32_t* d_partials;    // [blocks + 1][kSpStatWords], zero until the first run; the last row's first word is the guard
};

static SpArgs sp_args(const odo_speckle* s, const uint16_t* key, uint16_t* a, uint16_t* b) {
  SpArgs r;
  memset(&r, 0, sizeof(r));
  r.key = key; r.a = a; r.b = b; r.parent = s->d_parent; r.size = s->d_size; r.partials = s->d_partials;
  r.guard = s->d_partials + (size_t)kSpStatWords * s->blocks;
  r.rows = s->p.rows; r.cols = s->p.cols; r.max_diff = s->p.max_diff; r.min_size = s->p.min_size;
  return r;
}

static void sp_free(odo_speckle* s) {
  if (s->d_parent) (void)hipFree(s->d_parent);
  if (s->d_size) (void)hipFree(s->d_size);
  if (s->d_partials) (void)hipFree(s->d_partials);
}

extern "C" int odo_speckle_create(odo_ctx* ctx, const odo_speckle_params* p, odo_speckle** out) {
  const char* who = "odo_speckle_create";
  if (!ctx || !p || !out) return fail("%s: NULL arg", who);
  switch (sp_check_params(p->rows, p->cols, p->max_diff, p->min_size)) {
    case 0: break;
    case 1: return fail("%s: bad size %dx%d (1 .. %d each)", who, p->cols, p->rows, kSpMaxSize);
    case 2: return fail("%s: max_diff %d out of range (0 .. %d)", who, p->max_diff, kSpMaxDiff);
    default: return fail("%s: min_size %d out of range (1 .. %d)", who, p->min_size, kSpMaxMinSize);
  }
  HIP_OK(hipSetDevice(ctx->device));
  odo_speckle* s = new (std::nothrow) odo_speckle();
  if (!s) return fail("out of memory");
  memset((void*)s, 0, sizeof(*s));
  s->ctx = ctx; s->device = ctx->device; s->p = *p;
  s->blocks = sp_blocks_x(p->cols) * sp_blocks_y(p->rows);
  const size_t n = (size_t)p->rows * p->cols, pbytes = sizeof(uint32_t) * kSpStatWords * ((size_t)s->blocks + 1);
  const bool ok = hipMalloc((void**)&s->d_parent, sizeof(int32_t) * n) == hipSuccess &&
                  hipMalloc((void**)&s->d_size, sizeof(int32_t) * n) == hipSuccess &&
                  hipMalloc((void**)&s->d_partials, pbytes) == hipSuccess &&
                  hipMemsetAsync(s->d_partials, 0, pbytes, ctx->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(ctx->stream);
    sp_free(s);
    delete s;
    return fail("%s: device allocation failed (%dx%d)", who, p->cols, p->rows);
  }
  *out = s;
  return 0;
}

// NULL or misaligned frames, or two different targets that share a byte: -1 and nothing enqueued. A target may be the key frame.
static int sp_check_frames(const char* who, const odo_speckle* s, const uint16_t* key, const uint16_t* a, const uint16_t* b) {
  if (!s || !key || !a) return fail("%s: NULL arg", who);
  if (((uintptr_t)key | (uintptr_t)a | (uintptr_t)b) & 1) return fail("%s: misaligned frame", who);
  if (b && b != a) {
    const uintptr_t bytes = sizeof(uint16_t) * (uintptr_t)s->p.rows * s->p.cols, a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    if (a0 < b0 + bytes && b0 < a0 + bytes) return fail("%s: the two targets overlap", who);
  }
  return 0;
}

// One run's enqueues on the context's stream: the guard word cleared, then the four stages.
static int sp_enqueue(const odo_speckle* s, const SpArgs& a) {
  HIP_OK(hipMemsetAsync(a.guard, 0, sizeof(uint32_t), s->ctx->stream));
  for (int stage = 0; stage < kSpStages; stage++) launch_speckle_stage(a, stage, s->ctx->stream);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int odo_speckle_run_dev(odo_speckle* s, const uint16_t* key_dev, uint16_t* target_a_dev, uint16_t* target_b_dev) {
  if (sp_check_frames("odo_speckle_run_dev", s, key_dev, target_a_dev, target_b_dev)) return -1;
  HIP_OK(hipSetDevice(s->device));
  return sp_enqueue(s, sp_args(s, key_dev, target_a_dev, target_b_dev));
}

extern "C" int odo_speckle_stats(odo_speckle* s, long out[8]) {
  if (!s || !out) return fail("odo_speckle_stats: NULL arg");
  HIP_OK(hipSetDevice(s->device));
  std::vector<uint32_t> rows;
  try { rows.resize((size_t)kSpStatWords * (s->blocks + 1)); } catch (...) { return fail("out of memory"); }
  HIP_OK(hipMemcpyAsync(rows.data(), s->d_partials, sizeof(uint32_t) * rows.size(), hipMemcpyDeviceToHost, s->ctx->stream));
  HIP_OK(hipStreamSynchronize(s->ctx->stream));
  long long sum[4] = {0, 0, 0, 0};
  uint32_t largest = 0;
  for (int b = 0; b < s->blocks; b++) {   // in block order
    for (int k = 0; k < 4; k++) sum[k] += rows[(size_t)kSpStatWords * b + k];
    const uint32_t m = rows[(size_t)kSpStatWords * b + 4];
    largest = m > largest ? m : largest;
  }
  for (int k = 0; k < 4; k++) out[k] = (long)sum[k];
  out[4] = (long)largest;
  out[5] = (long)rows[(size_t)kSpStatWords * s->blocks];
  out[6] = out[7] = 0;
  return 0;
}

// Event timing (tools/speckle_cost.py). Kernels two to four are not repeatable on their own — a second count launch would add every
// count again — but every PREFIX of a run is, because the label launch rewrites both planes. So the timed stage q is the run's first
// q + 1 launches, `reps` of them between two events, on scratch copies of the key and of a target (a key that is its own target would
// change under the repeats); us[q] = that prefix's mean minus the one before, us[4] = the whole run. Then one run on the caller's
// frames: they and the statistics hold exactly one run's result afterwards.
extern "C" int odo_speckle_time_dev(odo_speckle* s, const uint16_t* key_dev, uint16_t* target_a_dev, uint16_t* target_b_dev, int reps,
                                    float us[5]) {
  const char* who = "odo_speckle_time_dev";
  if (!us) return fail("%s: NULL arg", who);
  if (sp_check_frames(who, s, key_dev, target_a_dev, target_b_dev)) return -1;
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  HIP_OK(hipSetDevice(s->device));
  hipStream_t st = s->ctx->stream;
  const size_t bytes = sizeof(uint16_t) * (size_t)s->p.rows * s->p.cols;
  uint16_t* scratch = nullptr;   // the key's copy, then a target
  if (hipMalloc((void**)&scratch, 2 * bytes) != hipSuccess) { (void)hipGetLastError(); return fail("%s: device allocation failed", who); }
  uint16_t* target = scratch + (size_t)s->p.rows * s->p.cols;
  float t[kSpStages] = {0.0f, 0.0f, 0.0f, 0.0f};
  int rc = -1;
  if (hipMemcpyAsync(scratch, key_dev, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess &&
      hipMemcpyAsync(target, target_a_dev, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess) {
    const SpArgs a = sp_args(s, scratch, target, target_b_dev ? target : nullptr);
    const auto prefix = [&](int q) { for (int k = 0; k <= q; k++) launch_speckle_stage(a, k, st); return true; };
    rc = time_stages(who, st, reps, kSpStages, t, [&]() { return prefix(kSpStages - 1); }, prefix);
  } else {
    (void)hipGetLastError();
    (void)fail("%s: copy failed", who);
  }
  (void)hipStreamSynchronize(st);
  (void)hipFree(scratch);
  if (rc) return -1;
  if (sp_enqueue(s, sp_args(s, key_dev, target_a_dev, target_b_dev))) return -1;
  HIP_OK(hipStreamSynchronize(st));
  us[0] = t[0];
  for (int q = 1; q < kSpStages; q++) us[q] = t[q] - t[q - 1];
  us[4] = t[kSpStages - 1];
  return 0;
}

extern "C" int odo_speckle_destroy(odo_speckle* s) {
  if (!s) return 0;
  (void)hipSetDevice(s->device);
  (void)hipStreamSynchronize(s->ctx->stream);   // a run in flight reads and writes every block below
  sp_free(s);
  delete s;
  return 0;
}
