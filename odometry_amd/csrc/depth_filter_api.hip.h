// depth_filter_api.hip.h — the bilateral depth filter (odo_depth_filter_*): the host object over the kernel of
// depth_filter_kernels.hip. A uint16 sensor depth frame on the device in, the filtered frame out, one launch on the CONTEXT's stream:
// whatever the caller enqueues on that stream afterwards (odo_dev_download, odo_volume_integrate_dev of a volume created on the same
// context) is ordered behind it without a host wait; a tracker reads its depth frame on a stream of its own and is not.
// Included by odometry_hip.hip.
#pragma once
#include "depth_filter.hip.h"

struct odo_depth_filter {
  odo_ctx* ctx;
  int device;
  odo_depth_filter_params p;
  int blocks;              // workgroups of one launch = rows of `d_partials`
  uint8_t* d_tables;       // the padded range table in 4 * kDfRangeWords bytes, then shift[256]
  uint32_t* d_partials;    // [blocks][kDfStatWords], zero until the first run
};

static DfArgs df_args(const odo_depth_filter* f, const uint16_t* in, uint16_t* out) {
  DfArgs a;
  memset(&a, 0, sizeof(a));
  a.in = in; a.out = out; a.wr0 = f->d_tables; a.shift = f->d_tables + 4 * kDfRangeWords; a.partials = f->d_partials;
  a.rows = f->p.rows; a.cols = f->p.cols; a.radius = f->p.radius;
  const int n = 2 * f->p.radius + 1;
  for (int dy = 0; dy < n; dy++)
    for (int dx = 0; dx < n; dx++) a.ws[dy][dx >> 2] |= (uint32_t)f->p.ws[dy * n + dx] << (8 * (dx & 3));
  return a;
}

extern "C" int odo_depth_filter_create(odo_ctx* ctx, const odo_depth_filter_params* p, odo_depth_filter** out) {
  const char* who = "odo_depth_filter_create";
  if (!ctx || !p || !out) return fail("%s: NULL arg", who);
  if (p->rows < 1 || p->cols < 1 || p->rows > 8192 || p->cols > 8192) return fail("%s: bad size %dx%d (1 .. 8192 each)", who, p->cols, p->rows);
  switch (df_check_tables(p->radius, p->ws, p->wr, p->shift)) {
    case 0: break;
    case 1: return fail("%s: radius %d out of range (1 .. %d)", who, p->radius, kDfMaxRadius);
    case 2: return fail("%s: a spatial weight is above %d", who, kDfWsMax);
    case 3: return fail("%s: the centre's spatial weight must be at least 1", who);
    case 4: return fail("%s: wr[0] must be at least 1", who);
    default: return fail("%s: a shift is above %d", who, kDfShiftMax);
  }
  HIP_OK(hipSetDevice(ctx->device));
  odo_depth_filter* f = new (std::nothrow) odo_depth_filter();
  if (!f) return fail("out of memory");
  memset((void*)f, 0, sizeof(*f));
  f->ctx = ctx; f->device = ctx->device; f->p = *p;
  f->blocks = df_blocks_x(p->cols) * df_blocks_y(p->rows);
  const size_t pbytes = sizeof(uint32_t) * kDfStatWords * (size_t)f->blocks;
  uint8_t tables[4 * kDfRangeWords + kDfRange];
  memset(tables, 0, sizeof(tables));
  df_pad_range(p->wr, tables);
  memcpy(tables + 4 * kDfRangeWords, p->shift, kDfRange);
  // (on the context's stream, in front of every run, and waited for: `tables` is on the stack)
  const bool ok = hipMalloc((void**)&f->d_tables, sizeof(tables)) == hipSuccess && hipMalloc((void**)&f->d_partials, pbytes) == hipSuccess &&
                  hipMemcpyAsync(f->d_tables, tables, sizeof(tables), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
                  hipMemsetAsync(f->d_partials, 0, pbytes, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    if (f->d_tables) (void)hipFree(f->d_tables);
    if (f->d_partials) (void)hipFree(f->d_partials);
    delete f;
    return fail("%s: device allocation failed (%dx%d)", who, p->cols, p->rows);
  }
  *out = f;
  return 0;
}

// NULL, misaligned, or frames that share a byte: -1 and nothing enqueued (the kernel reads a halo around every pixel it writes).
static int df_check_frames(const char* who, const odo_depth_filter* f, const uint16_t* in, const uint16_t* out) {
  if (!f || !in || !out) return fail("%s: NULL arg", who);
  if (((uintptr_t)in | (uintptr_t)out) & 1) return fail("%s: misaligned frame", who);
  const uintptr_t bytes = sizeof(uint16_t) * (uintptr_t)f->p.rows * f->p.cols, i0 = (uintptr_t)in, o0 = (uintptr_t)out;
  if (i0 < o0 + bytes && o0 < i0 + bytes) return fail("%s: the frames overlap (the filter does not run in place)", who);
  return 0;
}

extern "C" int odo_depth_filter_run_dev(odo_depth_filter* f, const uint16_t* in_dev, uint16_t* out_dev) {
  if (df_check_frames("odo_depth_filter_run_dev", f, in_dev, out_dev)) return -1;
  HIP_OK(hipSetDevice(f->device));
  launch_depth_filter(df_args(f, in_dev, out_dev), f->ctx->stream);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int odo_depth_filter_stats(odo_depth_filter* f, long out[3]) {
  if (!f || !out) return fail("odo_depth_filter_stats: NULL arg");
  HIP_OK(hipSetDevice(f->device));
  std::vector<uint32_t> rows;
  try { rows.resize((size_t)kDfStatWords * f->blocks); } catch (...) { return fail("out of memory"); }
  HIP_OK(hipMemcpyAsync(rows.data(), f->d_partials, sizeof(uint32_t) * rows.size(), hipMemcpyDeviceToHost, f->ctx->stream));
  HIP_OK(hipStreamSynchronize(f->ctx->stream));
  long long sum[3] = {0, 0, 0};
  for (int b = 0; b < f->blocks; b++)
    for (int k = 0; k < 3; k++) sum[k] += rows[(size_t)kDfStatWords * b + k];
  for (int k = 0; k < 3; k++) out[k] = (long)sum[k];
  return 0;
}

// Event timing (tools/depth_filter_cost.py): one launch to warm, then `reps` launches between two events on the context's stream;
// *us the mean time of one in microseconds. out_dev and the statistics hold the result of filtering in_dev afterwards.
extern "C" int odo_depth_filter_time_dev(odo_depth_filter* f, const uint16_t* in_dev, uint16_t* out_dev, int reps, float* us) {
  const char* who = "odo_depth_filter_time_dev";
  if (!us) return fail("%s: NULL arg", who);
  if (df_check_frames(who, f, in_dev, out_dev)) return -1;
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  HIP_OK(hipSetDevice(f->device));
  const DfArgs a = df_args(f, in_dev, out_dev);
  hipStream_t s = f->ctx->stream;
  const auto run = [&]() { launch_depth_filter(a, s); return true; };
  return time_stages(who, s, reps, 1, us, run, [&](int) { return run(); });
}

extern "C" int odo_depth_filter_destroy(odo_depth_filter* f) {
  if (!f) return 0;
  (void)hipSetDevice(f->device);
  (void)hipStreamSynchronize(f->ctx->stream);   // a run in flight reads the tables and writes the partial rows
  (void)hipFree(f->d_tables);
  (void)hipFree(f->d_partials);
  delete f;
  return 0;
}
