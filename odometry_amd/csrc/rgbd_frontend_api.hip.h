// rgbd_frontend_api.hip.h — the RGB-D front end (odo_rgbd_frontend_*): the host object over the kernels of rgbd_frontend_kernels.hip.
// Raw sensor frames in (interleaved 8-bit colour, uint16 depth in the depth imager's grid), the RGB-D tracker's inputs out (fp32
// grey, uint16 depth registered to the grey camera), on a stream of the front end's own so that frame k + 1 is prepared while the
// tracker works on frame k. The tracker is not involved: the caller waits for a slot and hands its two pointers to the _rgbd entry
// points. Included by odometry_hip.hip.
#pragma once
#include <cmath>
#include "rgbd_frontend.hip.h"

constexpr int kFeMaxSlots = 8;

struct odo_rgbd_frontend {
  odo_ctx* ctx;                 // host frames are uploaded through its pinned staging ring, on its stream
  int device;
  hipStream_t own;              // the three launches of every frame
  odo_rgbd_frontend_params p;
  size_t n, nd;                 // target / depth pixels
  int slots;
  float* d_gray[kFeMaxSlots];
  uint16_t* d_depth[kFeMaxSlots];
  uint8_t* d_colour_in[kFeMaxSlots];   // submit_host: the slot's raw frame on the device (allocated on first use)
  uint16_t* d_depth_in[kFeMaxSlots];
  long slot_frame[kFeMaxSlots]; // the frame the slot holds (or will hold), -1: none yet
  const uint8_t* slot_colour[kFeMaxSlots];   // the device colour frame the slot was made from (the caller's, or d_colour_in[slot])
  uint32_t* d_zbuf;
  FeCounters* d_ctr;
  long long* h_stats;           // host-mapped [slots][6]
  long long* d_stats_map;
  int* h_done;                  // host-mapped [slots]: the slot's completion word (frame number + 1)
  int* d_done_map;
  long submitted;               // frames enqueued so far
  long done_upto;               // frames 0 .. done_upto - 1 are known complete (the caller waited for one of them or a later one)
};

static int fe_release(odo_rgbd_frontend* f) {
  for (int s = 0; s < kFeMaxSlots; s++) {
    void* ps[] = {f->d_gray[s], f->d_depth[s], f->d_colour_in[s], f->d_depth_in[s]};
    for (void* q : ps) if (q) (void)hipFree(q);
  }
  if (f->d_zbuf) (void)hipFree(f->d_zbuf);
  if (f->d_ctr) (void)hipFree(f->d_ctr);
  if (f->h_stats) (void)hipHostFree(f->h_stats);
  if (f->h_done) (void)hipHostFree(f->h_done);
  if (f->own) (void)hipStreamDestroy(f->own);
  delete f;
  return 0;
}

static bool fe_pos(float v) { return std::isfinite(v) && v > 0.0f; }

extern "C" int odo_rgbd_frontend_create(odo_ctx* ctx, const odo_rgbd_frontend_params* p, odo_rgbd_frontend** out) {
  if (!p || !out) return fail("odo_rgbd_frontend_create: NULL arg");
  *out = nullptr;
  if (p->depth_rows < 1 || p->depth_cols < 1 || (long long)p->depth_rows * p->depth_cols > (1 << 28))
    return fail("odo_rgbd_frontend_create: bad depth size %dx%d", p->depth_cols, p->depth_rows);
  if (p->rows < 1 || p->cols < 1 || (long long)p->rows * p->cols > (1 << 28))
    return fail("odo_rgbd_frontend_create: bad size %dx%d", p->cols, p->rows);
  if (!fe_pos(p->depth_fx) || !fe_pos(p->depth_fy) || !fe_pos(p->K.f0))
    return fail("odo_rgbd_frontend_create: focal lengths must be finite and > 0");
  if (!std::isfinite(p->depth_cx) || !std::isfinite(p->depth_cy) || !std::isfinite(p->K.cx0) || !std::isfinite(p->K.cy0))
    return fail("odo_rgbd_frontend_create: principal points must be finite");
  if (!fe_pos(p->depth_scale_in) || !fe_pos(p->depth_scale_out))
    return fail("odo_rgbd_frontend_create: depth scales must be finite and > 0");
  for (float v : p->colour_from_depth)
    if (!std::isfinite(v)) return fail("odo_rgbd_frontend_create: colour_from_depth must be finite");
  if (p->colour_channels != 3 && p->colour_channels != 4)
    return fail("odo_rgbd_frontend_create: colour_channels %d (3 or 4)", p->colour_channels);
  if (p->colour_bgr != 0 && p->colour_bgr != 1) return fail("odo_rgbd_frontend_create: colour_bgr %d (0 or 1)", p->colour_bgr);
  if (p->slots < 2 || p->slots > kFeMaxSlots) return fail("odo_rgbd_frontend_create: slots %d out of range (2 .. %d)", p->slots, kFeMaxSlots);
  if (!ctx) return fail("odo_rgbd_frontend_create: NULL ctx");
  HIP_OK(hipSetDevice(ctx->device));
  odo_rgbd_frontend* f = new (std::nothrow) odo_rgbd_frontend();
  if (!f) return fail("out of memory");
  memset((void*)f, 0, sizeof(*f));
  f->ctx = ctx; f->device = ctx->device; f->p = *p; f->slots = p->slots;
  f->n = (size_t)p->rows * p->cols; f->nd = (size_t)p->depth_rows * p->depth_cols;
  for (int s = 0; s < kFeMaxSlots; s++) f->slot_frame[s] = -1;
  bool ok = hipStreamCreateWithFlags(&f->own, hipStreamNonBlocking) == hipSuccess &&
            hipMalloc((void**)&f->d_zbuf, sizeof(uint32_t) * f->n) == hipSuccess &&
            hipMalloc((void**)&f->d_ctr, sizeof(FeCounters)) == hipSuccess &&
            hipHostMalloc((void**)&f->h_stats, sizeof(long long) * 6 * kFeMaxSlots, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
            hipHostGetDevicePointer((void**)&f->d_stats_map, f->h_stats, 0) == hipSuccess &&
            hipHostMalloc((void**)&f->h_done, sizeof(int) * kFeMaxSlots, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
            hipHostGetDevicePointer((void**)&f->d_done_map, f->h_done, 0) == hipSuccess;
  for (int s = 0; ok && s < f->slots; s++)
    ok = hipMalloc((void**)&f->d_gray[s], sizeof(float) * f->n) == hipSuccess &&
         hipMalloc((void**)&f->d_depth[s], sizeof(uint16_t) * f->n) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    fe_release(f);
    return fail("odo_rgbd_frontend_create: device allocation failed (%dx%d, %d slots)", p->cols, p->rows, p->slots);
  }
  memset(f->h_stats, 0, sizeof(long long) * 6 * kFeMaxSlots);
  memset(f->h_done, 0, sizeof(int) * kFeMaxSlots);
  *out = f;
  return 0;
}

// The slot whose grey buffer is gray_out and that holds a submitted frame, or -1.
static int fe_slot_of(const odo_rgbd_frontend* f, const float* gray_out) {
  for (int s = 0; s < f->slots; s++)
    if (gray_out && f->d_gray[s] == gray_out) return f->slot_frame[s] >= 0 ? s : -1;
  return -1;
}

static int fe_enqueue(odo_rgbd_frontend* f, int s, const uint8_t* colour_dev, const uint16_t* depth_dev, const float** gray_out,
                      const uint16_t** depth_out) {
  const odo_rgbd_frontend_params& p = f->p;
  FeArgs a;
  memset(&a, 0, sizeof(a));
  a.colour = colour_dev; a.depth = depth_dev;
  a.rows = p.rows; a.cols = p.cols; a.channels = p.colour_channels; a.bgr = p.colour_bgr;
  a.depth_rows = p.depth_rows; a.depth_cols = p.depth_cols;
  a.fxd = p.depth_fx; a.fyd = p.depth_fy; a.cxd = p.depth_cx; a.cyd = p.depth_cy; a.scale_in = p.depth_scale_in;
  a.f = p.K.f0; a.cx = p.K.cx0; a.cy = p.K.cy0; a.scale_out = p.depth_scale_out;
  memcpy(a.e, p.colour_from_depth, sizeof(a.e));
  a.gray = f->d_gray[s]; a.zbuf = f->d_zbuf; a.out = f->d_depth[s]; a.ctr = f->d_ctr;
  a.stats = f->d_stats_map + 6 * s; a.done_flag = f->d_done_map + s;
  a.frame = f->submitted; a.token = (int)((f->submitted + 1) & 0x7fffffff);
  launch_rgbd_frontend(a, f->own);
  HIP_OK(hipGetLastError());
  f->slot_frame[s] = f->submitted;
  f->slot_colour[s] = colour_dev;
  f->submitted++;
  *gray_out = f->d_gray[s];
  *depth_out = f->d_depth[s];
  return 0;
}

// The slot of the next frame, or -1 (with a message) when the ring is full of frames the caller never waited for.
static int fe_next_slot(odo_rgbd_frontend* f, const char* who) {
  if (f->submitted - f->done_upto >= f->slots)
    return fail("%s: %d frames are outstanding (odo_rgbd_frontend_wait for the oldest first)", who, f->slots);
  if (f->submitted >= 0x7ffffffeL) return fail("%s: too many frames", who);
  return (int)(f->submitted % f->slots);
}

extern "C" int odo_rgbd_frontend_submit_dev(odo_rgbd_frontend* f, const uint8_t* colour_dev, const uint16_t* depth_dev,
                                            const float** gray_out, const uint16_t** depth_out) {
  if (!f || !colour_dev || !depth_dev || !gray_out || !depth_out) return fail("odo_rgbd_frontend_submit_dev: NULL arg");
  if (((uintptr_t)colour_dev & 3) || ((uintptr_t)depth_dev & 1)) return fail("odo_rgbd_frontend_submit_dev: misaligned frame");
  const int s = fe_next_slot(f, "odo_rgbd_frontend_submit_dev");
  if (s < 0) return -1;
  HIP_OK(hipSetDevice(f->device));
  return fe_enqueue(f, s, colour_dev, depth_dev, gray_out, depth_out);
}

extern "C" int odo_rgbd_frontend_submit_host(odo_rgbd_frontend* f, const uint8_t* colour, size_t colour_pitch, const uint16_t* depth,
                                             size_t depth_pitch, const float** gray_out, const uint16_t** depth_out) {
  if (!f || !colour || !depth || !gray_out || !depth_out) return fail("odo_rgbd_frontend_submit_host: NULL arg");
  const size_t crow = (size_t)f->p.cols * f->p.colour_channels, drow = sizeof(uint16_t) * (size_t)f->p.depth_cols;
  if (colour_pitch < crow || depth_pitch < drow) return fail("odo_rgbd_frontend_submit_host: a pitch is shorter than its row");
  const int s = fe_next_slot(f, "odo_rgbd_frontend_submit_host");
  if (s < 0) return -1;
  HIP_OK(hipSetDevice(f->device));
  // The slot's raw frame on the device. Its previous reader (the frame `slots` submits ago) is complete: the caller waited for it.
  if (!f->d_colour_in[s]) HIP_OK(hipMalloc((void**)&f->d_colour_in[s], crow * f->p.rows));
  if (!f->d_depth_in[s]) HIP_OK(hipMalloc((void**)&f->d_depth_in[s], drow * f->p.depth_rows));
  if (upload_rows_async(f->ctx, f->d_colour_in[s], colour, colour_pitch, crow, f->p.rows)) return -1;
  if (upload_rows_async(f->ctx, f->d_depth_in[s], depth, depth_pitch, drow, f->p.depth_rows)) return -1;
  // the kernels run behind the two uploads (the context's stream), on the front end's stream
  const unsigned long mark = odo_ctx_mark(f->ctx);
  if (mark == 0) return fail("odo_rgbd_frontend_submit_host: hipEventRecord failed");
  hipEvent_t ev;
  {
    std::lock_guard<std::mutex> lk(*f->ctx->mu);
    ev = f->ctx->sw_ev[mark % 32];
  }
  HIP_OK(hipStreamWaitEvent(f->own, ev, 0));
  return fe_enqueue(f, s, f->d_colour_in[s], f->d_depth_in[s], gray_out, depth_out);
}

extern "C" int odo_rgbd_frontend_wait(odo_rgbd_frontend* f, const float* gray_out) {
  if (!f) return fail("NULL front end");
  const int s = fe_slot_of(f, gray_out);
  if (s < 0) return fail("odo_rgbd_frontend_wait: not the grey buffer of a submitted frame");
  const long frame = f->slot_frame[s];
  if (frame < f->done_upto) return 0;
  const int token = (int)((frame + 1) & 0x7fffffff);
  volatile int* done = f->h_done + s;
  const auto t0 = std::chrono::steady_clock::now();
  long spins = 0;
  while (done[0] != token) {
    if ((++spins & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
      HIP_OK(hipSetDevice(f->device));
      HIP_OK(hipStreamSynchronize(f->own));
      if (done[0] != token) return fail("odo_rgbd_frontend_wait: frame %ld never completed", frame);
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  f->done_upto = frame + 1;   // the stream runs the frames in order: every earlier one is complete as well
  return 0;
}

extern "C" int odo_rgbd_frontend_colour(odo_rgbd_frontend* f, const float* gray_out, const uint8_t** colour_dev) {
  if (!f || !gray_out || !colour_dev) return fail("odo_rgbd_frontend_colour: NULL arg");
  *colour_dev = nullptr;
  const int s = fe_slot_of(f, gray_out);
  if (s < 0) return fail("odo_rgbd_frontend_colour: not the grey buffer of a submitted frame");
  *colour_dev = f->slot_colour[s];
  return 0;
}

extern "C" int odo_rgbd_frontend_stats(odo_rgbd_frontend* f, const float* gray_out, long out[6]) {
  if (!f || !out) return fail("odo_rgbd_frontend_stats: NULL arg");
  if (odo_rgbd_frontend_wait(f, gray_out)) return -1;
  const int s = fe_slot_of(f, gray_out);
  for (int k = 0; k < 6; k++) out[k] = (long)f->h_stats[6 * s + k];
  return 0;
}

extern "C" int odo_rgbd_frontend_destroy(odo_rgbd_frontend* f) {
  if (!f) return 0;
  (void)hipSetDevice(f->device);
  (void)hipStreamSynchronize(f->own);   // frames in flight, their uploads included (the stream waits for them)
  return fe_release(f);
}
