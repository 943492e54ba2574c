// volume_api.hip.h — the TSDF volume (odo_volume_*): the host object over the kernels of volume_kernels.hip. Every tracked RGB-D
// depth frame is fused into a dense truncated signed distance grid (Curless & Levoy), and the surface is read back out of it as an
// oriented point cloud: the "reconstructed 3D geometry" of the reference's README. Included by odometry_hip.hip before
// tracker.hip.h (an RGB-D tracker integrates its frames).
#pragma once
#include "volume.hip.h"
#include "volume_mesh.hip.h"
#include "volume_colour.hip.h"
#include "volume_raycast.hip.h"
#include "volume_shift.hip.h"
#include "volume_reentry.hip.h"

struct odo_volume {
  odo_ctx* ctx;                 // standalone integrations (odo_volume_integrate_dev) run on its stream
  int device;
  hipStream_t own;              // the attached tracker's integrations, extractions, downloads, clears
  hipEvent_t ev_last;           // behind the last operation that changed the volume, on `last`
  hipStream_t last;             // stream of that operation, nullptr: none yet
  odo_volume_params p;
  long n_vox;
  uint32_t* d_vox;
  unsigned long long* d_blk;    // integrate: the blocks' rows
  VolCounters* d_ctr;
  // Every buffer that is grown on demand (volume_grow) has a capacity of its own, in items.
  // extraction (the scratch sized on first use, the point buffers grown on demand)
  unsigned long long *d_wave, *d_off;
  int* d_cnt;
  float4 *d_xyz0, *d_nrmw;
  long xyz0_capacity, nrmw_capacity;
  // mesh (the scratch sized on first use: 5 B per voxel; the output buffers grown on demand)
  uint8_t* d_mesh_mask;
  uint32_t* d_mesh_base;
  unsigned* d_mesh_cnt;
  unsigned long long* d_mesh_off;
  MeshCounters* d_mesh_ctr;
  float4 *d_mesh_xyz0, *d_mesh_nrmw;
  int* d_mesh_tri;
  long mesh_xyz0_capacity, mesh_nrmw_capacity, mesh_triangle_capacity;
  long n_frames;                // integrations since create / clear
  odo_tracker* attached;
  // colour (odo_volume_enable_colour; nothing below is allocated without it)
  int colour;                   // 1: the colour grid exists
  odo_volume_colour_params cp;
  uint32_t* d_col;              // [n_vox]: {R, G, B, wc}
  uint32_t *d_rgba, *d_mesh_rgba;   // the colours of the extraction's points / the mesh's vertices, grown on demand
  long rgba_capacity, mesh_rgba_capacity;
  int colour_sampling;          // of the ray-cast's colour frame: 0 nearest voxel, 1 trilinear (odo_volume_set_colour_sampling)
  // ray-cast (odo_volume_raycast's frames on the device: sized on first use, grown on demand)
  float* d_ray_depth;
  uint16_t* d_ray_raw;
  float4* d_ray_nrmw;
  uint32_t* d_ray_rgba;
  long ray_depth_capacity, ray_raw_capacity, ray_nrmw_capacity, ray_rgba_capacity;   // pixels
  // the moving window (volume_shift_api.hip.h): p.origin = hostfp::window_origin(origin0, off, voxel_size) after every shift
  float origin0[3];             // the origin given to create
  int off[3];                   // the cumulative shift in voxels
  uint32_t *d_vox2, *d_col2;    // the grids' second buffers: allocated on the first shift, swapped with d_vox / d_col by every shift
  // the spill store (odo_volume_enable_spill; nothing below is allocated without it)
  long spill_capacity;          // points, 0: no store
  float4 *d_spill_xyz0, *d_spill_nrmw;
  uint32_t* d_spill_rgba;       // with colour
  VolSpillCounters* d_spill_ctr;
  // the mesh store (odo_volume_enable_spill_mesh, volume_shift_api.hip.h; nothing below is allocated without it)
  long smesh_vertex_capacity, smesh_triangle_capacity;   // 0: no store
  float4 *d_smesh_xyz0, *d_smesh_nrmw;
  uint32_t* d_smesh_rgba;       // with colour
  int* d_smesh_tri;
  VolSpillMeshCounters* d_smesh_ctr;
  // the re-entry store (odo_volume_enable_reentry, volume_reentry_api.hip.h; nothing below is allocated without it)
  long re_capacity;             // entries, 0: no store
  uint4 *d_re_ent, *d_re_ent2;  // {gx, gy, gz, word}: the live set and the second set, swapped by every shift
  uint32_t *d_re_col, *d_re_col2;   // with colour
  unsigned long long *d_re_save_mask, *d_re_save_off, *d_re_keep_mask, *d_re_keep_off;
  unsigned *d_re_save_cnt, *d_re_keep_cnt;
  VolReentryCounters *d_re_ctr, *d_re_ctr_time;   // (_time: the copy odo_volume_reentry_time works on)
  int follow;                   // 1: odo_volume_set_follow's parameters are set
  odo_volume_follow_params fp;
};

static int volume_release(odo_volume* v) {
  void* ps[] = {v->d_vox, v->d_blk, v->d_ctr, v->d_wave, v->d_off, v->d_cnt, v->d_xyz0, v->d_nrmw,
                v->d_mesh_mask, v->d_mesh_base, v->d_mesh_cnt, v->d_mesh_off, v->d_mesh_ctr, v->d_mesh_xyz0, v->d_mesh_nrmw, v->d_mesh_tri,
                v->d_col, v->d_rgba, v->d_mesh_rgba, v->d_ray_depth, v->d_ray_raw, v->d_ray_nrmw, v->d_ray_rgba,
                v->d_vox2, v->d_col2, v->d_spill_xyz0, v->d_spill_nrmw, v->d_spill_rgba, v->d_spill_ctr,
                v->d_smesh_xyz0, v->d_smesh_nrmw, v->d_smesh_rgba, v->d_smesh_tri, v->d_smesh_ctr,
                v->d_re_ent, v->d_re_ent2, v->d_re_col, v->d_re_col2, v->d_re_save_mask, v->d_re_save_off, v->d_re_keep_mask,
                v->d_re_keep_off, v->d_re_save_cnt, v->d_re_keep_cnt, v->d_re_ctr, v->d_re_ctr_time};
  for (void* p : ps) if (p) (void)hipFree(p);
  if (v->ev_last) (void)hipEventDestroy(v->ev_last);
  if (v->own) (void)hipStreamDestroy(v->own);
  delete v;
  return 0;
}

// Everything that changed the volume so far is ordered before the next operation on stream s.
static int volume_order_on(odo_volume* v, hipStream_t s) {
  if (v->last && v->last != s) HIP_OK(hipStreamWaitEvent(s, v->ev_last, 0));
  return 0;
}
static int volume_mark(odo_volume* v, hipStream_t s) {
  HIP_OK(hipEventRecord(v->ev_last, s));
  v->last = s;
  return 0;
}
// Waits for every pending integration; afterwards the volume's own stream is idle and ordered after them.
static int volume_sync(odo_volume* v) {
  HIP_OK(hipSetDevice(v->device));
  if (volume_order_on(v, v->own)) return -1;
  HIP_OK(hipStreamSynchronize(v->own));
  return 0;
}
// Waits, then reads one of the volume's device-resident counter blocks (the volume's own or a store's).
template <class Counters>
static int volume_read_counters(odo_volume* v, const Counters* dev, Counters* c) {
  if (volume_sync(v)) return -1;
  HIP_OK(hipMemcpyAsync(c, dev, sizeof(Counters), hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  return 0;
}

// Event timing in stages, the shape of every *_time entry point: warm() once, then for each of the n stages `reps` calls of stage(q)
// between two events on s; us[q] = the mean time of one call in microseconds. Both callables enqueue on s and return success. A
// failure anywhere drains s and is reported as who's.
constexpr int kTimedStages = 6;
template <class Warm, class Stage>
static int time_stages(const char* who, hipStream_t s, int reps, int n, float* us, Warm warm, Stage stage) {
  hipEvent_t ev[kTimedStages + 1] = {};
  bool ok = true;
  for (int q = 0; q <= n; q++) ok = ok && hipEventCreate(&ev[q]) == hipSuccess;
  ok = ok && warm() && hipEventRecord(ev[0], s) == hipSuccess;
  for (int q = 0; q < n && ok; q++) {
    for (int i = 0; i < reps && ok; i++) ok = stage(q);
    ok = ok && hipEventRecord(ev[q + 1], s) == hipSuccess;
  }
  ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  for (int q = 0; q < n && ok; q++) {
    float ms = 0.0f;
    ok = hipEventElapsedTime(&ms, ev[q], ev[q + 1]) == hipSuccess;
    us[q] = 1e3f * ms / (float)reps;
  }
  for (auto& e : ev) if (e) (void)hipEventDestroy(e);
  if (!ok) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s);
    return fail("%s: timing failed", who);
  }
  return 0;
}

static int volume_reset(odo_volume* v) {
  if (volume_order_on(v, v->own)) return -1;
  HIP_OK(hipMemsetAsync(v->d_vox, 0, sizeof(uint32_t) * (size_t)v->n_vox, v->own));
  if (v->colour) HIP_OK(hipMemsetAsync(v->d_col, 0, sizeof(uint32_t) * (size_t)v->n_vox, v->own));
  HIP_OK(hipMemsetAsync(v->d_ctr, 0, sizeof(VolCounters), v->own));
  if (v->d_spill_ctr) HIP_OK(hipMemsetAsync(v->d_spill_ctr, 0, sizeof(VolSpillCounters), v->own));   // (the window stays where it is)
  if (v->d_smesh_ctr) HIP_OK(hipMemsetAsync(v->d_smesh_ctr, 0, sizeof(VolSpillMeshCounters), v->own));
  if (v->d_re_ctr) HIP_OK(hipMemsetAsync(v->d_re_ctr, 0, sizeof(VolReentryCounters), v->own));
  v->n_frames = 0;
  return volume_mark(v, v->own);
}

extern "C" int odo_volume_create(odo_ctx* ctx, const odo_volume_params* p, odo_volume** out) {
  if (!ctx || !p || !out) return fail("odo_volume_create: NULL arg");
  *out = nullptr;
  if (p->nx < 2 || p->ny < 2 || p->nz < 2 || (long long)p->nx * p->ny * p->nz > (1LL << 30))
    return fail("odo_volume_create: bad grid %dx%dx%d (every dimension >= 2, at most 2^30 voxels)", p->nx, p->ny, p->nz);
  if (!(std::isfinite(p->voxel_size) && p->voxel_size > 0.0f)) return fail("odo_volume_create: voxel_size must be finite and > 0");
  for (int c = 0; c < 3; c++) if (!std::isfinite(p->origin[c])) return fail("odo_volume_create: origin must be finite");
  if (!(std::isfinite(p->mu) && p->mu > 0.0f)) return fail("odo_volume_create: mu must be finite and > 0");
  if (!(p->max_depth > 0.0f)) return fail("odo_volume_create: max_depth must be > 0");
  if (p->max_weight < 1 || p->max_weight > 65535) return fail("odo_volume_create: max_weight %d out of range (1 .. 65535)", p->max_weight);
  if (p->rows < 1 || p->cols < 1 || (long long)p->rows * p->cols > (1 << 28)) return fail("odo_volume_create: bad size %dx%d", p->rows, p->cols);
  if (!(std::isfinite(p->depth_scale) && p->depth_scale > 0.0f)) return fail("odo_volume_create: depth_scale must be finite and > 0");
  if (!(std::isfinite(p->K.f0) && std::isfinite(p->K.cx0) && std::isfinite(p->K.cy0))) return fail("odo_volume_create: K must be finite");
  HIP_OK(hipSetDevice(ctx->device));
  odo_volume* v = new (std::nothrow) odo_volume();
  if (!v) return fail("out of memory");
  v->ctx = ctx; v->device = ctx->device;   // (everything else is zero: new odo_volume())
  v->p = *p;
  for (int c = 0; c < 3; c++) v->origin0[c] = p->origin[c];
  v->n_vox = (long)p->nx * p->ny * p->nz;
  bool ok = hipStreamCreateWithFlags(&v->own, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&v->ev_last, hipEventDisableTiming) == hipSuccess &&
            hipMalloc((void**)&v->d_vox, sizeof(uint32_t) * (size_t)v->n_vox) == hipSuccess &&
            hipMalloc((void**)&v->d_blk, sizeof(unsigned long long) * 2 * kVolMaxBlocks) == hipSuccess &&
            hipMalloc((void**)&v->d_ctr, sizeof(VolCounters)) == hipSuccess;
  ok = ok && volume_reset(v) == 0 && volume_sync(v) == 0;
  if (!ok) {
    (void)hipGetLastError();
    const long n = v->n_vox;
    volume_release(v);
    return fail("odo_volume_create: device allocation failed (%ld voxels)", n);
  }
  *out = v;
  return 0;
}

static VolGrid volume_grid(const odo_volume* v) {
  VolGrid g;
  g.vox = v->d_vox; g.nx = v->p.nx; g.ny = v->p.ny; g.nz = v->p.nz;
  g.vs = v->p.voxel_size; g.ox = v->p.origin[0]; g.oy = v->p.origin[1]; g.oz = v->p.origin[2];
  return g;
}

static bool pose_finite(const float* A) {
  for (int i = 0; i < 16; i++) if (!std::isfinite(A[i])) return false;
  return true;
}

// One integration on stream s (async). depth: rows x cols uint16 on the device; A: camera-to-world, finite. colour: nullptr = the
// plain integration, else the frame's colour pixels on the device (the volume has a colour grid): the fused coloured launch.
static int volume_integrate(odo_volume* v, const uint16_t* depth, const float* A, hipStream_t s, const uint8_t* colour = nullptr) {
  HIP_OK(hipSetDevice(v->device));
  if (volume_order_on(v, s)) return -1;
  float M[16];
  hostfp::invert_rigid(A, M);
  VolIntegrateArgs a;
  memset(&a, 0, sizeof(a));
  a.g = volume_grid(v);
  a.raw = depth;
  VolFrame& f = a.f;
  f.rows = v->p.rows; f.cols = v->p.cols;
  f.f0 = v->p.K.f0; f.cx0 = v->p.K.cx0; f.cy0 = v->p.K.cy0;
  f.depth_scale = v->p.depth_scale; f.max_depth = v->p.max_depth; f.mu = v->p.mu; f.max_weight = v->p.max_weight;
  f.m0 = M[0]; f.m1 = M[1]; f.m2 = M[2]; f.m4 = M[4]; f.m5 = M[5]; f.m6 = M[6];
  f.m8 = M[8]; f.m9 = M[9]; f.m10 = M[10]; f.m12 = M[12]; f.m13 = M[13]; f.m14 = M[14];
  f.zc_far = (v->p.max_depth + v->p.mu) * 1.001f;
  a.tiles_x = (v->p.nx + kVolTileX - 1) / kVolTileX;
  a.tiles_y = (v->p.ny + kVolTileY - 1) / kVolTileY;
  a.tiles = (long long)a.tiles_x * a.tiles_y * v->p.nz;
  a.nblk = (int)std::min<long long>(a.tiles, kVolMaxBlocks);
  a.step_x = a.nblk % a.tiles_x; a.step_y = (a.nblk / a.tiles_x) % a.tiles_y; a.step_k = (a.nblk / a.tiles_x) / a.tiles_y;
  a.blk = v->d_blk; a.ctr = v->d_ctr;
  if (colour) {
    VolIntegrateColourArgs ac;
    ac.a = a;
    ac.c.col = v->d_col; ac.c.pix = colour; ac.c.channels = v->cp.channels; ac.c.bgr = v->cp.bgr; ac.c.max_weight = v->cp.max_weight;
    launch_volume_integrate_colour(ac, s);
  } else {
    launch_volume_integrate(a, s);
  }
  HIP_OK(hipGetLastError());
  v->n_frames++;
  return volume_mark(v, s);
}

extern "C" int odo_volume_integrate_dev(odo_volume* v, const uint16_t* depth_dev, const float abs_pose_colmajor[16]) {
  if (!v || !depth_dev || !abs_pose_colmajor) return fail("odo_volume_integrate_dev: NULL arg");
  if (!pose_finite(abs_pose_colmajor)) return fail("odo_volume_integrate_dev: the pose has a non-finite entry (a frame whose Solve failed?)");
  return volume_integrate(v, depth_dev, abs_pose_colmajor, v->ctx->stream);
}

extern "C" int odo_volume_enable_colour(odo_volume* v, const odo_volume_colour_params* p) {
  if (!v || !p) return fail("odo_volume_enable_colour: NULL arg");
  if (p->channels != 3 && p->channels != 4) return fail("odo_volume_enable_colour: channels %d (3 or 4)", p->channels);
  if (p->bgr != 0 && p->bgr != 1) return fail("odo_volume_enable_colour: bgr %d (0 or 1)", p->bgr);
  if (p->max_weight < 1 || p->max_weight > 255) return fail("odo_volume_enable_colour: max_weight %d out of range (1 .. 255)", p->max_weight);
  if (v->colour) return fail("odo_volume_enable_colour: the volume has a colour grid already");
  if (v->attached) return fail("odo_volume_enable_colour: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)");
  HIP_OK(hipSetDevice(v->device));
  uint32_t* col = nullptr;
  if (hipMalloc((void**)&col, sizeof(uint32_t) * (size_t)v->n_vox) != hipSuccess) {
    (void)hipGetLastError();
    return fail("odo_volume_enable_colour: device allocation failed (%ld voxels)", v->n_vox);
  }
  if (volume_order_on(v, v->own) || hipMemsetAsync(col, 0, sizeof(uint32_t) * (size_t)v->n_vox, v->own) != hipSuccess || volume_mark(v, v->own)) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(v->own);
    (void)hipFree(col);
    return fail("odo_volume_enable_colour: clearing the colour grid failed");
  }
  v->d_col = col; v->cp = *p; v->colour = 1;
  return 0;
}

extern "C" int odo_volume_integrate_colour_dev(odo_volume* v, const uint16_t* depth_dev, const uint8_t* colour_dev,
                                               const float abs_pose_colmajor[16]) {
  if (!v || !depth_dev || !colour_dev || !abs_pose_colmajor) return fail("odo_volume_integrate_colour_dev: NULL arg");
  if (!v->colour) return fail("odo_volume_integrate_colour_dev: the volume has no colour grid (odo_volume_enable_colour first)");
  if (v->cp.channels == 4 && ((uintptr_t)colour_dev & 3)) return fail("odo_volume_integrate_colour_dev: misaligned colour frame (4 channels: 4-byte aligned)");
  if (!pose_finite(abs_pose_colmajor))
    return fail("odo_volume_integrate_colour_dev: the pose has a non-finite entry (a frame whose Solve failed?)");
  return volume_integrate(v, depth_dev, abs_pose_colmajor, v->ctx->stream, colour_dev);
}

extern "C" int odo_volume_download_colour(odo_volume* v, uint8_t* rgbw) {
  if (!v || !rgbw) return fail("odo_volume_download_colour: NULL arg");
  if (!v->colour) return fail("odo_volume_download_colour: the volume has no colour grid (odo_volume_enable_colour first)");
  if (volume_sync(v)) return -1;
  HIP_OK(hipMemcpyAsync(rgbw, v->d_col, sizeof(uint32_t) * (size_t)v->n_vox, hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  return 0;
}

extern "C" int odo_volume_upload_colour(odo_volume* v, const uint8_t* rgbw) {
  if (!v || !rgbw) return fail("odo_volume_upload_colour: NULL arg");
  if (!v->colour) return fail("odo_volume_upload_colour: the volume has no colour grid (odo_volume_enable_colour first)");
  if (v->attached) return fail("odo_volume_upload_colour: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)");
  HIP_OK(hipSetDevice(v->device));
  if (volume_order_on(v, v->own)) return -1;
  HIP_OK(hipMemcpyAsync(v->d_col, rgbw, sizeof(uint32_t) * (size_t)v->n_vox, hipMemcpyHostToDevice, v->own));
  if (volume_mark(v, v->own)) return -1;
  HIP_OK(hipStreamSynchronize(v->own));   // (the caller's buffer is the caller's again)
  return 0;
}

extern "C" int odo_volume_sync(odo_volume* v) {
  if (!v) return fail("NULL volume");
  return volume_sync(v);
}

extern "C" int odo_volume_stats(odo_volume* v, long out[4]) {
  if (!v || !out) return fail("odo_volume_stats: NULL arg");
  VolCounters c;
  if (volume_read_counters(v, v->d_ctr, &c)) return -1;
  out[0] = v->n_frames; out[1] = (long)c.updated; out[2] = (long)c.band; out[3] = (long)c.cumulative;
  return 0;
}

// Grows one device buffer to `count` items of `item` bytes; *have = its capacity in items. The caller has waited for whatever used the
// buffer. After a failure the buffer is empty (nullptr, capacity 0): the volume stays usable and releases everything at destroy.
static int volume_grow(void** p, long* have, long count, size_t item, const char* who, const char* what) {
  if (count <= *have) return 0;
  if (*p) (void)hipFree(*p);
  *p = nullptr; *have = 0;
  if (hipMalloc(p, item * (size_t)count) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return fail("%s: device allocation failed (%ld %s)", who, count, what);
  }
  *have = count;
  return 0;
}

// odo_volume_extract and, with_colour, odo_volume_extract_colour: the three launches into the volume's own buffers and, with_colour,
// one launch more, the points' colours into d_rgba (skipped when no point is written).
static int volume_extract(const char* who, odo_volume* v, long capacity, float* xyz0, float* nrmw, uint8_t* rgba, long* n_points,
                          long* n_dropped, bool with_colour) {
  if (!v || !n_points || capacity < 0 || capacity > (1L << 28) || (capacity > 0 && (!xyz0 || !nrmw || (with_colour && !rgba))))
    return fail("%s: bad arg (capacity 0 .. 2^28, buffers for `capacity` points)", who);
  if (with_colour && !v->colour) return fail("%s: the volume has no colour grid (odo_volume_enable_colour first)", who);
  if (volume_sync(v)) return -1;
  const int nblk = (int)((v->n_vox + kVolExtBlock - 1) / kVolExtBlock);
  if (!v->d_cnt) {
    bool ok = hipMalloc((void**)&v->d_wave, sizeof(unsigned long long) * 3 * (kVolExtBlock / 64) * (size_t)nblk) == hipSuccess &&
              hipMalloc((void**)&v->d_off, sizeof(unsigned long long) * (size_t)nblk) == hipSuccess &&
              hipMalloc((void**)&v->d_cnt, sizeof(int) * (size_t)nblk) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      if (v->d_wave) (void)hipFree(v->d_wave);
      if (v->d_off) (void)hipFree(v->d_off);
      if (v->d_cnt) (void)hipFree(v->d_cnt);
      v->d_wave = v->d_off = nullptr; v->d_cnt = nullptr;
      return fail("%s: device allocation failed (%d blocks)", who, nblk);
    }
  }
  if (volume_grow((void**)&v->d_xyz0, &v->xyz0_capacity, capacity, sizeof(float4), who, "points") ||
      volume_grow((void**)&v->d_nrmw, &v->nrmw_capacity, capacity, sizeof(float4), who, "points") ||
      (with_colour && volume_grow((void**)&v->d_rgba, &v->rgba_capacity, capacity, sizeof(uint32_t), who, "point colours")))
    return -1;
  VolExtractArgs a;
  memset(&a, 0, sizeof(a));
  a.g = volume_grid(v);
  a.n = (int)v->n_vox; a.nblk = nblk; a.capacity = capacity;
  a.wave_mask = v->d_wave; a.blk = v->d_cnt; a.blk_off = v->d_off; a.ctr = v->d_ctr;
  a.xyz0 = v->d_xyz0; a.nrmw = v->d_nrmw;
  launch_volume_extract(a, v->own);
  HIP_OK(hipGetLastError());
  VolCounters c;
  HIP_OK(hipMemcpyAsync(&c, v->d_ctr, sizeof(VolCounters), hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  const size_t n = (size_t)c.ext_written;
  if (n > 0) {
    if (with_colour) {
      VolExtractColourArgs ac;
      ac.a = a; ac.col = v->d_col; ac.rgba = v->d_rgba;
      launch_volume_extract_colour(ac, v->own);
      HIP_OK(hipGetLastError());
    }
    HIP_OK(hipMemcpyAsync(xyz0, v->d_xyz0, sizeof(float4) * n, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipMemcpyAsync(nrmw, v->d_nrmw, sizeof(float4) * n, hipMemcpyDeviceToHost, v->own));
    if (with_colour) HIP_OK(hipMemcpyAsync(rgba, v->d_rgba, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipStreamSynchronize(v->own));
  }
  *n_points = (long)c.ext_written;
  if (n_dropped) *n_dropped = (long)(c.ext_total - c.ext_written);
  return 0;
}

extern "C" int odo_volume_extract(odo_volume* v, long capacity, float* xyz0, float* nrmw, long* n_points, long* n_dropped) {
  return volume_extract("odo_volume_extract", v, capacity, xyz0, nrmw, nullptr, n_points, n_dropped, false);
}

extern "C" int odo_volume_extract_colour(odo_volume* v, long capacity, float* xyz0, float* nrmw, uint8_t* rgba, long* n_points,
                                         long* n_dropped) {
  return volume_extract("odo_volume_extract_colour", v, capacity, xyz0, nrmw, rgba, n_points, n_dropped, true);
}

extern "C" int odo_volume_download(odo_volume* v, int16_t* q, uint16_t* w) {
  if (!v || (!q && !w)) return fail("odo_volume_download: NULL arg");
  if (volume_sync(v)) return -1;
  std::vector<uint32_t> host;
  try { host.resize((size_t)v->n_vox); } catch (...) { return fail("out of memory"); }
  HIP_OK(hipMemcpyAsync(host.data(), v->d_vox, sizeof(uint32_t) * (size_t)v->n_vox, hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  for (long i = 0; i < v->n_vox; i++) {
    if (q) q[i] = (int16_t)(host[(size_t)i] & 0xffffu);
    if (w) w[i] = (uint16_t)(host[(size_t)i] >> 16);
  }
  return 0;
}

extern "C" int odo_volume_upload(odo_volume* v, const int16_t* q, const uint16_t* w) {
  if (!v || !q || !w) return fail("odo_volume_upload: NULL arg (both arrays are required)");
  if (v->attached) return fail("odo_volume_upload: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)");
  std::vector<uint32_t> host;
  try { host.resize((size_t)v->n_vox); } catch (...) { return fail("out of memory"); }
  for (long i = 0; i < v->n_vox; i++) host[(size_t)i] = ((uint32_t)w[i] << 16) | (uint32_t)(uint16_t)q[i];
  HIP_OK(hipSetDevice(v->device));
  if (volume_order_on(v, v->own)) return -1;
  HIP_OK(hipMemcpyAsync(v->d_vox, host.data(), sizeof(uint32_t) * (size_t)v->n_vox, hipMemcpyHostToDevice, v->own));
  if (volume_mark(v, v->own)) return -1;
  HIP_OK(hipStreamSynchronize(v->own));   // (the staging buffer goes with this call)
  return 0;
}

// The mesh's scratch (5 B per voxel and the per-block counts): allocated by the first of odo_volume_mesh and
// odo_volume_enable_spill_mesh, which share it on the volume's own stream; kept until destroy.
static int volume_mesh_scratch(const char* who, odo_volume* v) {
  if (v->d_mesh_ctr) return 0;
  const int nblk = (int)((v->n_vox + kMeshBlock - 1) / kMeshBlock);
  bool ok = hipMalloc((void**)&v->d_mesh_mask, (size_t)v->n_vox) == hipSuccess &&
            hipMalloc((void**)&v->d_mesh_base, sizeof(uint32_t) * (size_t)v->n_vox) == hipSuccess &&
            hipMalloc((void**)&v->d_mesh_cnt, sizeof(unsigned) * 2 * (size_t)nblk) == hipSuccess &&
            hipMalloc((void**)&v->d_mesh_off, sizeof(unsigned long long) * 2 * (size_t)nblk) == hipSuccess &&
            hipMalloc((void**)&v->d_mesh_ctr, sizeof(MeshCounters)) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    void* ps[] = {v->d_mesh_mask, v->d_mesh_base, v->d_mesh_cnt, v->d_mesh_off, v->d_mesh_ctr};
    for (void* p : ps) if (p) (void)hipFree(p);
    v->d_mesh_mask = nullptr; v->d_mesh_base = nullptr; v->d_mesh_cnt = nullptr; v->d_mesh_off = nullptr; v->d_mesh_ctr = nullptr;
    return fail("%s: device allocation failed (scratch for %ld voxels)", who, v->n_vox);
  }
  return 0;
}

// odo_volume_mesh and, with_colour, odo_volume_mesh_colour (one launch more: the vertices' colours, skipped when no vertex is written).
static int volume_mesh(const char* who, odo_volume* v, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw, uint8_t* rgba,
                       int32_t* tri, long counts[4], bool with_colour) {
  if (!v || !counts || vertex_capacity < 0 || vertex_capacity > (1L << 28) || triangle_capacity < 0 || triangle_capacity > (1L << 28) ||
      (vertex_capacity > 0 && (!xyz0 || !nrmw || (with_colour && !rgba))) || (triangle_capacity > 0 && !tri))
    return fail("%s: bad arg (capacities 0 .. 2^28, buffers for `vertex_capacity` vertices and `triangle_capacity` triangles)", who);
  if (with_colour && !v->colour) return fail("%s: the volume has no colour grid (odo_volume_enable_colour first)", who);
  if (volume_sync(v)) return -1;
  const int nblk = (int)((v->n_vox + kMeshBlock - 1) / kMeshBlock);
  if (volume_mesh_scratch(who, v)) return -1;
  if (volume_grow((void**)&v->d_mesh_xyz0, &v->mesh_xyz0_capacity, vertex_capacity, sizeof(float4), who, "vertices") ||
      volume_grow((void**)&v->d_mesh_nrmw, &v->mesh_nrmw_capacity, vertex_capacity, sizeof(float4), who, "vertices") ||
      volume_grow((void**)&v->d_mesh_tri, &v->mesh_triangle_capacity, triangle_capacity, 3 * sizeof(int32_t), who, "triangles") ||
      (with_colour && volume_grow((void**)&v->d_mesh_rgba, &v->mesh_rgba_capacity, vertex_capacity, sizeof(uint32_t), who, "vertex colours")))
    return -1;
  VolMeshArgs a;
  memset(&a, 0, sizeof(a));
  a.g = volume_grid(v);
  a.n = (int)v->n_vox; a.nblk = nblk; a.vertex_capacity = vertex_capacity; a.triangle_capacity = triangle_capacity;
  a.edge_mask = v->d_mesh_mask; a.vertex_base = v->d_mesh_base; a.blk = v->d_mesh_cnt; a.blk_off = v->d_mesh_off; a.ctr = v->d_mesh_ctr;
  a.xyz0 = v->d_mesh_xyz0; a.nrmw = v->d_mesh_nrmw; a.tri = v->d_mesh_tri;
  launch_volume_mesh_count(a, v->own);
  HIP_OK(hipGetLastError());
  MeshCounters c;
  HIP_OK(hipMemcpyAsync(&c, v->d_mesh_ctr, sizeof(MeshCounters), hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  if (c.v_written > 0 || c.t_written > 0) {
    if (c.v_total > 0x7fffffffull)
      return fail("%s: %llu vertices: an index does not fit an int32 (totals are returned with both capacities 0)", who, c.v_total);
    launch_volume_mesh_emit(a, c.t_written > 0, v->own);
    HIP_OK(hipGetLastError());
    if (with_colour && c.v_written > 0) {
      VolMeshColourArgs ac;
      ac.a = a; ac.col = v->d_col; ac.rgba = v->d_mesh_rgba;
      launch_volume_mesh_colour(ac, v->own);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(rgba, v->d_mesh_rgba, sizeof(uint32_t) * (size_t)c.v_written, hipMemcpyDeviceToHost, v->own));
    }
    if (c.v_written > 0) {
      HIP_OK(hipMemcpyAsync(xyz0, v->d_mesh_xyz0, sizeof(float4) * (size_t)c.v_written, hipMemcpyDeviceToHost, v->own));
      HIP_OK(hipMemcpyAsync(nrmw, v->d_mesh_nrmw, sizeof(float4) * (size_t)c.v_written, hipMemcpyDeviceToHost, v->own));
    }
    if (c.t_written > 0) HIP_OK(hipMemcpyAsync(tri, v->d_mesh_tri, 3 * sizeof(int32_t) * (size_t)c.t_written, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipStreamSynchronize(v->own));
  }
  counts[0] = (long)c.v_written; counts[1] = (long)(c.v_total - c.v_written);
  counts[2] = (long)c.t_written; counts[3] = (long)(c.t_total - c.t_written);
  return 0;
}

extern "C" int odo_volume_mesh(odo_volume* v, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw, int32_t* tri,
                               long counts[4]) {
  return volume_mesh("odo_volume_mesh", v, vertex_capacity, triangle_capacity, xyz0, nrmw, nullptr, tri, counts, false);
}

extern "C" int odo_volume_mesh_colour(odo_volume* v, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw, uint8_t* rgba,
                                      int32_t* tri, long counts[4]) {
  return volume_mesh("odo_volume_mesh_colour", v, vertex_capacity, triangle_capacity, xyz0, nrmw, rgba, tri, counts, true);
}

// ---- ray-cast ----------------------------------------------------------------------------------------------------------------------
// Everything odo_volume_raycast_dev / odo_volume_raycast check before they look at the volume.
static int raycast_check(const char* who, const odo_raycast_params* rp, const float* A) {
  if (rp->rows < 1 || rp->rows > 4096 || rp->cols < 1 || rp->cols > 4096) return fail("%s: bad size %dx%d (1 .. 4096 each)", who, rp->rows, rp->cols);
  if (!(std::isfinite(rp->f) && rp->f > 0.0f)) return fail("%s: f must be finite and > 0", who);
  if (!(std::isfinite(rp->cx) && std::isfinite(rp->cy))) return fail("%s: cx and cy must be finite", who);
  if (!(std::isfinite(rp->t_min) && rp->t_min >= 0.0f)) return fail("%s: t_min must be finite and >= 0", who);
  if (!(std::isfinite(rp->step) && rp->step > 0.0f)) return fail("%s: step must be finite and > 0", who);
  if (rp->n_steps < 1 || rp->n_steps > 4096) return fail("%s: n_steps %d out of range (1 .. 4096)", who, rp->n_steps);
  if (!pose_finite(A)) return fail("%s: the pose has a non-finite entry (a frame whose Solve failed?)", who);
  return 0;
}

// The launch, on the volume's own stream behind the last change. The ray-cast is marked like a change: it reads the grid, and the
// next integration on another stream must not overtake it.
static int volume_raycast_launch(odo_volume* v, const odo_raycast_params* rp, const float* A, float* depth, uint16_t* raw, float4* nrmw,
                                 uint32_t* rgba) {
  HIP_OK(hipSetDevice(v->device));
  if (volume_order_on(v, v->own)) return -1;
  VolRaycastArgs a;
  memset(&a, 0, sizeof(a));
  a.vox = v->d_vox; a.col = v->d_col;
  a.nx = v->p.nx; a.ny = v->p.ny; a.nz = v->p.nz;
  a.rows = rp->rows; a.cols = rp->cols;
  a.f = rp->f; a.cx = rp->cx; a.cy = rp->cy; a.t_min = rp->t_min; a.step = rp->step; a.n_steps = rp->n_steps;
  a.depth_scale = v->p.depth_scale;
  float e[3], G[9];
  hostfp::raycast_frame(A, v->p.origin, v->p.voxel_size, e, G);
  a.ex = e[0]; a.ey = e[1]; a.ez = e[2];
  a.g00 = G[0]; a.g01 = G[1]; a.g02 = G[2]; a.g10 = G[3]; a.g11 = G[4]; a.g12 = G[5]; a.g20 = G[6]; a.g21 = G[7]; a.g22 = G[8];
  a.depth = depth; a.raw = raw; a.nrmw = nrmw; a.rgba = rgba;
  launch_volume_raycast(a, v->colour_sampling == 1, v->own);   // (the mode as it is now: nothing caches it)
  HIP_OK(hipGetLastError());
  return volume_mark(v, v->own);
}

extern "C" int odo_volume_set_colour_sampling(odo_volume* v, int mode) {
  if (!v) return fail("odo_volume_set_colour_sampling: NULL volume");
  if (mode != 0 && mode != 1) return fail("odo_volume_set_colour_sampling: mode %d (0 nearest, 1 trilinear)", mode);
  if (!v->colour) return fail("odo_volume_set_colour_sampling: the volume has no colour grid (odo_volume_enable_colour first)");
  v->colour_sampling = mode;
  return 0;
}

extern "C" int odo_volume_colour_sampling(odo_volume* v) {
  if (!v) return fail("odo_volume_colour_sampling: NULL volume");
  return v->colour_sampling;
}

extern "C" int odo_volume_raycast_dev(odo_volume* v, const odo_raycast_params* rp, const float abs_pose_colmajor[16], float* depth_dev,
                                      uint16_t* raw_dev, float* nrmw_dev, uint8_t* rgba_dev) {
  if (!v || !rp || !abs_pose_colmajor) return fail("odo_volume_raycast_dev: NULL arg");
  if (((uintptr_t)depth_dev & 3) || ((uintptr_t)raw_dev & 1) || ((uintptr_t)nrmw_dev & 15) || ((uintptr_t)rgba_dev & 3))
    return fail("odo_volume_raycast_dev: misaligned output (depth 4, raw 2, nrmw 16, rgba 4 bytes)");
  if (raycast_check("odo_volume_raycast_dev", rp, abs_pose_colmajor)) return -1;
  if (rgba_dev && !v->colour) return fail("odo_volume_raycast_dev: the volume has no colour grid (odo_volume_enable_colour first)");
  if (!depth_dev && !raw_dev && !nrmw_dev && !rgba_dev) return 0;   // nothing asked for
  return volume_raycast_launch(v, rp, abs_pose_colmajor, depth_dev, raw_dev, (float4*)nrmw_dev, (uint32_t*)rgba_dev);
}

// The ray-cast frames that the volume owns, for n pixels: depth, raw and normals, and the colours when asked for.
static int volume_ray_frames(const char* who, odo_volume* v, long n, bool with_colour) {
  if (n <= v->ray_depth_capacity && n <= v->ray_raw_capacity && n <= v->ray_nrmw_capacity && (!with_colour || n <= v->ray_rgba_capacity)) return 0;
  HIP_OK(hipStreamSynchronize(v->own));   // (an earlier ray-cast into these buffers has been waited for; be sure)
  if (volume_grow((void**)&v->d_ray_depth, &v->ray_depth_capacity, n, sizeof(float), who, "pixels") ||
      volume_grow((void**)&v->d_ray_raw, &v->ray_raw_capacity, n, sizeof(uint16_t), who, "pixels") ||
      volume_grow((void**)&v->d_ray_nrmw, &v->ray_nrmw_capacity, n, sizeof(float4), who, "pixels") ||
      (with_colour && volume_grow((void**)&v->d_ray_rgba, &v->ray_rgba_capacity, n, sizeof(uint32_t), who, "pixel colours")))
    return -1;
  return 0;
}

extern "C" int odo_volume_raycast(odo_volume* v, const odo_raycast_params* rp, const float abs_pose_colmajor[16], float* depth,
                                  uint16_t* raw, float* nrmw, uint8_t* rgba) {
  if (!v || !rp || !abs_pose_colmajor) return fail("odo_volume_raycast: NULL arg");
  if (raycast_check("odo_volume_raycast", rp, abs_pose_colmajor)) return -1;
  if (rgba && !v->colour) return fail("odo_volume_raycast: the volume has no colour grid (odo_volume_enable_colour first)");
  if (!depth && !raw && !nrmw && !rgba) return 0;
  HIP_OK(hipSetDevice(v->device));
  const long n = (long)rp->rows * rp->cols;
  if (volume_ray_frames("odo_volume_raycast", v, n, rgba != nullptr)) return -1;
  if (volume_raycast_launch(v, rp, abs_pose_colmajor, depth ? v->d_ray_depth : nullptr, raw ? v->d_ray_raw : nullptr,
                            nrmw ? v->d_ray_nrmw : nullptr, rgba ? v->d_ray_rgba : nullptr)) return -1;
  if (depth) HIP_OK(hipMemcpyAsync(depth, v->d_ray_depth, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, v->own));
  if (raw) HIP_OK(hipMemcpyAsync(raw, v->d_ray_raw, sizeof(uint16_t) * (size_t)n, hipMemcpyDeviceToHost, v->own));
  if (nrmw) HIP_OK(hipMemcpyAsync(nrmw, v->d_ray_nrmw, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, v->own));
  if (rgba) HIP_OK(hipMemcpyAsync(rgba, v->d_ray_rgba, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost, v->own));
  HIP_OK(hipStreamSynchronize(v->own));
  return 0;
}

// Diagnostic: one ray-cast to warm, then `reps` of them between two events on the volume's stream, into the frames the volume owns
// (depth and nrmw; rgba as well with_colour), under the colour sampling mode as it is. *us: microseconds per launch.
extern "C" int odo_volume_raycast_time(odo_volume* v, const odo_raycast_params* rp, const float abs_pose_colmajor[16], int with_colour,
                                       int reps, float* us) {
  const char* who = "odo_volume_raycast_time";
  if (!v || !rp || !abs_pose_colmajor || !us) return fail("%s: NULL arg", who);
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  if (raycast_check(who, rp, abs_pose_colmajor)) return -1;
  if (with_colour && !v->colour) return fail("%s: the volume has no colour grid (odo_volume_enable_colour first)", who);
  HIP_OK(hipSetDevice(v->device));
  if (volume_ray_frames(who, v, (long)rp->rows * rp->cols, with_colour != 0)) return -1;
  const auto cast = [&]() {
    return volume_raycast_launch(v, rp, abs_pose_colmajor, v->d_ray_depth, nullptr, v->d_ray_nrmw, with_colour ? v->d_ray_rgba : nullptr) == 0;
  };
  return time_stages(who, v->own, reps, 1, us, cast, [&](int) { return cast(); });
}

extern "C" int odo_volume_clear(odo_volume* v) {
  if (!v) return fail("NULL volume");
  HIP_OK(hipSetDevice(v->device));
  return volume_reset(v);
}

extern "C" int odo_volume_destroy(odo_volume* v) {
  if (!v) return 0;
  if (v->attached) return fail("odo_volume_destroy: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)");
  (void)hipSetDevice(v->device);
  if (v->last && v->last != v->own) (void)hipEventSynchronize(v->ev_last);
  (void)hipStreamSynchronize(v->own);
  return volume_release(v);
}
