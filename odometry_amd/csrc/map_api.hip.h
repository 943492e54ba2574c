// map_api.hip.h — the keyframe point-cloud map (odo_map_*): the host object over the insertion kernels of map_kernels.hip.
// Replaces the reference's GlobalMap keyframe holder (include/global_map.h, GlobalMap::InsertKeyFrame) and the host-side
// export of save_to_vis (run_odometry_kitti_offline.cpp:432-471): the keyframes' points are back-projected, voxel-filtered
// and appended on the device. Included by odometry_hip.hip before tracker.hip.h (the tracker inserts its keyframes).
#pragma once
#include "map.hip.h"

struct odo_map {
  odo_ctx* ctx;                 // standalone insertions (odo_map_insert_dev) run on its stream
  int device;
  hipStream_t own;              // the attached tracker's insertions, downloads, clears
  hipEvent_t ev_last;           // behind the last operation that changed the map, on `last`
  hipStream_t last;             // stream of that operation, nullptr: none yet
  int rows, cols, nblk;
  long capacity;
  float voxel;
  unsigned long long slots;
  unsigned long long *d_keys, *d_payload, *d_wave;
  int *d_pix, *d_blk, *d_off;
  MapCounters* d_ctr;
  float4* d_xyzi;
  int2* d_kp;
  long n_ins;                   // insertions so far (the next insertion's keyframe number)
  std::vector<float> poses;     // 16 per insertion, column-major
  odo_tracker* attached;
};

static int map_release(odo_map* m) {
  void* ps[] = {m->d_keys, m->d_payload, m->d_wave, m->d_pix, m->d_blk, m->d_off, m->d_ctr, m->d_xyzi, m->d_kp};
  for (void* p : ps) if (p) (void)hipFree(p);
  if (m->ev_last) (void)hipEventDestroy(m->ev_last);
  if (m->own) (void)hipStreamDestroy(m->own);
  delete m;
  return 0;
}

// Everything that changed the map so far is ordered before the next operation on stream s.
static int map_order_on(odo_map* m, hipStream_t s) {
  if (m->last && m->last != s) HIP_OK(hipStreamWaitEvent(s, m->ev_last, 0));
  return 0;
}
static int map_mark(odo_map* m, hipStream_t s) {
  HIP_OK(hipEventRecord(m->ev_last, s));
  m->last = s;
  return 0;
}
// Waits for every pending insertion; afterwards the map's own stream is idle and ordered after them.
static int map_sync(odo_map* m) {
  HIP_OK(hipSetDevice(m->device));
  if (map_order_on(m, m->own)) return -1;
  HIP_OK(hipStreamSynchronize(m->own));
  return 0;
}
static int map_reset(odo_map* m) {
  if (map_order_on(m, m->own)) return -1;
  HIP_OK(hipMemsetAsync(m->d_keys, 0xff, sizeof(unsigned long long) * m->slots, m->own));
  HIP_OK(hipMemsetAsync(m->d_payload, 0xff, sizeof(unsigned long long) * m->slots, m->own));
  HIP_OK(hipMemsetAsync(m->d_ctr, 0, sizeof(MapCounters), m->own));
  m->n_ins = 0;
  m->poses.clear();
  return map_mark(m, m->own);
}

extern "C" int odo_map_create(odo_ctx* ctx, int rows, int cols, long capacity, float voxel_size, odo_map** out) {
  if (!ctx || !out) return fail("odo_map_create: NULL arg");
  *out = nullptr;
  if (rows < 1 || cols < 1 || (long long)rows * cols > (1 << 28)) return fail("odo_map_create: bad size %dx%d", rows, cols);
  if (capacity < 1 || capacity > (1L << 28)) return fail("odo_map_create: capacity %ld out of range (1 .. 2^28)", capacity);
  if (!(voxel_size >= 0.0f) || isinf(voxel_size)) return fail("odo_map_create: voxel_size must be finite and >= 0");
  HIP_OK(hipSetDevice(ctx->device));
  odo_map* m = new (std::nothrow) odo_map();
  if (!m) return fail("out of memory");
  m->ctx = ctx; m->device = ctx->device; m->own = nullptr; m->ev_last = nullptr; m->last = nullptr;
  m->rows = rows; m->cols = cols; m->capacity = capacity; m->voxel = voxel_size;
  const long n = (long)rows * cols;
  m->nblk = (int)((n + kMapBlock - 1) / kMapBlock);
  m->slots = 1;
  // a power of two >= 2 (capacity + rows * cols): the most keys the table can ever hold (map_claim_kernel)
  if (voxel_size > 0.0f) while (m->slots < 2ull * (unsigned long long)(capacity + n)) m->slots <<= 1;
  m->d_keys = m->d_payload = m->d_wave = nullptr; m->d_pix = m->d_blk = m->d_off = nullptr; m->d_ctr = nullptr;
  m->d_xyzi = nullptr; m->d_kp = nullptr;
  m->n_ins = 0; m->attached = nullptr;
  bool ok = hipStreamCreateWithFlags(&m->own, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&m->ev_last, hipEventDisableTiming) == hipSuccess &&
            hipMalloc((void**)&m->d_keys, sizeof(unsigned long long) * m->slots) == hipSuccess &&
            hipMalloc((void**)&m->d_payload, sizeof(unsigned long long) * m->slots) == hipSuccess &&
            hipMalloc((void**)&m->d_wave, sizeof(unsigned long long) * (kMapBlock / 64) * m->nblk) == hipSuccess &&
            hipMalloc((void**)&m->d_pix, sizeof(int) * n) == hipSuccess &&
            hipMalloc((void**)&m->d_blk, sizeof(int) * 3 * m->nblk) == hipSuccess &&
            hipMalloc((void**)&m->d_off, sizeof(int) * m->nblk) == hipSuccess &&
            hipMalloc((void**)&m->d_ctr, sizeof(MapCounters)) == hipSuccess &&
            hipMalloc((void**)&m->d_xyzi, sizeof(float4) * capacity) == hipSuccess &&
            hipMalloc((void**)&m->d_kp, sizeof(int2) * capacity) == hipSuccess;
  ok = ok && map_reset(m) == 0 && map_sync(m) == 0;
  if (!ok) {
    (void)hipGetLastError();
    map_release(m);
    return fail("odo_map_create: device allocation failed (%ld points, %llu hash slots)", capacity, m->slots);
  }
  *out = m;
  return 0;
}

// One insertion on stream s (async). Inputs: rows x cols device buffers.
static int map_insert(odo_map* m, const uint8_t* val, const float* dep, const float* img, const odo_intrinsics* K, const float* A,
                      hipStream_t s) {
  if (m->n_ins >= 0x7fffffffL) return fail("odo_map_insert: too many insertions");
  HIP_OK(hipSetDevice(m->device));
  if (map_order_on(m, s)) return -1;
  MapInsertArgs a;
  memset(&a, 0, sizeof(a));
  a.val = val; a.dep = dep; a.img = img;
  a.rows = m->rows; a.cols = m->cols; a.n = m->rows * m->cols; a.nblk = m->nblk;
  a.f0 = K->f0; a.cx0 = K->cx0; a.cy0 = K->cy0;
  a.a0 = A[0]; a.a1 = A[1]; a.a2 = A[2]; a.a4 = A[4]; a.a5 = A[5]; a.a6 = A[6];
  a.a8 = A[8]; a.a9 = A[9]; a.a10 = A[10]; a.a12 = A[12]; a.a13 = A[13]; a.a14 = A[14];
  a.voxel = m->voxel; a.ins = (unsigned)m->n_ins; a.capacity = m->capacity; a.slot_mask = m->slots - 1;
  a.keys = m->d_keys; a.payload = m->d_payload; a.pix_slot = m->d_pix; a.wave_mask = m->d_wave; a.blk = m->d_blk; a.blk_off = m->d_off;
  a.ctr = m->d_ctr; a.xyzi = m->d_xyzi; a.kf_pixel = m->d_kp;
  launch_map_insert(a, s);
  HIP_OK(hipGetLastError());
  m->poses.insert(m->poses.end(), A, A + 16);
  m->n_ins++;
  return map_mark(m, s);
}

extern "C" int odo_map_insert_dev(odo_map* m, const uint8_t* val_dev, const float* dep_dev, const float* img_dev,
                                  const odo_intrinsics* K, const float abs_pose_colmajor[16]) {
  if (!m || !dep_dev || !abs_pose_colmajor) return fail("odo_map_insert_dev: NULL arg");
  return map_insert(m, val_dev, dep_dev, img_dev, K ? K : &kKitti00, abs_pose_colmajor, m->ctx->stream);
}

static int map_counters(odo_map* m, MapCounters* c) {
  if (map_sync(m)) return -1;
  HIP_OK(hipMemcpyAsync(c, m->d_ctr, sizeof(MapCounters), hipMemcpyDeviceToHost, m->own));
  HIP_OK(hipStreamSynchronize(m->own));
  return 0;
}

extern "C" long odo_map_size(odo_map* m) {
  if (!m) return fail("NULL map");
  MapCounters c;
  if (map_counters(m, &c)) return -1;
  return (long)c.size;
}

extern "C" int odo_map_download(odo_map* m, long first, long count, float* xyzi, int* kf_pixel) {
  if (!m || (!xyzi && count > 0) || first < 0 || count < 0) return fail("odo_map_download: bad arg");
  MapCounters c;
  if (map_counters(m, &c)) return -1;
  if (first + count > (long)c.size) return fail("odo_map_download: points %ld .. %ld requested, the map holds %llu", first, first + count, c.size);
  if (count == 0) return 0;
  HIP_OK(hipMemcpyAsync(xyzi, m->d_xyzi + first, sizeof(float4) * count, hipMemcpyDeviceToHost, m->own));
  if (kf_pixel) HIP_OK(hipMemcpyAsync(kf_pixel, m->d_kp + first, sizeof(int2) * count, hipMemcpyDeviceToHost, m->own));
  HIP_OK(hipStreamSynchronize(m->own));
  return 0;
}

extern "C" int odo_map_stats(odo_map* m, long out[6]) {
  if (!m || !out) return fail("odo_map_stats: NULL arg");
  MapCounters c;
  if (map_counters(m, &c)) return -1;
  out[0] = (long)c.size; out[1] = m->n_ins; out[2] = (long)c.candidates;
  out[3] = (long)c.dropped_voxel; out[4] = (long)c.dropped_range; out[5] = (long)c.dropped_capacity;
  return 0;
}

// Test only (include/odometry_hip.h): the hash table as it stands, held slot by slot by tests/test_gpu_map_hash_cases.py.
extern "C" int odo_debug_map_table(odo_map* m, unsigned long long n_slots_cap, unsigned long long* keys, unsigned long long* payload,
                                   unsigned long long* n_slots) {
  if (!m || !keys || !payload || !n_slots) return fail("odo_debug_map_table: NULL arg");
  *n_slots = m->slots;
  if (!(m->voxel > 0.0f)) return fail("odo_debug_map_table: the map has no voxel filter (voxel_size == 0)");
  if (n_slots_cap < m->slots) return fail("odo_debug_map_table: room for %llu slots, the table has %llu", n_slots_cap, m->slots);
  if (map_sync(m)) return -1;
  const size_t bytes = sizeof(unsigned long long) * (size_t)m->slots;
  HIP_OK(hipMemcpyAsync(keys, m->d_keys, bytes, hipMemcpyDeviceToHost, m->own));
  HIP_OK(hipMemcpyAsync(payload, m->d_payload, bytes, hipMemcpyDeviceToHost, m->own));
  HIP_OK(hipStreamSynchronize(m->own));
  return 0;
}

extern "C" int odo_map_keyframe_pose(const odo_map* m, int keyframe, float abs_pose_colmajor[16]) {
  if (!m || !abs_pose_colmajor) return fail("odo_map_keyframe_pose: NULL arg");
  if (keyframe < 0 || keyframe >= m->n_ins) return fail("odo_map_keyframe_pose: keyframe %d of %ld", keyframe, m->n_ins);
  memcpy(abs_pose_colmajor, m->poses.data() + 16 * (size_t)keyframe, sizeof(float) * 16);
  return 0;
}

extern "C" int odo_map_clear(odo_map* m) {
  if (!m) return fail("NULL map");
  HIP_OK(hipSetDevice(m->device));
  return map_reset(m);
}

extern "C" int odo_map_destroy(odo_map* m) {
  if (!m) return 0;
  if (m->attached) return fail("odo_map_destroy: the map is attached to a tracker (odo_tracker_attach_map(t, NULL) first)");
  (void)hipSetDevice(m->device);
  if (m->last && m->last != m->own) (void)hipEventSynchronize(m->ev_last);
  (void)hipStreamSynchronize(m->own);
  return map_release(m);
}
