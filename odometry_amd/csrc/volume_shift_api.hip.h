// volume_shift_api.hip.h — the moving TSDF volume (odo_volume_shift, _follow, _enable_spill, _spill_points, _window, _set_follow):
// the host side over the kernels of volume_shift_kernels.hip. The grid is shifted by whole voxels so that it follows the camera, and
// the surface points a shift would destroy are first appended to a device-resident store. Included by odometry_hip.hip behind
// volume_api.hip.h (the volume's object) and before tracker.hip.h (an attached tracker follows before it integrates).
//
// Nothing here waits for the device but odo_volume_spill_points and odo_volume_spill_mesh (and the diagnostics, odo_volume_shift_time,
// odo_volume_spill_mesh_time and the two guard hooks): a spill and a shift are five launches on the volume's own stream, a mesh spill
// (odo_volume_enable_spill_mesh) five or six more in front of the shift's, and a re-entry store
// (odo_volume_enable_reentry, volume_reentry_api.hip.h) two in front of the shift's and five behind it.
// The shift writes into the grids' second buffers and the host swaps the pointers when it enqueues: launches enqueued earlier hold
// the old pointers by value and are ordered in front by volume_order_on / volume_mark, and every later launcher reads v->d_vox,
// v->d_col and v->p.origin when it is called.
#pragma once
#include "volume_shift.hip.h"
#include "volume_shift_math.h"

// Test scaffolding, not part of the interface an integrator uses: every buffer of the spill store is allocated with a guard of this
// many points behind its capacity and filled with 0xAB once, guard included. A spill writes the points [written, written + count) and
// nothing else, so behind `written` every byte still holds 0xAB until the store is emptied for the first time:
// odo_debug_volume_spill_guard counts the bytes there that do not (held by tests/test_gpu_volume_shift.py).
constexpr long kSpillGuard = 64;

// One device allocation of a store: `items` of `item` bytes. kGuarded: kSpillGuard items more, all of it filled with 0xAB; kZeroed:
// cleared (the counters); kPlain: left as allocated (the passes' scratch). p == nullptr: not wanted (no colour, scratch that exists).
enum StoreFill { kPlain, kZeroed, kGuarded };
struct StoreBuf {
  void** p;
  size_t item, items;
  StoreFill fill;
};

// Allocates a store's buffers and fills them on the volume's own stream, behind whatever changed the volume last. Any failure: the
// stream is drained, every buffer allocated here is freed and its pointer nullptr again, false (the message is the caller's).
static bool volume_store_alloc(odo_volume* v, std::initializer_list<StoreBuf> bufs) {
  const auto bytes = [](const StoreBuf& b) { return b.item * (b.items + (b.fill == kGuarded ? (size_t)kSpillGuard : 0)); };
  bool ok = true;
  for (const StoreBuf& b : bufs) ok = ok && (!b.p || hipMalloc(b.p, bytes(b)) == hipSuccess);
  ok = ok && volume_order_on(v, v->own) == 0;
  for (const StoreBuf& b : bufs)
    ok = ok && (!b.p || b.fill == kPlain || hipMemsetAsync(*b.p, b.fill == kGuarded ? 0xAB : 0, bytes(b), v->own) == hipSuccess);
  ok = ok && volume_mark(v, v->own) == 0;
  if (ok) return true;
  (void)hipGetLastError();
  (void)hipStreamSynchronize(v->own);
  for (const StoreBuf& b : bufs) {
    if (b.p && *b.p) (void)hipFree(*b.p);
    if (b.p) *b.p = nullptr;
  }
  return false;
}

// The guard hooks: copies each span of device memory back and adds the bytes that are not 0xAB to *bad. at == nullptr: no such span.
struct GuardSpan {
  const void* at;
  size_t bytes;
};
static int volume_count_not_ab(odo_volume* v, std::initializer_list<GuardSpan> spans, long* bad) {
  size_t most = 0;
  for (const GuardSpan& g : spans) most = std::max(most, g.at ? g.bytes : 0);
  std::vector<uint8_t> host;
  try { host.resize(most); } catch (...) { return fail("out of memory"); }
  for (const GuardSpan& g : spans) {
    if (!g.at) continue;
    HIP_OK(hipMemcpyAsync(host.data(), g.at, g.bytes, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipStreamSynchronize(v->own));
    for (size_t i = 0; i < g.bytes; i++) *bad += host[i] != 0xAB;
  }
  return 0;
}

// The window's offsets after a shift by d, refused when an axis would leave the range that the origin's arithmetic is exact on.
static int volume_shift_window(const char* who, const odo_volume* v, const int d[3], int off[3]) {
  for (int c = 0; c < 3; c++)
    if (!shift_offset(v->off[c], d[c], &off[c]))
      return fail("%s: the window would be %lld voxels from where it was created on axis %d (at most 2^24)", who, (long long)v->off[c] + d[c], c);
  return 0;
}

// The grids' second buffers, which a shift writes into: allocated by the first of odo_volume_set_follow (so that an attached
// tracker's frame call never allocates), the first shift, and the first shift after odo_volume_enable_colour; kept until destroy.
static int volume_shift_buffers(const char* who, odo_volume* v) {
  HIP_OK(hipSetDevice(v->device));
  const size_t bytes = sizeof(uint32_t) * (size_t)v->n_vox;
  if (!v->d_vox2 && hipMalloc((void**)&v->d_vox2, bytes) != hipSuccess) {
    (void)hipGetLastError();
    v->d_vox2 = nullptr;
    return fail("%s: device allocation failed (the second voxel buffer, %ld voxels)", who, v->n_vox);
  }
  if (v->colour && !v->d_col2 && hipMalloc((void**)&v->d_col2, bytes) != hipSuccess) {
    (void)hipGetLastError();
    v->d_col2 = nullptr;
    return fail("%s: device allocation failed (the second colour buffer, %ld voxels)", who, v->n_vox);
  }
  return 0;
}

static VolSpillArgs volume_spill_args(odo_volume* v, const int d[3]) {
  VolSpillArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.a.g = volume_grid(v);
  sa.a.n = (int)v->n_vox; sa.a.nblk = (int)((v->n_vox + kVolExtBlock - 1) / kVolExtBlock); sa.a.capacity = v->spill_capacity;
  sa.a.wave_mask = v->d_wave; sa.a.blk = v->d_cnt; sa.a.blk_off = v->d_off;
  sa.a.xyz0 = v->d_spill_xyz0; sa.a.nrmw = v->d_spill_nrmw;
  sa.dx = d[0]; sa.dy = d[1]; sa.dz = d[2];
  // (a store made before odo_volume_enable_colour has no colours: its points are spilled without them)
  sa.col = v->d_spill_rgba ? v->d_col : nullptr; sa.rgba = v->d_spill_rgba;
  sa.sc = v->d_spill_ctr;
  return sa;
}

static VolSpillMeshArgs volume_spill_mesh_args(odo_volume* v, const int d[3]) {
  VolSpillMeshArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.a.g = volume_grid(v);
  sa.a.n = (int)v->n_vox; sa.a.nblk = (int)((v->n_vox + kMeshBlock - 1) / kMeshBlock);
  sa.a.vertex_capacity = v->smesh_vertex_capacity; sa.a.triangle_capacity = v->smesh_triangle_capacity;
  sa.a.edge_mask = v->d_mesh_mask; sa.a.vertex_base = v->d_mesh_base; sa.a.blk = v->d_mesh_cnt; sa.a.blk_off = v->d_mesh_off;
  sa.a.xyz0 = v->d_smesh_xyz0; sa.a.nrmw = v->d_smesh_nrmw; sa.a.tri = v->d_smesh_tri;
  sa.dx = d[0]; sa.dy = d[1]; sa.dz = d[2];
  // (a store made before odo_volume_enable_colour has no colours: its vertices are spilled without them)
  sa.col = v->d_smesh_rgba ? v->d_col : nullptr; sa.rgba = v->d_smesh_rgba;
  sa.sc = v->d_smesh_ctr;
  return sa;
}

static VolShiftArgs volume_shift_args(odo_volume* v, const int d[3]) {
  VolShiftArgs a;
  memset(&a, 0, sizeof(a));
  a.src = v->d_vox; a.dst = v->d_vox2;
  if (v->colour) { a.src_col = v->d_col; a.dst_col = v->d_col2; }
  a.nx = v->p.nx; a.ny = v->p.ny; a.nz = v->p.nz; a.n = (int)v->n_vox;
  a.dx = d[0]; a.dy = d[1]; a.dz = d[2];
  return a;
}

static VolReentryArgs volume_reentry_args(odo_volume* v, const int d[3], const int off_new[3]);   // (volume_reentry_api.hip.h)

// Spill (when the volume has a store) and shift by d, on the volume's own stream. 0: enqueued, or d = 0 and nothing to do.
static int volume_shift(const char* who, odo_volume* v, const int d[3]) {
  int off[3];
  if (volume_shift_window(who, v, d, off)) return -1;
  if (d[0] == 0 && d[1] == 0 && d[2] == 0) return 0;
  if (volume_shift_buffers(who, v)) return -1;
  if (volume_order_on(v, v->own)) return -1;
  if (v->spill_capacity > 0) {
    launch_volume_spill(volume_spill_args(v, d), v->own);
    HIP_OK(hipGetLastError());
  }
  if (v->smesh_vertex_capacity > 0) {
    launch_volume_spill_mesh(volume_spill_mesh_args(v, d), v->own);
    HIP_OK(hipGetLastError());
  }
  // (the re-entry store, DESIGN.md section 9.14: its arguments hold the grids and the store's two sets as they are in front of the swaps)
  const VolReentryArgs ra = v->re_capacity > 0 ? volume_reentry_args(v, d, off) : VolReentryArgs{};
  if (v->re_capacity > 0) launch_volume_reentry_save(ra, v->own);
  launch_volume_shift(volume_shift_args(v, d), v->own);
  if (v->re_capacity > 0) {
    launch_volume_reentry_store(ra, v->own);
    std::swap(v->d_re_ent, v->d_re_ent2);
    std::swap(v->d_re_col, v->d_re_col2);
  }
  HIP_OK(hipGetLastError());
  std::swap(v->d_vox, v->d_vox2);
  if (v->colour) std::swap(v->d_col, v->d_col2);
  for (int c = 0; c < 3; c++) v->off[c] = off[c];
  hostfp::window_origin(v->origin0, v->off, v->p.voxel_size, v->p.origin);
  return volume_mark(v, v->own);
}

extern "C" int odo_volume_shift(odo_volume* v, const int d[3]) {
  if (!v || !d) return fail("odo_volume_shift: NULL arg");
  return volume_shift("odo_volume_shift", v, d);
}

// Event timing (tools/volume_cost.py shift): batches of `reps` launches between events on the volume's own stream, the mean time of
// one in microseconds. us[0] the shift by d into the second buffers (not swapped: the grids and the window stay as they are); us[1]
// device-to-device hipMemcpyAsync of the same bytes (grid, and colour grid when there is one) into the second buffers; us[2]
// hipMemsetAsync of the second buffers; us[3 .. 5] the spill's count, scan and scatter for d (0 without a store). The scatter writes
// the store behind its counted points and the counters do not move, so the store's contents and counts read the same afterwards.
extern "C" int odo_volume_shift_time(odo_volume* v, const int d[3], int reps, float us[6]) {
  const char* who = "odo_volume_shift_time";
  if (!v || !d || !us) return fail("%s: NULL arg", who);
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  if (v->attached) return fail("%s: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)", who);
  if (volume_shift_buffers(who, v)) return -1;
  if (volume_order_on(v, v->own)) return -1;
  const VolShiftArgs a = volume_shift_args(v, d);
  const bool store = v->spill_capacity > 0;
  const VolSpillArgs sa = store ? volume_spill_args(v, d) : VolSpillArgs{};
  const size_t bytes = sizeof(uint32_t) * (size_t)v->n_vox;
  hipStream_t s = v->own;
  const auto warm = [&]() {
    launch_volume_shift(a, s);
    if (store) for (int st = 0; st < 3; st++) launch_volume_spill_stage(sa, st, s);
    return true;
  };
  const auto stage = [&](int q) {
    if (q == 0) launch_volume_shift(a, s);
    else if (q == 1) return hipMemcpyAsync(v->d_vox2, v->d_vox, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess &&
                            (!v->colour || hipMemcpyAsync(v->d_col2, v->d_col, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess);
    else if (q == 2) return hipMemsetAsync(v->d_vox2, 0, bytes, s) == hipSuccess && (!v->colour || hipMemsetAsync(v->d_col2, 0, bytes, s) == hipSuccess);
    else if (store) launch_volume_spill_stage(sa, q - 3, s);
    return true;
  };
  if (time_stages(who, s, reps, 6, us, warm, stage)) return -1;
  if (!store) us[3] = us[4] = us[5] = 0.0f;
  return volume_mark(v, s);
}

extern "C" int odo_volume_window(odo_volume* v, int off[3], float origin[3]) {
  if (!v) return fail("odo_volume_window: NULL volume");
  for (int c = 0; c < 3; c++) {
    if (off) off[c] = v->off[c];
    if (origin) origin[c] = v->p.origin[c];
  }
  return 0;
}

extern "C" int odo_volume_enable_spill(odo_volume* v, long capacity) {
  if (!v) return fail("odo_volume_enable_spill: NULL volume");
  if (capacity < 1 || capacity > (1L << 28)) return fail("odo_volume_enable_spill: capacity %ld out of range (1 .. 2^28)", capacity);
  if (v->spill_capacity > 0) return fail("odo_volume_enable_spill: the volume has a spill store already");
  if (v->attached) return fail("odo_volume_enable_spill: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)");
  HIP_OK(hipSetDevice(v->device));
  const int nblk = (int)((v->n_vox + kVolExtBlock - 1) / kVolExtBlock);
  // the extraction's scratch is the spill's too (both run on the volume's own stream); whichever comes first allocates all three
  const bool scratch = v->d_cnt != nullptr;
  const size_t n = (size_t)capacity;
  if (!volume_store_alloc(v, {{scratch ? nullptr : (void**)&v->d_wave, sizeof(unsigned long long), 3 * (kVolExtBlock / 64) * (size_t)nblk, kPlain},
                              {scratch ? nullptr : (void**)&v->d_off, sizeof(unsigned long long), (size_t)nblk, kPlain},
                              {scratch ? nullptr : (void**)&v->d_cnt, sizeof(int), (size_t)nblk, kPlain},
                              {(void**)&v->d_spill_xyz0, sizeof(float4), n, kGuarded},
                              {(void**)&v->d_spill_nrmw, sizeof(float4), n, kGuarded},
                              {v->colour ? (void**)&v->d_spill_rgba : nullptr, sizeof(uint32_t), n, kGuarded},
                              {(void**)&v->d_spill_ctr, sizeof(VolSpillCounters), 1, kZeroed}}))
    return fail("odo_volume_enable_spill: device allocation failed (%ld points)", capacity);
  v->spill_capacity = capacity;
  return 0;
}

extern "C" int odo_volume_spill_points(odo_volume* v, long capacity, float* xyz0, float* nrmw, uint8_t* rgba, long* n_points,
                                       long* n_dropped, int clear) {
  if (!v || !n_points || capacity < 0 || capacity > (1L << 28) || (capacity > 0 && (!xyz0 || !nrmw)))
    return fail("odo_volume_spill_points: bad arg (capacity 0 .. 2^28, buffers for `capacity` points)");
  if (v->spill_capacity <= 0) return fail("odo_volume_spill_points: the volume has no spill store (odo_volume_enable_spill first)");
  if (rgba && !v->d_spill_rgba)
    return fail("odo_volume_spill_points: the store has no colours (odo_volume_enable_colour before odo_volume_enable_spill)");
  VolSpillCounters c;
  if (volume_read_counters(v, v->d_spill_ctr, &c)) return -1;
  const size_t n = (size_t)std::min<unsigned long long>(c.written, (unsigned long long)capacity);
  if (n > 0) {
    HIP_OK(hipMemcpyAsync(xyz0, v->d_spill_xyz0, sizeof(float4) * n, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipMemcpyAsync(nrmw, v->d_spill_nrmw, sizeof(float4) * n, hipMemcpyDeviceToHost, v->own));
    if (rgba) HIP_OK(hipMemcpyAsync(rgba, v->d_spill_rgba, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipStreamSynchronize(v->own));
  }
  if (clear) {
    HIP_OK(hipMemsetAsync(v->d_spill_ctr, 0, sizeof(VolSpillCounters), v->own));
    if (volume_mark(v, v->own)) return -1;
  }
  *n_points = (long)n;
  if (n_dropped) *n_dropped = (long)(c.total - c.written);
  return 0;
}

extern "C" int odo_debug_volume_spill_guard(odo_volume* v, long* n_changed) {
  if (!v || !n_changed) return fail("odo_debug_volume_spill_guard: NULL arg");
  if (v->spill_capacity <= 0) return fail("odo_debug_volume_spill_guard: the volume has no spill store (odo_volume_enable_spill first)");
  VolSpillCounters c;
  if (volume_read_counters(v, v->d_spill_ctr, &c)) return -1;
  const size_t from = (size_t)std::min<unsigned long long>(c.written, (unsigned long long)v->spill_capacity);
  const size_t points = (size_t)(v->spill_capacity + kSpillGuard) - from;
  long bad = 0;
  if (volume_count_not_ab(v, {{v->d_spill_xyz0 + from, sizeof(float4) * points}, {v->d_spill_nrmw + from, sizeof(float4) * points},
                              {v->d_spill_rgba ? v->d_spill_rgba + from : nullptr, sizeof(uint32_t) * points}}, &bad)) return -1;
  *n_changed = bad;
  return 0;
}

// ---- the mesh store ---------------------------------------------------------------------------------------
// As the point store: every buffer has a guard of kSpillGuard items behind its capacity and is filled with 0xAB once. The mesh's
// scratch is allocated here when no mesh was asked for yet, so that no shift (no frame call of an attached tracker) allocates.
extern "C" int odo_volume_enable_spill_mesh(odo_volume* v, long vertex_capacity, long triangle_capacity) {
  const char* who = "odo_volume_enable_spill_mesh";
  if (!v) return fail("%s: NULL volume", who);
  if (vertex_capacity < 1 || vertex_capacity > (1L << 28) || triangle_capacity < 1 || triangle_capacity > (1L << 28))
    return fail("%s: capacities %ld, %ld out of range (1 .. 2^28 each)", who, vertex_capacity, triangle_capacity);
  if (v->smesh_vertex_capacity > 0) return fail("%s: the volume has a mesh store already", who);
  if (v->attached) return fail("%s: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)", who);
  HIP_OK(hipSetDevice(v->device));
  if (volume_mesh_scratch(who, v)) return -1;
  const size_t nv = (size_t)vertex_capacity, nt = (size_t)triangle_capacity;
  if (!volume_store_alloc(v, {{(void**)&v->d_smesh_xyz0, sizeof(float4), nv, kGuarded},
                              {(void**)&v->d_smesh_nrmw, sizeof(float4), nv, kGuarded},
                              {v->colour ? (void**)&v->d_smesh_rgba : nullptr, sizeof(uint32_t), nv, kGuarded},
                              {(void**)&v->d_smesh_tri, 3 * sizeof(int), nt, kGuarded},
                              {(void**)&v->d_smesh_ctr, sizeof(VolSpillMeshCounters), 1, kZeroed}}))
    return fail("%s: device allocation failed (%ld vertices, %ld triangles)", who, vertex_capacity, triangle_capacity);
  v->smesh_vertex_capacity = vertex_capacity; v->smesh_triangle_capacity = triangle_capacity;
  return 0;
}

extern "C" int odo_volume_spill_mesh(odo_volume* v, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw, uint8_t* rgba,
                                     int32_t* tri, long* n_vertices, long* n_triangles, long dropped[2], int clear) {
  const char* who = "odo_volume_spill_mesh";
  if (!v || !n_vertices || !n_triangles || vertex_capacity < 0 || vertex_capacity > (1L << 28) || triangle_capacity < 0 ||
      triangle_capacity > (1L << 28) || (vertex_capacity > 0 && (!xyz0 || !nrmw)) || (triangle_capacity > 0 && !tri))
    return fail("%s: bad arg (capacities 0 .. 2^28, buffers for `vertex_capacity` vertices and `triangle_capacity` triangles)", who);
  if (v->smesh_vertex_capacity <= 0) return fail("%s: the volume has no mesh store (odo_volume_enable_spill_mesh first)", who);
  if (rgba && !v->d_smesh_rgba)
    return fail("%s: the store has no colours (odo_volume_enable_colour before odo_volume_enable_spill_mesh)", who);
  VolSpillMeshCounters c;
  if (volume_read_counters(v, v->d_smesh_ctr, &c)) return -1;
  *n_vertices = (long)c.v_written;
  *n_triangles = (long)c.t_written;
  if (dropped) { dropped[0] = (long)(c.v_total - c.v_written); dropped[1] = (long)(c.t_total - c.t_written); }
  const bool query = vertex_capacity == 0 && triangle_capacity == 0;
  if (!query && (c.v_written > (unsigned long long)vertex_capacity || c.t_written > (unsigned long long)triangle_capacity))
    return fail("%s: the store holds %llu vertices and %llu triangles, the buffers %ld and %ld: a cut would leave triangles without "
                "their vertices (nothing copied, nothing cleared; the counts are returned)", who, c.v_written, c.t_written,
                vertex_capacity, triangle_capacity);
  if (!query) {
    const size_t nv = (size_t)c.v_written, nt = (size_t)c.t_written;
    if (nv > 0) {
      HIP_OK(hipMemcpyAsync(xyz0, v->d_smesh_xyz0, sizeof(float4) * nv, hipMemcpyDeviceToHost, v->own));
      HIP_OK(hipMemcpyAsync(nrmw, v->d_smesh_nrmw, sizeof(float4) * nv, hipMemcpyDeviceToHost, v->own));
      if (rgba) HIP_OK(hipMemcpyAsync(rgba, v->d_smesh_rgba, sizeof(uint32_t) * nv, hipMemcpyDeviceToHost, v->own));
    }
    if (nt > 0) HIP_OK(hipMemcpyAsync(tri, v->d_smesh_tri, 3 * sizeof(int32_t) * nt, hipMemcpyDeviceToHost, v->own));
    HIP_OK(hipStreamSynchronize(v->own));
  }
  if (clear) {
    HIP_OK(hipMemsetAsync(v->d_smesh_ctr, 0, sizeof(VolSpillMeshCounters), v->own));
    if (volume_mark(v, v->own)) return -1;
  }
  return 0;
}

// Event timing of the mesh spill's five stages for d, as odo_volume_shift_time times the point spill's: batches of `reps` launches
// between events. The advance kernel is not run, so the counters do not move: the emitting stages write the store behind its
// counted items (or nothing, when the spill would not fit), and its contents and counts read the same afterwards.
extern "C" int odo_volume_spill_mesh_time(odo_volume* v, const int d[3], int reps, float us[5]) {
  const char* who = "odo_volume_spill_mesh_time";
  if (!v || !d || !us) return fail("%s: NULL arg", who);
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  if (v->smesh_vertex_capacity <= 0) return fail("%s: the volume has no mesh store (odo_volume_enable_spill_mesh first)", who);
  if (v->attached) return fail("%s: the volume is attached to a tracker (odo_tracker_attach_volume(t, NULL) first)", who);
  HIP_OK(hipSetDevice(v->device));
  if (volume_order_on(v, v->own)) return -1;
  const VolSpillMeshArgs sa = volume_spill_mesh_args(v, d);
  hipStream_t s = v->own;
  const auto stage = [&](int st) { launch_volume_spill_mesh_stage(sa, st, s); return true; };
  const auto warm = [&]() { for (int st = 0; st < 5; st++) stage(st); return true; };
  if (time_stages(who, s, reps, 5, us, warm, stage)) return -1;
  if (!sa.col) us[4] = 0.0f;
  return volume_mark(v, s);
}

extern "C" int odo_debug_volume_spill_mesh_guard(odo_volume* v, long* n_changed) {
  const char* who = "odo_debug_volume_spill_mesh_guard";
  if (!v || !n_changed) return fail("%s: NULL arg", who);
  if (v->smesh_vertex_capacity <= 0) return fail("%s: the volume has no mesh store (odo_volume_enable_spill_mesh first)", who);
  VolSpillMeshCounters c;
  if (volume_read_counters(v, v->d_smesh_ctr, &c)) return -1;
  const size_t vfrom = (size_t)std::min<unsigned long long>(c.v_written, (unsigned long long)v->smesh_vertex_capacity);
  const size_t tfrom = (size_t)std::min<unsigned long long>(c.t_written, (unsigned long long)v->smesh_triangle_capacity);
  const size_t nv = (size_t)(v->smesh_vertex_capacity + kSpillGuard) - vfrom, nt = (size_t)(v->smesh_triangle_capacity + kSpillGuard) - tfrom;
  long bad = 0;
  if (volume_count_not_ab(v, {{v->d_smesh_xyz0 + vfrom, sizeof(float4) * nv}, {v->d_smesh_nrmw + vfrom, sizeof(float4) * nv},
                              {v->d_smesh_rgba ? v->d_smesh_rgba + vfrom : nullptr, sizeof(uint32_t) * nv},
                              {v->d_smesh_tri + 3 * tfrom, 3 * sizeof(int32_t) * nt}}, &bad)) return -1;
  *n_changed = bad;
  return 0;
}

extern "C" int odo_volume_set_follow(odo_volume* v, const odo_volume_follow_params* p) {
  if (!v) return fail("odo_volume_set_follow: NULL volume");
  if (!p) { v->follow = 0; return 0; }
  if (!(std::isfinite(p->focus) && p->focus >= 0.0f)) return fail("odo_volume_set_follow: focus must be finite and >= 0");
  if (p->threshold < 1) return fail("odo_volume_set_follow: threshold %d (at least 1 voxel)", p->threshold);
  if (volume_shift_buffers("odo_volume_set_follow", v)) return -1;   // (here, not in an attached tracker's frame call)
  v->fp = *p; v->follow = 1;
  return 0;
}

// The follow step: the shift that the pose asks for (volume_shift_math.h, follow_shift), applied. d_out may be nullptr.
static int volume_follow(const char* who, odo_volume* v, const float* A, int* d_out) {
  if (!v->follow) return fail("%s: no follow parameters (odo_volume_set_follow first)", who);
  const int n[3] = {v->p.nx, v->p.ny, v->p.nz};
  int d[3];
  if (!follow_shift(A, v->p.origin, n, v->p.voxel_size, v->fp.focus, v->fp.threshold, d))
    return fail("%s: the pose has a non-finite entry (a frame whose Solve failed?)", who);
  if (volume_shift(who, v, d)) return -1;
  if (d_out) for (int c = 0; c < 3; c++) d_out[c] = d[c];
  return 0;
}

extern "C" int odo_volume_follow(odo_volume* v, const float abs_pose_colmajor[16], int d_out[3]) {
  if (!v || !abs_pose_colmajor) return fail("odo_volume_follow: NULL arg");
  if (!pose_finite(abs_pose_colmajor)) return fail("odo_volume_follow: the pose has a non-finite entry (a frame whose Solve failed?)");
  return volume_follow("odo_volume_follow", v, abs_pose_colmajor, d_out);
}
