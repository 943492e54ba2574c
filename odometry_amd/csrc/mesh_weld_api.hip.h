// mesh_weld_api.hip.h — the mesh welder (odo_mesh_weld_*): the host object over the kernels of mesh_weld_kernels.hip. A mesh on the
// device in, the welded mesh in the welder's own buffers out; every pass's launches go to the CONTEXT's stream with no host wait, so
// the ordering rules are those of the speckle filter (speckle_api.hip.h). Included by odometry_hip.hip.
#pragma once
#include "mesh_weld.hip.h"

struct odo_mesh_weld {
  odo_ctx* ctx;
  int device;
  odo_mesh_weld_params p;
  uint32_t vslots, tslots;
  int vblocks, tblocks;            // workgroups at the capacities: the rows of the per-block counts
  char* d_block;                   // the one device allocation everything below lies in
  size_t block_bytes;
  float4* d_xyz0[2];               // the two sets of output buffers: pass k writes set k & 1
  float4* d_nrmw[2];
  uint32_t* d_rgba[2];             // NULL without colour
  int32_t* d_tri[2];
  unsigned long long* d_vkeys;
  uint32_t* d_vmin;
  int32_t* d_ttab;
  int32_t* d_vaux;
  int32_t* d_rep;
  uint8_t* d_vref;
  int32_t* d_rtri;
  int32_t* d_tslot;
  uint32_t* d_vblk;
  uint32_t* d_tblk;
  unsigned long long* d_vblk_off;
  unsigned long long* d_tblk_off;
  WeldState* d_state;              // [kWeldMaxPasses + 1], zero until the first run
  unsigned long long* d_ctr;       // [kWeldStatWords], zero until the first run
  int last_passes;                 // of the last run enqueued: its result is state[last_passes], in set (last_passes - 1) & 1
  int last_colour;                 // ... and whether it carried colours
};

// Lays the welder's blocks out behind one another, each on a 256-byte boundary: the pointers when base is given, the size always.
static size_t mw_carve(odo_mesh_weld* w, char* base) {
  size_t off = 0;
  const auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
  const size_t nv = (size_t)w->p.vertex_capacity, nt = (size_t)w->p.triangle_capacity;
  for (int k = 0; k < 2; k++) {
    w->d_xyz0[k] = (float4*)take(sizeof(float4) * nv);
    w->d_nrmw[k] = (float4*)take(sizeof(float4) * nv);
    w->d_rgba[k] = w->p.colour ? (uint32_t*)take(sizeof(uint32_t) * nv) : nullptr;
    w->d_tri[k] = (int32_t*)take(sizeof(int32_t) * 3 * nt);
  }
  w->d_vkeys = (unsigned long long*)take(sizeof(unsigned long long) * w->vslots);
  w->d_vmin = (uint32_t*)take(sizeof(uint32_t) * w->vslots);
  w->d_ttab = (int32_t*)take(sizeof(int32_t) * w->tslots);
  w->d_vaux = (int32_t*)take(sizeof(int32_t) * nv);
  w->d_rep = (int32_t*)take(sizeof(int32_t) * nv);
  w->d_vref = (uint8_t*)take(nv);
  w->d_rtri = (int32_t*)take(sizeof(int32_t) * 3 * nt);
  w->d_tslot = (int32_t*)take(sizeof(int32_t) * nt);
  w->d_vblk = (uint32_t*)take(sizeof(uint32_t) * w->vblocks);
  w->d_tblk = (uint32_t*)take(sizeof(uint32_t) * w->tblocks);
  w->d_vblk_off = (unsigned long long*)take(sizeof(unsigned long long) * w->vblocks);
  w->d_tblk_off = (unsigned long long*)take(sizeof(unsigned long long) * w->tblocks);
  w->d_state = (WeldState*)take(sizeof(WeldState) * (kWeldMaxPasses + 1));
  w->d_ctr = (unsigned long long*)take(sizeof(unsigned long long) * kWeldStatWords);
  return off;
}

extern "C" int odo_mesh_weld_create(odo_ctx* ctx, const odo_mesh_weld_params* p, odo_mesh_weld** out) {
  const char* who = "odo_mesh_weld_create";
  if (!ctx || !p || !out) return fail("%s: NULL arg", who);
  switch (weld_check_create(p->vertex_capacity, p->triangle_capacity, p->colour)) {
    case 0: break;
    case 1: return fail("%s: vertex_capacity %d out of range (1 .. %d)", who, p->vertex_capacity, kWeldMaxCapacity);
    case 2: return fail("%s: triangle_capacity %d out of range (1 .. %d)", who, p->triangle_capacity, kWeldMaxCapacity);
    default: return fail("%s: colour %d is not 0 or 1", who, p->colour);
  }
  HIP_OK(hipSetDevice(ctx->device));
  odo_mesh_weld* w = new (std::nothrow) odo_mesh_weld();
  if (!w) return fail("out of memory");
  memset((void*)w, 0, sizeof(*w));
  w->ctx = ctx; w->device = ctx->device; w->p = *p;
  w->vslots = weld_slots(p->vertex_capacity);
  w->tslots = weld_slots(p->triangle_capacity);
  w->vblocks = weld_blocks(p->vertex_capacity);
  w->tblocks = weld_blocks(p->triangle_capacity);
  w->block_bytes = mw_carve(w, nullptr);
  bool ok = hipMalloc((void**)&w->d_block, w->block_bytes) == hipSuccess;
  if (ok) {
    mw_carve(w, w->d_block);
    ok = hipMemsetAsync(w->d_state, 0, sizeof(WeldState) * (kWeldMaxPasses + 1), ctx->stream) == hipSuccess &&
         hipMemsetAsync(w->d_ctr, 0, sizeof(unsigned long long) * kWeldStatWords, ctx->stream) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(ctx->stream);
    if (w->d_block) (void)hipFree(w->d_block);
    delete w;
    return fail("%s: device allocation failed (%d vertices, %d triangles)", who, p->vertex_capacity, p->triangle_capacity);
  }
  *out = w;
  return 0;
}

// Everything odo_mesh_weld_run_dev refuses, in two halves: what the arguments alone decide, before the welder is read, then what its
// capacities and its buffers decide. -1 with the reason named, 0 when the run may be enqueued.
static int mw_check_run(const char* who, const odo_mesh_weld* w, const odo_mesh_weld_rule* rule, long n_v, long n_t, const float* xyz0,
                        const float* nrmw, const uint8_t* rgba, const int32_t* tri) {
  if (!w || !rule) return fail("%s: NULL arg", who);
  switch (weld_check_rule(rule->eps, rule->origin, rule->grids, rule->drop_unreferenced)) {
    case 0: break;
    case 1: return fail("%s: eps must be finite and > 0", who);
    case 2: return fail("%s: origin must be finite", who);
    case 3: return fail("%s: grids %d is not 1 or 8", who, rule->grids);
    default: return fail("%s: drop_unreferenced %d is not 0 or 1", who, rule->drop_unreferenced);
  }
  if (n_v < 0 || n_v > kWeldMaxCapacity) return fail("%s: n_vertices %ld out of range (0 .. %d)", who, n_v, kWeldMaxCapacity);
  if (n_t < 0 || n_t > kWeldMaxCapacity) return fail("%s: n_triangles %ld out of range (0 .. %d)", who, n_t, kWeldMaxCapacity);
  if ((n_v > 0 && (!xyz0 || !nrmw)) || (n_t > 0 && !tri)) return fail("%s: NULL mesh", who);
  if ((((uintptr_t)xyz0 | (uintptr_t)nrmw) & 15) || (((uintptr_t)rgba | (uintptr_t)tri) & 3))
    return fail("%s: misaligned pointer (16 bytes for xyz0 and nrmw, 4 for rgba and tri)", who);
  switch (weld_check_counts(n_v, n_t, w->p.vertex_capacity, w->p.triangle_capacity)) {
    case 0: break;
    case 1: return fail("%s: %ld vertices exceed the welder's capacity %d", who, n_v, w->p.vertex_capacity);
    default: return fail("%s: %ld triangles exceed the welder's capacity %d", who, n_t, w->p.triangle_capacity);
  }
  if (rgba && !w->p.colour) return fail("%s: colours on a welder created without colour", who);
  const uintptr_t b0 = (uintptr_t)w->d_block, b1 = b0 + w->block_bytes;
  const uintptr_t in0[4] = {(uintptr_t)xyz0, (uintptr_t)nrmw, (uintptr_t)rgba, (uintptr_t)tri};
  const uintptr_t len[4] = {16u * (uintptr_t)n_v, 16u * (uintptr_t)n_v, 4u * (uintptr_t)n_v, 12u * (uintptr_t)n_t};
  for (int k = 0; k < 4; k++)
    if (in0[k] && len[k] && in0[k] < b1 && b0 < in0[k] + len[k]) return fail("%s: an input overlaps the welder's own buffers", who);
  return 0;
}

// The arguments of pass k of a run.
static WeldArgs mw_args(const odo_mesh_weld* w, const odo_mesh_weld_rule* rule, int k, int passes, int n_v, int n_t, const float* xyz0,
                        const float* nrmw, const uint8_t* rgba, const int32_t* tri) {
  WeldArgs a;
  memset(&a, 0, sizeof(a));
  const int o = k & 1, i = o ^ 1;
  a.in_xyz0 = k ? w->d_xyz0[i] : (const float4*)xyz0;
  a.in_nrmw = k ? w->d_nrmw[i] : (const float4*)nrmw;
  a.in_rgba = !rgba ? nullptr : k ? w->d_rgba[i] : (const uint32_t*)rgba;
  a.in_tri = k ? w->d_tri[i] : tri;
  a.out_xyz0 = w->d_xyz0[o]; a.out_nrmw = w->d_nrmw[o]; a.out_rgba = w->d_rgba[o]; a.out_tri = w->d_tri[o];
  a.vkeys = w->d_vkeys; a.vmin = w->d_vmin; a.ttab = w->d_ttab;
  a.vaux = w->d_vaux; a.rep = w->d_rep; a.vref = w->d_vref; a.rtri = w->d_rtri; a.tslot = w->d_tslot;
  a.vblk = w->d_vblk; a.tblk = w->d_tblk; a.vblk_off = w->d_vblk_off; a.tblk_off = w->d_tblk_off;
  a.in = w->d_state + k; a.out = w->d_state + k + 1; a.ctr = w->d_ctr;
  a.vslots = w->vslots; a.tslots = w->tslots;
  a.inv = weld_inv(rule->eps); a.ox = rule->origin[0]; a.oy = rule->origin[1]; a.oz = rule->origin[2];
  a.grid = k; a.drop_unreferenced = rule->drop_unreferenced;
  a.first = k == 0; a.last = k == passes - 1;
  a.n_v_max = n_v; a.n_t_max = n_t;
  return a;
}

// One run's enqueues on the context's stream: the counts and the counters set, then every pass's six groups.
static int mw_enqueue(odo_mesh_weld* w, const odo_mesh_weld_rule* rule, int n_v, int n_t, const float* xyz0, const float* nrmw,
                      const uint8_t* rgba, const int32_t* tri) {
  hipStream_t s = w->ctx->stream;
  const int passes = rule->grids;
  w->last_passes = passes;
  w->last_colour = rgba != nullptr;
  launch_weld_begin(w->d_state, w->d_ctr, n_v, n_t, s);
  for (int k = 0; k < passes; k++) {
    const WeldArgs a = mw_args(w, rule, k, passes, n_v, n_t, xyz0, nrmw, rgba, tri);
    for (int g = 0; g < kWeldGroups; g++)
      if (launch_weld_group(a, g, s)) { (void)hipGetLastError(); return fail("odo_mesh_weld: a table could not be cleared"); }
  }
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int odo_mesh_weld_run_dev(odo_mesh_weld* w, const odo_mesh_weld_rule* rule, long n_vertices, long n_triangles,
                                     const float* xyz0_dev, const float* nrmw_dev, const uint8_t* rgba_dev, const int32_t* tri_dev) {
  if (mw_check_run("odo_mesh_weld_run_dev", w, rule, n_vertices, n_triangles, xyz0_dev, nrmw_dev, rgba_dev, tri_dev)) return -1;
  HIP_OK(hipSetDevice(w->device));
  return mw_enqueue(w, rule, (int)n_vertices, (int)n_triangles, xyz0_dev, nrmw_dev, rgba_dev, tri_dev);
}

// Waits for the stream and reads the last run's two counts (0, 0 before the first run).
static int mw_counts(odo_mesh_weld* w, long* n_v, long* n_t) {
  WeldState st;
  HIP_OK(hipSetDevice(w->device));
  HIP_OK(hipMemcpyAsync(&st, w->d_state + w->last_passes, sizeof(st), hipMemcpyDeviceToHost, w->ctx->stream));
  HIP_OK(hipStreamSynchronize(w->ctx->stream));
  *n_v = (long)st.n_v;
  *n_t = (long)st.n_t;
  return 0;
}

extern "C" int odo_mesh_weld_result_dev(odo_mesh_weld* w, const float** xyz0_dev, const float** nrmw_dev, const uint8_t** rgba_dev,
                                        const int32_t** tri_dev, long* n_vertices, long* n_triangles) {
  if (!w || !n_vertices || !n_triangles) return fail("odo_mesh_weld_result_dev: NULL arg");
  if (mw_counts(w, n_vertices, n_triangles)) return -1;
  const int o = w->last_passes ? (w->last_passes - 1) & 1 : 0;
  if (xyz0_dev) *xyz0_dev = (const float*)w->d_xyz0[o];
  if (nrmw_dev) *nrmw_dev = (const float*)w->d_nrmw[o];
  if (rgba_dev) *rgba_dev = w->last_colour ? (const uint8_t*)w->d_rgba[o] : nullptr;
  if (tri_dev) *tri_dev = w->d_tri[o];
  return 0;
}

extern "C" int odo_mesh_weld_download(odo_mesh_weld* w, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw,
                                      uint8_t* rgba, int32_t* tri, long* n_vertices, long* n_triangles) {
  const char* who = "odo_mesh_weld_download";
  if (!w || !n_vertices || !n_triangles || vertex_capacity < 0 || triangle_capacity < 0 || (vertex_capacity > 0 && (!xyz0 || !nrmw)) ||
      (triangle_capacity > 0 && !tri))
    return fail("%s: bad arg (buffers for `vertex_capacity` vertices and `triangle_capacity` triangles)", who);
  if (rgba && !w->last_colour) return fail("%s: the last run carried no colours", who);
  if (mw_counts(w, n_vertices, n_triangles)) return -1;
  if (vertex_capacity == 0 && triangle_capacity == 0) return 0;   // the counts alone
  if (*n_vertices > vertex_capacity || *n_triangles > triangle_capacity)
    return fail("%s: the result (%ld vertices, %ld triangles) does not fit the capacities (%ld, %ld)", who, *n_vertices, *n_triangles,
                vertex_capacity, triangle_capacity);
  const int o = w->last_passes ? (w->last_passes - 1) & 1 : 0;
  hipStream_t s = w->ctx->stream;
  const size_t nv = (size_t)*n_vertices, nt = (size_t)*n_triangles;
  if (nv) {
    HIP_OK(hipMemcpyAsync(xyz0, w->d_xyz0[o], sizeof(float4) * nv, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(nrmw, w->d_nrmw[o], sizeof(float4) * nv, hipMemcpyDeviceToHost, s));
    if (rgba) HIP_OK(hipMemcpyAsync(rgba, w->d_rgba[o], sizeof(uint32_t) * nv, hipMemcpyDeviceToHost, s));
  }
  if (nt) HIP_OK(hipMemcpyAsync(tri, w->d_tri[o], sizeof(int32_t) * 3 * nt, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

extern "C" int odo_mesh_weld_run(odo_mesh_weld* w, const odo_mesh_weld_rule* rule, long n_vertices, long n_triangles, const float* xyz0,
                                 const float* nrmw, const uint8_t* rgba, const int32_t* tri, long vertex_capacity, long triangle_capacity,
                                 float* out_xyz0, float* out_nrmw, uint8_t* out_rgba, int32_t* out_tri, long* out_vertices,
                                 long* out_triangles) {
  const char* who = "odo_mesh_weld_run";
  if (!w || !rule || !out_vertices || !out_triangles) return fail("%s: NULL arg", who);
  if (n_vertices < 0 || n_vertices > kWeldMaxCapacity || n_triangles < 0 || n_triangles > kWeldMaxCapacity)
    return fail("%s: counts out of range (0 .. %d)", who, kWeldMaxCapacity);
  if ((n_vertices > 0 && (!xyz0 || !nrmw)) || (n_triangles > 0 && !tri)) return fail("%s: NULL mesh", who);
  HIP_OK(hipSetDevice(w->device));
  // one staging block for the inputs, each on a 256-byte boundary
  const size_t nv = (size_t)n_vertices, nt = (size_t)n_triangles;
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_n = up(16 * nv), o_c = o_n + up(16 * nv), o_t = o_c + up(4 * nv), total = o_t + up(12 * nt) + 256;
  char* d = nullptr;
  if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); return fail("%s: device allocation failed", who); }
  hipStream_t s = w->ctx->stream;
  int rc = -1;
  const bool ok = (!nv || (hipMemcpyAsync(d, xyz0, 16 * nv, hipMemcpyHostToDevice, s) == hipSuccess &&
                           hipMemcpyAsync(d + o_n, nrmw, 16 * nv, hipMemcpyHostToDevice, s) == hipSuccess &&
                           (!rgba || hipMemcpyAsync(d + o_c, rgba, 4 * nv, hipMemcpyHostToDevice, s) == hipSuccess))) &&
                  (!nt || hipMemcpyAsync(d + o_t, tri, 12 * nt, hipMemcpyHostToDevice, s) == hipSuccess);
  if (!ok) {
    (void)hipGetLastError();
    (void)fail("%s: upload failed", who);
  } else if (!mw_check_run(who, w, rule, n_vertices, n_triangles, (const float*)d, (const float*)(d + o_n),
                           rgba ? (const uint8_t*)(d + o_c) : nullptr, (const int32_t*)(d + o_t)) &&
             !mw_enqueue(w, rule, (int)n_vertices, (int)n_triangles, (const float*)d, (const float*)(d + o_n),
                         rgba ? (const uint8_t*)(d + o_c) : nullptr, (const int32_t*)(d + o_t))) {
    rc = odo_mesh_weld_download(w, vertex_capacity, triangle_capacity, out_xyz0, out_nrmw, out_rgba, out_tri, out_vertices, out_triangles);
  }
  (void)hipStreamSynchronize(s);   // the run reads the staging block
  (void)hipFree(d);
  return rc;
}

extern "C" int odo_mesh_weld_stats(odo_mesh_weld* w, long out[12]) {
  if (!w || !out) return fail("odo_mesh_weld_stats: NULL arg");
  HIP_OK(hipSetDevice(w->device));
  unsigned long long c[kWeldStatWords];
  HIP_OK(hipMemcpyAsync(c, w->d_ctr, sizeof(c), hipMemcpyDeviceToHost, w->ctx->stream));
  HIP_OK(hipStreamSynchronize(w->ctx->stream));
  for (int k = 0; k < kWeldStatWords; k++) out[k] = (long)c[k];
  return 0;
}

// Event timing (tools/mesh_weld_cost.py). A group repeated in place gives the same bytes every time (the tables are cleared inside
// the groups that fill them; only the counters run on), and a pass needs the one before it whole, so the passes run in order and
// within a pass each group is launched `reps` times between two events before the next begins. us[q] = group q's mean time summed
// over the passes, us[6] = their sum. Then one run: the outputs and the statistics are exactly one run's afterwards.
extern "C" int odo_mesh_weld_time_dev(odo_mesh_weld* w, const odo_mesh_weld_rule* rule, long n_vertices, long n_triangles,
                                      const float* xyz0_dev, const float* nrmw_dev, const uint8_t* rgba_dev, const int32_t* tri_dev, int reps,
                                      float us[7]) {
  const char* who = "odo_mesh_weld_time_dev";
  if (!us) return fail("%s: NULL arg", who);
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  if (mw_check_run(who, w, rule, n_vertices, n_triangles, xyz0_dev, nrmw_dev, rgba_dev, tri_dev)) return -1;
  HIP_OK(hipSetDevice(w->device));
  hipStream_t s = w->ctx->stream;
  const int passes = rule->grids, n_v = (int)n_vertices, n_t = (int)n_triangles;
  float sum[kWeldGroups] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = 0; k < passes; k++) {
    const WeldArgs a = mw_args(w, rule, k, passes, n_v, n_t, xyz0_dev, nrmw_dev, rgba_dev, tri_dev);
    float t[kWeldGroups];
    const auto warm = [&]() { if (k == 0) launch_weld_begin(w->d_state, w->d_ctr, n_v, n_t, s); return true; };
    if (time_stages(who, s, reps, kWeldGroups, t, warm, [&](int g) { return launch_weld_group(a, g, s) == 0; })) return -1;
    for (int g = 0; g < kWeldGroups; g++) sum[g] += t[g];
  }
  if (mw_enqueue(w, rule, n_v, n_t, xyz0_dev, nrmw_dev, rgba_dev, tri_dev)) return -1;
  HIP_OK(hipStreamSynchronize(s));
  us[6] = 0.0f;
  for (int g = 0; g < kWeldGroups; g++) { us[g] = sum[g]; us[6] += sum[g]; }
  return 0;
}

extern "C" int odo_mesh_weld_destroy(odo_mesh_weld* w) {
  if (!w) return 0;
  (void)hipSetDevice(w->device);
  (void)hipStreamSynchronize(w->ctx->stream);   // a run in flight reads and writes the block
  if (w->d_block) (void)hipFree(w->d_block);
  delete w;
  return 0;
}
