// mesh_components_api.hip.h — the mesh component filter (odo_mesh_components_*): the host object over the kernels of
// mesh_components_kernels.hip. A mesh on the device in — the welder's result_dev pointers, say — and the filtered mesh in the filter's
// own buffers out; every launch goes to the CONTEXT's stream with no host wait, so the ordering rules are the welder's
// (mesh_weld_api.hip.h). Included by odometry_hip.hip.
#pragma once
#include "mesh_components.hip.h"

struct odo_mesh_components {
  odo_ctx* ctx;
  int device;
  odo_mesh_components_params p;
  uint32_t eslots;                 // 0 without edge statistics
  int vblocks, tblocks;            // workgroups at the capacities: the rows of the per-block counts
  char* d_block;                   // the one device allocation everything below lies in
  size_t block_bytes;
  float4* d_xyz0;
  float4* d_nrmw;
  uint32_t* d_rgba;                // NULL without colour
  int32_t* d_tri;
  int32_t* d_parent;
  uint32_t* d_size;
  int32_t* d_vnew;
  uint8_t* d_vref;
  int32_t* d_label;
  unsigned long long* d_ekeys;     // NULL without edge statistics
  uint32_t* d_euse;
  uint32_t* d_vblk;
  uint32_t* d_tblk;
  unsigned long long* d_vblk_off;
  unsigned long long* d_tblk_off;
  McState* d_state;                // zero until the first run
  unsigned long long* d_ctr;       // [kMcStatWords], zero until the first run
  long last_triangles;             // of the last run enqueued: the labels that are valid
  int last_colour;                 // ... and whether it carried colours
};

// Lays the filter's blocks out behind one another, each on a 256-byte boundary: the pointers when base is given, the size always.
static size_t mc_carve(odo_mesh_components* f, char* base) {
  size_t off = 0;
  const auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return p; };
  const size_t nv = (size_t)f->p.vertex_capacity, nt = (size_t)f->p.triangle_capacity;
  f->d_xyz0 = (float4*)take(sizeof(float4) * nv);
  f->d_nrmw = (float4*)take(sizeof(float4) * nv);
  f->d_rgba = f->p.colour ? (uint32_t*)take(sizeof(uint32_t) * nv) : nullptr;
  f->d_tri = (int32_t*)take(sizeof(int32_t) * 3 * nt);
  f->d_parent = (int32_t*)take(sizeof(int32_t) * nv);
  f->d_size = (uint32_t*)take(sizeof(uint32_t) * nv);
  f->d_vnew = (int32_t*)take(sizeof(int32_t) * nv);
  f->d_vref = (uint8_t*)take(nv);
  f->d_label = (int32_t*)take(sizeof(int32_t) * nt);
  f->d_ekeys = f->eslots ? (unsigned long long*)take(sizeof(unsigned long long) * f->eslots) : nullptr;
  f->d_euse = f->eslots ? (uint32_t*)take(sizeof(uint32_t) * f->eslots) : nullptr;
  f->d_vblk = (uint32_t*)take(sizeof(uint32_t) * f->vblocks);
  f->d_tblk = (uint32_t*)take(sizeof(uint32_t) * f->tblocks);
  f->d_vblk_off = (unsigned long long*)take(sizeof(unsigned long long) * f->vblocks);
  f->d_tblk_off = (unsigned long long*)take(sizeof(unsigned long long) * f->tblocks);
  f->d_state = (McState*)take(sizeof(McState));
  f->d_ctr = (unsigned long long*)take(sizeof(unsigned long long) * kMcStatWords);
  return off;
}

extern "C" int odo_mesh_components_create(odo_ctx* ctx, const odo_mesh_components_params* p, odo_mesh_components** out) {
  const char* who = "odo_mesh_components_create";
  if (!ctx || !p || !out) return fail("%s: NULL arg", who);
  switch (mc_check_create(p->vertex_capacity, p->triangle_capacity, p->colour, p->edge_stats)) {
    case 0: break;
    case 1: return fail("%s: vertex_capacity %d out of range (1 .. %d)", who, p->vertex_capacity, kMcMaxCapacity);
    case 2: return fail("%s: triangle_capacity %d out of range (1 .. %d)", who, p->triangle_capacity, kMcMaxCapacity);
    case 3: return fail("%s: colour %d is not 0 or 1", who, p->colour);
    default: return fail("%s: edge_stats %d is not 0 or 1", who, p->edge_stats);
  }
  HIP_OK(hipSetDevice(ctx->device));
  odo_mesh_components* f = new (std::nothrow) odo_mesh_components();
  if (!f) return fail("out of memory");
  memset((void*)f, 0, sizeof(*f));
  f->ctx = ctx; f->device = ctx->device; f->p = *p;
  f->eslots = p->edge_stats ? mc_edge_slots(p->triangle_capacity) : 0u;
  f->vblocks = mc_blocks(p->vertex_capacity);
  f->tblocks = mc_blocks(p->triangle_capacity);
  f->block_bytes = mc_carve(f, nullptr);
  bool ok = hipMalloc((void**)&f->d_block, f->block_bytes) == hipSuccess;
  if (ok) {
    mc_carve(f, f->d_block);
    ok = hipMemsetAsync(f->d_state, 0, sizeof(McState), ctx->stream) == hipSuccess &&
         hipMemsetAsync(f->d_ctr, 0, sizeof(unsigned long long) * kMcStatWords, ctx->stream) == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(ctx->stream);
    if (f->d_block) (void)hipFree(f->d_block);
    delete f;
    return fail("%s: device allocation failed (%d vertices, %d triangles)", who, p->vertex_capacity, p->triangle_capacity);
  }
  *out = f;
  return 0;
}

// Everything odo_mesh_components_run_dev refuses, in two halves: what the arguments alone decide, before the filter is read, then
// what its capacities and its buffers decide. -1 with the reason named, 0 when the run may be enqueued.
static int mc_check_run(const char* who, const odo_mesh_components* f, const odo_mesh_components_rule* rule, long n_v, long n_t,
                        const float* xyz0, const float* nrmw, const uint8_t* rgba, const int32_t* tri) {
  if (!f || !rule) return fail("%s: NULL arg", who);
  switch (mc_check_rule(rule->min_triangles, rule->keep_largest, rule->drop_unreferenced)) {
    case 0: break;
    case 1: return fail("%s: min_triangles %d is negative", who, rule->min_triangles);
    case 2: return fail("%s: keep_largest %d is not 0 or 1", who, rule->keep_largest);
    default: return fail("%s: drop_unreferenced %d is not 0 or 1", who, rule->drop_unreferenced);
  }
  if (n_v < 0 || n_v > kMcMaxCapacity) return fail("%s: n_vertices %ld out of range (0 .. %d)", who, n_v, kMcMaxCapacity);
  if (n_t < 0 || n_t > kMcMaxCapacity) return fail("%s: n_triangles %ld out of range (0 .. %d)", who, n_t, kMcMaxCapacity);
  if ((n_v > 0 && (!xyz0 || !nrmw)) || (n_t > 0 && !tri)) return fail("%s: NULL mesh", who);
  if ((((uintptr_t)xyz0 | (uintptr_t)nrmw) & 15) || (((uintptr_t)rgba | (uintptr_t)tri) & 3))
    return fail("%s: misaligned pointer (16 bytes for xyz0 and nrmw, 4 for rgba and tri)", who);
  switch (mc_check_counts(n_v, n_t, f->p.vertex_capacity, f->p.triangle_capacity)) {
    case 0: break;
    case 1: return fail("%s: %ld vertices exceed the filter's capacity %d", who, n_v, f->p.vertex_capacity);
    default: return fail("%s: %ld triangles exceed the filter's capacity %d", who, n_t, f->p.triangle_capacity);
  }
  if (rgba && !f->p.colour) return fail("%s: colours on a filter created without colour", who);
  const uintptr_t b0 = (uintptr_t)f->d_block, b1 = b0 + f->block_bytes;
  const uintptr_t in0[4] = {(uintptr_t)xyz0, (uintptr_t)nrmw, (uintptr_t)rgba, (uintptr_t)tri};
  const uintptr_t len[4] = {16u * (uintptr_t)n_v, 16u * (uintptr_t)n_v, 4u * (uintptr_t)n_v, 12u * (uintptr_t)n_t};
  for (int k = 0; k < 4; k++)
    if (in0[k] && len[k] && in0[k] < b1 && b0 < in0[k] + len[k]) return fail("%s: an input overlaps the filter's own buffers", who);
  return 0;
}

static McArgs mc_args(const odo_mesh_components* f, const odo_mesh_components_rule* rule, int n_v, int n_t, const float* xyz0,
                      const float* nrmw, const uint8_t* rgba, const int32_t* tri) {
  McArgs a;
  memset(&a, 0, sizeof(a));
  a.in_xyz0 = (const float4*)xyz0; a.in_nrmw = (const float4*)nrmw; a.in_rgba = (const uint32_t*)rgba; a.in_tri = tri;
  a.out_xyz0 = f->d_xyz0; a.out_nrmw = f->d_nrmw; a.out_rgba = f->d_rgba; a.out_tri = f->d_tri;
  a.parent = f->d_parent; a.size = f->d_size; a.vnew = f->d_vnew; a.vref = f->d_vref; a.label = f->d_label;
  a.ekeys = f->d_ekeys; a.euse = f->d_euse;
  a.vblk = f->d_vblk; a.tblk = f->d_tblk; a.vblk_off = f->d_vblk_off; a.tblk_off = f->d_tblk_off;
  a.state = f->d_state; a.ctr = f->d_ctr;
  a.eslots = f->eslots;
  a.n_v = n_v; a.n_t = n_t;
  a.min_triangles = rule->min_triangles; a.keep_largest = rule->keep_largest; a.drop_unreferenced = rule->drop_unreferenced;
  return a;
}

// One run's enqueues on the context's stream: the counts and the counters set, then the six groups.
static int mc_enqueue(odo_mesh_components* f, const McArgs& a) {
  hipStream_t s = f->ctx->stream;
  f->last_triangles = a.n_t;
  f->last_colour = a.in_rgba != nullptr;
  launch_mc_begin(f->d_state, f->d_ctr, s);
  for (int g = 0; g < kMcGroups; g++)
    if (launch_mc_group(a, g, s)) { (void)hipGetLastError(); return fail("odo_mesh_components: a table could not be cleared"); }
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int odo_mesh_components_run_dev(odo_mesh_components* f, const odo_mesh_components_rule* rule, long n_vertices,
                                           long n_triangles, const float* xyz0_dev, const float* nrmw_dev, const uint8_t* rgba_dev,
                                           const int32_t* tri_dev) {
  if (mc_check_run("odo_mesh_components_run_dev", f, rule, n_vertices, n_triangles, xyz0_dev, nrmw_dev, rgba_dev, tri_dev)) return -1;
  HIP_OK(hipSetDevice(f->device));
  return mc_enqueue(f, mc_args(f, rule, (int)n_vertices, (int)n_triangles, xyz0_dev, nrmw_dev, rgba_dev, tri_dev));
}

// Waits for the stream and reads the last run's two counts (0, 0 before the first run).
static int mc_counts(odo_mesh_components* f, long* n_v, long* n_t) {
  McState st;
  HIP_OK(hipSetDevice(f->device));
  HIP_OK(hipMemcpyAsync(&st, f->d_state, sizeof(st), hipMemcpyDeviceToHost, f->ctx->stream));
  HIP_OK(hipStreamSynchronize(f->ctx->stream));
  *n_v = (long)st.n_v;
  *n_t = (long)st.n_t;
  return 0;
}

extern "C" int odo_mesh_components_result_dev(odo_mesh_components* f, const float** xyz0_dev, const float** nrmw_dev,
                                              const uint8_t** rgba_dev, const int32_t** tri_dev, long* n_vertices, long* n_triangles) {
  if (!f || !n_vertices || !n_triangles) return fail("odo_mesh_components_result_dev: NULL arg");
  if (mc_counts(f, n_vertices, n_triangles)) return -1;
  if (xyz0_dev) *xyz0_dev = (const float*)f->d_xyz0;
  if (nrmw_dev) *nrmw_dev = (const float*)f->d_nrmw;
  if (rgba_dev) *rgba_dev = f->last_colour ? (const uint8_t*)f->d_rgba : nullptr;
  if (tri_dev) *tri_dev = f->d_tri;
  return 0;
}

extern "C" int odo_mesh_components_download(odo_mesh_components* f, long vertex_capacity, long triangle_capacity, float* xyz0,
                                            float* nrmw, uint8_t* rgba, int32_t* tri, long* n_vertices, long* n_triangles) {
  const char* who = "odo_mesh_components_download";
  if (!f || !n_vertices || !n_triangles || vertex_capacity < 0 || triangle_capacity < 0 || (vertex_capacity > 0 && (!xyz0 || !nrmw)) ||
      (triangle_capacity > 0 && !tri))
    return fail("%s: bad arg (buffers for `vertex_capacity` vertices and `triangle_capacity` triangles)", who);
  if (rgba && !f->last_colour) return fail("%s: the last run carried no colours", who);
  if (mc_counts(f, n_vertices, n_triangles)) return -1;
  if (vertex_capacity == 0 && triangle_capacity == 0) return 0;   // the counts alone
  if (*n_vertices > vertex_capacity || *n_triangles > triangle_capacity)
    return fail("%s: the result (%ld vertices, %ld triangles) does not fit the capacities (%ld, %ld)", who, *n_vertices, *n_triangles,
                vertex_capacity, triangle_capacity);
  hipStream_t s = f->ctx->stream;
  const size_t nv = (size_t)*n_vertices, nt = (size_t)*n_triangles;
  if (nv) {
    HIP_OK(hipMemcpyAsync(xyz0, f->d_xyz0, sizeof(float4) * nv, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(nrmw, f->d_nrmw, sizeof(float4) * nv, hipMemcpyDeviceToHost, s));
    if (rgba) HIP_OK(hipMemcpyAsync(rgba, f->d_rgba, sizeof(uint32_t) * nv, hipMemcpyDeviceToHost, s));
  }
  if (nt) HIP_OK(hipMemcpyAsync(tri, f->d_tri, sizeof(int32_t) * 3 * nt, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

extern "C" int odo_mesh_components_run(odo_mesh_components* f, const odo_mesh_components_rule* rule, long n_vertices, long n_triangles,
                                       const float* xyz0, const float* nrmw, const uint8_t* rgba, const int32_t* tri,
                                       long vertex_capacity, long triangle_capacity, float* out_xyz0, float* out_nrmw, uint8_t* out_rgba,
                                       int32_t* out_tri, long* out_vertices, long* out_triangles) {
  const char* who = "odo_mesh_components_run";
  if (!f || !rule || !out_vertices || !out_triangles) return fail("%s: NULL arg", who);
  if (n_vertices < 0 || n_vertices > kMcMaxCapacity || n_triangles < 0 || n_triangles > kMcMaxCapacity)
    return fail("%s: counts out of range (0 .. %d)", who, kMcMaxCapacity);
  if ((n_vertices > 0 && (!xyz0 || !nrmw)) || (n_triangles > 0 && !tri)) return fail("%s: NULL mesh", who);
  HIP_OK(hipSetDevice(f->device));
  // one staging block for the inputs, each on a 256-byte boundary
  const size_t nv = (size_t)n_vertices, nt = (size_t)n_triangles;
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_n = up(16 * nv), o_c = o_n + up(16 * nv), o_t = o_c + up(4 * nv), total = o_t + up(12 * nt) + 256;
  char* d = nullptr;
  if (hipMalloc((void**)&d, total) != hipSuccess) { (void)hipGetLastError(); return fail("%s: device allocation failed", who); }
  hipStream_t s = f->ctx->stream;
  int rc = -1;
  const bool ok = (!nv || (hipMemcpyAsync(d, xyz0, 16 * nv, hipMemcpyHostToDevice, s) == hipSuccess &&
                           hipMemcpyAsync(d + o_n, nrmw, 16 * nv, hipMemcpyHostToDevice, s) == hipSuccess &&
                           (!rgba || hipMemcpyAsync(d + o_c, rgba, 4 * nv, hipMemcpyHostToDevice, s) == hipSuccess))) &&
                  (!nt || hipMemcpyAsync(d + o_t, tri, 12 * nt, hipMemcpyHostToDevice, s) == hipSuccess);
  const float* dx = (const float*)d;
  const float* dn = (const float*)(d + o_n);
  const uint8_t* dc = rgba ? (const uint8_t*)(d + o_c) : nullptr;
  const int32_t* dt = (const int32_t*)(d + o_t);
  if (!ok) {
    (void)hipGetLastError();
    (void)fail("%s: upload failed", who);
  } else if (!mc_check_run(who, f, rule, n_vertices, n_triangles, dx, dn, dc, dt) &&
             !mc_enqueue(f, mc_args(f, rule, (int)n_vertices, (int)n_triangles, dx, dn, dc, dt))) {
    rc = odo_mesh_components_download(f, vertex_capacity, triangle_capacity, out_xyz0, out_nrmw, out_rgba, out_tri, out_vertices,
                                      out_triangles);
  }
  (void)hipStreamSynchronize(s);   // the run reads the staging block
  (void)hipFree(d);
  return rc;
}

extern "C" int odo_mesh_components_labels_dev(odo_mesh_components* f, const int32_t** labels_dev, long* n_triangles) {
  if (!f || !labels_dev || !n_triangles) return fail("odo_mesh_components_labels_dev: NULL arg");
  *labels_dev = f->d_label;
  *n_triangles = f->last_triangles;
  return 0;
}

extern "C" int odo_mesh_components_labels(odo_mesh_components* f, long capacity, int32_t* labels, long* n_triangles) {
  const char* who = "odo_mesh_components_labels";
  if (!f || !n_triangles || capacity < 0 || (capacity > 0 && !labels)) return fail("%s: bad arg (a buffer for `capacity` labels)", who);
  *n_triangles = f->last_triangles;
  if (capacity == 0) return 0;   // the count alone
  if (f->last_triangles > capacity) return fail("%s: %ld labels do not fit the capacity %ld", who, f->last_triangles, capacity);
  HIP_OK(hipSetDevice(f->device));
  if (f->last_triangles)
    HIP_OK(hipMemcpyAsync(labels, f->d_label, sizeof(int32_t) * (size_t)f->last_triangles, hipMemcpyDeviceToHost, f->ctx->stream));
  HIP_OK(hipStreamSynchronize(f->ctx->stream));
  return 0;
}

extern "C" int odo_mesh_components_stats(odo_mesh_components* f, long out[19]) {
  if (!f || !out) return fail("odo_mesh_components_stats: NULL arg");
  HIP_OK(hipSetDevice(f->device));
  unsigned long long c[kMcStatWords];
  HIP_OK(hipMemcpyAsync(c, f->d_ctr, sizeof(c), hipMemcpyDeviceToHost, f->ctx->stream));
  HIP_OK(hipStreamSynchronize(f->ctx->stream));
  for (int k = 0; k < kMcStatWords; k++) out[k] = (long)c[k];
  return 0;
}

// Event timing (tools/mesh_components_cost.py). A group repeated in place gives the same bytes every time — the unions start from
// parent[i] = i, the sizes are zeroed by the launch that flattens, the edge table is cleared inside its group, the largest is a
// maximum — and only the counters run on. So each group is launched `reps` times between two events before the next begins. Then
// one run: the outputs, the labels and the statistics are exactly one run's afterwards.
extern "C" int odo_mesh_components_time_dev(odo_mesh_components* f, const odo_mesh_components_rule* rule, long n_vertices,
                                            long n_triangles, const float* xyz0_dev, const float* nrmw_dev, const uint8_t* rgba_dev,
                                            const int32_t* tri_dev, int reps, float us[7]) {
  const char* who = "odo_mesh_components_time_dev";
  if (!us) return fail("%s: NULL arg", who);
  if (reps < 1 || reps > 10000) return fail("%s: reps 1 .. 10000", who);
  if (mc_check_run(who, f, rule, n_vertices, n_triangles, xyz0_dev, nrmw_dev, rgba_dev, tri_dev)) return -1;
  HIP_OK(hipSetDevice(f->device));
  hipStream_t s = f->ctx->stream;
  const McArgs a = mc_args(f, rule, (int)n_vertices, (int)n_triangles, xyz0_dev, nrmw_dev, rgba_dev, tri_dev);
  float t[kMcGroups];
  const auto warm = [&]() { launch_mc_begin(f->d_state, f->d_ctr, s); return true; };
  if (time_stages(who, s, reps, kMcGroups, t, warm, [&](int g) { return launch_mc_group(a, g, s) == 0; })) return -1;
  if (mc_enqueue(f, a)) return -1;
  HIP_OK(hipStreamSynchronize(s));
  us[6] = 0.0f;
  for (int g = 0; g < kMcGroups; g++) { us[g] = t[g]; us[6] += t[g]; }
  return 0;
}

extern "C" int odo_mesh_components_destroy(odo_mesh_components* f) {
  if (!f) return 0;
  (void)hipSetDevice(f->device);
  (void)hipStreamSynchronize(f->ctx->stream);   // a run in flight reads and writes the block
  if (f->d_block) (void)hipFree(f->d_block);
  delete f;
  return 0;
}
