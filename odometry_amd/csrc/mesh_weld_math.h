// mesh_weld_math.h — the rule of the mesh welder (include/odometry_hip.h, odo_mesh_weld_create), host + device
// like speckle_math.h: the kernels of mesh_weld_kernels.hip, the host object (mesh_weld_api.hip.h, the bounds it validates) and the
// g++ harness of tests/mesh_weld_math_harness.cpp compile these same lines. A vertex's cell and key, the two hashes, the rotation of
// a triangle and the parameter checks are each written once, here, with a sequential reference pass over the same open-addressing
// tables the kernels use. Three fp32 operations make a cell; everything behind it is integers, so nothing depends on an order of
// evaluation.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ODO_WELD_HD __host__ __device__ __forceinline__
#else
#define ODO_WELD_HD static inline
#endif

namespace odo {

constexpr int kWeldMaxCapacity = 1 << 28;             // vertices, triangles: an index, a slot and a block count fit int32
constexpr int kWeldCellLimit = 1 << 20;               // |cell| below this: three 21-bit fields
constexpr unsigned long long kWeldNoKey = ~0ull;      // an empty slot of the vertex table; the key of a keyless vertex
constexpr uint32_t kWeldNoIndex = 0xFFFFFFFFu;        // the smallest-index word of an empty slot
constexpr int32_t kWeldNoTri = -1;                    // an empty slot of the triangle table
constexpr int32_t kWeldTriBad = -1;                   // first word of a remapped triangle that named an index outside [0, n_v)
constexpr int32_t kWeldTriDegenerate = -2;            // ... whose representatives are not three different vertices
constexpr int kWeldStatWords = 12;
// the counters, in the order of odo_mesh_weld_stats
enum {
  kWeldVerticesIn = 0, kWeldVerticesOut, kWeldMerged, kWeldKeyless, kWeldUnreferenced, kWeldTrianglesIn, kWeldTrianglesOut,
  kWeldDegenerate, kWeldDuplicate, kWeldBadIndex, kWeldGuard, kWeldPasses
};
// the guard word's bits: which bounded probe loop ran into its bound (never, with a load of at most one half)
constexpr int kWeldGuardVertexProbe = 1;
constexpr int kWeldGuardTriangleProbe = 2;

// The bounds odo_mesh_weld_create validates. 0: fine; otherwise the number of the bound that fails (1 vertex_capacity,
// 2 triangle_capacity, 3 colour).
ODO_WELD_HD int weld_check_create(long long vertex_capacity, long long triangle_capacity, int colour) {
  if (vertex_capacity < 1 || vertex_capacity > kWeldMaxCapacity) return 1;
  if (triangle_capacity < 1 || triangle_capacity > kWeldMaxCapacity) return 2;
  if (colour != 0 && colour != 1) return 3;
  return 0;
}

// The bounds of a run's rule, in the order of the specification (1 eps, 2 origin, 3 grids, 4 drop_unreferenced).
ODO_WELD_HD int weld_check_rule(float eps, const float* origin, int grids, int drop_unreferenced) {
  if (!(__builtin_isfinite(eps) && eps > 0.0f)) return 1;
  if (!(__builtin_isfinite(origin[0]) && __builtin_isfinite(origin[1]) && __builtin_isfinite(origin[2]))) return 2;
  if (grids != 1 && grids != 8) return 3;
  if (drop_unreferenced != 0 && drop_unreferenced != 1) return 4;
  return 0;
}

// The counts of a run against the welder's capacities (1 n_v, 2 n_t).
ODO_WELD_HD int weld_check_counts(long long n_v, long long n_t, int vertex_capacity, int triangle_capacity) {
  if (n_v < 0 || n_v > vertex_capacity) return 1;
  if (n_t < 0 || n_t > triangle_capacity) return 2;
  return 0;
}

// Slots of a table for `capacity` items: 2^ceil(log2(2 capacity)), so that the load never exceeds one half. 2 .. 2^29.
ODO_WELD_HD uint32_t weld_slots(int capacity) {
  uint32_t s = 2u;
  while (s < 2u * (uint32_t)capacity) s <<= 1;
  return s;
}

// inv = 1 / eps, correctly rounded (every unit that compiles this divides IEEE).
ODO_WELD_HD float weld_inv(float eps) { return 1.0f / eps; }

// One axis' cell in grid bit `half` (0 or 1): floorf((x - o) * inv + (half ? 0.5f : 0.0f)), every operation rounded on its own. False
// for a keyless coordinate: x or the cell not finite, or |cell| >= 2^20.
ODO_WELD_HD bool weld_cell(float x, float o, float inv, int half, int* c) {
  const float d = x - o;
  const float s = d * inv;
  const float t = s + (half ? 0.5f : 0.0f);
  const float f = floorf(t);
  if (!__builtin_isfinite(x) || !__builtin_isfinite(f) || !(fabsf(f) < (float)kWeldCellLimit)) return false;
  *c = (int)f;
  return true;
}

// The 63-bit key of a vertex in grid k (bit a of k belongs to axis a): the cells + 2^20 as three 21-bit fields, the map's packing
// (map_kernels.hip). kWeldNoKey for a keyless vertex; no key has bit 63.
ODO_WELD_HD unsigned long long weld_key(float x, float y, float z, const float* origin, float inv, int grid) {
  int cx, cy, cz;
  if (!weld_cell(x, origin[0], inv, grid & 1, &cx) || !weld_cell(y, origin[1], inv, (grid >> 1) & 1, &cy) ||
      !weld_cell(z, origin[2], inv, (grid >> 2) & 1, &cz))
    return kWeldNoKey;
  return (unsigned long long)(unsigned)(cx + kWeldCellLimit) | ((unsigned long long)(unsigned)(cy + kWeldCellLimit) << 21) |
         ((unsigned long long)(unsigned)(cz + kWeldCellLimit) << 42);
}

ODO_WELD_HD unsigned long long weld_hash(unsigned long long k) {   // splitmix64 finaliser, as map_kernels.hip's
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27; k *= 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

// The hash of a rotated triple: the finaliser over its first two indices, mixed with the finaliser over the third.
ODO_WELD_HD unsigned long long weld_tri_hash(int32_t a, int32_t b, int32_t c) {
  return weld_hash((((unsigned long long)(uint32_t)a << 32) | (uint32_t)b) ^ weld_hash((unsigned long long)(uint32_t)c + 0x9e3779b97f4a7c15ull));
}

// A triangle of input indices under the representatives `rep`: r[0] = kWeldTriBad for an index outside [0, n_v) (rep is not read for
// it), kWeldTriDegenerate when two representatives agree; otherwise the three representatives rotated so that the smallest comes
// first, winding kept.
ODO_WELD_HD void weld_remap(const int32_t* t, const int32_t* rep, int n_v, int32_t* r) {
  r[1] = r[2] = 0;
  if ((uint32_t)t[0] >= (uint32_t)n_v || (uint32_t)t[1] >= (uint32_t)n_v || (uint32_t)t[2] >= (uint32_t)n_v) { r[0] = kWeldTriBad; return; }
  const int32_t a = rep[t[0]], b = rep[t[1]], c = rep[t[2]];
  if (a == b || b == c || a == c) { r[0] = kWeldTriDegenerate; return; }
  if (a < b && a < c) { r[0] = a; r[1] = b; r[2] = c; }
  else if (b < c) { r[0] = b; r[1] = c; r[2] = a; }
  else { r[0] = c; r[1] = a; r[2] = b; }
}

// ---- the sequential reference pass over the kernels' own tables -------------------------------------------------------------------------
// Step 1 of a pass: which vertices and triangles stay. Tables: vkeys / vmin of `vslots` slots and ttab of `tslots` (powers of two),
// cleared here. Scratch: rep, vnew and vref of n_v items, rtri of 3 n_t, tkeep of n_t. Afterwards vnew[i] is vertex i's index in the
// output or -1, tkeep[t] is 1 for a surviving triangle, *out_nv and *out_nt are the output's counts, and the pass's counters are
// added to st[kWeldStatWords] (vertices_in, triangles_in, vertices_out, triangles_out and passes are the caller's). xyz0 is four
// floats per vertex, tri three indices per triangle.
ODO_WELD_HD void weld_ref_plan(const float* xyz0, const int32_t* tri, int n_v, int n_t, float inv, const float* origin, int grid,
                               int drop_unreferenced, unsigned long long* vkeys, uint32_t* vmin, uint32_t vslots, int32_t* ttab,
                               uint32_t tslots, int32_t* rep, int32_t* vnew, uint8_t* vref, int32_t* rtri, uint8_t* tkeep, int64_t* st,
                               int* out_nv, int* out_nt) {
  for (uint32_t s = 0; s < vslots; s++) { vkeys[s] = kWeldNoKey; vmin[s] = kWeldNoIndex; }
  for (uint32_t s = 0; s < tslots; s++) ttab[s] = kWeldNoTri;
  // the vertex table: claim the key's slot, lower its smallest index
  for (int i = 0; i < n_v; i++) {
    vref[i] = 0;
    vnew[i] = -1;   // (until the second loop: the vertex's slot)
    const unsigned long long key = weld_key(xyz0[4 * i], xyz0[4 * i + 1], xyz0[4 * i + 2], origin, inv, grid);
    if (key == kWeldNoKey) { st[kWeldKeyless] += 1; continue; }
    uint32_t s = (uint32_t)weld_hash(key) & (vslots - 1u), trips = 0;
    for (;;) {
      if (vkeys[s] == kWeldNoKey) vkeys[s] = key;
      if (vkeys[s] == key) break;
      if (++trips >= vslots) { st[kWeldGuard] |= kWeldGuardVertexProbe; break; }
      s = (s + 1u) & (vslots - 1u);
    }
    if (vkeys[s] != key) continue;
    if ((uint32_t)i < vmin[s]) vmin[s] = (uint32_t)i;
    vnew[i] = (int32_t)s;
  }
  for (int i = 0; i < n_v; i++) {
    rep[i] = vnew[i] < 0 ? i : (int32_t)vmin[vnew[i]];
    st[kWeldMerged] += rep[i] != i;
  }
  // the triangle table: a slot holds the smallest index of the triangles with its triple
  for (int t = 0; t < n_t; t++) {
    int32_t* r = rtri + 3 * t;
    weld_remap(tri + 3 * t, rep, n_v, r);
    tkeep[t] = 0;
    if (r[0] == kWeldTriBad) { st[kWeldBadIndex] += 1; continue; }
    if (r[0] == kWeldTriDegenerate) { st[kWeldDegenerate] += 1; continue; }
    uint32_t s = (uint32_t)weld_tri_hash(r[0], r[1], r[2]) & (tslots - 1u), trips = 0;
    for (;;) {
      if (ttab[s] == kWeldNoTri) { ttab[s] = t; tkeep[t] = 1; break; }
      const int32_t* u = rtri + 3 * ttab[s];
      if (u[0] == r[0] && u[1] == r[1] && u[2] == r[2]) { st[kWeldDuplicate] += 1; break; }   // (ttab[s] < t: it stays)
      if (++trips >= tslots) { st[kWeldGuard] |= kWeldGuardTriangleProbe; break; }
      s = (s + 1u) & (tslots - 1u);
    }
    if (tkeep[t]) vref[r[0]] = vref[r[1]] = vref[r[2]] = 1;
  }
  int nv = 0, nt = 0;
  for (int i = 0; i < n_v; i++) {
    if (rep[i] != i) { vnew[i] = -1; continue; }
    if (drop_unreferenced && !vref[i]) { vnew[i] = -1; st[kWeldUnreferenced] += 1; continue; }
    vnew[i] = nv++;
  }
  for (int t = 0; t < n_t; t++) nt += tkeep[t];
  *out_nv = nv;
  *out_nt = nt;
}

// Step 2: the output, into blocks of exactly *out_nv vertices and *out_nt triangles. A kept vertex carries its own 16 + 16 (+ 4)
// bytes; a surviving triangle is its rotated triple in the output's indices. rgba and out_rgba may both be NULL.
ODO_WELD_HD void weld_ref_emit(const float* xyz0, const float* nrmw, const uint8_t* rgba, int n_v, int n_t, const int32_t* vnew,
                               const int32_t* rtri, const uint8_t* tkeep, float* out_xyz0, float* out_nrmw, uint8_t* out_rgba,
                               int32_t* out_tri) {
  for (int i = 0; i < n_v; i++) {
    if (vnew[i] < 0) continue;
    __builtin_memcpy(out_xyz0 + 4 * vnew[i], xyz0 + 4 * i, 16);   // (bytes, not floats: a NaN keeps its payload)
    __builtin_memcpy(out_nrmw + 4 * vnew[i], nrmw + 4 * i, 16);
    if (rgba) __builtin_memcpy(out_rgba + 4 * vnew[i], rgba + 4 * i, 4);
  }
  int m = 0;
  for (int t = 0; t < n_t; t++) {
    if (!tkeep[t]) continue;
    for (int c = 0; c < 3; c++) out_tri[3 * m + c] = vnew[rtri[3 * t + c]];
    m++;
  }
}

}  // namespace odo
