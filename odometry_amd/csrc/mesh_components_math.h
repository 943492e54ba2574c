// mesh_components_math.h — the rule of the mesh component filter (include/odometry_hip.h, odo_mesh_components_create; DESIGN.md
// section 9.20), host + device like mesh_weld_math.h: the kernels of mesh_components_kernels.hip, the host object
// (mesh_components_api.hip.h, the bounds it validates) and the g++ harness of tests/mesh_components_math_harness.cpp compile these same
// lines. A triangle's validity, a component's survival, the word the largest component is found with, an edge's key and the parameter
// checks are each written once, here, with a sequential reference pass over the same parent array and the same open-addressing edge
// table the kernels use. Everything is integers, so nothing depends on an order of evaluation.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ODO_MC_HD __host__ __device__ __forceinline__
#else
#define ODO_MC_HD static inline
#endif

namespace odo {

constexpr int kMcMaxCapacity = 1 << 28;               // vertices, triangles: an index fits 28 bits, an edge key has bit 63 clear
constexpr unsigned long long kMcNoEdge = ~0ull;       // an empty slot of the edge table
constexpr int32_t kMcNoLabel = -1;                    // the label of a triangle that names an index outside [0, n_v)
constexpr int kMcStatWords = 19;
// the counters, in the order of odo_mesh_components_stats
enum {
  kMcVerticesIn = 0, kMcTrianglesIn, kMcVerticesOut, kMcTrianglesOut, kMcComponents, kMcRemovedComponents, kMcRemovedTriangles,
  kMcRemovedVertices, kMcLargest, kMcBadIndex, kMcDegenerate, kMcUnreferenced, kMcEdges, kMcOpenEdges, kMcNonmanifoldEdges, kMcEdgesOut,
  kMcOpenEdgesOut, kMcNonmanifoldEdgesOut, kMcGuard
};
// the guard word's bits: which bounded loop ran into its bound (never: DESIGN.md section 9.20)
constexpr int kMcGuardFind = 1;
constexpr int kMcGuardUnion = 2;
constexpr int kMcGuardEdgeProbe = 4;

// The bounds odo_mesh_components_create validates. 0: fine; otherwise the number of the bound that fails (1 vertex_capacity,
// 2 triangle_capacity, 3 colour, 4 edge_stats).
ODO_MC_HD int mc_check_create(long long vertex_capacity, long long triangle_capacity, int colour, int edge_stats) {
  if (vertex_capacity < 1 || vertex_capacity > kMcMaxCapacity) return 1;
  if (triangle_capacity < 1 || triangle_capacity > kMcMaxCapacity) return 2;
  if (colour != 0 && colour != 1) return 3;
  if (edge_stats != 0 && edge_stats != 1) return 4;
  return 0;
}

// The bounds of a run's rule, in the order of the specification (1 min_triangles, 2 keep_largest, 3 drop_unreferenced).
ODO_MC_HD int mc_check_rule(int min_triangles, int keep_largest, int drop_unreferenced) {
  if (min_triangles < 0) return 1;
  if (keep_largest != 0 && keep_largest != 1) return 2;
  if (drop_unreferenced != 0 && drop_unreferenced != 1) return 3;
  return 0;
}

// The counts of a run against the filter's capacities (1 n_v, 2 n_t).
ODO_MC_HD int mc_check_counts(long long n_v, long long n_t, int vertex_capacity, int triangle_capacity) {
  if (n_v < 0 || n_v > vertex_capacity) return 1;
  if (n_t < 0 || n_t > triangle_capacity) return 2;
  return 0;
}

// Slots of the edge table for `triangle_capacity` triangles: 2^ceil(log2(2 * 3 * triangle_capacity)), so that the load never exceeds
// one half. 8 .. 2^31.
ODO_MC_HD uint32_t mc_edge_slots(int triangle_capacity) {
  uint32_t s = 2u;
  while ((unsigned long long)s < 6ull * (unsigned long long)triangle_capacity) s <<= 1;
  return s;
}

// A triangle is valid iff its three indices lie in [0, n_v); the indices of an invalid one are never dereferenced.
ODO_MC_HD bool mc_valid(const int32_t* t, int n_v) {
  return (uint32_t)t[0] < (uint32_t)n_v && (uint32_t)t[1] < (uint32_t)n_v && (uint32_t)t[2] < (uint32_t)n_v;
}
ODO_MC_HD bool mc_degenerate(const int32_t* t) { return t[0] == t[1] || t[1] == t[2] || t[0] == t[2]; }

// The word whose maximum over the components names the largest: the size above the complement of the label, so that of two
// components of one size the smaller label wins. 0: no component.
ODO_MC_HD unsigned long long mc_best_word(uint32_t size, int32_t label) {
  return ((unsigned long long)size << 32) | (unsigned long long)(~(uint32_t)label);
}
ODO_MC_HD uint32_t mc_best_size(unsigned long long best) { return (uint32_t)(best >> 32); }

// A component (size > 0) survives iff size >= min_triangles and, with keep_largest, it is the one `best` names.
ODO_MC_HD bool mc_survives(uint32_t size, int32_t label, int min_triangles, int keep_largest, unsigned long long best) {
  if (size == 0u || size < (uint32_t)min_triangles) return false;
  return !keep_largest || mc_best_word(size, label) == best;
}

// The key of the undirected edge a | b, a != b, both below 2^28: bit 63 is clear.
ODO_MC_HD unsigned long long mc_edge_key(int32_t a, int32_t b) {
  const uint32_t lo = (uint32_t)(a < b ? a : b), hi = (uint32_t)(a < b ? b : a);
  return ((unsigned long long)lo << 32) | hi;
}
ODO_MC_HD int32_t mc_edge_low(unsigned long long key) { return (int32_t)(key >> 32); }

ODO_MC_HD unsigned long long mc_hash(unsigned long long k) {   // splitmix64 finaliser, as map_kernels.hip's
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27; k *= 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

// ---- the sequential reference pass over the kernels' own arrays --------------------------------------------------------------------------
// The root above vertex i: parent[i] <= i with equality only at a root. A walk of more than `bound` trips, or one that meets a word
// breaking the invariant, sets the bit and ends where it is.
ODO_MC_HD int32_t mc_ref_find(const int32_t* parent, int32_t i, int bound, int64_t* st) {
  int trips = 0;
  for (;;) {
    const int32_t p = parent[i];
    if (p == i) break;
    if ((uint32_t)p > (uint32_t)i || ++trips > bound) { st[kMcGuard] |= kMcGuardFind; break; }
    i = p;
  }
  return i;
}

// Step 1: the components, what survives, the edges. Arrays: parent, size and vnew of n_v items, vref of n_v bytes, label of n_t;
// ekeys / euse of `eslots` slots (a power of two; NULL and 0 without edge statistics), cleared here. Afterwards label[t] is triangle
// t's component (kMcNoLabel for an invalid one), vnew[i] vertex i's index in the output or -1, *out_nv and *out_nt the output's
// counts, and st[kMcStatWords] holds every counter.
ODO_MC_HD void mc_ref_plan(const int32_t* tri, int n_v, int n_t, int min_triangles, int keep_largest, int drop_unreferenced,
                           int32_t* parent, uint32_t* size, int32_t* vnew, uint8_t* vref, int32_t* label, unsigned long long* ekeys,
                           uint32_t* euse, uint32_t eslots, int64_t* st, int* out_nv, int* out_nt) {
  for (int k = 0; k < kMcStatWords; k++) st[k] = 0;
  st[kMcVerticesIn] = n_v;
  st[kMcTrianglesIn] = n_t;
  for (int i = 0; i < n_v; i++) { parent[i] = i; size[i] = 0u; vref[i] = 0; }
  for (uint32_t s = 0; s < eslots; s++) { ekeys[s] = kMcNoEdge; euse[s] = 0u; }
  // union: the larger root goes under the smaller
  for (int t = 0; t < n_t; t++) {
    const int32_t* v = tri + 3 * (size_t)t;
    if (!mc_valid(v, n_v)) continue;
    for (int c = 1; c < 3; c++) {
      int32_t a = mc_ref_find(parent, v[0], n_v, st), b = mc_ref_find(parent, v[c], n_v, st);
      if (a == b) continue;
      if (a < b) { const int32_t x = a; a = b; b = x; }
      parent[a] = b;
    }
  }
  for (int i = 0; i < n_v; i++) parent[i] = mc_ref_find(parent, i, n_v, st);
  // labels, sizes, edges
  for (int t = 0; t < n_t; t++) {
    const int32_t* v = tri + 3 * (size_t)t;
    if (!mc_valid(v, n_v)) { label[t] = kMcNoLabel; st[kMcBadIndex] += 1; continue; }
    label[t] = parent[v[0]];
    size[label[t]] += 1u;
    st[kMcDegenerate] += mc_degenerate(v);
    for (int c = 0; c < 3 && eslots; c++) {
      const int32_t a = v[c], b = v[(c + 1) % 3];
      if (a == b) continue;
      const unsigned long long key = mc_edge_key(a, b);
      uint32_t s = (uint32_t)mc_hash(key) & (eslots - 1u), trips = 0;
      for (;;) {
        if (ekeys[s] == kMcNoEdge) ekeys[s] = key;
        if (ekeys[s] == key) { euse[s] += 1u; break; }
        if (++trips >= eslots) { st[kMcGuard] |= kMcGuardEdgeProbe; break; }
        s = (s + 1u) & (eslots - 1u);
      }
    }
  }
  unsigned long long best = 0ull;
  for (int i = 0; i < n_v; i++) {
    if (parent[i] != i || size[i] == 0u) continue;
    st[kMcComponents] += 1;
    const unsigned long long w = mc_best_word(size[i], i);
    if (w > best) best = w;
  }
  st[kMcLargest] = mc_best_size(best);
  // survivors
  int nv = 0, nt = 0;
  for (int t = 0; t < n_t; t++) {
    if (label[t] == kMcNoLabel) continue;
    if (!mc_survives(size[label[t]], label[t], min_triangles, keep_largest, best)) { st[kMcRemovedTriangles] += 1; continue; }
    nt++;
    const int32_t* v = tri + 3 * (size_t)t;
    vref[v[0]] = vref[v[1]] = vref[v[2]] = 1;
  }
  for (int i = 0; i < n_v; i++) {
    const uint32_t sz = size[parent[i]];
    vnew[i] = -1;
    if (sz == 0u) {   // no valid triangle names it
      if (drop_unreferenced) st[kMcUnreferenced] += 1;
      else vnew[i] = nv++;
    } else if (vref[i]) {
      vnew[i] = nv++;
    } else {
      st[kMcRemovedVertices] += 1;
      st[kMcRemovedComponents] += parent[i] == i;
    }
  }
  for (uint32_t s = 0; s < eslots; s++) {
    if (ekeys[s] == kMcNoEdge) continue;
    const int32_t r = parent[mc_edge_low(ekeys[s])];
    const bool out = mc_survives(size[r], r, min_triangles, keep_largest, best);
    st[kMcEdges] += 1;              st[kMcEdgesOut] += out;
    if (euse[s] == 1u) { st[kMcOpenEdges] += 1; st[kMcOpenEdgesOut] += out; }
    if (euse[s] > 2u) { st[kMcNonmanifoldEdges] += 1; st[kMcNonmanifoldEdgesOut] += out; }
  }
  st[kMcVerticesOut] = nv;
  st[kMcTrianglesOut] = nt;
  *out_nv = nv;
  *out_nt = nt;
}

// Step 2: the output, into blocks of exactly *out_nv vertices and *out_nt triangles. A kept vertex carries its own 16 + 16 (+ 4)
// bytes; a surviving triangle is its three indices in the output's numbering. rgba and out_rgba may both be NULL.
ODO_MC_HD void mc_ref_emit(const float* xyz0, const float* nrmw, const uint8_t* rgba, const int32_t* tri, int n_v, int n_t,
                           const int32_t* vnew, const int32_t* label, float* out_xyz0, float* out_nrmw, uint8_t* out_rgba,
                           int32_t* out_tri) {
  for (int i = 0; i < n_v; i++) {
    if (vnew[i] < 0) continue;
    __builtin_memcpy(out_xyz0 + 4 * (size_t)vnew[i], xyz0 + 4 * (size_t)i, 16);   // (bytes, not floats: a NaN keeps its payload)
    __builtin_memcpy(out_nrmw + 4 * (size_t)vnew[i], nrmw + 4 * (size_t)i, 16);
    if (rgba) __builtin_memcpy(out_rgba + 4 * (size_t)vnew[i], rgba + 4 * (size_t)i, 4);
  }
  int m = 0;
  for (int t = 0; t < n_t; t++) {
    if (label[t] == kMcNoLabel || vnew[tri[3 * (size_t)t]] < 0) continue;   // (a valid triangle's vertices stay or leave with it)
    for (int c = 0; c < 3; c++) out_tri[3 * (size_t)m + c] = vnew[tri[3 * (size_t)t + c]];
    m++;
  }
}

}  // namespace odo
