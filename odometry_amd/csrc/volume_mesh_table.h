// volume_mesh_table.h — marching tetrahedra on the Kuhn split of a cell: the sign pattern -> triangles table of the TSDF volume's
// mesh (include/odometry_hip.h, odo_volume_mesh / DESIGN.md section 9.5) and its lookup. Plain C++17: it compiles under g++ (the
// test harness tests/volume_mesh_table_harness.cpp prints it) and under hipcc (volume_mesh_kernels.hip keeps it in constant memory).
// Nothing here is typed in: the table is DERIVED at compile time by the rule of the specification, the winding from the sign of a
// 3 x 3 determinant of corner offsets.
//
// Corners of a cell: c = dx + 2 dy + 4 dz. The seven edge directions e = 0 .. 6 are (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1)
// (1,1,1), i.e. the corner offsets 1 2 4 3 5 6 7. Tetrahedron t has the corner path (0, a_t, b_t, 7); every edge of it joins two
// path corners lo < hi and is owned by (the voxel at corner lo, the direction of hi - lo).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ODO_MT_HD __host__ __device__ __forceinline__
#else
#define ODO_MT_HD static inline
#endif

namespace odo {

constexpr unsigned kMtetDirOffsets = 0x7653421u;   // nibble e: the corner offset of direction e
constexpr unsigned kMtetOffsetDirs = 0x65423100u;  // nibble d: the direction of corner offset d (d = 1 .. 7)
constexpr unsigned kMtetPathA = 0x442211u;         // nibble t: the second corner of tetrahedron t's path
constexpr unsigned kMtetPathB = 0x656353u;        // nibble t: the third; paths (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7) (0,4,5,7) (0,4,6,7)

ODO_MT_HD constexpr int mtet_dir_offset(int e) { return (int)((kMtetDirOffsets >> (4 * e)) & 7u); }
ODO_MT_HD constexpr int mtet_offset_dir(int d) { return (int)((kMtetOffsetDirs >> (4 * d)) & 7u); }
ODO_MT_HD constexpr int mtet_corner(int t, int p) {
  return p == 0 ? 0 : p == 3 ? 7 : (int)(((p == 1 ? kMtetPathA : kMtetPathB) >> (4 * t)) & 7u);
}
// pos8: bit c set iff corner c has q > 0. The tetrahedron's pattern: bit p set iff its path corner p is positive.
ODO_MT_HD constexpr int mtet_mask(int t, unsigned pos8) {
  return (int)((pos8 & 1u) | (((pos8 >> mtet_corner(t, 1)) & 1u) << 1) | (((pos8 >> mtet_corner(t, 2)) & 1u) << 2) | (((pos8 >> 7) & 1u) << 3));
}
ODO_MT_HD constexpr int mtet_popcount4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }
// Triangles of a pattern: none for 0 or 4 positive corners, one for an isolated corner, two for two and two.
ODO_MT_HD constexpr int mtet_count(int m) { return mtet_popcount4(m) == 2 ? 2 : (mtet_popcount4(m) & 1); }
// Triangles of a live cell.
ODO_MT_HD constexpr int mtet_cell_count(unsigned pos8) {
  int n = 0;
  if (pos8 != 0u && pos8 != 0xffu)
    for (int t = 0; t < 6; t++) n += mtet_count(mtet_mask(t, pos8));
  return n;
}

// One entry: n triangles; triangle r has the vertices v[3 r .. 3 r + 2], each an edge as (corner of the owner voxel) | e << 3,
// wound counter-clockwise seen from the positive side (before the rotation that puts the smallest vertex index first).
struct MtetEntry {
  uint8_t n;
  uint8_t v[6];
};
struct MtetTable {
  MtetEntry e[6][16];
};

namespace mtet_detail {

struct I3 {
  int x, y, z;
};
constexpr I3 corner_xyz(int c) { return I3{c & 1, (c >> 1) & 1, (c >> 2) & 1}; }
constexpr I3 sub(I3 a, I3 b) { return I3{a.x - b.x, a.y - b.y, a.z - b.z}; }
constexpr I3 add(I3 a, I3 b) { return I3{a.x + b.x, a.y + b.y, a.z + b.z}; }
constexpr int det(I3 a, I3 b, I3 c) {   // (a x b) . c
  return (a.y * b.z - a.z * b.y) * c.x + (a.z * b.x - a.x * b.z) * c.y + (a.x * b.y - a.y * b.x) * c.z;
}
// The edge between path positions pa and pb of tetrahedron t.
constexpr uint8_t edge(int t, int pa, int pb) {
  const int lo = pa < pb ? pa : pb, hi = pa < pb ? pb : pa;
  const int ca = mtet_corner(t, lo), cb = mtet_corner(t, hi);
  return (uint8_t)(ca | (mtet_offset_dir(cb - ca) << 3));   // (the path only ever adds bits: cb - ca is the offset)
}

constexpr MtetEntry entry(int t, int m) {
  MtetEntry out{};
  I3 P[4] = {corner_xyz(mtet_corner(t, 0)), corner_xyz(mtet_corner(t, 1)), corner_xyz(mtet_corner(t, 2)), corner_xyz(mtet_corner(t, 3))};
  const int pc = mtet_popcount4(m);
  if (pc == 1 || pc == 3) {
    // the isolated corner s, the others r0 < r1 < r2 in path order: (s,r0) (s,r1) (s,r2). Seen at alpha = 1/2 the triangle's normal is
    // (r1 - r0) x (r2 - r0) / 4; it has to point towards s iff s is the positive corner.
    int s = 0, r[3] = {0, 0, 0}, nr = 0;
    for (int p = 0; p < 4; p++) {
      if ((((m >> p) & 1) == 1) == (pc == 1)) s = p;
      else r[nr++] = p;
    }
    const int d = det(sub(P[r[1]], P[r[0]]), sub(P[r[2]], P[r[0]]), sub(P[s], P[r[0]]));
    const bool keep = (d > 0) == (pc == 1);
    out.n = d == 0 ? 255 : 1;
    out.v[0] = edge(t, s, r[0]);
    out.v[1] = edge(t, s, keep ? r[1] : r[2]);
    out.v[2] = edge(t, s, keep ? r[2] : r[1]);
  } else if (pc == 2) {
    // positives a < b, the others c < d: the quad V0 = (a,c) V1 = (a,d) V2 = (b,d) V3 = (b,c), a parallelogram at alpha = 1/2 with
    // the normal (V1 - V0) x (V2 - V0) = (d - c) x ((b + d) - (a + c)) / 4; the positive side is towards (a + b) - (c + d).
    int pos[2] = {0, 0}, neg[2] = {0, 0}, np = 0, nn = 0;
    for (int p = 0; p < 4; p++) {
      if ((m >> p) & 1) pos[np++] = p;
      else neg[nn++] = p;
    }
    const int a = pos[0], b = pos[1], c = neg[0], d = neg[1];
    const int dd = det(sub(P[d], P[c]), sub(add(P[b], P[d]), add(P[a], P[c])), sub(add(P[a], P[b]), add(P[c], P[d])));
    const uint8_t V0 = edge(t, a, c), V1 = edge(t, a, d), V2 = edge(t, b, d), V3 = edge(t, b, c);
    out.n = dd == 0 ? 255 : 2;
    if (dd > 0) {
      out.v[0] = V0; out.v[1] = V1; out.v[2] = V2;
      out.v[3] = V0; out.v[4] = V2; out.v[5] = V3;
    } else {
      out.v[0] = V0; out.v[1] = V2; out.v[2] = V1;
      out.v[3] = V0; out.v[4] = V3; out.v[5] = V2;
    }
  }
  return out;
}

constexpr bool consistent(const MtetTable& T) {
  for (int t = 0; t < 6; t++)
    for (int m = 0; m < 16; m++)
      if ((int)T.e[t][m].n != mtet_count(m)) return false;   // (also: no determinant was 0)
  return true;
}

}  // namespace mtet_detail

constexpr MtetTable make_mtet_table() {
  MtetTable T{};
  for (int t = 0; t < 6; t++)
    for (int m = 0; m < 16; m++) T.e[t][m] = mtet_detail::entry(t, m);
  return T;
}
static_assert(mtet_detail::consistent(make_mtet_table()), "a tetrahedron of the split is degenerate or the counts disagree");

// Vertex x (0 .. 2) of triangle r of tetrahedron t under pattern m: *corner = the owner voxel's corner in the cell, *e = its edge.
ODO_MT_HD void mtet_lookup(const MtetTable& T, int t, int m, int r, int x, int* corner, int* e) {
  const int code = T.e[t][m].v[3 * r + x];
  *corner = code & 7;
  *e = code >> 3;
}

}  // namespace odo
