// volume_mesh_emit.hip.h — the device code that the mesh of the window (volume_mesh_kernels.hip) and the mesh of the leaving slab
// (volume_shift_kernels.hip) share: what a voxel contributes to the mesh (mesh_voxel), and a voxel's
// vertices, its cell's triangles and its vertices' colours as functions. Both units' vertex and triangle kernels call mesh_vertices
// and mesh_triangles: in the window's kernels the call moves an if-conversion and two operand orders (vertices, 16 of 2 298 lines
// of gfx950 code) or one instruction's place (triangles), same registers, and their times are the parent's within what kernels
// with identical code move in the same runs. mesh_vertex_colours is called by the slab's colour kernel
// only: volume_mesh_colour_kernel (volume_colour_kernels.hip) keeps the same body in its own text, because calling the function
// cost it 15 instructions more and, measured against the parent in alternating runs, 15.64 -> 16.38 us on the pinned grid and
// 97.78 -> 100.98 us on the large one (+4.7 % / +3.3 %, identical kernels within 2.3 %); the tests hold the two to the same bits.
// The arithmetic is volume_math.h's and volume_colour_math.h's (fp32, one rounding per operation: every unit is built with
// -ffp-contract=off and correctly rounded divide / sqrt), the triangles are integers out of volume_mesh_table.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "volume.hip.h"
#include "volume_mesh_table.h"
#include "volume_colour_math.h"

namespace odo {

// What the count and the triangle pass both need of voxel v (< n): the 7-bit mask of its edges that carry a vertex, and of its cell
// whether it is live (all eight corners observed) and which corners are positive. A neighbour outside the grid is never loaded.
__device__ __forceinline__ void mesh_voxel(const VolGrid& g, int v, unsigned* edge_mask, bool* live, unsigned* pos8) {
  *edge_mask = 0;
  *live = false;
  *pos8 = 0;
  const uint32_t va = g.vox[v];
  if (vox_w(va) == 0) return;   // no edge of an unobserved voxel carries a vertex, and its cell is not live
  int i, j, k;
  vox_ijk(g, v, &i, &j, &k);
  const bool in_x = i + 1 < g.nx, in_y = j + 1 < g.ny, in_z = k + 1 < g.nz;
  const bool pa = vox_q(va) > 0;
  unsigned mask = 0, pos = pa ? 1u : 0u, observed = 1u;
#pragma unroll
  for (int e = 0; e < 7; e++) {
    const int c = mtet_dir_offset(e);
    const bool inside = (!(c & 1) || in_x) && (!(c & 2) || in_y) && (!(c & 4) || in_z);
    if (!inside) continue;
    const uint32_t vb = g.vox[vox_corner_word(g, v, c)];
    if (vox_w(vb) == 0) continue;
    const bool pb = vox_q(vb) > 0;
    observed |= 1u << c;
    pos |= (pb ? 1u : 0u) << c;
    mask |= (pa != pb ? 1u : 0u) << e;
  }
  *edge_mask = mask;
  *live = observed == 0xffu;
  *pos8 = pos;
}

// The vertices of voxel v (mask != 0), from index idx on: position and edge number, normal and weight. Nothing at or beyond cap.
__device__ __forceinline__ void mesh_vertices(const VolGrid& g, int v, unsigned mask, unsigned long long idx, unsigned long long cap,
                                              float4* xyz0, float4* nrmw) {
  int i, j, k;
  vox_ijk(g, v, &i, &j, &k);
  const uint32_t va = g.vox[v];
  float ga[3], gb[3];
  const bool has_a = vox_gradient(g, v, i, j, k, va, ga);
  const float cx = vox_centre(g.ox, i, g.vs), cy = vox_centre(g.oy, j, g.vs), cz = vox_centre(g.oz, k, g.vs);
  for (int e = 0; e < 7; e++) {
    if (!((mask >> e) & 1u)) continue;
    if (idx >= cap) return;
    const int c = mtet_dir_offset(e);
    const int dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
    const long long vb_i = vox_corner_word(g, v, c);
    const uint32_t vb = g.vox[vb_i];
    const bool has_b = vox_gradient(g, vb_i, i + dx, j + dy, k + dz, vb, gb);
    const VoxEdgePoint p = vox_edge_point(va, vb, has_a, ga, has_b, gb, cx, cy, cz, g.vs, dx, dy, dz);
    xyz0[idx] = make_float4(p.x, p.y, p.z, (float)e);
    nrmw[idx] = make_float4(p.nx, p.ny, p.nz, p.w);
    idx++;
  }
}

// The triangles of the live cell v with corner signs pos8, from index idx on: per triangle vertex the owner voxel's first index +
// the rank of the edge in the owner's mask; wound by the table, rotated to the smallest index first. Nothing at or beyond cap.
__device__ __forceinline__ void mesh_triangles(const VolGrid& g, const MtetTable& table, int v, unsigned pos8, unsigned long long idx,
                                               unsigned long long cap, const uint32_t* vertex_base, const uint8_t* edge_mask, int* tri) {
  for (int t = 0; t < 6; t++) {
    const int m = mtet_mask(t, pos8);
    const int n = mtet_count(m);
    for (int r = 0; r < n; r++) {
      if (idx >= cap) return;   // (so are the cell's later triangles)
      int id[3];
#pragma unroll
      for (int x = 0; x < 3; x++) {
        int c, e;
        mtet_lookup(table, t, m, r, x, &c, &e);
        const long long owner = vox_corner_word(g, v, c);   // (a live cell: all eight corners are inside the grid)
        id[x] = (int)(vertex_base[owner] + (unsigned)__popc((unsigned)edge_mask[owner] & ((1u << e) - 1u)));
      }
      // the smallest index first, the cyclic order kept
      int o0 = id[0], o1 = id[1], o2 = id[2];
      if (id[1] < id[0] && id[1] < id[2]) { o0 = id[1]; o1 = id[2]; o2 = id[0]; }
      else if (id[2] < id[0] && id[2] < id[1]) { o0 = id[2]; o1 = id[0]; o2 = id[1]; }
      int* out = tri + 3 * idx;
      out[0] = o0; out[1] = o1; out[2] = o2;
      idx++;
    }
  }
}

// The colours of voxel v's vertices (mask != 0), from index idx on: volume_colour_math.h's interpolation at the edge's alpha.
__device__ __forceinline__ void mesh_vertex_colours(const VolGrid& g, const uint32_t* col, int v, unsigned mask, unsigned long long idx,
                                                    unsigned long long cap, uint32_t* rgba) {
  const uint32_t va = g.vox[v], ca = col[v];
#pragma unroll
  for (int e = 0; e < 7; e++) {
    if (!((mask >> e) & 1u)) continue;
    if (idx >= cap) return;
    const long long vb = vox_corner_word(g, v, mtet_dir_offset(e));
    rgba[idx] = colour_interpolate(ca, col[vb], vox_alpha(va, g.vox[vb]));
    idx++;
  }
}

}  // namespace odo
