// volume_mesh.hip.h — what the TSDF volume's mesh kernels (volume_mesh_kernels.hip, a translation unit of their own) and the host
// object (volume_api.hip.h, in the main unit) share: the launch arguments, the device-resident counters and the launchers.
//
// One mesh (odo_volume_mesh; include/odometry_hip.h / DESIGN.md section 9.5: marching tetrahedra on the Kuhn split of every live
// cell) = four launches on the volume's own stream, no atomics, the shape of the point extraction:
//   count      per voxel its own word and the seven neighbour words (+x +y +z +xy +xz +yz +xyz: the cell's eight corners): the 7-bit
//              mask of owned edges that carry a vertex, stored per voxel, and the cell's triangle count; per block the two sums.
//   scan       one block: exclusive block offsets of both counts, the totals, the clamps at the two capacities.
//   (the host reads the totals here: with nothing to write, or more than 2^31 - 1 vertices, the call ends)
//   vertices   per voxel the exclusive vertex base = block offset + rank in the block (stored per voxel, uint32), positions and
//              normals at base + rank in the mask.
//   triangles  per live cell block offset + rank in the block; per triangle vertex the owner voxel's base + rank of the edge in
//              the owner's mask; wound by the table, rotated to the smallest index first, three int32 stored.
// Output order = (voxel in raster order, e) and (cell in raster order, tetrahedron, triangle); nothing depends on timing.
// Scratch: 5 B per voxel (base + mask), 31 MB for a 240 x 128 x 200 grid, allocated by the first mesh call or by
// odo_volume_enable_spill_mesh (the mesh of the leaving slab, volume_shift.hip.h, uses it on the same stream), released with the volume.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "volume.hip.h"

namespace odo {

constexpr int kMeshBlock = 1024;         // threads (= voxels = cells) per block of count, vertices and triangles
constexpr int kMeshScanThreads = 1024;

// Device-resident counters of the last mesh.
struct MeshCounters {
  unsigned long long v_total, v_written;   // vertices found, vertices written (<= vertex capacity)
  unsigned long long t_total, t_written;   // triangles likewise
};

struct VolMeshArgs {
  VolGrid g;
  int n;       // nx * ny * nz
  int nblk;    // ceil(n / kMeshBlock)
  long long vertex_capacity, triangle_capacity;
  uint8_t* edge_mask;             // [n]: bit e set iff the edge (voxel, e) carries a vertex
  uint32_t* vertex_base;          // [n]: index of the voxel's first vertex
  unsigned* blk;                  // [2 * nblk]: vertices, triangles per block
  unsigned long long* blk_off;    // [2 * nblk]: their exclusive offsets
  MeshCounters* ctr;
  float4* xyz0;   // [vertex_capacity]
  float4* nrmw;   // [vertex_capacity]
  int* tri;       // [3 * triangle_capacity]
};

void launch_volume_mesh_count(const VolMeshArgs& a, hipStream_t s);                   // count, scan
void launch_volume_mesh_emit(const VolMeshArgs& a, bool triangles, hipStream_t s);    // vertices (always: the bases), triangles

}  // namespace odo
