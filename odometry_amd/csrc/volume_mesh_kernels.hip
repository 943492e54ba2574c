// volume_mesh_kernels.hip — the TSDF volume's mesh kernels (volume_mesh.hip.h) as a translation unit of their own, plus their
// host-side launchers. The arithmetic is the table of include/odometry_hip.h (odo_volume_mesh) / DESIGN.md section 9.5: the vertices
// are the points of the extraction carried over to seven edge directions: the same functions of volume_math.h, fp32, one rounding
// per operation (the unit is built with -ffp-contract=off and correctly rounded divide / sqrt); the triangles are integers out of the
// table of volume_mesh_table.h. Nothing is combined across threads but counts.
#include <hip/hip_runtime.h>
#include "volume_mesh.hip.h"
#include "volume_mesh_emit.hip.h"   // shared with the mesh of the leaving slab
#include "volume_scan.hip.h"

namespace odo {

__constant__ MtetTable c_mtet = make_mtet_table();   // 672 bytes, derived at compile time

__global__ void __launch_bounds__(kMeshBlock) volume_mesh_count_kernel(VolMeshArgs a) {
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  unsigned nv = 0, nt = 0;
  if (v < a.n) {
    unsigned mask, pos8;
    bool live;
    mesh_voxel(a.g, v, &mask, &live, &pos8);
    a.edge_mask[v] = (uint8_t)mask;
    nv = (unsigned)__popc(mask);
    nt = live ? (unsigned)mtet_cell_count(pos8) : 0u;
  }
  block_sum2<kMeshBlock>(nv, nt, a.blk);   // (<= 7 168 vertices, <= 12 288 triangles per block)
}

// One block: both per-block counts' exclusive offsets (volume_scan.hip.h), the totals, the clamps.
__global__ void __launch_bounds__(kMeshScanThreads) volume_mesh_scan_kernel(VolMeshArgs a) {
  const ScanTotals<2> total = scan_counts<kMeshScanThreads, 2>(a.blk, a.blk_off, a.nblk);
  if (threadIdx.x == 0) {
    const unsigned long long vc = (unsigned long long)a.vertex_capacity, tc = (unsigned long long)a.triangle_capacity;
    a.ctr->v_total = total.t[0];
    a.ctr->v_written = total.t[0] < vc ? total.t[0] : vc;
    a.ctr->t_total = total.t[1];
    a.ctr->t_written = total.t[1] < tc ? total.t[1] : tc;
  }
}

__global__ void __launch_bounds__(kMeshBlock) volume_mesh_vertex_kernel(VolMeshArgs a) {
  __shared__ unsigned wsum[kMeshBlock / 64];
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  const unsigned mask = v < a.n ? (unsigned)a.edge_mask[v] : 0u;
  const unsigned rank = scan_block<kMeshBlock>((unsigned)__popc(mask), wsum).rank;
  const unsigned long long idx = a.blk_off[2 * blockIdx.x] + rank;
  if (v < a.n) a.vertex_base[v] = (uint32_t)idx;   // (the host ends the call when the total does not fit 31 bits)
  const unsigned long long cap = (unsigned long long)a.vertex_capacity;
  if (!mask || idx >= cap) return;   // (so are this voxel's later vertices)
  mesh_vertices(a.g, v, mask, idx, cap, a.xyz0, a.nrmw);
}

__global__ void __launch_bounds__(kMeshBlock) volume_mesh_triangle_kernel(VolMeshArgs a) {
  __shared__ unsigned wsum[kMeshBlock / 64];
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  unsigned nt = 0, pos8 = 0;
  if (v < a.n) {
    unsigned mask;
    bool live;
    mesh_voxel(a.g, v, &mask, &live, &pos8);
    nt = live ? (unsigned)mtet_cell_count(pos8) : 0u;
  }
  const unsigned rank = scan_block<kMeshBlock>(nt, wsum).rank;
  const unsigned long long idx = a.blk_off[2 * blockIdx.x + 1] + rank;
  if (!nt) return;
  mesh_triangles(a.g, c_mtet, v, pos8, idx, (unsigned long long)a.triangle_capacity, a.vertex_base, a.edge_mask, a.tri);
}

void launch_volume_mesh_count(const VolMeshArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_mesh_count_kernel, dim3(a.nblk), dim3(kMeshBlock), 0, s, a);
  hipLaunchKernelGGL(volume_mesh_scan_kernel, dim3(1), dim3(kMeshScanThreads), 0, s, a);
}

void launch_volume_mesh_emit(const VolMeshArgs& a, bool triangles, hipStream_t s) {
  hipLaunchKernelGGL(volume_mesh_vertex_kernel, dim3(a.nblk), dim3(kMeshBlock), 0, s, a);
  if (triangles) hipLaunchKernelGGL(volume_mesh_triangle_kernel, dim3(a.nblk), dim3(kMeshBlock), 0, s, a);
}

}  // namespace odo
