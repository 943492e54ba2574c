// volume_mesh_kernels.hip — the TSDF volume's mesh kernels (volume_mesh.hip.h) as a translation unit of their own, plus their
// host-side launchers. The arithmetic is the table of include/odometry_hip.h (odo_volume_mesh) / DESIGN.md section 9.5: the vertices
// are the points of the extraction carried over to seven edge directions: the same functions of volume_math.h, fp32, one rounding
// per operation (the unit is built with -ffp-contract=off and correctly rounded divide / sqrt); the triangles are integers out of the
// table of volume_mesh_table.h. Nothing is combined across threads but counts.
#include <hip/hip_runtime.h>
#include "volume_mesh.hip.h"
#include "volume_mesh_emit.hip.h"   // mesh_voxel: shared with the mesh of the leaving slab
#include "volume_scan.hip.h"

namespace odo {

__constant__ MtetTable c_mtet = make_mtet_table();   // 672 bytes, derived at compile time

__global__ void __launch_bounds__(kMeshBlock) volume_mesh_count_kernel(VolMeshArgs a) {
  __shared__ unsigned sh[2][kMeshBlock / 64];
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
  for (int o = 32; o > 0; o >>= 1) { nv += __shfl_xor(nv, o, 64); nt += __shfl_xor(nt, o, 64); }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][w] = nv; sh[1][w] = nt; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned t = 0;
    for (int q = 0; q < kMeshBlock / 64; q++) t += sh[threadIdx.x][q];
    a.blk[2 * blockIdx.x + threadIdx.x] = t;   // (<= 7 168 vertices, <= 12 288 triangles per block)
  }
}

// One block: exclusive scans of both per-block counts, 1024 blocks at a time (coalesced, a running base), the totals, the clamps.
__global__ void __launch_bounds__(kMeshScanThreads) volume_mesh_scan_kernel(VolMeshArgs a) {
  __shared__ unsigned wsum[2][kMeshScanThreads / 64];
  const int t = threadIdx.x;
  unsigned long long base[2] = {0, 0};
  for (int c0 = 0; c0 < a.nblk; c0 += kMeshScanThreads) {
    const int b = c0 + t;
    unsigned s[2], inc[2];
#pragma unroll
    for (int x = 0; x < 2; x++) {
      s[x] = b < a.nblk ? a.blk[2 * b + x] : 0u;   // (a chunk's sum is at most 1024 * 12 288: far below 2^32)
      inc[x] = scan_wave(s[x], wsum[x]);
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 2; x++) {
      const ScanRank r = scan_rank<kMeshScanThreads>(s[x], inc[x], wsum[x]);
      if (b < a.nblk) a.blk_off[2 * b + x] = base[x] + (unsigned long long)r.rank;
      base[x] += r.total;
    }
    __syncthreads();   // wsum is written again
  }
  if (t == 0) {
    const unsigned long long vc = (unsigned long long)a.vertex_capacity, tc = (unsigned long long)a.triangle_capacity;
    a.ctr->v_total = base[0];
    a.ctr->v_written = base[0] < vc ? base[0] : vc;
    a.ctr->t_total = base[1];
    a.ctr->t_written = base[1] < tc ? base[1] : tc;
  }
}

__global__ void __launch_bounds__(kMeshBlock) volume_mesh_vertex_kernel(VolMeshArgs a) {
  __shared__ unsigned wsum[kMeshBlock / 64];
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  const unsigned mask = v < a.n ? (unsigned)a.edge_mask[v] : 0u;
  const unsigned rank = scan_block<kMeshBlock>((unsigned)__popc(mask), wsum).rank;
  unsigned long long idx = a.blk_off[2 * blockIdx.x] + rank;
  if (v < a.n) a.vertex_base[v] = (uint32_t)idx;   // (the host ends the call when the total does not fit 31 bits)
  const unsigned long long cap = (unsigned long long)a.vertex_capacity;
  if (!mask || idx >= cap) return;   // (so are this voxel's later vertices)
  int i, j, k;
  vox_ijk(a.g, v, &i, &j, &k);
  const uint32_t va = a.g.vox[v];
  float ga[3], gb[3];
  const bool has_a = vox_gradient(a.g, v, i, j, k, va, ga);
  const float cx = vox_centre(a.g.ox, i, a.g.vs), cy = vox_centre(a.g.oy, j, a.g.vs), cz = vox_centre(a.g.oz, k, a.g.vs);
  for (int e = 0; e < 7; e++) {
    if (!((mask >> e) & 1u)) continue;
    if (idx >= cap) return;
    const int c = mtet_dir_offset(e);
    const int dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
    const long long vb_i = vox_corner_word(a.g, v, c);
    const uint32_t vb = a.g.vox[vb_i];
    const bool has_b = vox_gradient(a.g, vb_i, i + dx, j + dy, k + dz, vb, gb);
    const VoxEdgePoint p = vox_edge_point(va, vb, has_a, ga, has_b, gb, cx, cy, cz, a.g.vs, dx, dy, dz);
    a.xyz0[idx] = make_float4(p.x, p.y, p.z, (float)e);
    a.nrmw[idx] = make_float4(p.nx, p.ny, p.nz, p.w);
    idx++;
  }
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
  unsigned long long idx = a.blk_off[2 * blockIdx.x + 1] + rank;
  const unsigned long long cap = (unsigned long long)a.triangle_capacity;
  if (!nt) return;
  for (int t = 0; t < 6; t++) {
    const int m = mtet_mask(t, pos8);
    const int n = mtet_count(m);
    for (int r = 0; r < n; r++) {
      if (idx >= cap) return;   // (so are the cell's later triangles)
      int id[3];
#pragma unroll
      for (int x = 0; x < 3; x++) {
        int c, e;
        mtet_lookup(c_mtet, t, m, r, x, &c, &e);
        const long long owner = vox_corner_word(a.g, v, c);   // (a live cell: all eight corners are inside the grid)
        id[x] = (int)(a.vertex_base[owner] + (unsigned)__popc((unsigned)a.edge_mask[owner] & ((1u << e) - 1u)));
      }
      // the smallest index first, the cyclic order kept
      int o0 = id[0], o1 = id[1], o2 = id[2];
      if (id[1] < id[0] && id[1] < id[2]) { o0 = id[1]; o1 = id[2]; o2 = id[0]; }
      else if (id[2] < id[0] && id[2] < id[1]) { o0 = id[2]; o1 = id[0]; o2 = id[1]; }
      int* out = a.tri + 3 * idx;
      out[0] = o0; out[1] = o1; out[2] = o2;
      idx++;
    }
  }
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
