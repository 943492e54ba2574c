// volume_mesh_kernels.hip — the TSDF volume's mesh kernels (volume_mesh.hip.h) as a translation unit of their own, plus their
// host-side launchers. The arithmetic is the table of include/odometry_hip.h (odo_volume_mesh) / DESIGN.md section 9.5: the vertices
// are the points of the extraction (volume_kernels.hip) carried over to seven edge directions, fp32, one rounding per operation (the
// unit is built with -ffp-contract=off and correctly rounded divide / sqrt); the triangles are integers out of the table of
// volume_mesh_table.h. Nothing is combined across threads but counts.
#include <hip/hip_runtime.h>
#include "volume_mesh.hip.h"
#include "volume_mesh_table.h"

namespace odo {

__constant__ MtetTable c_mtet = make_mtet_table();   // 672 bytes, derived at compile time

__device__ __forceinline__ int mesh_q(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }
__device__ __forceinline__ int mesh_w(uint32_t v) { return (int)(v >> 16); }
__device__ __forceinline__ float mesh_centre(float o, int i, float vs) { return o + ((float)i + 0.5f) * vs; }

__device__ __forceinline__ void mesh_ijk(const VolGrid& g, int v, int* i, int* j, int* k) {
  const int row = v / g.nx;
  *i = v - row * g.nx;
  *k = row / g.ny;
  *j = row - *k * g.ny;
}

// Word of the voxel at corner c (= dx + 2 dy + 4 dz) of the cell whose corner 0 is word v.
__device__ __forceinline__ long long mesh_corner_word(const VolGrid& g, int v, int c) {
  return (long long)v + (c & 1) + (long long)((c >> 1) & 1) * g.nx + (long long)((c >> 2) & 1) * g.nx * g.ny;
}

// What the count and the triangle pass both need of voxel v (< n): the 7-bit mask of its edges that carry a vertex, and of its cell
// whether it is live (all eight corners observed) and which corners are positive. A neighbour outside the grid is never loaded.
__device__ __forceinline__ void mesh_voxel(const VolGrid& g, int v, unsigned* edge_mask, bool* live, unsigned* pos8) {
  *edge_mask = 0;
  *live = false;
  *pos8 = 0;
  const uint32_t va = g.vox[v];
  if (mesh_w(va) == 0) return;   // no edge of an unobserved voxel carries a vertex, and its cell is not live
  int i, j, k;
  mesh_ijk(g, v, &i, &j, &k);
  const bool in_x = i + 1 < g.nx, in_y = j + 1 < g.ny, in_z = k + 1 < g.nz;
  const bool pa = mesh_q(va) > 0;
  unsigned mask = 0, pos = pa ? 1u : 0u, observed = 1u;
#pragma unroll
  for (int e = 0; e < 7; e++) {
    const int c = mtet_dir_offset(e);
    const bool inside = (!(c & 1) || in_x) && (!(c & 2) || in_y) && (!(c & 4) || in_z);
    if (!inside) continue;
    const uint32_t vb = g.vox[mesh_corner_word(g, v, c)];
    if (mesh_w(vb) == 0) continue;
    const bool pb = mesh_q(vb) > 0;
    observed |= 1u << c;
    pos |= (pb ? 1u : 0u) << c;
    mask |= (pa != pb ? 1u : 0u) << e;
  }
  *edge_mask = mask;
  *live = observed == 0xffu;
  *pos8 = pos;
}

// Exclusive rank of s among the block's threads in thread order. Every thread of the block calls it.
__device__ __forceinline__ unsigned mesh_block_rank(unsigned s, unsigned* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned inc = s;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  unsigned before = 0;
  for (int q = 0; q < kMeshBlock / 64; q++)
    if (q < w) before += wsum[q];
  return before + inc - s;
}

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
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned long long base[2] = {0, 0};
  for (int c0 = 0; c0 < a.nblk; c0 += kMeshScanThreads) {
    const int b = c0 + t;
    unsigned s[2], inc[2];
#pragma unroll
    for (int x = 0; x < 2; x++) {
      s[x] = b < a.nblk ? a.blk[2 * b + x] : 0u;   // (a chunk's sum is at most 1024 * 12 288: far below 2^32)
      inc[x] = s[x];
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(inc[x], o, 64);
        if (lane >= o) inc[x] += v;
      }
      if (lane == 63) wsum[x][w] = inc[x];
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 2; x++) {
      unsigned before = 0, total = 0;
      for (int q = 0; q < kMeshScanThreads / 64; q++) {
        if (q < w) before += wsum[x][q];
        total += wsum[x][q];
      }
      if (b < a.nblk) a.blk_off[2 * b + x] = base[x] + (unsigned long long)(before + inc[x] - s[x]);
      base[x] += total;
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

// The gradient of Q = (float)q at voxel (i, j, k), whose own word is vc: the extraction's rule unchanged.
__device__ __forceinline__ bool mesh_gradient(const VolGrid& g, long long v, int i, int j, int k, uint32_t vc, float* gx, float* gy, float* gz) {
  const float Q = (float)mesh_q(vc);
  const int pos[3] = {i, j, k}, dim[3] = {g.nx, g.ny, g.nz};
  const long long stride[3] = {1, g.nx, (long long)g.nx * g.ny};
  float out[3];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    uint32_t vp = 0, vm = 0;
    if (pos[c] + 1 < dim[c]) vp = g.vox[v + stride[c]];
    if (pos[c] > 0) vm = g.vox[v - stride[c]];
    const bool up = mesh_w(vp) > 0, um = mesh_w(vm) > 0;   // (a neighbour outside the grid stays 0: w = 0, not usable)
    const float Qp = (float)mesh_q(vp), Qm = (float)mesh_q(vm);
    float d = 0.0f;
    if (up && um) d = Qp - Qm;
    else if (up) d = 2.0f * (Qp - Q);
    else if (um) d = 2.0f * (Q - Qm);
    else ok = false;
    out[c] = d;
  }
  *gx = out[0]; *gy = out[1]; *gz = out[2];
  return ok;
}

__global__ void __launch_bounds__(kMeshBlock) volume_mesh_vertex_kernel(VolMeshArgs a) {
  __shared__ unsigned wsum[kMeshBlock / 64];
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  const unsigned mask = v < a.n ? (unsigned)a.edge_mask[v] : 0u;
  const unsigned rank = mesh_block_rank((unsigned)__popc(mask), wsum);
  unsigned long long idx = a.blk_off[2 * blockIdx.x] + rank;
  if (v < a.n) a.vertex_base[v] = (uint32_t)idx;   // (the host ends the call when the total does not fit 31 bits)
  const unsigned long long cap = (unsigned long long)a.vertex_capacity;
  if (!mask || idx >= cap) return;   // (so are this voxel's later vertices)
  int i, j, k;
  mesh_ijk(a.g, v, &i, &j, &k);
  const uint32_t va = a.g.vox[v];
  const float qa = (float)mesh_q(va);
  float gax, gay, gaz;
  const bool has_a = mesh_gradient(a.g, v, i, j, k, va, &gax, &gay, &gaz);
  const float cx = mesh_centre(a.g.ox, i, a.g.vs), cy = mesh_centre(a.g.oy, j, a.g.vs), cz = mesh_centre(a.g.oz, k, a.g.vs);
  for (int e = 0; e < 7; e++) {
    if (!((mask >> e) & 1u)) continue;
    if (idx >= cap) return;
    const int c = mtet_dir_offset(e);
    const int dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
    const long long vb_i = mesh_corner_word(a.g, v, c);
    const uint32_t vb = a.g.vox[vb_i];
    const float alpha = qa / (qa - (float)mesh_q(vb));
    const float step = alpha * a.g.vs;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, gbx, gby, gbz;
    const bool has_b = mesh_gradient(a.g, vb_i, i + dx, j + dy, k + dz, vb, &gbx, &gby, &gbz);
    if (has_a && has_b) {
      const float mx = gax + alpha * (gbx - gax), my = gay + alpha * (gby - gay), mz = gaz + alpha * (gbz - gaz);
      const float len = sqrtf((mx * mx + my * my) + mz * mz);
      if (len > 0.0f) { nx = mx / len; ny = my / len; nz = mz / len; }
    }
    a.xyz0[idx] = make_float4(dx ? cx + step : cx, dy ? cy + step : cy, dz ? cz + step : cz, (float)e);
    a.nrmw[idx] = make_float4(nx, ny, nz, (float)min(mesh_w(va), mesh_w(vb)));
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
  const unsigned rank = mesh_block_rank(nt, wsum);
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
        const long long owner = mesh_corner_word(a.g, v, c);   // (a live cell: all eight corners are inside the grid)
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
