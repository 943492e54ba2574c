// volume_shift_kernels.hip — the moving TSDF volume's kernels (volume_shift.hip.h) as a translation unit of their own, plus their
// host-side launchers: the shift of both grids by whole voxels, and the spill of the surface points that a shift destroys into the
// volume's store. The rules are volume_shift_math.h's, the points volume_math.h's and volume_colour_math.h's (fp32, one rounding per
// operation: the unit is built with -ffp-contract=off and correctly rounded divide / sqrt), so a spilled point is bit for bit the
// point odo_volume_extract / _extract_colour gives for the same edge of the pre-shift grid. include/odometry_hip.h, odo_volume_shift;
// DESIGN.md section 9.9. Behind them the spill of the leaving slab's MESH into the volume's mesh store.
#include <hip/hip_runtime.h>
#include "volume_shift.hip.h"
#include "volume_shift_math.h"
#include "volume_colour_math.h"
#include "volume_mesh_emit.hip.h"
#include "volume_scan.hip.h"

namespace odo {

// ---- the shift -------------------------------------------------------------------------------------------------------------------
// Four x-consecutive voxels of the new grid per thread. Aligned on the destination: with nx % 4 == 0 (Vec) a thread's four words are
// one 16-byte store and a wave's stores cover 1 KiB without a gap; the sources are dx words off and are read as one 16-byte load only
// when dx % 4 == 0 and all four lie inside the old row, as four dword loads otherwise (the neighbouring lanes use the rest of every
// line they touch). A row whose (j + dy, k + dz) lies outside the old grid loads nothing and stores zeros. Any nx: the same walk with
// dword stores and a guard at the row's end.
template <bool Vec>
__device__ __forceinline__ void shift_quad(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t drow, size_t srow, bool row_in,
                                           int i0, int nx, int dx) {
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (row_in) {
    int s0, s3;
    const bool in0 = shift_source(i0, dx, nx, &s0), in3 = shift_source(i0 + 3, dx, nx, &s3);
    if (Vec && (dx & 3) == 0 && in0 && in3) {
      const uint4 q = *reinterpret_cast<const uint4*>(src + srow + s0);   // (s0 = i0 + dx, a multiple of 4; rows are multiples of 4 words)
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
#pragma unroll
      for (int t = 0; t < 4; t++) {
        int si;
        if (i0 + t < nx && shift_source(i0 + t, dx, nx, &si)) w[t] = src[srow + si];
      }
    }
  }
  if (Vec) {
    *reinterpret_cast<uint4*>(dst + drow + i0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (i0 + t < nx) dst[drow + i0 + t] = w[t];
  }
}

// A block is kVolShiftLanes x kVolShiftRows threads: threadIdx.y picks one of kVolShiftRows consecutive rows j of the plane k, and the
// row's quads are walked kVolShiftLanes at a time; blockIdx.y walks the planes (in strides of the grid's y extent, which the launch
// keeps within 65 535). No thread divides: j, k and the quad come straight from the launch geometry.
template <bool Vec>
__global__ void __launch_bounds__(kVolShiftBlock) volume_shift_kernel(VolShiftArgs a) {
  const int qpr = (a.nx + 3) >> 2;                                             // quads per row
  const int j = (int)blockIdx.x * kVolShiftRows + (int)threadIdx.y;
  if (j >= a.ny) return;
  int sj, sk;
  const bool j_in = shift_source(j, a.dy, a.ny, &sj);
  for (int k = (int)blockIdx.y; k < a.nz; k += (int)gridDim.y) {
    const bool row_in = j_in & shift_source(k, a.dz, a.nz, &sk);
    const size_t drow = ((size_t)k * a.ny + j) * a.nx, srow = row_in ? ((size_t)sk * a.ny + sj) * a.nx : 0;
    for (int qi = (int)threadIdx.x; qi < qpr; qi += kVolShiftLanes) {
      shift_quad<Vec>(a.src, a.dst, drow, srow, row_in, qi << 2, a.nx, a.dx);
      if (a.src_col) shift_quad<Vec>(a.src_col, a.dst_col, drow, srow, row_in, qi << 2, a.nx, a.dx);
    }
  }
}

void launch_volume_shift(const VolShiftArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.ny + kVolShiftRows - 1) / kVolShiftRows), (unsigned)(a.nz < 65535 ? a.nz : 65535)), block(kVolShiftLanes, kVolShiftRows);
  if ((a.nx & 3) == 0) hipLaunchKernelGGL(volume_shift_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(volume_shift_kernel<false>, grid, block, 0, s, a);
}

// ---- the spill -------------------------------------------------------------------------------------------------------------------
// The extraction's passes (volume_scan.hip.h) with the predicate ANDed in: the edge a -> b counts iff it carries a point and a or b
// leaves.
__global__ void __launch_bounds__(kVolExtBlock) volume_spill_count_kernel(VolSpillArgs sa) {
  const VolExtractArgs& a = sa.a;
  const int v = blockIdx.x * kVolExtBlock + threadIdx.x;
  bool ex = false, ey = false, ez = false;
  if (v < a.n) {
    const uint32_t va = a.g.vox[v];
    if (vox_w(va) > 0) {
      int i, j, k;
      vox_ijk(a.g, v, &i, &j, &k);
      const size_t sy = (size_t)a.g.nx, sz = (size_t)a.g.nx * a.g.ny;
      const bool la = shift_leaves(i, sa.dx, a.g.nx) || shift_leaves(j, sa.dy, a.g.ny) || shift_leaves(k, sa.dz, a.g.nz);
      ex = i + 1 < a.g.nx && (la || shift_leaves(i + 1, sa.dx, a.g.nx)) && vox_edge(va, a.g.vox[v + 1]);
      ey = j + 1 < a.g.ny && (la || shift_leaves(j + 1, sa.dy, a.g.ny)) && vox_edge(va, a.g.vox[v + sy]);
      ez = k + 1 < a.g.nz && (la || shift_leaves(k + 1, sa.dz, a.g.nz)) && vox_edge(va, a.g.vox[v + sz]);
    }
  }
  const unsigned long long b[3] = {__ballot(ex), __ballot(ey), __ballot(ez)};
  ballot_counts(b, a.wave_mask, a.blk);
}

// One block: the blocks' exclusive offsets; the sum is left for scatter's clamp and advance.
__global__ void __launch_bounds__(kVolScanThreads) volume_spill_scan_kernel(VolSpillArgs sa) {
  const unsigned long long total = scan_counts<kVolScanThreads, 1>(sa.a.blk, sa.a.blk_off, sa.a.nblk).t[0];
  if (threadIdx.x == 0) sa.sc->pending = total;
}

// The points behind the store's earlier ones: index = written + block offset + rank; nothing at or beyond capacity is written. With
// the colours, when the store has them.
__global__ void __launch_bounds__(kVolExtBlock) volume_spill_scatter_kernel(VolSpillArgs sa) {
  const VolExtractArgs& a = sa.a;
  const int v = blockIdx.x * kVolExtBlock + threadIdx.x;
  const unsigned long long bit = 1ull << (threadIdx.x & 63);
  unsigned long long e[3];
  ballot_wave(a.wave_mask, e);
  if (v >= a.n || !((e[0] | e[1] | e[2]) & bit)) return;
  const int rank = ballot_rank<3, int>(a.wave_mask, e);
  const unsigned long long idx = sa.sc->written + a.blk_off[blockIdx.x] + (unsigned long long)rank;
  extract_points(a.g, v, e, bit, idx, (unsigned long long)a.capacity, a.xyz0, a.nrmw, sa.col, sa.rgba);
}

// One thread, behind the scatter that read `written`: the counters move on.
__global__ void volume_spill_advance_kernel(VolSpillArgs sa) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  // Both stores carry values computed from the loads, so neither can be issued before its loads have returned, whichever kind of
  // load the compiler picks. Volatile in addition makes the three reads vector loads that are each waited for: read from the
  // gfx950 disassembly, flat_load_dwordx2 ... sc0 sc1 followed by s_waitcnt vmcnt(0), three times, in front of the two stores.
  // (Only supposed, not shown: that a uniform read through a plain pointer, which the compiler may turn into a scalar load, can be
  // overtaken by a store of this thread that does not depend on it. An earlier form of this kernel had such a store.)
  volatile VolSpillCounters* sc = sa.sc;
  const unsigned long long written = sc->written, total = sc->total, pending = sc->pending;
  const unsigned long long cap = (unsigned long long)sa.a.capacity, end = written + pending;
  sc->total = total + pending;
  sc->written = end < cap ? end : cap;   // (pending stays: the next spill's scan writes it before anything reads it)
}

void launch_volume_spill(const VolSpillArgs& a, hipStream_t s) {
  const dim3 grid(a.a.nblk), block(kVolExtBlock);
  hipLaunchKernelGGL(volume_spill_count_kernel, grid, block, 0, s, a);
  hipLaunchKernelGGL(volume_spill_scan_kernel, dim3(1), dim3(kVolScanThreads), 0, s, a);
  hipLaunchKernelGGL(volume_spill_scatter_kernel, grid, block, 0, s, a);
  hipLaunchKernelGGL(volume_spill_advance_kernel, dim3(1), dim3(64), 0, s, a);
}

void launch_volume_spill_stage(const VolSpillArgs& a, int stage, hipStream_t s) {
  const dim3 grid(a.a.nblk), block(kVolExtBlock);
  if (stage == 0) hipLaunchKernelGGL(volume_spill_count_kernel, grid, block, 0, s, a);
  else if (stage == 1) hipLaunchKernelGGL(volume_spill_scan_kernel, dim3(1), dim3(kVolScanThreads), 0, s, a);
  else hipLaunchKernelGGL(volume_spill_scatter_kernel, grid, block, 0, s, a);
}

// ---- the mesh of the leaving slab ----------------------------------------------------------------------------------------------------
// volume_mesh_kernels.hip's four passes (the device code is volume_mesh_emit.hip.h's, compiled by both units) over the pre-shift grid,
// with the predicates of volume_shift_math.h ANDed in; see volume_shift.hip.h.
__constant__ MtetTable c_spill_mtet = make_mtet_table();

// Voxel v's coordinates and whether it is within one voxel of a leaving voxel. Arithmetic only: nothing is loaded.
__device__ __forceinline__ bool spill_mesh_near(const VolSpillMeshArgs& sa, int v, int* i, int* j, int* k) {
  const VolGrid& g = sa.a.g;
  if (v >= sa.a.n) return false;
  vox_ijk(g, v, i, j, k);
  return shift_near(*i, *j, *k, sa.dx, sa.dy, sa.dz, g.nx, g.ny, g.nz);
}

// Whether the spill that the scan counted fits what is left of both capacities, and the store's fill in front of it. Every block of
// every emitting kernel reads the same four counters (the advance kernel moves them behind the last of those kernels).
__device__ __forceinline__ bool spill_mesh_fits(const VolSpillMeshArgs& sa, unsigned long long* v_written, unsigned long long* t_written) {
  const VolSpillMeshCounters* sc = sa.sc;
  *v_written = sc->v_written;
  *t_written = sc->t_written;
  return *v_written + sc->v_pending <= (unsigned long long)sa.a.vertex_capacity &&
         *t_written + sc->t_pending <= (unsigned long long)sa.a.triangle_capacity;
}

__global__ void __launch_bounds__(kMeshBlock) volume_spill_mesh_count_kernel(VolSpillMeshArgs sa) {
  const VolMeshArgs& a = sa.a;
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  int i = 0, j = 0, k = 0;
  const bool near = spill_mesh_near(sa, v, &i, &j, &k);
  if (!__syncthreads_or(near)) {   // no voxel of this block is near the slab: its two zero counts, nothing loaded
    if (threadIdx.x < 2) a.blk[2 * blockIdx.x + threadIdx.x] = 0u;
    return;
  }
  unsigned nv = 0, nt = 0;
  if (near) {
    unsigned mask, pos8;
    bool live;
    mesh_voxel(a.g, v, &mask, &live, &pos8);
    unsigned spilled = 0;
#pragma unroll
    for (int e = 0; e < 7; e++)
      spilled |= (shift_edge_spilled(i, j, k, mtet_dir_offset(e), sa.dx, sa.dy, sa.dz, a.g.nx, a.g.ny, a.g.nz) ? 1u : 0u) << e;
    mask &= spilled;
    a.edge_mask[v] = (uint8_t)mask;
    nv = (unsigned)__popc(mask);
    // (a live cell has all eight corners inside the grid: i + 1 < nx, j + 1 < ny, k + 1 < nz)
    nt = live && shift_cell_spilled(i, j, k, sa.dx, sa.dy, sa.dz, a.g.nx, a.g.ny, a.g.nz) ? (unsigned)mtet_cell_count(pos8) : 0u;
  }
  block_sum2<kMeshBlock>(nv, nt, a.blk);
}

// One block: both per-block counts' exclusive offsets; the two sums are left for the emitting kernels and advance.
__global__ void __launch_bounds__(kMeshScanThreads) volume_spill_mesh_scan_kernel(VolSpillMeshArgs sa) {
  const ScanTotals<2> total = scan_counts<kMeshScanThreads, 2>(sa.a.blk, sa.a.blk_off, sa.a.nblk);
  if (threadIdx.x == 0) { sa.sc->v_pending = total.t[0]; sa.sc->t_pending = total.t[1]; }
}

// volume_mesh_vertex_kernel behind the store's earlier vertices: index = v_written + block offset + rank, left per voxel as the
// store's index of the voxel's first vertex (what the triangles and the colours look up). A block without a vertex, and every block
// of a spill that does not fit, writes nothing.
__global__ void __launch_bounds__(kMeshBlock) volume_spill_mesh_vertex_kernel(VolSpillMeshArgs sa) {
  const VolMeshArgs& a = sa.a;
  __shared__ unsigned wsum[kMeshBlock / 64];
  unsigned long long v_written, t_written;
  if (a.blk[2 * blockIdx.x] == 0u || !spill_mesh_fits(sa, &v_written, &t_written)) return;   // (block-uniform)
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  int i, j, k;
  const unsigned mask = spill_mesh_near(sa, v, &i, &j, &k) ? (unsigned)a.edge_mask[v] : 0u;   // (count wrote it for near voxels only)
  const unsigned rank = scan_block<kMeshBlock>((unsigned)__popc(mask), wsum).rank;
  const unsigned long long idx = v_written + a.blk_off[2 * blockIdx.x] + rank;
  if (!mask) return;
  a.vertex_base[v] = (uint32_t)idx;   // (< 2^28: the spill fits the store)
  mesh_vertices(a.g, v, mask, idx, (unsigned long long)a.vertex_capacity, a.xyz0, a.nrmw);
}

// volume_mesh_triangle_kernel for the spilled cells. Every vertex a spilled cell's triangle names lies on an edge of that cell, which
// is a spilled edge by definition: its owner was near, and the vertex kernel left the owner's first index.
__global__ void __launch_bounds__(kMeshBlock) volume_spill_mesh_triangle_kernel(VolSpillMeshArgs sa) {
  const VolMeshArgs& a = sa.a;
  __shared__ unsigned wsum[kMeshBlock / 64];
  unsigned long long v_written, t_written;
  if (a.blk[2 * blockIdx.x + 1] == 0u || !spill_mesh_fits(sa, &v_written, &t_written)) return;   // (block-uniform)
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  int i, j, k;
  unsigned nt = 0, pos8 = 0;
  if (spill_mesh_near(sa, v, &i, &j, &k)) {
    unsigned mask;
    bool live;
    mesh_voxel(a.g, v, &mask, &live, &pos8);
    nt = live && shift_cell_spilled(i, j, k, sa.dx, sa.dy, sa.dz, a.g.nx, a.g.ny, a.g.nz) ? (unsigned)mtet_cell_count(pos8) : 0u;
  }
  const unsigned rank = scan_block<kMeshBlock>(nt, wsum).rank;
  const unsigned long long idx = t_written + a.blk_off[2 * blockIdx.x + 1] + rank;
  if (!nt) return;
  mesh_triangles(a.g, c_spill_mtet, v, pos8, idx, (unsigned long long)a.triangle_capacity, a.vertex_base, a.edge_mask, a.tri);
}

// volume_mesh_colour_kernel for the spilled vertices, at the indices the vertex kernel left.
__global__ void __launch_bounds__(kMeshBlock) volume_spill_mesh_colour_kernel(VolSpillMeshArgs sa) {
  const VolMeshArgs& a = sa.a;
  unsigned long long v_written, t_written;
  if (a.blk[2 * blockIdx.x] == 0u || !spill_mesh_fits(sa, &v_written, &t_written)) return;   // (block-uniform)
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  int i, j, k;
  if (!spill_mesh_near(sa, v, &i, &j, &k)) return;
  const unsigned mask = (unsigned)a.edge_mask[v];
  if (!mask) return;
  mesh_vertex_colours(a.g, sa.col, v, mask, a.vertex_base[v], (unsigned long long)a.vertex_capacity, sa.rgba);
}

// One thread, behind the kernels that read the counters: they move on, by the whole spill or not at all.
__global__ void volume_spill_mesh_advance_kernel(VolSpillMeshArgs sa) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  // As volume_spill_advance_kernel: the counters are read through a volatile pointer (vector loads, each waited for), and every
  // store carries a value computed from those loads, so none can be issued before its loads have returned. The pending counts stay:
  // the next spill's scan writes them before anything reads them.
  volatile VolSpillMeshCounters* sc = sa.sc;
  const unsigned long long vw = sc->v_written, tw = sc->t_written, vt = sc->v_total, tt = sc->t_total;
  const unsigned long long vp = sc->v_pending, tp = sc->t_pending;
  const bool fits = vw + vp <= (unsigned long long)sa.a.vertex_capacity && tw + tp <= (unsigned long long)sa.a.triangle_capacity;
  sc->v_total = vt + vp;
  sc->t_total = tt + tp;
  sc->v_written = vw + (fits ? vp : 0ull);
  sc->t_written = tw + (fits ? tp : 0ull);
}

void launch_volume_spill_mesh_stage(const VolSpillMeshArgs& a, int stage, hipStream_t s) {
  const dim3 grid(a.a.nblk), block(kMeshBlock);
  if (stage == 0) hipLaunchKernelGGL(volume_spill_mesh_count_kernel, grid, block, 0, s, a);
  else if (stage == 1) hipLaunchKernelGGL(volume_spill_mesh_scan_kernel, dim3(1), dim3(kMeshScanThreads), 0, s, a);
  else if (stage == 2) hipLaunchKernelGGL(volume_spill_mesh_vertex_kernel, grid, block, 0, s, a);
  else if (stage == 3) hipLaunchKernelGGL(volume_spill_mesh_triangle_kernel, grid, block, 0, s, a);
  else if (a.col) hipLaunchKernelGGL(volume_spill_mesh_colour_kernel, grid, block, 0, s, a);
}

void launch_volume_spill_mesh(const VolSpillMeshArgs& a, hipStream_t s) {
  for (int stage = 0; stage < 5; stage++) launch_volume_spill_mesh_stage(a, stage, s);
  hipLaunchKernelGGL(volume_spill_mesh_advance_kernel, dim3(1), dim3(64), 0, s, a);
}

}  // namespace odo
