// volume_colour_kernels.hip — the colours of the TSDF volume's extracted points and mesh vertices (volume_colour.hip.h) as a translation
// unit of their own, plus their host-side launchers. The arithmetic is the table of include/odometry_hip.h (odo_volume_extract_colour,
// odo_volume_mesh_colour) / DESIGN.md section 9.6: the edge's alpha out of volume_math.h (fp32, one rounding per operation: the unit is
// built with -ffp-contract=off and correctly rounded divide), the interpolation out of volume_colour_math.h. The coloured integration
// is volume_kernels.hip's.
#include <hip/hip_runtime.h>
#include "volume_colour.hip.h"
#include "volume_colour_math.h"
#include "volume_mesh_table.h"
#include "volume_scan.hip.h"

namespace odo {

// ---- colours of the extraction's points -------------------------------------------------------------------------------------------
// A thread per voxel at volume_scatter_kernel's index (block offset + volume_scan.hip.h's rank); one dword per point.
__global__ void __launch_bounds__(kVolExtBlock) volume_extract_colour_kernel(VolExtractColourArgs ac) {
  const VolExtractArgs& a = ac.a;
  const int v = blockIdx.x * kVolExtBlock + threadIdx.x;
  const unsigned long long bit = 1ull << (threadIdx.x & 63);
  unsigned long long e[3];
  ballot_wave(a.wave_mask, e);
  const unsigned long long bx = e[0], by = e[1], bz = e[2];
  if (v >= a.n || !((bx | by | bz) & bit)) return;
  const int rank = ballot_rank<3, int>(a.wave_mask, e);
  unsigned long long idx = a.blk_off[blockIdx.x] + (unsigned long long)rank;
  const unsigned long long cap = (unsigned long long)a.capacity;
  if (idx >= cap) return;
  const uint32_t va = a.g.vox[v], ca = ac.col[v];
  const size_t sy = (size_t)a.g.nx, sz = (size_t)a.g.nx * a.g.ny;
  if (bx & bit) {
    ac.rgba[idx++] = colour_interpolate(ca, ac.col[v + 1], vox_alpha(va, a.g.vox[v + 1]));
    if (idx >= cap) return;
  }
  if (by & bit) {
    ac.rgba[idx++] = colour_interpolate(ca, ac.col[v + sy], vox_alpha(va, a.g.vox[v + sy]));
    if (idx >= cap) return;
  }
  if (bz & bit) ac.rgba[idx] = colour_interpolate(ca, ac.col[v + sz], vox_alpha(va, a.g.vox[v + sz]));
}

void launch_volume_extract_colour(const VolExtractColourArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_extract_colour_kernel, dim3(a.a.nblk), dim3(kVolExtBlock), 0, s, a);
}

// ---- colours of the mesh's vertices -----------------------------------------------------------------------------------------------
// A thread per voxel: the vertex kernel left the voxel's first index (vertex_base) beside its edge mask. The body is
// volume_mesh_emit.hip.h's mesh_vertex_colours in this kernel's own text: calling the function cost 3 to 5 % (see that header).
__global__ void __launch_bounds__(kMeshBlock) volume_mesh_colour_kernel(VolMeshColourArgs ac) {
  const VolMeshArgs& a = ac.a;
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  if (v >= a.n) return;
  const unsigned mask = (unsigned)a.edge_mask[v];
  if (!mask) return;
  unsigned long long idx = a.vertex_base[v];
  const unsigned long long cap = (unsigned long long)a.vertex_capacity;
  if (idx >= cap) return;
  const uint32_t va = a.g.vox[v], ca = ac.col[v];
#pragma unroll
  for (int e = 0; e < 7; e++) {
    if (!((mask >> e) & 1u)) continue;
    if (idx >= cap) return;
    const long long vb = vox_corner_word(a.g, v, mtet_dir_offset(e));
    ac.rgba[idx] = colour_interpolate(ca, ac.col[vb], vox_alpha(va, a.g.vox[vb]));
    idx++;
  }
}

void launch_volume_mesh_colour(const VolMeshColourArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_mesh_colour_kernel, dim3(a.a.nblk), dim3(kMeshBlock), 0, s, a);
}

}  // namespace odo
