// volume_raycast_kernels.hip — the TSDF volume's ray-cast kernel (volume_raycast.hip.h) as a translation unit of its own, plus its
// host-side launcher. The arithmetic is the table of include/odometry_hip.h (odo_volume_raycast_dev) / DESIGN.md section 9.7 and lives
// in volume_raycast_math.h — fp32, one rounding per operation, the unit is built with -ffp-contract=off and correctly rounded divide
// and sqrt. The kernel adds the pixel of a thread, the loads and the stores. It is instantiated twice: volume_raycast_kernel writes the
// nearest voxel's colour, volume_raycast_interp_kernel the trilinear average of the cell's coloured corners.
#include <hip/hip_runtime.h>
#include "volume_raycast.hip.h"
#include "volume_raycast_math.h"

namespace odo {

// Two x-adjacent voxel words as one 8-byte access. The pair starts at any word, so it is only 4-byte aligned; the last word read
// is that of voxel (bx + 1, by + 1, bz + 1) with b + 1 <= dim - 1 on every axis (rc_in), inside the grid.
struct RayLoad2 {
  const uint32_t* vox;
  __device__ __forceinline__ uint64_t operator()(size_t word) const {
    uint64_t two;
    __builtin_memcpy(&two, vox + word, 8);
    return two;
  }
};

// The voxel pair and, beside it, the colour pair at the same index of the colour grid (the grids share their layout): rc_cell's four
// loads become eight that are issued together and waited for once. The pairs land in cp in the order of rc_cell's calls, which is
// the corner order of RcCell::c; the colour grid's last word read is that of the voxel grid's, inside the grid by rc_in.
struct RayLoad2Colour {
  const uint32_t* vox;
  const uint32_t* col;
  uint64_t* cp;   // [4]
  int* n;         // the calls so far
  __device__ __forceinline__ uint64_t operator()(size_t word) const {
    uint64_t two;
    __builtin_memcpy(&two, vox + word, 8);
    __builtin_memcpy(&cp[(*n)++ & 3], col + word, 8);
    return two;
  }
};

// A thread per pixel. Every sample is taken as the specification states it (no sample is skipped): a sample outside the grid costs
// its position and the comparisons and loads nothing. kInterp: the colour frame is rc_colour_interp's (launched only with rgba set).
// The arguments by value, as the kernel has them: through a reference volume_raycast_kernel's blocks come out in another order.
template <bool kInterp>
__device__ __forceinline__ void volume_raycast_body(const VolRaycastArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int x = blockIdx.x * kRayTile + (w & 1) * kRayWave + (lane & 7);
  const int y = blockIdx.y * kRayTile + (w >> 1) * kRayWave + (lane >> 3);
  if (x >= a.cols || y >= a.rows) return;
  const float dx = rc_pixel(x, a.cx, a.f), dy = rc_pixel(y, a.cy, a.f);
  RcRay r;
  r.nx = a.nx; r.ny = a.ny; r.nz = a.nz;
  r.ex = a.ex; r.ey = a.ey; r.ez = a.ez;
  r.gx = rc_dir(a.g00, a.g01, a.g02, dx, dy);
  r.gy = rc_dir(a.g10, a.g11, a.g12, dx, dy);
  r.gz = rc_dir(a.g20, a.g21, a.g22, dx, dy);
  const RayLoad2 load = {a.vox};
  float z = 0.0f;
  const bool hit = rc_march(load, r, a.t_min, a.step, a.n_steps, &z);
  if (!hit) z = 0.0f;
  const size_t pixel = (size_t)y * a.cols + x;   // (< 4096 * 4096)
  if (a.depth) a.depth[pixel] = z;
  if (a.raw) a.raw[pixel] = hit ? rc_raw(z, a.depth_scale) : (uint16_t)0;
  if (!a.nrmw && !a.rgba) return;
  float4 n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  uint32_t colour = 0u;
  RcCell cell;
  if constexpr (kInterp) {
    uint64_t cp[4];
    int calls = 0;
    const RayLoad2Colour both = {a.vox, a.col, cp, &calls};
    if (hit && rc_cell(both, r, z, &cell)) {   // the sample arithmetic once more, at t = z, with the corners' colour words
      if (rc_normal(cell, &n.x, &n.y, &n.z)) n.w = (float)cell.wmin;
      colour = rc_colour_interp(cell, cp);
    } else {
      // (a reader of the pairs on this side too: with one on the valid side only, the compiler moves the colour loads behind the
      // wait for the voxels and the test of their weights, and a hit waits for memory twice)
      asm volatile("" : : "v"(cp[0]), "v"(cp[1]), "v"(cp[2]), "v"(cp[3]));
    }
  } else {
    if (hit && rc_cell(load, r, z, &cell)) {   // the sample arithmetic once more, at t = z
      if (rc_normal(cell, &n.x, &n.y, &n.z)) n.w = (float)cell.wmin;
      if (a.rgba) {
        const uint32_t cw = a.col[rc_nearest(cell, r)];
        if (cw >> 24) colour = (cw & 0xffffffu) | 0xff000000u;
      }
    }
  }
  if (a.nrmw) a.nrmw[pixel] = n;
  if (a.rgba) a.rgba[pixel] = colour;
}

__global__ void __launch_bounds__(kRayBlock) volume_raycast_kernel(VolRaycastArgs a) { volume_raycast_body<false>(a); }
__global__ void __launch_bounds__(kRayBlock) volume_raycast_interp_kernel(VolRaycastArgs a) { volume_raycast_body<true>(a); }

void launch_volume_raycast(const VolRaycastArgs& a, bool interp, hipStream_t s) {
  const dim3 grid((unsigned)((a.cols + kRayTile - 1) / kRayTile), (unsigned)((a.rows + kRayTile - 1) / kRayTile));
  if (interp && a.rgba) hipLaunchKernelGGL(volume_raycast_interp_kernel, grid, dim3(kRayBlock), 0, s, a);
  else hipLaunchKernelGGL(volume_raycast_kernel, grid, dim3(kRayBlock), 0, s, a);
}

}  // namespace odo
