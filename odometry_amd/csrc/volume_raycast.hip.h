// volume_raycast.hip.h — what the TSDF volume's ray-cast kernel (volume_raycast_kernels.hip, a translation unit of its own) and the
// host object (volume_api.hip.h, in the main unit) share: the launch arguments and the launcher.
//
// One ray-cast (odo_volume_raycast_dev) = one launch on the volume's own stream, a thread per pixel of the output frame, no atomics,
// nothing combined across threads: the result is a pure function of the grid, the pose and the parameters (include/odometry_hip.h /
// DESIGN.md section 9.7). A block is 16 x 16 pixels, each of its four waves a square of 8 x 8, so that the rays of a wave walk
// neighbouring cells.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace odo {

constexpr int kRayBlock = 256;   // threads per block: 2 x 2 waves
constexpr int kRayWave = 8;      // a wave is 8 x 8 pixels
constexpr int kRayTile = 16;     // a block is 16 x 16 pixels

struct VolRaycastArgs {
  const uint32_t* vox;     // [nx * ny * nz]
  const uint32_t* col;     // the colour grid; read only when rgba is set
  int nx, ny, nz;
  int rows, cols;          // of the output frame
  float f, cx, cy;
  float t_min, step;
  int n_steps;
  float depth_scale;       // the volume's: raw units per metre
  float ex, ey, ez;        // the camera centre in voxel-index coordinates
  float g00, g01, g02, g10, g11, g12, g20, g21, g22;   // G = R / vs, row r column c
  float* depth;            // rows x cols, nullptr: not written
  uint16_t* raw;           // likewise
  float4* nrmw;            // likewise
  uint32_t* rgba;          // likewise
};

// interp: the colour frame is the trilinear average of the cell's coloured corners (volume_raycast_interp_kernel, DESIGN.md section
// 9.11) instead of the nearest voxel's colour. Without a colour frame the two kernels write the same frames, and the first is launched.
void launch_volume_raycast(const VolRaycastArgs& a, bool interp, hipStream_t s);

}  // namespace odo
