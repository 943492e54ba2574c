// stereo_depth_kernels.hip — the dense stereo matcher's kernels (stereo_depth.hip.h) as a translation unit of its own, plus their
// host-side launcher. The census bit, the candidate walk, the rejections and the rounded division are stereo_depth_math.h's.
// include/odometry_hip.h, odo_stereo_depth_create; DESIGN.md section 9.16.
#include <hip/hip_runtime.h>
#include "stereo_depth.hip.h"

namespace odo {

// ---- census: blockIdx.z = 0 the left image, 1 the right. What lies outside the frame is staged as 0 and reaches only words that are
// not written.
__global__ void __launch_bounds__(kSdBlock) stereo_census_kernel(SdArgs a) {
  constexpr int kRows = kSdTileH + 2 * kSdCensusRy;
  __shared__ float tile[kRows * kSdCensusStride];
  const float* img = blockIdx.z ? a.right : a.left;
  uint64_t* out = blockIdx.z ? a.cr : a.cl;
  const int rows = a.rows, cols = a.cols;
  const int tid = (int)threadIdx.x;
  const int gx0 = (int)blockIdx.x * kSdTileW, gy0 = (int)blockIdx.y * kSdTileH;
  for (int i = tid; i < kRows * kSdCensusStride; i += kSdBlock) {
    const int r = i / kSdCensusStride, c = i - r * kSdCensusStride;
    const int gy = gy0 - kSdCensusRy + r, gx = gx0 - kSdCensusRx + c;
    float v = 0.0f;
    if (gy >= 0 && gy < rows && gx >= 0 && gx < cols) v = img[(size_t)gy * cols + gx];
    tile[i] = v;
  }
  __syncthreads();
  const int tx = tid & (kSdTileW - 1), ty = tid / kSdTileW;
  const int x = gx0 + tx, y = gy0 + ty;
  const uint64_t w = sd_census(tile + (ty + kSdCensusRy) * kSdCensusStride + tx + kSdCensusRx, kSdCensusStride);
  if (x >= kSdCensusRx && x < cols - kSdCensusRx && y >= kSdCensusRy && y < rows - kSdCensusRy) out[(size_t)y * cols + x] = w;
}

// ---- match: the staging, the taps and the left pixel's outputs are stereo_depth.hip.h's (sd_stage_tile, sd_tap_cost,
// sd_left_outputs). Right = false: the tile is of left pixels; Right = true: of right pixels, and the kernel ends with dr.
// Vec (Right = false only): cols % 4 == 0 and both output frames 8-byte aligned. Then four lanes' outputs leave as one 8-byte store.
template <int A, bool Right, bool Vec>
__global__ void __launch_bounds__(kSdBlock) stereo_match_kernel(SdArgs a) {
  using T = SdTile<A>;
  __shared__ __attribute__((aligned(16))) uint64_t s_own[T::kRows * T::kOwnStride];
  __shared__ __attribute__((aligned(16))) uint64_t s_other[T::kRows * T::kOtherStride];
  __shared__ uint32_t s_red[kSdBlock / 64][6];

  const int rows = a.rows, cols = a.cols, dmin = a.r.dmin, dmax = a.r.dmax;
  const int tid = (int)threadIdx.x;
  sd_stage_tile<A, Right>(a, s_own, s_other);

  // ---- the walk
  const int tx = tid & (kSdTileW - 1), ty = tid / kSdTileW;
  const int x = (int)blockIdx.x * kSdTileW + tx, y = (int)blockIdx.y * kSdTileH + ty;
  uint64_t win[T::kN][T::kN];
  sd_window<A>(s_own, tx, ty, win);
  const int last = sd_last<A, Right>(a, x, y);                 // the largest admissible candidate; none: no trip
  SdWalk w;
  sd_walk_init(&w);
  const uint64_t* base = s_other + ty * T::kOtherStride + tx;
#pragma unroll 1
  for (int d = dmin; d <= last; d++) sd_walk_step(&w, d, sd_tap_cost<A, Right>(win, base, d, dmin, dmax));

  if (Right) {
    if (x < cols && y < rows) a.dr[(size_t)y * cols + x] = w.c0 == kSdNone ? (uint8_t)kSdNoRight : (uint8_t)w.dl;
    return;
  }
  sd_left_outputs<Vec>(a, w, A, x, y, s_red);
}

template <int A>
static void launch_match(const SdArgs& a, int stage, const dim3& grid, hipStream_t s) {
  if (stage == 1) { hipLaunchKernelGGL((stereo_match_kernel<A, true, false>), grid, dim3(kSdBlock), 0, s, a); return; }
  const bool vec = (a.cols & 3) == 0 && (((uintptr_t)a.depth | (uintptr_t)a.q) & 7) == 0;
  if (vec) hipLaunchKernelGGL((stereo_match_kernel<A, false, true>), grid, dim3(kSdBlock), 0, s, a);
  else hipLaunchKernelGGL((stereo_match_kernel<A, false, false>), grid, dim3(kSdBlock), 0, s, a);
}

void launch_stereo_depth_stage(const SdArgs& a, int stage, hipStream_t s) {
  const dim3 grid((unsigned)sd_blocks_x(a.cols), (unsigned)sd_blocks_y(a.rows));
  if (stage == 0) {
    hipLaunchKernelGGL(stereo_census_kernel, dim3(grid.x, grid.y, 2), dim3(kSdBlock), 0, s, a);
    return;
  }
  switch (a.r.A) {
    case 0: launch_match<0>(a, stage, grid, s); break;
    case 1: launch_match<1>(a, stage, grid, s); break;
    case 2: launch_match<2>(a, stage, grid, s); break;
    default: launch_match<3>(a, stage, grid, s); break;
  }
}

}  // namespace odo
