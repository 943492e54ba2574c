// rgbd_kernels.hip — the RGB-D tracker's sensor-depth kernels (rgbd.hip.h) as a translation unit of their own, plus their host-side
// launchers. Compiled with the library's flags: -ffp-contract=off and IEEE fp32 divides, so every operation below rounds once.
#include <hip/hip_runtime.h>
#include "rgbd.hip.h"

namespace odo {

// The edge guard of one 4-neighbour: a reading that differs from the centre's by more than max_depth_step * r (one fp32 rounding).
// Neighbours outside the image and holes pass.
__device__ __forceinline__ bool rgbd_step_ok(const uint16_t* __restrict__ raw, int x, int y, int rows, int cols, int r, float lim) {
  if (x < 0 || x >= cols || y < 0 || y >= rows) return true;
  const int q = raw[(size_t)y * cols + x];
  if (q == 0) return true;
  const int diff = q > r ? q - r : r - q;
  return !((float)diff > lim);
}

__global__ void __launch_bounds__(kRgbdBlock) rgbd_depth_kernel(RgbdDepthArgs a) {
  __shared__ int sh[kRgbdBlock / 64][3];
  const int t = threadIdx.x;
  const int s = blockIdx.x * kRgbdBlock + t;   // < kRgbdSlots: the grid is exactly kRgbdBlocks blocks
  const bool sel = (s % kRgbdSelCap) < a.cnt[s / kRgbdSelCap];
  bool matched = false, good = false;
  if (sel) {
    const uint32_t pk = a.pts[s];
    const int x = (int)(pk & 0xffffu), y = (int)(pk >> 16);
    const size_t o = (size_t)y * a.cols + x;
    const int r = a.raw[o];
    float d = 0.0f;
    matched = r != 0;
    if (matched) {
      d = a.depth_scale / (float)r;
      const float z = 1.0f / d;
      good = !(z > a.max_depth || z < a.min_depth);   // ref: src/depth_estimate.cpp:183, stated on d
      const float lim = a.max_depth_step * (float)r;
      good = good && rgbd_step_ok(a.raw, x - 1, y, a.rows, a.cols, r, lim) && rgbd_step_ok(a.raw, x + 1, y, a.rows, a.cols, r, lim) &&
             rgbd_step_ok(a.raw, x, y - 1, a.rows, a.cols, r, lim) && rgbd_step_ok(a.raw, x, y + 1, a.rows, a.cols, r, lim);
    }
    a.val[o] = good ? 1 : 0;
    a.dep[o] = good ? d : 0.0f;
  }
  const unsigned long long bv = __ballot(good), bs = __ballot(sel), bm = __ballot(matched);
  const int lane = t & 63, w = t >> 6;
  if (lane == 0) {
    sh[w][0] = __popcll(bv);
    sh[w][1] = __popcll(bs);
    sh[w][2] = __popcll(bm);
  }
  __syncthreads();
  if (t < 3) {
    int n = 0;
    for (int k = 0; k < kRgbdBlock / 64; k++) n += sh[k][t];
    a.counts[blockIdx.x * 3 + t] = n;
  }
}

__global__ void __launch_bounds__(kRgbdBlock) rgbd_stats_kernel(const int* __restrict__ counts, RgbdStats* __restrict__ stats,
                                                                 int* __restrict__ done_flag, int token) {
  __shared__ int sh[3][kRgbdBlock];
  const int t = threadIdx.x;
  for (int q = 0; q < 3; q++) sh[q][t] = (t < kRgbdBlocks) ? counts[t * 3 + q] : 0;
  __syncthreads();
  for (int o = kRgbdBlock / 2; o > 0; o >>= 1) {
    if (t < o) { sh[0][t] += sh[0][t + o]; sh[1][t] += sh[1][t + o]; sh[2][t] += sh[2][t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    stats->iters = 0;
    stats->cost = 0.0f;
    stats->n_valid = sh[0][0];
    stats->n_selected = sh[1][0];
    stats->n_matched = sh[2][0];
    stats->status = sh[0][0] < kRgbdMinValid ? -1 : 0;   // ref: src/depth_estimate.cpp:192-197
    __hip_atomic_store(done_flag, token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

void launch_rgbd_depth(const RgbdDepthArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(rgbd_depth_kernel, dim3(kRgbdBlocks), dim3(kRgbdBlock), 0, s, a);
}

void launch_rgbd_stats(const int* counts, RgbdStats* stats, int* done_flag, int token, hipStream_t s) {
  hipLaunchKernelGGL(rgbd_stats_kernel, dim3(1), dim3(kRgbdBlock), 0, s, counts, stats, done_flag, token);
}

}  // namespace odo
