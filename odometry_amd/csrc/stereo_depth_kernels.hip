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

// A census word of a plane, 0 outside the census domain (where the plane was never written).
__device__ __forceinline__ uint64_t sd_word(const uint64_t* plane, int rows, int cols, int y, int x) {
  uint64_t v = 0;
  if (x >= kSdCensusRx && x < cols - kSdCensusRx && y >= kSdCensusRy && y < rows - kSdCensusRy) v = plane[(size_t)y * cols + x];
  return v;
}

// ---- match. Right = false: the tile is of left pixels, the other image is the right one, candidate d of the pixel at tile column tx
// pairs own column tx + i with the other image's column x + i - d. Right = true: the tile is of right pixels, candidate d pairs own
// column tx + i with the LEFT image's column x + i + d (CR(x, y, d) = C(x + d, y, d)). In the other block, column 0 is the image
// column gx0 - A - dmax (Right: gx0 - A + dmin), so that the tap sits at tx + i + s with s = dmax - d (Right: d - dmin), 0 <= s <=
// dmax - dmin: inside the block for every admissible candidate, whatever the frame's size.
// Vec (Right = false only): cols % 4 == 0 and both output frames 8-byte aligned. Then four lanes' outputs leave as one 8-byte store.
template <int A, bool Right, bool Vec>
__global__ void __launch_bounds__(kSdBlock) stereo_match_kernel(SdArgs a) {
  constexpr int kN = 2 * A + 1;
  constexpr int kRows = kSdTileH + 2 * A;
  constexpr int kOwnStride = kSdTileW + 2 * A;
  constexpr int kOtherStride = kSdTileW + 2 * A + kSdMaxSpan;
  __shared__ __attribute__((aligned(16))) uint64_t s_own[kRows * kOwnStride];
  __shared__ __attribute__((aligned(16))) uint64_t s_other[kRows * kOtherStride];
  __shared__ uint32_t s_red[kSdBlock / 64][6];

  const int rows = a.rows, cols = a.cols, dmin = a.r.dmin, dmax = a.r.dmax;
  const int tid = (int)threadIdx.x;
  const int gx0 = (int)blockIdx.x * kSdTileW, gy0 = (int)blockIdx.y * kSdTileH;
  const uint64_t* own = Right ? a.cr : a.cl;
  const uint64_t* other = Right ? a.cl : a.cr;

  // ---- stage
  for (int i = tid; i < kRows * kOwnStride; i += kSdBlock) {
    const int r = i / kOwnStride, c = i - r * kOwnStride;
    s_own[i] = sd_word(own, rows, cols, gy0 - A + r, gx0 - A + c);
  }
  const int span = kSdTileW + 2 * A + dmax - dmin;            // columns of the other block in use
  const int ox0 = Right ? gx0 - A + dmin : gx0 - A - dmax;    // image column of its column 0
  for (int i = tid; i < kRows * span; i += kSdBlock) {
    const int r = i / span, c = i - r * span;
    s_other[r * kOtherStride + c] = sd_word(other, rows, cols, gy0 - A + r, ox0 + c);
  }
  __syncthreads();

  // ---- the walk
  const int tx = tid & (kSdTileW - 1), ty = tid / kSdTileW;
  const int x = gx0 + tx, y = gy0 + ty;
  uint64_t win[kN][kN];
#pragma unroll
  for (int j = 0; j < kN; j++)
#pragma unroll
    for (int i = 0; i < kN; i++) win[j][i] = s_own[(ty + j) * kOwnStride + tx + i];
  int last = dmin - 1;                                         // the largest admissible candidate; none: no trip
  if (sd_interior_row(y, rows, A)) {
    if (Right) { if (x >= A + kSdCensusRx) last = sd_right_last(x, cols, dmax, A); }
    else if (sd_interior_col(x, cols, A)) last = sd_left_last(x, dmax, A);
  }
  SdWalk w;
  sd_walk_init(&w);
  const uint64_t* base = s_other + ty * kOtherStride + tx;
#pragma unroll 1
  for (int d = dmin; d <= last; d++) {
    const uint64_t* p = base + (Right ? d - dmin : dmax - d);
    int c = 0;
#pragma unroll
    for (int j = 0; j < kN; j++)
#pragma unroll
      for (int i = 0; i < kN; i++) c += sd_hamming(win[j][i], p[j * kOtherStride + i]);
    sd_walk_step(&w, d, c);
  }

  if (Right) {
    if (x < cols && y < rows) a.dr[(size_t)y * cols + x] = w.c0 == kSdNone ? (uint8_t)kSdNoRight : (uint8_t)w.dl;
    return;
  }

  // ---- the left pixel's rejections, outputs and the workgroup's counters
  SdRule rule;
  rule.dmin = dmin; rule.dmax = dmax; rule.A = A; rule.uniq = a.r.uniq; rule.lr_max = a.r.lr_max; rule.max_raw = a.r.max_raw; rule.k = a.r.k;
  uint16_t depth, q;
  const int outcome = sd_finish(w, rule, a.dr + (size_t)(y < rows ? y : 0) * cols, x, &depth, &q);
  if (Vec) {
    uint32_t d01 = (uint32_t)depth, q01 = (uint32_t)q;
    d01 |= (uint32_t)__shfl_down(d01, 1) << 16;
    q01 |= (uint32_t)__shfl_down(q01, 1) << 16;
    const uint32_t d23 = (uint32_t)__shfl_down(d01, 2), q23 = (uint32_t)__shfl_down(q01, 2);
    if ((tx & 3) == 0 && x < cols && y < rows) {
      *reinterpret_cast<uint2*>(a.depth + (size_t)y * cols + x) = make_uint2(d01, d23);
      *reinterpret_cast<uint2*>(a.q + (size_t)y * cols + x) = make_uint2(q01, q23);
    }
  } else if (x < cols && y < rows) {
    a.depth[(size_t)y * cols + x] = depth;
    a.q[(size_t)y * cols + x] = q;
  }
  uint32_t n[6] = {(uint32_t)(outcome != kSdNotInterior), (uint32_t)(outcome == kSdMatched), (uint32_t)(outcome == kSdRejUnique),
                   (uint32_t)(outcome == kSdRejLr), (uint32_t)(outcome == kSdRejRange), (uint32_t)q};
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 6; k++) n[k] += __shfl_down(n[k], off);
  if (tx == 0)
#pragma unroll
    for (int k = 0; k < 6; k++) s_red[ty][k] = n[k];
  __syncthreads();
  if (tid == 0) {
    uint32_t r[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int v = 0; v < kSdBlock / 64; v++)
#pragma unroll
      for (int k = 0; k < 6; k++) r[k] += s_red[v][k];
    const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    uint4* row = reinterpret_cast<uint4*>(a.partials + kSdStatWords * b);
    row[0] = make_uint4(r[0], r[1], r[2], r[3]);
    row[1] = make_uint4(r[4], r[5], 0u, 0u);   // (a workgroup's sum of q fits its low word)
  }
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
