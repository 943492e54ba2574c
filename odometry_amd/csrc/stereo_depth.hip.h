// stereo_depth.hip.h — what the dense stereo matcher's kernels (stereo_depth_kernels.hip, a translation unit of its own) and its host
// object (stereo_depth_api.hip.h, in the main unit) share: the launch constants, the launch arguments and the launchers.
// include/odometry_hip.h, odo_stereo_depth_create / DESIGN.md section 9.16; the rule is stereo_depth_math.h's.
//
// One pair = three launches on one stream. Every kernel gives a 256-thread workgroup a tile of kSdTileW x kSdTileH pixels, one pixel
// per thread, a wave per tile row.
//   stereo_census_kernel            blockIdx.z = image. The tile with its 4 / 3-pixel halo is staged in LDS as fp32; a thread makes its
//                                   pixel's 64-bit census word and stores it with one 8-byte store where the window lies in the frame.
//   stereo_match_kernel<A, true>    the right image's winners dr, a byte per pixel.
//   stereo_match_kernel<A, false>   the left image's winners, the rule's rejections, the depth and q frames, the counters.
// A match kernel stages two blocks of census words: its OWN image's tile with an A-pixel halo, which each thread then keeps as its
// (2A + 1)^2 window in registers for the whole walk, and the OTHER image's words that the tile's windows can reach over all
// candidates, kSdTileW + 2A + (dmax - dmin) columns by kSdTileH + 2A rows. Per candidate a thread reads the (2A + 1)^2 words of the
// other window out of LDS — a wave's lanes read consecutive words, so without bank conflicts — and adds the Hamming distances;
// the walk's state (sd_walk_step) is seven registers. Words outside the census domain are staged as 0 and never enter a cost.
// The counters are one row of kSdStatWords words per workgroup, written by one lane with two 16-byte vector stores; the host sums
// the rows (odo_stereo_depth_stats). No atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stereo_depth_math.h"

namespace odo {

constexpr int kSdBlock = 256;                         // threads per workgroup
constexpr int kSdTileW = 64;                          // the tile: a wave across ...
constexpr int kSdTileH = 4;                           // ... by kSdTileH rows
constexpr int kSdMaxSpan = 254;                       // dmax - dmin at the most (dmin >= 1, dmax <= 255)
constexpr int kSdCensusStride = 72;                   // floats per staged row of the census tile: kSdTileW + 2 * kSdCensusRx
static_assert(kSdBlock == kSdTileW * kSdTileH && kSdTileW == 64, "one pixel per thread, one wave per tile row");
static_assert(kSdCensusStride == kSdTileW + 2 * kSdCensusRx && kSdMaxSpan == kSdMaxDisp - 1, "the staged widths");
// Static LDS of the widest build (A = 3): the other image's block and the own tile, 8 bytes a word.
constexpr int kSdLdsWordsMax = (kSdTileH + 2 * kSdMaxAgg) * (2 * (kSdTileW + 2 * kSdMaxAgg) + kSdMaxSpan);
static_assert(8 * kSdLdsWordsMax + 256 <= 64 * 1024, "a match kernel's static LDS stays under 64 KiB");
// sum_q of one workgroup fits a word: at most 256 pixels of q <= 16 * 255 + 8
static_assert((long long)kSdBlock * (16 * kSdMaxDisp + 8) < (1LL << 32), "a workgroup's sum fits uint32");

struct SdArgs {
  const float* left;      // rows x cols fp32, dense, rectified
  const float* right;
  uint64_t* cl;           // rows x cols census words of the left image (written inside the census domain only)
  uint64_t* cr;
  uint8_t* dr;            // rows x cols: the right image's winners, kSdNoRight where there is no candidate
  uint16_t* depth;        // rows x cols
  uint16_t* q;            // rows x cols, 8-byte aligned
  uint32_t* partials;     // [blocks][kSdStatWords], 16-byte aligned
  int rows, cols;
  SdRule r;
};

inline int sd_blocks_x(int cols) { return (cols + kSdTileW - 1) / kSdTileW; }
inline int sd_blocks_y(int rows) { return (rows + kSdTileH - 1) / kSdTileH; }

// stage: 0 census (both images), 1 right winners, 2 left winners and outputs. Each is one launch on s.
void launch_stereo_depth_stage(const SdArgs& a, int stage, hipStream_t s);

// ---- what a kernel that walks a tile's candidates is made of: stereo_match_kernel, and the semi-global mode's sgm_cost_kernel and
// sgm_select_kernel (stereo_sgm_kernels.hip). The staging, the taps and the left pixel's outputs are written once, here.
template <int A>
struct SdTile {
  static constexpr int kN = 2 * A + 1;
  static constexpr int kRows = kSdTileH + 2 * A;
  static constexpr int kOwnStride = kSdTileW + 2 * A;
  static constexpr int kOtherStride = kSdTileW + 2 * A + kSdMaxSpan;
};

// A census word of a plane, 0 outside the census domain (where the plane was never written).
__device__ __forceinline__ uint64_t sd_word(const uint64_t* plane, int rows, int cols, int y, int x) {
  uint64_t v = 0;
  if (x >= kSdCensusRx && x < cols - kSdCensusRx && y >= kSdCensusRy && y < rows - kSdCensusRy) v = plane[(size_t)y * cols + x];
  return v;
}

// Stages the workgroup's OWN tile (kRows x kOwnStride words) and the OTHER image's block (kRows x kOtherStride) and waits for them.
// Right = false: the tile is of left pixels, the other image is the right one, candidate d of the pixel at tile column tx pairs own
// column tx + i with the other image's column x + i - d. Right = true: the tile is of right pixels, candidate d pairs own column
// tx + i with the LEFT image's column x + i + d (CR(x, y, d) = C(x + d, y, d)). In the other block, column 0 is the image column
// gx0 - A - dmax (Right: gx0 - A + dmin), so that the tap sits at tx + i + s with s = dmax - d (Right: d - dmin), 0 <= s <= dmax -
// dmin: inside the block for every admissible candidate, whatever the frame's size.
template <int A, bool Right>
__device__ __forceinline__ void sd_stage_tile(const SdArgs& a, uint64_t* s_own, uint64_t* s_other) {
  using T = SdTile<A>;
  const int rows = a.rows, cols = a.cols, dmin = a.r.dmin, dmax = a.r.dmax;
  const int tid = (int)threadIdx.x;
  const int gx0 = (int)blockIdx.x * kSdTileW, gy0 = (int)blockIdx.y * kSdTileH;
  const uint64_t* own = Right ? a.cr : a.cl;
  const uint64_t* other = Right ? a.cl : a.cr;
  for (int i = tid; i < T::kRows * T::kOwnStride; i += kSdBlock) {
    const int r = i / T::kOwnStride, c = i - r * T::kOwnStride;
    s_own[i] = sd_word(own, rows, cols, gy0 - A + r, gx0 - A + c);
  }
  const int span = kSdTileW + 2 * A + dmax - dmin;            // columns of the other block in use
  const int ox0 = Right ? gx0 - A + dmin : gx0 - A - dmax;    // image column of its column 0
  for (int i = tid; i < T::kRows * span; i += kSdBlock) {
    const int r = i / span, c = i - r * span;
    s_other[r * T::kOtherStride + c] = sd_word(other, rows, cols, gy0 - A + r, ox0 + c);
  }
  __syncthreads();
}

// The thread's own (2A + 1)^2 window out of the staged tile, kept in registers for the whole walk.
template <int A>
__device__ __forceinline__ void sd_window(const uint64_t* s_own, int tx, int ty, uint64_t (&win)[2 * A + 1][2 * A + 1]) {
  using T = SdTile<A>;
#pragma unroll
  for (int j = 0; j < T::kN; j++)
#pragma unroll
    for (int i = 0; i < T::kN; i++) win[j][i] = s_own[(ty + j) * T::kOwnStride + tx + i];
}

// The largest admissible candidate of the pixel (x, y); none: dmin - 1.
template <int A, bool Right>
__device__ __forceinline__ int sd_last(const SdArgs& a, int x, int y) {
  int last = a.r.dmin - 1;
  if (sd_interior_row(y, a.rows, A)) {
    if (Right) { if (x >= A + kSdCensusRx) last = sd_right_last(x, a.cols, a.r.dmax, A); }
    else if (sd_interior_col(x, a.cols, A)) last = sd_left_last(x, a.r.dmax, A);
  }
  return last;
}

// The cost of candidate d: base = s_other + ty * kOtherStride + tx.
template <int A, bool Right>
__device__ __forceinline__ int sd_tap_cost(const uint64_t (&win)[2 * A + 1][2 * A + 1], const uint64_t* base, int d, int dmin, int dmax) {
  using T = SdTile<A>;
  const uint64_t* p = base + (Right ? d - dmin : dmax - d);
  int c = 0;
#pragma unroll
  for (int j = 0; j < T::kN; j++)
#pragma unroll
    for (int i = 0; i < T::kN; i++) c += sd_hamming(win[j][i], p[j * T::kOtherStride + i]);
  return c;
}

// The end of a left pixel after its walk: the rule's rejections (sd_finish), the two output frames and the workgroup's row of
// counters. Every thread of the workgroup calls it (it holds a barrier). Vec: cols % 4 == 0 and both output frames 8-byte aligned;
// then four lanes' outputs leave as one 8-byte store.
template <bool Vec>
__device__ __forceinline__ void sd_left_outputs(const SdArgs& a, const SdWalk& w, int A, int x, int y, uint32_t (*s_red)[6]) {
  const int rows = a.rows, cols = a.cols;
  const int tid = (int)threadIdx.x, tx = tid & (kSdTileW - 1), ty = tid / kSdTileW;
  SdRule rule;
  rule.dmin = a.r.dmin; rule.dmax = a.r.dmax; rule.A = A; rule.uniq = a.r.uniq; rule.lr_max = a.r.lr_max; rule.max_raw = a.r.max_raw; rule.k = a.r.k;
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

}  // namespace odo
