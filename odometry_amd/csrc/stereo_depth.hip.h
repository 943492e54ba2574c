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

}  // namespace odo
