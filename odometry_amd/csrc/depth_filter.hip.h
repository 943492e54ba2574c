// depth_filter.hip.h — what the bilateral depth filter's kernel (depth_filter_kernels.hip, a translation unit of its own) and its host
// object (depth_filter_api.hip.h, in the main unit) share: the launch constants, the launch arguments and the launcher.
// include/odometry_hip.h, odo_depth_filter_create / DESIGN.md section 9.12; the rule is depth_filter_math.h's.
//
// One frame = one launch. A 256-thread workgroup owns a tile of kDfTileW x kDfTileH pixels: it stages the tile and its halo in LDS as
// packed uint16 (kDfPad columns left and right, R rows above and below; what lies outside the frame is zero there, and a zero is a
// tap that does not count, so the window loop has no bounds test), the range and shift tables beside it, and each thread then makes
// kDfPerThread horizontally adjacent outputs of one row: every window row is read from LDS once, as dwords, and serves all of them.
// The spatial weights arrive by value in the kernel arguments, a window row's in three dwords, which the (wave-uniform) row loop
// reads as scalars; within a row every index is a compile-time constant.
// The statistics are one row of kDfStatWords words per workgroup, written by one lane with one 16-byte vector store; the host sums the
// rows (odo_depth_filter_stats). No atomics, no floating point.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "depth_filter_math.h"

namespace odo {

constexpr int kDfBlock = 256;                         // threads per workgroup
constexpr int kDfPerThread = 4;                       // horizontally adjacent outputs of one thread
constexpr int kDfTileW = 64;                          // the tile: kDfTileW / kDfPerThread threads across ...
constexpr int kDfTileH = 16;                          // ... by kDfTileH rows
constexpr int kDfPad = 4;                             // halo columns staged left and right of the tile (>= kDfMaxRadius, a multiple of 4)
constexpr int kDfLdsStride = kDfTileW + 2 * kDfPad;   // uint16 per staged row: 72 = 36 dwords, a multiple of 8 bytes
constexpr int kDfStatWords = 4;                       // per workgroup: n_valid, n_changed, sum_abs_change, 0
constexpr int kDfRangeWords = 65;                     // the padded range table's 257 bytes, in whole dwords
constexpr int kDfWsRowWords = 3;                     // a window row's 2R + 1 <= 9 spatial weights, four to a word
static_assert(kDfBlock == (kDfTileW / kDfPerThread) * kDfTileH, "one thread per kDfPerThread outputs of the tile");
static_assert(4 * kDfRangeWords >= kDfRangePadded && kDfRangeWords + kDfRange / 4 <= kDfBlock, "a dword of the tables per thread");
static_assert(kDfPad >= kDfMaxRadius && kDfPad % 4 == 0 && kDfPerThread == 4, "the staged row is walked in groups of four pixels");
// sum_abs_change of one workgroup fits a word: at most kDfTileW * kDfTileH pixels, each moved by less than 256 << kDfShiftMax
static_assert((long long)kDfTileW * kDfTileH * ((256 << kDfShiftMax) - 1) < (1LL << 32), "a workgroup's sum fits uint32");

struct DfArgs {
  const uint16_t* in;     // rows x cols, dense; 0: no reading
  uint16_t* out;          // rows x cols
  const uint8_t* wr0;     // [4 * kDfRangeWords] on the device, 4-byte aligned: the padded range table (df_pad_range), then zeros
  const uint8_t* shift;   // [256] on the device, 4-byte aligned
  uint32_t* partials;     // [blocks][kDfStatWords], 16-byte aligned
  int rows, cols, radius;
  uint32_t ws[2 * kDfMaxRadius + 1][kDfWsRowWords];   // the spatial weights: window row dy, column dx in byte dx & 3 of word dx >> 2
};

inline int df_blocks_x(int cols) { return (cols + kDfTileW - 1) / kDfTileW; }
inline int df_blocks_y(int rows) { return (rows + kDfTileH - 1) / kDfTileH; }

void launch_depth_filter(const DfArgs& a, hipStream_t s);

}  // namespace odo
