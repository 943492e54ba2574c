// stereo_sgm.hip.h — what the semi-global mode's kernels (stereo_sgm_kernels.hip, a translation unit of its own) and the matcher's
// host object (stereo_depth_api.hip.h, in the main unit) share: the launch constants, the launch arguments and the launchers.
// include/odometry_hip.h, odo_stereo_depth_enable_sgm / DESIGN.md section 9.18; the rule is stereo_sgm_math.h's.
//
// One pair = census (the matcher's own launch), then on the same stream
//   sgm_cost_kernel<A>          the match kernel's tile, staging and taps (stereo_depth.hip.h); instead of walking, a thread makes
//                               its pixel's costs kSgmCostChunk candidates at a time into LDS, from where the wave stores them
//                               with consecutive candidates in consecutive lanes: C[y][x][d - dmin] as uint16, kSgmNone where d is
//                               not admissible — and kSgmNone into the same entries of S, which the path launches never touch.
//   sgm_path_kernel<dx, dy>     one launch per direction, one wave per line (sgm_line), kSgmLinesPerBlock lines a workgroup. A lane
//                               holds the candidates dmin + lane + 64 j, j < kSgmSlots; a step loads the pixel's costs coalesced along
//                               d (kSgmAhead pixels before they are used, and S with them), takes L_r(q, d -+ 1) from the
//                               neighbouring lane (across a slot seam: from the other end of the neighbouring slot) and M by a wave
//                               reduction. The walk along a line is one wave's serial chain: no barrier, no atomics, no spin, and the
//                               trip count is the line's length. The first direction stores S, the later ones read, add and store.
//   sgm_select_kernel<Right>    the match kernel's tile again, one pixel per thread. S is staged through LDS in chunks of kSgmChunk
//                               candidates, a wave per tile row: every global load is 64 consecutive candidates of one pixel. Right:
//                               the staged entry of thread t, chunk candidate i is S(x' + d, y, d), the diagonal. The walk and the
//                               end of a pixel are sd_walk_step / sd_finish / sd_left_outputs, as in the match kernel; the counters
//                               go to the same rows of `partials`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stereo_depth.hip.h"
#include "stereo_sgm_math.h"

namespace odo {

constexpr int kSgmBlock = 256;                        // threads per workgroup of a path launch
constexpr int kSgmLinesPerBlock = 4;                  // a wave per line
constexpr int kSgmSlots = 4;                          // candidates per lane: 64 * kSgmSlots covers D <= 255
constexpr int kSgmAhead = 6;                          // steps a line's loads run ahead of their use
constexpr int kSgmCostChunk = 32;                     // candidates a thread of the cost launch makes between two stores of the tile
constexpr int kSgmCostStride = 33;                    // uint16 per pixel of that block
constexpr int kSgmChunk = 64;                         // candidates staged at a time by the selection
constexpr int kSgmChunkStride = 65;                   // uint16 per staged pixel: odd, so a wave's reads spread over the banks
static_assert(kSgmBlock == 64 * kSgmLinesPerBlock && 64 * kSgmSlots >= kSdMaxDisp, "a wave per line, a lane per candidate and slot");
static_assert(kSdTileW % kSgmCostChunk == 0 && kSgmCostStride == kSgmCostChunk + 1, "whole pixels per store of the cost launch");
static_assert(8 * kSdLdsWordsMax + 2 * kSdTileH * kSdTileW * kSgmCostStride <= 64 * 1024, "the cost kernel's static LDS stays under 64 KiB");
static_assert(kSgmChunk == kSdTileW && kSgmChunkStride == kSgmChunk + 1, "the selection stages a wave's width of candidates");

struct SgmArgs {
  SdArgs sd;              // the matcher's own arguments: planes, dr, outputs, counters, the rule
  uint16_t* C;            // [rows][cols][D]
  uint16_t* S;            // [rows][cols][D]
  int p1, p2, paths;
};

void launch_sgm_cost(const SgmArgs& g, hipStream_t s);            // one launch
void launch_sgm_paths(const SgmArgs& g, hipStream_t s);           // `paths` launches; none when there is no active pixel
void launch_sgm_select(const SgmArgs& g, bool right, hipStream_t s);

}  // namespace odo
