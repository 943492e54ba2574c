// rgbd.hip.h — what the sensor-depth kernels (rgbd_kernels.hip, a translation unit of their own) and the RGB-D tracker (tracker.hip.h,
// in the main unit) share: the launch arguments and the launchers.
//
// An RGB-D frame's depth job replaces ComputeDepth of a stereo pair on the tracker's stream B. Its front end is the main unit's
// blur3x3_kernel (one image, zero-fills val / disp / dep) and depth_select_kernel (the point selection D2: the same fixed-slot list
// pts[block * 80 + k] = x | y << 16, cnt[block] as ComputeDepth's), then
//   depth    one thread per selection slot (512 x 80 = 40 960, 256-thread blocks): the slot's raw sensor value and its 4-neighbours,
//            the spec of include/odometry_hip.h (odo_tracker_create_rgbd), val / dep of the slot's pixel, per-block counts
//            {valid, selected, matched} in the [blocks][3] layout depth_finalize_kernel writes
//   stats    one block: the counts reduced into the host-mapped statistics (iters = 0, cost = 0, status -1 below 500 valid), then the
//            completion word — launched by the tracker AFTER the depth / candidate pyramids, so that the word covers them too
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace odo {

constexpr int kRgbdSelCap = 80;                                  // = kSelCap (ref: src/depth_estimate.cpp:334)
constexpr int kRgbdSlots = 512 * kRgbdSelCap;                    // = kSelBlocks * kSelCap
constexpr int kRgbdBlock = 256;                                  // = kDlmBlock
constexpr int kRgbdBlocks = kRgbdSlots / kRgbdBlock;             // 160 = kDlmBlocks
constexpr int kRgbdMinValid = 500;                               // ref: src/depth_estimate.cpp:192

// Layout of the depth estimator's statistics (DepthLmStats, kernels.hip.h; the main unit checks the two agree).
struct RgbdStats {
  int iters;
  float cost;
  int n_valid;
  int n_selected;
  int n_matched;
  int status;
};

struct RgbdDepthArgs {
  const uint16_t* raw;    // rows x cols, dense row-major; 0: no reading
  const uint32_t* pts;    // [kRgbdSlots] selection slots
  const int* cnt;         // [512] slots used per selection block
  int rows, cols;
  float depth_scale;      // raw units per metre
  float max_depth_step;   // edge guard: relative step to a 4-neighbour (INFINITY: off)
  float min_depth, max_depth;
  uint8_t* val;           // rows x cols, zero-filled by the front end
  float* dep;             // rows x cols, zero-filled by the front end
  int* counts;            // [kRgbdBlocks][3]: valid, selected, matched
};

void launch_rgbd_depth(const RgbdDepthArgs& a, hipStream_t s);
// counts: [kRgbdBlocks][3]; stats: host-mapped; done_flag: host-mapped word that receives `token` (release, system scope) last.
void launch_rgbd_stats(const int* counts, RgbdStats* stats, int* done_flag, int token, hipStream_t s);

}  // namespace odo
