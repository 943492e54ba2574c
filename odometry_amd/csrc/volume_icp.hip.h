// volume_icp.hip.h — what the kernels of the TSDF volume's frame-to-model alignment (volume_icp_kernels.hip, a translation unit of
// its own) and the host side (volume_icp_api.hip.h, in the main unit) share: the state in device memory, the launch arguments and
// the launchers. Everything is written once over the number of sums N: ODO_NACC = 29 for the geometric rows alone (DESIGN.md
// section 9.8), kIcpPhotoAcc = 31 with the photometric rows beside them (section 9.10).
//
// One alignment (odo_volume_icp_align_dev, odo_volume_icp_photo_align_dev) = one launch that writes the state, then per iteration of
// per level a pair of ordinary launches on the volume's own stream: volume_icp_rows_kernel sums the rows of one stride into one
// N-double partial per block, volume_icp_step_kernel (one block) folds the partials in block order and takes the step. Both read
// the state first and return at once when the level is done or the alignment has failed, so the host enqueues every pair and waits
// once, at the end. No atomics, nothing waits for another workgroup: every sum is a pure function of the inputs and the constants
// below (include/odometry_hip.h).
//
// A block of the rows kernel is kIcpTile x kIcpTile pixels of the stride's lattice: thread t has lattice point (t % kIcpTile,
// t / kIcpTile) of the block's tile, a wave kIcpTile x (64 / kIcpTile) of them, and pixel = stride * lattice point.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "odo_math.h"
#include "volume_icp_photo_math.h"

namespace odo {

constexpr int kIcpBlock = 256;    // threads per block of either kernel
constexpr int kIcpTile = 16;      // a block is 16 x 16 lattice points
constexpr int kIcpRow = 9;        // floats per row in LDS: {J0 .. J5, res, w, pair? 1 : 0}; odd, so that eight rows apart is no bank conflict
constexpr int kIcpFoldLanes = 8;  // lanes that share one of the sums, in the block's reduction and in the fold of the partials
constexpr int kIcpMaxLevels = 3;
constexpr int kIcpPhotoRows = 2 * kIcpBlock;   // rows a block publishes in LDS with the photometric term: i < 256 geometric of thread i, i >= 256 photometric of thread i - 256

template <int N>
struct IcpStateT {
  float C[16];                 // sensor camera -> model camera, column-major: the estimate
  int status;                  // 0 running / aligned, 1 too few pairs or a sum that is not finite
  int done[kIcpMaxLevels];     // 1: the level has converged
  int iterations;              // steps taken
  int trace_n;                 // trace rows written
  int evaluated;               // 1: acc below holds an evaluation
  int pad_;
  double acc[N];               // the folded sums of the last evaluation
  float delta[6];              // the last step
};
using IcpState = IcpStateT<ODO_NACC>;
using IcpPhotoState = IcpStateT<kIcpPhotoAcc>;

template <int N>
struct IcpTraceRowT {          // odo_icp_trace_row, odo_icp_photo_trace_row
  int level, iteration;
  double acc[N];
  float delta[6];
  float C[16];
};
using IcpTraceRow = IcpTraceRowT<ODO_NACC>;
using IcpPhotoTraceRow = IcpTraceRowT<kIcpPhotoAcc>;

struct IcpInit {               // volume_icp_init_kernel: the state's first value
  float C[16];
};

template <int N>
struct VolIcpRowsArgs {        // N = kIcpPhotoAcc; the geometric rows' arguments are the specialisation below
  const uint16_t* raw;         // the sensor frame, rows x cols
  const float* grey;           // and its grey values, rows x cols
  const float* depth_m;        // the model frame's depth, rows x cols
  const float* nrmw_m;         // its world normals, rows x cols x 4
  const uint32_t* rgba_m;      // and its colours, rows x cols words (R, G, B, A in memory order)
  int rows, cols;
  float f, cx, cy;
  float depth_scale, max_depth;
  float dist_max, huber_delta;
  float photo_weight, photo_huber;
  float m0, m1, m2, m3, m4, m5, m6, m7, m8;   // rotation of the model camera's world-to-camera transform, row-major
  int stride;
  int level;                   // whose done flag is read
  const IcpStateT<N>* state;
  double* partials;            // [blocks][N], block = blockIdx.y * gridDim.x + blockIdx.x
  float* rows_dev;             // nullptr, or rows x cols x 16: every pixel of the frame is written
};

// The same without the two frames and the two floats of the photometric term. One struct with those left null was measured: the
// geometric rows kernel sits on the launch floor, and the longer argument block cost it 0.06 - 0.10 us of 6.3 - 8.4 (DESIGN.md
// section 9.10.1). With this layout the kernel's executed path is the parent's instruction for instruction.
template <>
struct VolIcpRowsArgs<ODO_NACC> {
  const uint16_t* raw;
  const float* depth_m;
  const float* nrmw_m;
  int rows, cols;
  float f, cx, cy;
  float depth_scale, max_depth;
  float dist_max, huber_delta;
  float m0, m1, m2, m3, m4, m5, m6, m7, m8;
  int stride;
  int level;
  const IcpStateT<ODO_NACC>* state;
  double* partials;            // [blocks][29]
  float* rows_dev;             // nullptr, or rows x cols x 8
};

template <int N>
struct VolIcpStepArgs {
  const double* partials;
  int nblk;
  int level;
  int min_pairs;
  float eps_t, eps_r;
  int take_step;               // 0: fold only (odo_volume_icp_eval_dev, odo_volume_icp_photo_eval_dev)
  IcpStateT<N>* state;
  IcpTraceRowT<N>* trace;      // nullptr, or room for trace_capacity rows
  int trace_capacity;
};

inline dim3 volume_icp_grid(int rows, int cols, int stride) {
  const int lx = (cols + stride - 1) / stride, ly = (rows + stride - 1) / stride;
  return dim3((unsigned)((lx + kIcpTile - 1) / kIcpTile), (unsigned)((ly + kIcpTile - 1) / kIcpTile));
}

// Instantiated in volume_icp_kernels.hip for N = ODO_NACC and N = kIcpPhotoAcc.
template <int N> void launch_volume_icp_init(IcpStateT<N>* state, const IcpInit& init, hipStream_t s);
template <int N> void launch_volume_icp_rows(const VolIcpRowsArgs<N>& a, hipStream_t s);
template <int N> void launch_volume_icp_step(const VolIcpStepArgs<N>& a, hipStream_t s);

}  // namespace odo
