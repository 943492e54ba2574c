// volume_icp_photo.hip.h — what the kernels of the alignment with a photometric term (volume_icp_photo_kernels.hip, a translation
// unit of its own) and the host side (volume_icp_photo_api.hip.h, in the main unit) share: the state in device memory, the launch
// arguments and the launchers. The twin of volume_icp.hip.h, whose constants, grid and launch pattern it keeps: one launch writes the
// state, then per iteration of per level a pair of ordinary launches on the volume's own stream; both read the state first and
// return at once when the level is done or the alignment has failed. No atomics, nothing waits for another workgroup
// (include/odometry_hip.h / DESIGN.md section 9.10).
//
// The state is IcpState with 31 sums in place of 29, so it has an init kernel of its own.
#pragma once
#include "volume_icp.hip.h"
#include "volume_icp_photo_math.h"

namespace odo {

constexpr int kIcpPhotoRows = 2 * kIcpBlock;   // rows a block publishes in LDS: i < 256 geometric of thread i, i >= 256 photometric of thread i - 256

struct IcpPhotoState {
  float C[16];
  int status;
  int done[kIcpMaxLevels];
  int iterations;
  int trace_n;
  int evaluated;
  int pad_;
  double acc[kIcpPhotoAcc];
  float delta[6];
};

struct IcpPhotoTraceRow {      // odo_icp_photo_trace_row
  int level, iteration;
  double acc[kIcpPhotoAcc];
  float delta[6];
  float C[16];
};

struct VolIcpPhotoRowsArgs {
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
  float m0, m1, m2, m3, m4, m5, m6, m7, m8;
  int stride;
  int level;
  const IcpPhotoState* state;
  double* partials;            // [blocks][31], block = blockIdx.y * gridDim.x + blockIdx.x
  float* rows_dev;             // nullptr, or rows x cols x 16: every pixel of the frame is written
};

struct VolIcpPhotoStepArgs {
  const double* partials;
  int nblk;
  int level;
  int min_pairs;
  float eps_t, eps_r;
  int take_step;               // 0: fold only (odo_volume_icp_photo_eval_dev)
  IcpPhotoState* state;
  IcpPhotoTraceRow* trace;
  int trace_capacity;
};

void launch_volume_icp_photo_init(IcpPhotoState* state, const IcpInit& init, hipStream_t s);
void launch_volume_icp_photo_rows(const VolIcpPhotoRowsArgs& a, hipStream_t s);
void launch_volume_icp_photo_step(const VolIcpPhotoStepArgs& a, hipStream_t s);

}  // namespace odo
