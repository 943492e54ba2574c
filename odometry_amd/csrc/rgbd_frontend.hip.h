// rgbd_frontend.hip.h — what the RGB-D front end's kernels (rgbd_frontend_kernels.hip, a translation unit of their own) and its host
// object (rgbd_frontend_api.hip.h, in the main unit) share: the launch arguments and the launcher.
//
// One raw sensor frame (interleaved 8-bit colour + uint16 depth in the depth imager's grid) becomes the two inputs of the RGB-D
// tracker (fp32 grey + uint16 depth in the grey camera's grid) in three launches on the front end's stream, no host synchronisation:
//   grey     one thread per four pixels of the flat colour frame: the bytes read as whole dwords, grey = (R 4899 + G 9617 + B 1868
//            + 8192) >> 14 written as one float4, and the four z-buffer words set to 0xFFFFFFFF as one uint4; the last (< 4) pixels of
//            a frame whose size is not a multiple of four go pixel by pixel. Zeroes the resolve kernel's ticket.
//   register one thread per depth pixel and grid stride: the spec of include/odometry_hip.h (odo_rgbd_frontend_create): back-projection
//            of the pixel's two footprint corners and its centre, the extrinsic, projection into the target frame, and an atomic minimum
//            of the quantised depth on every target pixel whose centre lies in the footprint (at most 4 x 4). Counters: one ballot and
//            popcount per wave and counter, summed over the block's pixels, one row of plain stores per block.
//   resolve  one thread per four target pixels and grid stride: z-buffer -> uint16 depth (0xFFFFFFFF -> 0), filled pixels counted by
//            ballot, one atomic per block; the block that finishes last sums the register kernel's rows, writes the statistics into
//            host-mapped memory, then the slot's completion word.
// The result does not depend on the atomics' timing: the only combining operation is a minimum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace odo {

constexpr int kFeBlock = 256;            // threads per block of the three kernels
constexpr int kFeMaxSplat = 4;           // a footprint wider or taller than this many target pixels is dropped
constexpr uint32_t kFeEmpty = 0xFFFFFFFFu;   // a z-buffer word nothing was written to
// register and resolve walk their pixels with a grid stride, so that what a block contributes to the frame's counters is ONE row of
// plain stores (register) or ONE atomic (resolve): an atomic add per wave on one word costs 11-13 ns each once a few thousand waves
// arrive (measured: 4 800 waves, 56 us for a kernel whose z-buffer work takes a fraction of that)
constexpr int kFeRegBlocksMax = 512;
constexpr int kFeResBlocksMax = 128;

// Device-resident counters of the frame in flight (one set per front end: its launches are ordered by its stream).
struct FeCounters {
  unsigned long long fill_ticket;          // resolve: blocks done << 32 | target pixels filled so far
  unsigned reg[kFeRegBlocksMax][4];        // register, per block: n_depth, dropped_behind, dropped_range, dropped_splat
};

struct FeArgs {
  const uint8_t* colour;   // rows x cols x channels, dense; 4-byte aligned
  const uint16_t* depth;   // depth_rows x depth_cols, dense; 0: no reading
  int rows, cols, channels, bgr;
  int depth_rows, depth_cols;
  float fxd, fyd, cxd, cyd, scale_in;
  float f, cx, cy, scale_out;
  float e[12];             // colour_from_depth, row-major 3 x 4
  float* gray;             // rows x cols
  uint32_t* zbuf;          // rows x cols
  uint16_t* out;           // rows x cols
  FeCounters* ctr;
  long long* stats;        // host-mapped [6]: n_depth, n_filled, dropped_behind, dropped_range, dropped_splat, frame number
  int* done_flag;          // host-mapped: receives `token` (release, system scope) last
  int token;
  long long frame;
};

void launch_rgbd_frontend(const FeArgs& a, hipStream_t s);

}  // namespace odo
