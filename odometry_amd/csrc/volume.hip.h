// volume.hip.h — what the TSDF volume's kernels (volume_kernels.hip, a translation unit of their own) and its host object
// (volume_api.hip.h, in the main unit) share: the launch arguments, the device-resident counters and the launchers.
//
// A voxel is 4 bytes, {int16 q, uint16 w} = one 32-bit word (q in the low half): q = truncated signed distance * 32767, w = weight,
// 0 = never observed. Voxel (i, j, k) is word (k * ny + j) * nx + i.
//
// One integration (odo_volume_integrate_dev) = two launches, no host synchronisation, no atomics:
//   integrate  a grid-stride launch of at most kVolMaxBlocks blocks over tiles of 64 (x) by 4 (y) voxels: a wave's voxels are 64
//              consecutive words. Projection of the voxel centre, depth pixel, tests, and only then the voxel's load and store. Each
//              block leaves its two counts (updated, in band) in a row of its own. The stride is added to the tile's three digits
//              (x tile, y tile, k): no division in the loop.
//   sum        one block adds the rows into the counters.
// One extraction (odo_volume_extract) = three launches, the map's shape: count (three ballot words per wave: the +x, +y, +z edges
// that carry a point), scan (one block: exclusive offsets of the blocks, totals, the clamp at capacity), scatter (points and
// normals at block offset + rank in the block). Output order = (voxel in raster order, axis); nothing depends on timing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace odo {

constexpr int kVolBlock = 256;        // threads per block of the integration
constexpr int kVolExtBlock = 1024;    // threads (= voxels) per block of the extraction's count and scatter: fewer blocks to scan
constexpr int kVolTileX = 64;         // integrate: a tile is 64 voxels along x (one wave) ...
constexpr int kVolTileY = 4;          // ... by 4 along y (the block's four waves)
constexpr int kVolMaxBlocks = 2048;   // integrate: 8 blocks for each of 256 CUs
constexpr int kVolScanThreads = 1024;

// Device-resident counters of one volume.
struct VolCounters {
  unsigned long long updated, band;   // the last integration: voxels updated, and of those the ones with |sdf| <= mu
  unsigned long long cumulative;      // voxel updates since create / clear
  unsigned long long ext_total, ext_written;   // the last extraction: points found, points written (<= capacity)
};

struct VolGrid {
  uint32_t* vox;   // [nx * ny * nz]
  int nx, ny, nz;
  float vs, ox, oy, oz;
};

struct VolIntegrateArgs {
  VolGrid g;
  const uint16_t* raw;   // rows x cols depth frame
  int rows, cols;
  float f0, cx0, cy0;
  float depth_scale, max_depth, mu;
  int max_weight;
  float m0, m1, m2, m4, m5, m6, m8, m9, m10, m12, m13, m14;   // world-to-camera, column-major indices
  float zc_far;   // the kernel's early-out: 1.001 (max_depth + mu)
  int tiles_x, tiles_y;   // ceil(nx / 64), ceil(ny / 4)
  long long tiles;        // tiles_x * tiles_y * nz
  int nblk;               // blocks of the launch (<= kVolMaxBlocks)
  int step_x, step_y, step_k;   // nblk = (step_k * tiles_y + step_y) * tiles_x + step_x
  unsigned long long* blk;   // [2 * kVolMaxBlocks]: updated, in band per block
  VolCounters* ctr;
};

struct VolExtractArgs {
  VolGrid g;
  int n;       // nx * ny * nz
  int nblk;    // ceil(n / kVolExtBlock)
  long long capacity;
  unsigned long long* wave_mask;   // [3 * nblk * 16]: the +x, +y, +z ballots of every wave
  int* blk;                        // [nblk]: points per block
  unsigned long long* blk_off;     // [nblk]: exclusive offset of the block's points
  VolCounters* ctr;
  float4* xyz0;   // [capacity]
  float4* nrmw;   // [capacity]
};

void launch_volume_integrate(const VolIntegrateArgs& a, hipStream_t s);
void launch_volume_sum(const VolIntegrateArgs& a, hipStream_t s);   // the sum alone: behind the coloured integration (volume_colour.hip.h)
void launch_volume_extract(const VolExtractArgs& a, hipStream_t s);

}  // namespace odo
