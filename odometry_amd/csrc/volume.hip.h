// volume.hip.h — what the TSDF volume's kernels (volume_kernels.hip, a translation unit of their own) and its host object
// (volume_api.hip.h, in the main unit) share: the launch arguments, the device-resident counters and the launchers.
//
// The voxel word, the grid and every piece of voxel arithmetic are volume_math.h's (host + device); the kernels add the walk, the
// loads and the stores.
//
// One integration (odo_volume_integrate_dev) = two launches, no host synchronisation, no atomics:
//   integrate  a grid-stride launch of at most kVolMaxBlocks blocks over tiles of 64 (x) by 4 (y) voxels: a wave's voxels are 64
//              consecutive words. Projection of the voxel centre, depth pixel, tests, and only then the voxel's load and store. Each
//              block leaves its two counts (updated, in band) in a row of its own. The stride is added to the tile's three digits
//              (x tile, y tile, k): no division in the loop.
//   sum        one block adds the rows into the counters.
// A coloured integration (odo_volume_integrate_colour_dev) is the same two launches: volume_integrate_colour_kernel is the same body
// with the colour update compiled in. A lane in the band (|sdf| <= mu) also loads the colour pixel its depth reading came from (a
// 16-bit and a byte load, or one dword with 4 channels) and its colour word (the neighbour of its voxel word: as coalesced as the
// grid) in front of the voxel's load, and behind the voxel's store applies volume_colour_math.h and stores one dword.
// One extraction (odo_volume_extract) = three launches, the map's shape: count (three ballot words per wave: the +x, +y, +z edges
// that carry a point), scan (one block: exclusive offsets of the blocks, totals, the clamp at capacity), scatter (points and
// normals at block offset + rank in the block). Output order = (voxel in raster order, axis); nothing depends on timing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "volume_math.h"

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

struct VolIntegrateArgs {
  VolGrid g;
  const uint16_t* raw;   // rows x cols depth frame
  VolFrame f;
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

// The colour grid (volume_colour.hip.h) and the colour frame of a coloured integration.
struct VolColourFrame {
  uint32_t* col;          // [nx * ny * nz]: {R, G, B, wc}
  const uint8_t* pix;     // rows x cols x channels, dense
  int channels;           // 3 | 4
  int bgr;                // 0: R first, 1: B first
  int max_weight;         // 1 .. 255
};

struct VolIntegrateColourArgs {
  VolIntegrateArgs a;
  VolColourFrame c;
};

void launch_volume_integrate(const VolIntegrateArgs& a, hipStream_t s);                      // integrate, sum
void launch_volume_integrate_colour(const VolIntegrateColourArgs& a, hipStream_t s);         // likewise
void launch_volume_extract(const VolExtractArgs& a, hipStream_t s);

}  // namespace odo
