// speckle.hip.h — what the speckle filter's kernels (speckle_kernels.hip, a translation unit of its own) and its host object
// (speckle_api.hip.h, in the main unit) share: the launch constants, the launch arguments and the launcher.
// include/odometry_hip.h, odo_speckle_create / DESIGN.md section 9.17; the rule is speckle_math.h's.
//
// One run = four launches on one stream, a union-find whose every root is the smallest linear index of its component:
//   speckle_label_kernel   a 256-thread workgroup labels a tile of kSpTileW x kSpTileH keys, kSpPerThread pixels per thread, by a
//                          union-find in static LDS (int32 parents, LDS atomicMin). Each pixel's `parent` becomes the GLOBAL linear
//                          index of its tile-local root (kSpNoLabel where the key is 0); `size` becomes the tile-local component's
//                          pixel count at that root and 0 everywhere else.
//   speckle_seam_kernel    one thread per pixel pair across a horizontal or vertical tile seam: find both roots, atomicMin the larger
//                          root's parent to the smaller, go on from the returned value until the roots agree. Only tile-local roots
//                          are ever re-parented. Not launched for a frame of one tile.
//   speckle_count_kernel   every tile-local root (size > 0) that is not its component's root adds its count to the root's `size`
//                          (int32 atomicAdd) and is pointed at the root directly.
//   speckle_apply_kernel   a pixel's root is parent[parent[i]]: two loads, no walk. A pixel whose root's size is below min_size is
//                          zeroed in the targets; a workgroup reduces its counters and one lane writes its row of kSpStatWords words
//                          with two 16-byte vector stores. The host folds the rows in block order (odo_speckle_stats).
// Every loop whose trip count depends on data walks strictly downhill (parent[i] <= i; the larger root of a union strictly decreases)
// and carries a hard trip bound besides; hitting it ORs a bit of kSpGuard* into the guard word and leaves the loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "speckle_math.h"

namespace odo {

constexpr int kSpBlock = 256;                         // threads per workgroup
constexpr int kSpTileW = 64;                          // the tile: a wave across ...
constexpr int kSpTileH = 16;                          // ... by kSpTileH rows
constexpr int kSpPerThread = 4;                       // pixels per thread: tile rows ty, ty + 4, ty + 8, ty + 12
constexpr int kSpTile = 1024;                         // pixels per tile
constexpr int kSpStages = 4;                          // launches per run
static_assert(kSpTile == kSpTileW * kSpTileH && kSpTile == kSpBlock * kSpPerThread && kSpTileW == 64, "a wave per tile row");
// the guard word's bits: which bounded loop ran into its bound (never, unless the code is wrong)
constexpr int kSpGuardTileFind = 1;
constexpr int kSpGuardTileUnion = 2;
constexpr int kSpGuardSeamFind = 4;
constexpr int kSpGuardSeamUnion = 8;
constexpr int kSpGuardCountFind = 16;

struct SpArgs {
  const uint16_t* key;    // rows x cols, dense; may be one of the targets
  uint16_t* a;            // target, rows x cols
  uint16_t* b;            // second target or NULL
  int32_t* parent;        // rows x cols
  int32_t* size;          // rows x cols
  uint32_t* partials;     // [blocks][kSpStatWords], 16-byte aligned; one more row behind them whose first word is the guard
  uint32_t* guard;
  int rows, cols, max_diff, min_size;
};

inline int sp_blocks_x(int cols) { return (cols + kSpTileW - 1) / kSpTileW; }
inline int sp_blocks_y(int rows) { return (rows + kSpTileH - 1) / kSpTileH; }
// pixel pairs across the horizontal seams, then across the vertical ones: the threads of speckle_seam_kernel
inline long long sp_seam_pairs(int rows, int cols) {
  return (long long)(sp_blocks_y(rows) - 1) * cols + (long long)(sp_blocks_x(cols) - 1) * rows;
}

// stage: 0 label, 1 seams, 2 count, 3 apply. Each is one launch on s (stage 1 none for a frame of one tile).
void launch_speckle_stage(const SpArgs& a, int stage, hipStream_t s);

}  // namespace odo
