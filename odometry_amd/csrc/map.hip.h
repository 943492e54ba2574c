// map.hip.h — what the keyframe point-cloud map's kernels (map_kernels.hip, a translation unit of its own) and its host object
// (map_api.hip.h, in the main unit) share: the launch arguments, the device-resident counters and the launcher.
//
// One insertion (odo_map_insert_dev) = four launches, no host synchronisation:
//   claim    one thread per pixel: candidate test, world point, voxel key; claims the key's slot of an open-addressing hash
//            (64-bit CAS at agent scope: the XCDs do not share an L2) and folds (insertion << 32 | pixel) into the slot's payload
//            with a 64-bit atomicMin. Skipped when the voxel filter is off.
//   count    survivors = candidates whose slot payload is their own (every candidate when the filter is off): one ballot word per
//            wave, survivor / candidate / out-of-range counts per block
//   scan     one block: exclusive scan of the block counts, the append base (the device-resident size), the clamp at capacity,
//            the counters
//   scatter  survivors write {x, y, z, intensity} and {keyframe, pixel} at base + block offset + rank in the block
// The result does not depend on the atomics' timing: the payload a slot ends with is the minimum over its claimants, and the
// appended order is (insertion, pixel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace odo {

constexpr int kMapBlock = 256;       // threads (= pixels) per block of the per-pixel kernels
constexpr int kMapScanThreads = 1024;
constexpr unsigned long long kMapEmpty = ~0ull;   // an unclaimed slot's key and payload

// Device-resident counters of one map (odo_map_stats reads the first five).
struct MapCounters {
  unsigned long long size, candidates, dropped_voxel, dropped_range, dropped_capacity;
  unsigned long long base;   // the current insertion's append base (scan -> scatter)
};

struct MapInsertArgs {
  const uint8_t* val;   // NULL: every pixel passes the mask
  const float* dep;     // inverse depth
  const float* img;     // NULL: intensity 0
  int rows, cols, n;    // n = rows * cols
  int nblk;             // ceil(n / kMapBlock)
  float f0, cx0, cy0;
  float a0, a1, a2, a4, a5, a6, a8, a9, a10, a12, a13, a14;   // camera-to-world pose, column-major indices
  float voxel;          // 0: filter off
  unsigned ins;         // insertion index (the points' keyframe)
  long long capacity;
  unsigned long long slot_mask;   // slots - 1 (a power of two)
  unsigned long long* keys;       // [slots]
  unsigned long long* payload;    // [slots]
  int* pix_slot;                  // [n]: the pixel's slot, -1 not a candidate, -2 out of key range (filter on only)
  unsigned long long* wave_mask;  // [nblk * 4]: survivor ballot per wave
  int* blk;                       // [3 * nblk]: survivors, candidates, out of range per block
  int* blk_off;                   // [nblk]: exclusive offset of the block's survivors
  MapCounters* ctr;
  float4* xyzi;                   // [capacity]
  int2* kf_pixel;                 // [capacity]
};

void launch_map_insert(const MapInsertArgs& a, hipStream_t s);

}  // namespace odo
