// volume_reentry.hip.h — what the re-entry store's kernels (volume_reentry_kernels.hip, a translation unit of their own) and the host
// object (volume_reentry_api.hip.h, in the main unit) share: the launch arguments, the store's counters and the launchers.
// include/odometry_hip.h, odo_volume_enable_reentry / DESIGN.md section 9.14; the rules are volume_shift_math.h's.
//
// The store keeps the VOXELS a shift pushes out of the window, keyed by their global index, and every shift puts back those whose
// index lies inside the new window. An entry is {gx, gy, gz, voxel word} (one 16-byte load or store) and, when the store has colours,
// a colour word in a second array. The store has two sets of buffers: a shift reads one and writes the other, and the host swaps the
// pointers when it enqueues, as the shift swaps its grids.
// One shift with a store = eight launches round the shift's own, all on the volume's stream, no host wait, no atomics:
//   in front of the shift  save count   a block per kVolExtBlock voxels of the PRE-shift grid in raster order: one ballot per wave of
//                                       "leaves and has a non-zero bit". A thread whose voxel stays loads nothing; a block without
//                                       a leaving voxel writes its zero count and returns.
//                          save scan    one block: the blocks' exclusive offsets and the sum (counters.pending).
//   behind the shift       store count  a thread per entry of the old store, the launch sized for the capacity: blocks beyond the live
//                                       count return after one uniform read. An entry inside the new window writes its words into
//                                       the shifted grid (entering voxels are 0 there: it overwrites zeros only, and no two entries
//                                       share a key); the others set their bit of the wave's ballot.
//                          store scan   one block over ceil(live / kVolExtBlock) counts: offsets and the sum (counters.kept).
//                          compact      the kept entries, in order, into the second set at block offset + rank.
//                          save scatter the saved voxels behind them at kept + block offset + rank; nothing at or beyond capacity.
//                          advance      one thread: live, saved, restored and dropped move on.
// The pre-shift grid is the grids' second buffer after the host's swap and stays intact until the next shift: the scatter reads it there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "volume.hip.h"

namespace odo {

// Device-resident counters of one re-entry store.
struct VolReentryCounters {
  unsigned long long live;       // entries in the store (<= capacity)
  unsigned long long saved;      // entries appended since enable / clear
  unsigned long long restored;   // entries put back into the grid since enable / clear: live = saved - restored
  unsigned long long dropped;    // leaving voxels that found the store full since enable / clear
  unsigned long long kept;       // of the shift enqueued last: the old entries that stay (store scan -> scatter, advance)
  unsigned long long pending;    // of the shift enqueued last: the voxels to save (save scan -> advance)
};

struct VolReentryArgs {
  const uint32_t* old_vox;   // [n]: the pre-shift grid
  const uint32_t* old_col;   // its colour grid, nullptr: the volume has no colour
  uint32_t* new_vox;         // [n]: the shifted grid
  uint32_t* new_col;         // nullptr: the volume or the store has no colour (restored voxels keep colour word 0)
  int nx, ny, nz, n;
  int nblk;                  // ceil(n / kVolExtBlock)
  int dx, dy, dz;
  int off_old[3], off_new[3];
  long long capacity;
  int store_nblk;            // ceil(capacity / kVolExtBlock)
  const uint4* src;          // [capacity]: the old store, {gx, gy, gz, word}
  const uint32_t* src_col;   // nullptr: the store has no colours
  uint4* dst;                // the second set
  uint32_t* dst_col;
  unsigned long long* save_mask;   // [nblk * kVolExtBlock / 64]: the save's ballot of every wave
  unsigned* save_cnt;              // [nblk]
  unsigned long long* save_off;    // [nblk]
  unsigned long long* keep_mask;   // [store_nblk * kVolExtBlock / 64]: "stays in the store" of every wave of entries
  unsigned* keep_cnt;              // [store_nblk]
  unsigned long long* keep_off;    // [store_nblk]
  VolReentryCounters* rc;
};

void launch_volume_reentry_save(const VolReentryArgs& a, hipStream_t s);    // save count, save scan: in front of the shift
void launch_volume_reentry_store(const VolReentryArgs& a, hipStream_t s);   // store count .. advance: behind the shift
// one of save count (0), save scan (1), save scatter (2), store count + scan + compact (3), advance (4): timing
void launch_volume_reentry_stage(const VolReentryArgs& a, int stage, hipStream_t s);

}  // namespace odo
