// volume_reentry_kernels.hip — the re-entry store's kernels (volume_reentry.hip.h) as a translation unit of their own, plus their
// host-side launchers: the voxels a shift pushes out of the window are saved with their global index, and those whose index lies in
// the new window are put back. Integers only; the rules are volume_shift_math.h's, the ballots with their counts, the ranks and the
// scans of the counts volume_scan.hip.h's with one mask per wave. include/odometry_hip.h, odo_volume_enable_reentry; DESIGN.md
// section 9.14.
#include <hip/hip_runtime.h>
#include "volume_reentry.hip.h"
#include "volume_shift_math.h"
#include "volume_scan.hip.h"

namespace odo {

// Voxel v's index on the three axes. The save's blocks are runs of kVolExtBlock voxels in raster order, so that block order and rank
// give the store's order and the scan has as few blocks as the extraction's: the launch geometry does not hold (i, j, k).
__device__ __forceinline__ void reentry_ijk(const VolReentryArgs& a, int v, int* i, int* j, int* k) {
  const int row = v / a.nx;
  *i = v - row * a.nx;
  *k = row / a.ny;
  *j = row - *k * a.ny;
}

// ---- the save ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kVolExtBlock) volume_reentry_save_count_kernel(VolReentryArgs a) {
  const int v = blockIdx.x * kVolExtBlock + threadIdx.x;
  bool leaves = false;
  if (v < a.n) {
    int i, j, k;
    reentry_ijk(a, v, &i, &j, &k);
    leaves = shift_leaves(i, a.dx, a.nx) || shift_leaves(j, a.dy, a.ny) || shift_leaves(k, a.dz, a.nz);
  }
  if (!__syncthreads_or(leaves)) {   // no voxel of this block leaves: its zero count, nothing loaded
    if (threadIdx.x == 0) a.save_cnt[blockIdx.x] = 0u;
    return;
  }
  const bool save = leaves && reentry_saved(a.old_vox[v], a.old_col ? a.old_col[v] : 0u);
  const unsigned long long b[1] = {__ballot(save)};
  ballot_counts(b, a.save_mask, a.save_cnt);
}

__global__ void __launch_bounds__(kVolScanThreads) volume_reentry_save_scan_kernel(VolReentryArgs a) {
  const unsigned long long total = scan_counts<kVolScanThreads, 1>(a.save_cnt, a.save_off, a.nblk).t[0];
  if (threadIdx.x == 0) a.rc->pending = total;
}

// The saved voxels behind the kept entries: index = kept + block offset + rank; nothing at or beyond capacity is written.
__global__ void __launch_bounds__(kVolExtBlock) volume_reentry_save_scatter_kernel(VolReentryArgs a) {
  if (a.save_cnt[blockIdx.x] == 0u) return;   // (block-uniform; the count kernel left no masks for such a block)
  const int v = blockIdx.x * kVolExtBlock + threadIdx.x;
  unsigned long long m[1];
  ballot_wave(a.save_mask, m);
  if (!((m[0] >> (threadIdx.x & 63)) & 1ull)) return;   // (set for v < n only)
  const unsigned long long idx = a.rc->kept + a.save_off[blockIdx.x] + ballot_rank<1, unsigned>(a.save_mask, m);
  if (idx >= (unsigned long long)a.capacity) return;
  int i, j, k;
  reentry_ijk(a, v, &i, &j, &k);
  a.dst[idx] = make_uint4((uint32_t)(int)reentry_global(a.off_old[0], i), (uint32_t)(int)reentry_global(a.off_old[1], j),
                          (uint32_t)(int)reentry_global(a.off_old[2], k), a.old_vox[v]);
  if (a.dst_col) a.dst_col[idx] = a.old_col[v];   // (a store with colours: the volume has a colour grid)
}

// ---- the store pass ----------------------------------------------------------------------------------------------------------------
// A thread per old entry. Inside the new window: its words go back into the shifted grid. Outside: its bit of the ballot.
__global__ void __launch_bounds__(kVolExtBlock) volume_reentry_store_count_kernel(VolReentryArgs a) {
  const unsigned long long live = a.rc->live, e = (unsigned long long)blockIdx.x * kVolExtBlock + threadIdx.x;
  if ((unsigned long long)blockIdx.x * kVolExtBlock >= live) return;   // (block-uniform: the scan stops in front of this block)
  bool keep = false;
  if (e < live) {
    const uint4 en = a.src[e];
    const int g[3] = {(int)en.x, (int)en.y, (int)en.z};
    long long word;
    if (reentry_dest(g, a.off_new, a.nx, a.ny, a.nz, &word)) {
      a.new_vox[word] = en.w;
      if (a.new_col) a.new_col[word] = a.src_col[e];
    } else {
      keep = true;
    }
  }
  const unsigned long long b[1] = {__ballot(keep)};
  ballot_counts(b, a.keep_mask, a.keep_cnt);
}

__global__ void __launch_bounds__(kVolScanThreads) volume_reentry_store_scan_kernel(VolReentryArgs a) {
  const unsigned long long live = a.rc->live;
  const unsigned long long total = scan_counts<kVolScanThreads, 1>(a.keep_cnt, a.keep_off, (int)((live + kVolExtBlock - 1) / kVolExtBlock)).t[0];
  if (threadIdx.x == 0) a.rc->kept = total;
}

// The kept entries in their order into the second set: index = block offset + rank (< live <= capacity).
__global__ void __launch_bounds__(kVolExtBlock) volume_reentry_compact_kernel(VolReentryArgs a) {
  const unsigned long long live = a.rc->live, e = (unsigned long long)blockIdx.x * kVolExtBlock + threadIdx.x;
  if ((unsigned long long)blockIdx.x * kVolExtBlock >= live) return;   // (block-uniform)
  unsigned long long m[1];
  ballot_wave(a.keep_mask, m);
  if (!((m[0] >> (threadIdx.x & 63)) & 1ull)) return;   // (set for e < live only)
  const unsigned long long idx = a.keep_off[blockIdx.x] + ballot_rank<1, unsigned>(a.keep_mask, m);
  a.dst[idx] = a.src[e];
  if (a.dst_col) a.dst_col[idx] = a.src_col[e];
}

// One thread, behind the kernels that read the counters: they move on.
__global__ void volume_reentry_advance_kernel(VolReentryArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  // As volume_spill_advance_kernel ("the advance kernel's reads"): the counters are read through a volatile
  // pointer (vector loads, each waited for), and every store carries a value computed from those loads, so none can be issued
  // before its loads have returned. kept and pending stay: the next shift's scans write them before anything reads them.
  volatile VolReentryCounters* rc = a.rc;
  const unsigned long long live = rc->live, saved = rc->saved, restored = rc->restored, dropped = rc->dropped;
  const unsigned long long kept = rc->kept, pending = rc->pending;
  const unsigned long long cap = (unsigned long long)a.capacity, end = kept + pending;
  const unsigned long long now = end < cap ? end : cap;   // (kept <= live <= capacity: the kept entries always fit)
  rc->live = now;
  rc->saved = saved + (now - kept);
  rc->restored = restored + (live - kept);
  rc->dropped = dropped + (end - now);
}

void launch_volume_reentry_stage(const VolReentryArgs& a, int stage, hipStream_t s) {
  const dim3 grid(a.nblk), sgrid(a.store_nblk), block(kVolExtBlock);
  if (stage == 0) hipLaunchKernelGGL(volume_reentry_save_count_kernel, grid, block, 0, s, a);
  else if (stage == 1) hipLaunchKernelGGL(volume_reentry_save_scan_kernel, dim3(1), dim3(kVolScanThreads), 0, s, a);
  else if (stage == 2) hipLaunchKernelGGL(volume_reentry_save_scatter_kernel, grid, block, 0, s, a);
  else if (stage == 3) {
    hipLaunchKernelGGL(volume_reentry_store_count_kernel, sgrid, block, 0, s, a);
    hipLaunchKernelGGL(volume_reentry_store_scan_kernel, dim3(1), dim3(kVolScanThreads), 0, s, a);
    hipLaunchKernelGGL(volume_reentry_compact_kernel, sgrid, block, 0, s, a);
  } else hipLaunchKernelGGL(volume_reentry_advance_kernel, dim3(1), dim3(64), 0, s, a);
}

void launch_volume_reentry_save(const VolReentryArgs& a, hipStream_t s) {
  launch_volume_reentry_stage(a, 0, s);
  launch_volume_reentry_stage(a, 1, s);
}

void launch_volume_reentry_store(const VolReentryArgs& a, hipStream_t s) {
  launch_volume_reentry_stage(a, 3, s);
  launch_volume_reentry_stage(a, 2, s);
  launch_volume_reentry_stage(a, 4, s);
}

}  // namespace odo
