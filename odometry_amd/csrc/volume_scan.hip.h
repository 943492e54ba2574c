// volume_scan.hip.h — the block-wide exclusive scan of the TSDF volume's kernels (device only): volume_scan_kernel
// (volume_kernels.hip), volume_mesh_scan_kernel and the ranks of the mesh's vertices and triangles (volume_mesh_kernels.hip).
// Every thread of the block calls each step; wsum holds a word per wave and is free again after a barrier behind scan_rank.
#pragma once
#include <hip/hip_runtime.h>

namespace odo {

// Step 1: the sum of s over this lane and the lanes below it; lane 63 leaves the wave's sum in wsum.
__device__ __forceinline__ unsigned scan_wave(unsigned s, unsigned* wsum) {
  const int lane = threadIdx.x & 63;
  unsigned inc = s;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wsum[threadIdx.x >> 6] = inc;
  return inc;
}

struct ScanRank {
  unsigned rank;    // the sum of s over the threads below this one: the exclusive rank in thread order
  unsigned total;   // the block's sum
};

// Step 2, behind a barrier (inc = step 1's).
template <int Threads>
__device__ __forceinline__ ScanRank scan_rank(unsigned s, unsigned inc, const unsigned* wsum) {
  const int w = threadIdx.x >> 6;
  unsigned before = 0, total = 0;
  for (int q = 0; q < Threads / 64; q++) {
    if (q < w) before += wsum[q];
    total += wsum[q];
  }
  return {before + inc - s, total};
}

// Both steps for one value.
template <int Threads>
__device__ __forceinline__ ScanRank scan_block(unsigned s, unsigned* wsum) {
  const unsigned inc = scan_wave(s, wsum);
  __syncthreads();
  return scan_rank<Threads>(s, inc, wsum);
}

}  // namespace odo
