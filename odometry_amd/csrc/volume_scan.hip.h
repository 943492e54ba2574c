// volume_scan.hip.h — the compaction passes of the TSDF volume's kernels, written once (device only): the block-wide exclusive scan
// (the ranks of the mesh's vertices and triangles), the one-block scan of per-block counts (the five scan kernels of
// volume_kernels.hip, volume_mesh_kernels.hip, volume_shift_kernels.hip and volume_reentry_kernels.hip), the ballots of a block with
// its count and a thread's rank among them (the extraction, the point spill, the re-entry store), a voxel's edge points from an index
// on (the extraction's and the point spill's scatter), and the block's sums of two counts (the two mesh counts).
// Every thread of the block calls each of the block-wide functions; wsum holds a word per wave and is free again after a barrier
// behind scan_rank.
#pragma once
#include <hip/hip_runtime.h>
#include "volume.hip.h"
#include "volume_colour_math.h"

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

template <int N>
struct ScanTotals {
  unsigned long long t[N];
};

// One block of Threads: the exclusive scans of N interleaved streams of per-block counts, cnt[N * b + x] -> off[N * b + x] for
// b < nb, Threads blocks at a time (coalesced loads and stores, a running base); the N sums are returned to every thread. A chunk's
// sum stays far below 2^32: a block counts at most 3 072 points, 7 168 vertices, 12 288 triangles or 1 024 entries.
template <int Threads, int N, class Count>
__device__ __forceinline__ ScanTotals<N> scan_counts(const Count* cnt, unsigned long long* off, int nb) {
  __shared__ unsigned wsum[N][Threads / 64];
  const int t = threadIdx.x;
  ScanTotals<N> base = {};
  for (int c0 = 0; c0 < nb; c0 += Threads) {
    const int b = c0 + t;
    unsigned s[N], inc[N];
#pragma unroll
    for (int x = 0; x < N; x++) {
      s[x] = b < nb ? (unsigned)cnt[N * b + x] : 0u;
      inc[x] = scan_wave(s[x], wsum[x]);
    }
    __syncthreads();
#pragma unroll
    for (int x = 0; x < N; x++) {
      const ScanRank r = scan_rank<Threads>(s[x], inc[x], wsum[x]);
      if (b < nb) off[N * b + x] = base.t[x] + (unsigned long long)r.rank;
      base.t[x] += r.total;
    }
    __syncthreads();   // wsum is written again
  }
  return base;
}

// ---- ballots: blocks of kVolExtBlock threads, M mask words per wave ------------------------------------------------------------------
constexpr int kBallotWaves = kVolExtBlock / 64;

// A block's ballots and their count: b[0 .. M) = this wave's __ballot of each of M predicates (taken by the kernel, where the
// predicates are computed) into mask[(block * waves + wave) * M + m], the block's count of set bits into cnt[block].
template <int M, class Count>
__device__ __forceinline__ void ballot_counts(const unsigned long long (&b)[M], unsigned long long* mask, Count* cnt) {
  __shared__ Count sh[kBallotWaves];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* wm = mask + M * ((size_t)blockIdx.x * kBallotWaves + w);
    Count n = 0;
#pragma unroll
    for (int m = 0; m < M; m++) {
      wm[m] = b[m];
      n += (Count)__popcll(b[m]);
    }
    sh[w] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Count t = 0;
    for (int q = 0; q < kBallotWaves; q++) t += sh[q];
    cnt[blockIdx.x] = t;
  }
}

// The M mask words of this thread's wave.
template <int M>
__device__ __forceinline__ void ballot_wave(const unsigned long long* mask, unsigned long long (&own)[M]) {
  const unsigned long long* wm = mask + M * (size_t)blockIdx.x * kBallotWaves;
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < M; m++) own[m] = wm[M * w + m];
}

// The rank of this thread's first set bit among the set bits of its block's masks, in (thread, m) order: the bits of the waves
// before + the bits of the lanes before in own, ballot_wave's words.
template <int M, class Count>
__device__ __forceinline__ Count ballot_rank(const unsigned long long* mask, const unsigned long long (&own)[M]) {
  const unsigned long long* wm = mask + M * (size_t)blockIdx.x * kBallotWaves;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  Count pre = 0;
  for (int q = 0; q < M * w; q++) pre += (Count)__popcll(wm[q]);
  const unsigned long long bit = 1ull << lane, below = bit - 1ull;
#pragma unroll
  for (int m = 0; m < M; m++) pre += (Count)__popcll(own[m] & below);
  return pre;
}

// The edge points of voxel v from index idx on: of its +x, +y, +z edges those whose mask (the wave's three ballots) has the lane's
// bit; position, normal and weight, and with col the colour of volume_colour_math.h at the edge's alpha. Nothing at or beyond cap.
__device__ __forceinline__ void extract_points(const VolGrid& g, int v, const unsigned long long (&edges)[3], unsigned long long bit,
                                               unsigned long long idx, unsigned long long cap, float4* xyz0, float4* nrmw,
                                               const uint32_t* col, uint32_t* rgba) {
  if (idx >= cap) return;   // (so are this voxel's later edges)
  int i, j, k;
  vox_ijk(g, v, &i, &j, &k);
  const uint32_t va = g.vox[v];
  float ga[3], gb[3];
  const bool has_a = vox_gradient(g, v, i, j, k, va, ga);
  const float cx = vox_centre(g.ox, i, g.vs), cy = vox_centre(g.oy, j, g.vs), cz = vox_centre(g.oz, k, g.vs);
  const uint32_t ca = col ? col[v] : 0u;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (!(edges[c] & bit)) continue;
    if (idx >= cap) return;
    const int dx = c == 0, dy = c == 1, dz = c == 2;
    const long long vb_i = vox_corner_word(g, v, 1 << c);
    const uint32_t vb = g.vox[vb_i];
    const bool has_b = vox_gradient(g, vb_i, i + dx, j + dy, k + dz, vb, gb);
    const VoxEdgePoint e = vox_edge_point(va, vb, has_a, ga, has_b, gb, cx, cy, cz, g.vs, dx, dy, dz);
    xyz0[idx] = make_float4(e.x, e.y, e.z, 0.0f);
    nrmw[idx] = make_float4(e.nx, e.ny, e.nz, e.w);
    if (col) rgba[idx] = colour_interpolate(ca, col[vb_i], vox_alpha(va, vb));
    idx++;
  }
}

// The block's sums of two per-thread counts into cnt[2 * block] and cnt[2 * block + 1].
template <int Threads>
__device__ __forceinline__ void block_sum2(unsigned a, unsigned b, unsigned* cnt) {
  __shared__ unsigned sh[2][Threads / 64];
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[0][w] = a; sh[1][w] = b; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned t = 0;
    for (int q = 0; q < Threads / 64; q++) t += sh[threadIdx.x][q];
    cnt[2 * blockIdx.x + threadIdx.x] = t;
  }
}

}  // namespace odo
