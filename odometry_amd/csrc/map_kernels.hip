// map_kernels.hip — the keyframe point-cloud map's insertion kernels (map.hip.h) as a translation unit of their own, plus their
// host-side launcher. Same per-point arithmetic as the tracker (odo_math.h: point_xyz, world_point, voxel_index).
#include <hip/hip_runtime.h>
#include "map.hip.h"
#include "odo_math.h"

namespace odo {

// Candidate test of the spec: mask set (or no mask), valid (depth_valid) and positive inverse depth.
__device__ __forceinline__ bool map_is_candidate(const MapInsertArgs& a, int i) {
  if (a.val && a.val[i] == 0) return false;
  const float d = a.dep[i];
  return depth_valid(d) && d > 0.0f;
}

__device__ __forceinline__ void map_world(const MapInsertArgs& a, int i, float* xw, float* yw, float* zw) {
  const int y = i / a.cols, x = i - y * a.cols;
  float X, Y, Z;
  point_xyz(x, y, a.dep[i], make_level_k(a.f0, a.cx0, a.cy0, 0), &X, &Y, &Z);
  const float A[16] = {a.a0, a.a1, a.a2, 0.0f, a.a4, a.a5, a.a6, 0.0f, a.a8, a.a9, a.a10, 0.0f, a.a12, a.a13, a.a14, 1.0f};
  world_point(X, Y, Z, A, xw, yw, zw);
}

// 63-bit key: three 21-bit fields k + 2^20 (|k| < 2^20), never all ones.
__device__ __forceinline__ unsigned long long map_key(int kx, int ky, int kz) {
  return (unsigned long long)(unsigned)(kx + (1 << 20)) | ((unsigned long long)(unsigned)(ky + (1 << 20)) << 21) |
         ((unsigned long long)(unsigned)(kz + (1 << 20)) << 42);
}
__device__ __forceinline__ unsigned long long map_hash(unsigned long long k) {   // splitmix64 finaliser
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27; k *= 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}

__global__ void __launch_bounds__(kMapBlock) map_claim_kernel(MapInsertArgs a) {
  const int i = blockIdx.x * kMapBlock + threadIdx.x;
  if (i >= a.n) return;
  if (a.ctr->size >= (unsigned long long)a.capacity) return;   // a full map: the insertion changes nothing (count writes no survivor)
  int code = -1;
  if (map_is_candidate(a, i)) {
    float xw, yw, zw;
    map_world(a, i, &xw, &yw, &zw);
    int kx, ky, kz;
    if (voxel_index(xw, a.voxel, &kx) && voxel_index(yw, a.voxel, &ky) && voxel_index(zw, a.voxel, &kz)) {
      const unsigned long long key = map_key(kx, ky, kz);
      unsigned long long s = map_hash(key) & a.slot_mask;
      // Linear probing. The table holds at most capacity + rows * cols keys in 2 * that many slots (a full map claims nothing), so
      // an empty slot is always found. Every claimant of a key walks the same sequence and stops at the first slot holding it.
      for (;;) {
        unsigned long long expected = kMapEmpty;
        __hip_atomic_compare_exchange_strong(&a.keys[s], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (expected == kMapEmpty || expected == key) break;
        s = (s + 1) & a.slot_mask;
      }
      __hip_atomic_fetch_min(&a.payload[s], ((unsigned long long)a.ins << 32) | (unsigned)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      code = (int)s;
    } else {
      code = -2;
    }
  }
  a.pix_slot[i] = code;
}

__global__ void __launch_bounds__(kMapBlock) map_count_kernel(MapInsertArgs a) {
  __shared__ int sh[3][kMapBlock / 64];
  const int i = blockIdx.x * kMapBlock + threadIdx.x;
  const bool open = a.ctr->size < (unsigned long long)a.capacity;
  bool surv = false, cand = false, range = false;
  if (i < a.n && open) {
    if (a.voxel > 0.0f) {
      const int s = a.pix_slot[i];
      cand = s != -1;
      range = s == -2;
      surv = s >= 0 && __hip_atomic_load(&a.payload[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                           (((unsigned long long)a.ins << 32) | (unsigned)i);
    } else {
      cand = map_is_candidate(a, i);
      surv = cand;
    }
  }
  const unsigned long long bs = __ballot(surv), bc = __ballot(cand), br = __ballot(range);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    a.wave_mask[blockIdx.x * (kMapBlock / 64) + w] = bs;
    sh[0][w] = __popcll(bs); sh[1][w] = __popcll(bc); sh[2][w] = __popcll(br);
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int t = 0;
    for (int k = 0; k < kMapBlock / 64; k++) t += sh[threadIdx.x][k];
    a.blk[3 * blockIdx.x + threadIdx.x] = t;
  }
}

// One block: exclusive scan of the per-block survivor counts (each thread a contiguous chunk), totals, counters.
__global__ void __launch_bounds__(kMapScanThreads) map_scan_kernel(MapInsertArgs a) {
  __shared__ long long wsum[3][kMapScanThreads / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int per = (a.nblk + kMapScanThreads - 1) / kMapScanThreads;
  const int b0 = t * per, b1 = min(b0 + per, a.nblk);
  long long s = 0, c = 0, r = 0;
  for (int b = b0; b < b1; b++) { s += a.blk[3 * b]; c += a.blk[3 * b + 1]; r += a.blk[3 * b + 2]; }
  // inclusive scan of s over the wave, then over the waves
  long long inc = s;
  for (int o = 1; o < 64; o <<= 1) {
    const long long v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  long long cs = c, rs = r;
  for (int o = 32; o > 0; o >>= 1) { cs += __shfl_xor(cs, o, 64); rs += __shfl_xor(rs, o, 64); }
  if (lane == 63) wsum[0][w] = inc;
  if (lane == 0) { wsum[1][w] = cs; wsum[2][w] = rs; }
  __syncthreads();
  long long before = 0, total = 0, cand = 0, rng = 0;
  for (int k = 0; k < kMapScanThreads / 64; k++) {
    if (k < w) before += wsum[0][k];
    total += wsum[0][k]; cand += wsum[1][k]; rng += wsum[2][k];
  }
  long long off = before + inc - s;
  for (int b = b0; b < b1; b++) { a.blk_off[b] = (int)off; off += a.blk[3 * b]; }
  if (t == 0) {
    MapCounters* m = a.ctr;
    const unsigned long long size = m->size;
    if (size < (unsigned long long)a.capacity) {
      const unsigned long long room = (unsigned long long)a.capacity - size;
      const unsigned long long app = (unsigned long long)total < room ? (unsigned long long)total : room;
      m->base = size;
      m->size = size + app;
      m->candidates += (unsigned long long)cand;
      m->dropped_range += (unsigned long long)rng;
      m->dropped_voxel += (unsigned long long)(cand - rng - total);
      m->dropped_capacity += (unsigned long long)total - app;
    }
  }
}

__global__ void __launch_bounds__(kMapBlock) map_scatter_kernel(MapInsertArgs a) {
  const int i = blockIdx.x * kMapBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long* wm = a.wave_mask + blockIdx.x * (kMapBlock / 64);
  const unsigned long long mine = wm[w];
  if (i >= a.n || !((mine >> lane) & 1ull)) return;
  int pre = 0;
  for (int k = 0; k < w; k++) pre += __popcll(wm[k]);
  const unsigned long long below = lane ? (mine & (~0ull >> (64 - lane))) : 0ull;
  const unsigned long long idx = a.ctr->base + (unsigned long long)a.blk_off[blockIdx.x] + (unsigned long long)(pre + __popcll(below));
  if (idx >= (unsigned long long)a.capacity) return;
  float xw, yw, zw;
  map_world(a, i, &xw, &yw, &zw);
  a.xyzi[idx] = make_float4(xw, yw, zw, a.img ? a.img[i] : 0.0f);
  a.kf_pixel[idx] = make_int2((int)a.ins, i);
}

void launch_map_insert(const MapInsertArgs& a, hipStream_t s) {
  const dim3 grid(a.nblk), block(kMapBlock);
  if (a.voxel > 0.0f) hipLaunchKernelGGL(map_claim_kernel, grid, block, 0, s, a);
  hipLaunchKernelGGL(map_count_kernel, grid, block, 0, s, a);
  hipLaunchKernelGGL(map_scan_kernel, dim3(1), dim3(kMapScanThreads), 0, s, a);
  hipLaunchKernelGGL(map_scatter_kernel, grid, block, 0, s, a);
}

}  // namespace odo
