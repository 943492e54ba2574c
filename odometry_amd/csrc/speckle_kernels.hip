// speckle_kernels.hip — the speckle filter's kernels (speckle.hip.h) as a translation unit of its own, plus their host-side launcher.
// The connection predicate and the survival test are speckle_math.h's. include/odometry_hip.h, odo_speckle_create; DESIGN.md
// section 9.17.
#include <hip/hip_runtime.h>
#include "speckle.hip.h"

namespace odo {

// A parent word that other lanes lower with atomicMin while it is read. Any value it ever held is a pixel of the same component with
// an index no larger than the word's own, so a stale read only makes a walk longer.
template <int Scope>
__device__ __forceinline__ int sp_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, Scope); }

// The root above pixel i. Terminates because parent[i] <= i with equality only at a root: the index strictly decreases. `bound` is the
// number of pixels the plane has, which that invariant cannot exceed; a walk that does, or that meets a word breaking the invariant,
// sets `bit` in *guard and ends where it is.
template <int Scope>
__device__ __forceinline__ int sp_find(const int* parent, int i, int bound, int bit, uint32_t* guard) {
  int trips = 0;
  for (;;) {
    const int p = sp_load<Scope>(parent + i);
    if (p == i) break;
    if ((unsigned)p > (unsigned)i || ++trips > bound) { *guard |= (uint32_t)bit; break; }
    i = p;
  }
  return i;
}

// Unites the components of pixels a and b: the larger root is put under the smaller with atomicMin. If the word was no longer a root —
// another lane lowered it to `old` first — the link to `old` may have been replaced, so the union goes on from `old`. The larger of
// the two roots strictly decreases from trip to trip, so it ends within `bound` (the plane's pixel count) trips.
template <int Scope>
__device__ __forceinline__ void sp_union(int* parent, int a, int b, int bound, int find_bit, int union_bit, uint32_t* guard) {
  int trips = 0;
  for (;;) {
    a = sp_find<Scope>(parent, a, bound, find_bit, guard);
    b = sp_find<Scope>(parent, b, bound, find_bit, guard);
    if (a == b) break;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) break;
    if (++trips > bound) { *guard |= (uint32_t)union_bit; break; }
    a = old;
  }
}

// ---- label: the tile's union-find in LDS. A wave holds a tile row: a pixel starts under the first pixel of its horizontal run (from a
// ballot of the run starts), then every pixel connected to the one above unites the two runs.
__global__ void __launch_bounds__(kSpBlock) speckle_label_kernel(SpArgs a) {
  __shared__ int s_par[kSpTile];
  __shared__ int s_cnt[kSpTile];
  __shared__ uint16_t s_key[kSpTile];
  constexpr int kScope = __HIP_MEMORY_SCOPE_WORKGROUP;
  const int rows = a.rows, cols = a.cols, max_diff = a.max_diff;
  const int tid = (int)threadIdx.x, tx = tid & (kSpTileW - 1), ty = tid / kSpTileW;
  const int gx0 = (int)blockIdx.x * kSpTileW, gy0 = (int)blockIdx.y * kSpTileH;
  const int x = gx0 + tx;
  int key[kSpPerThread];
#pragma unroll
  for (int k = 0; k < kSpPerThread; k++) {
    const int ly = ty + k * (kSpBlock / kSpTileW), y = gy0 + ly;
    key[k] = (x < cols && y < rows) ? (int)a.key[(size_t)y * cols + x] : 0;
    const int left = __shfl_up(key[k], 1);
    const bool starts = tx == 0 || !sp_connected(key[k], left, max_diff);
    const unsigned long long runs = __ballot(starts) & (~0ull >> (kSpTileW - 1 - tx));      // the run starts at or before this lane
    const int l = ly * kSpTileW + tx;
    s_key[l] = (uint16_t)key[k];
    s_par[l] = ly * kSpTileW + (63 - __clzll((long long)runs));
    s_cnt[l] = 0;
  }
  __syncthreads();
  uint32_t guard = 0;
#pragma unroll
  for (int k = 0; k < kSpPerThread; k++) {
    const int ly = ty + k * (kSpBlock / kSpTileW), l = ly * kSpTileW + tx;
    if (ly > 0 && sp_connected(key[k], (int)s_key[l - kSpTileW], max_diff))
      sp_union<kScope>(s_par, l, l - kSpTileW, kSpTile, kSpGuardTileFind, kSpGuardTileUnion, &guard);
  }
  __syncthreads();
  int root[kSpPerThread];
#pragma unroll
  for (int k = 0; k < kSpPerThread; k++) {
    const int l = (ty + k * (kSpBlock / kSpTileW)) * kSpTileW + tx;
    root[k] = l;
    if (key[k]) {
      root[k] = sp_find<kScope>(s_par, l, kSpTile, kSpGuardTileFind, &guard);
      atomicAdd(s_cnt + root[k], 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSpPerThread; k++) {
    const int ly = ty + k * (kSpBlock / kSpTileW), y = gy0 + ly;
    if (x < cols && y < rows) {
      const size_t g = (size_t)y * cols + x;
      a.parent[g] = key[k] ? (gy0 + root[k] / kSpTileW) * cols + gx0 + (root[k] & (kSpTileW - 1)) : kSpNoLabel;
      a.size[g] = s_cnt[ly * kSpTileW + tx];
    }
  }
  if (guard) atomicOr(a.guard, guard);
}

// ---- seams: thread t < n_h is the pair (y - 1, x) | (y, x) on the horizontal seam y = (t / cols + 1) * kSpTileH; the others are the
// pairs (y, x - 1) | (y, x) on the vertical seams x = (u / rows + 1) * kSpTileW, u = t - n_h.
__global__ void __launch_bounds__(kSpBlock) speckle_seam_kernel(SpArgs a, int n_h, int n_pairs) {
  constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
  const int t = (int)blockIdx.x * kSpBlock + (int)threadIdx.x;
  if (t >= n_pairs) return;
  const int rows = a.rows, cols = a.cols;
  int i, j;
  if (t < n_h) {
    const int s = t / cols, x = t - s * cols;
    i = (s + 1) * kSpTileH * cols + x;
    j = i - cols;
  } else {
    const int u = t - n_h, s = u / rows, y = u - s * rows;
    i = y * cols + (s + 1) * kSpTileW;
    j = i - 1;
  }
  if (!sp_connected((int)a.key[i], (int)a.key[j], a.max_diff)) return;
  uint32_t guard = 0;
  sp_union<kScope>(a.parent, i, j, rows * cols, kSpGuardSeamFind, kSpGuardSeamUnion, &guard);
  if (guard) atomicOr(a.guard, guard);
}

// ---- count: a tile-local root (size > 0) that came under another root hands its count to its component's root and points at it.
// While this runs parents only move to the root itself, so every walk ends at the component's smallest index.
__global__ void __launch_bounds__(kSpBlock) speckle_count_kernel(SpArgs a) {
  constexpr int kScope = __HIP_MEMORY_SCOPE_AGENT;
  const int n = a.rows * a.cols;
  const int i = (int)blockIdx.x * kSpBlock + (int)threadIdx.x;
  if (i >= n) return;
  const int c = a.size[i];
  if (c <= 0) return;
  uint32_t guard = 0;
  const int r = sp_find<kScope>(a.parent, i, n, kSpGuardCountFind, &guard);
  if (r != i) {
    __hip_atomic_store(a.parent + i, r, __ATOMIC_RELAXED, kScope);
    atomicAdd(a.size + r, c);
  }
  if (guard) atomicOr(a.guard, guard);
}

// ---- apply: after the count every tile-local root points at its component's root, and every other pixel at its tile-local root.
__global__ void __launch_bounds__(kSpBlock) speckle_apply_kernel(SpArgs a) {
  __shared__ uint32_t s_red[kSpBlock / 64][5];
  const int rows = a.rows, cols = a.cols, min_size = a.min_size;
  const int tid = (int)threadIdx.x, tx = tid & (kSpTileW - 1), ty = tid / kSpTileW;
  const int x = (int)blockIdx.x * kSpTileW + tx, gy0 = (int)blockIdx.y * kSpTileH;
  uint32_t n[5] = {0u, 0u, 0u, 0u, 0u};                  // pixels, components, removed_components, removed_pixels, largest
#pragma unroll
  for (int k = 0; k < kSpPerThread; k++) {
    const int y = gy0 + ty + k * (kSpBlock / kSpTileW);
    if (x >= cols || y >= rows) continue;
    const int g = y * cols + x;
    const int p = a.parent[g];
    if (p < 0) continue;
    const int r = a.parent[p];
    const int sz = a.size[r];
    const bool keep = sp_survives(sz, min_size);
    n[0] += 1u;
    if (r == g) {
      n[1] += 1u;
      n[2] += (uint32_t)!keep;
      n[4] = (uint32_t)sz > n[4] ? (uint32_t)sz : n[4];
    }
    if (!keep) {
      n[3] += 1u;
      a.a[g] = 0;
      if (a.b) a.b[g] = 0;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; k++) n[k] += __shfl_down(n[k], off);
    const uint32_t m = __shfl_down(n[4], off);
    n[4] = m > n[4] ? m : n[4];
  }
  if (tx == 0)
#pragma unroll
    for (int k = 0; k < 5; k++) s_red[ty][k] = n[k];
  __syncthreads();
  if (tid == 0) {
    uint32_t r[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int v = 0; v < kSpBlock / 64; v++) {
#pragma unroll
      for (int k = 0; k < 4; k++) r[k] += s_red[v][k];
      r[4] = s_red[v][4] > r[4] ? s_red[v][4] : r[4];
    }
    const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    uint4* row = reinterpret_cast<uint4*>(a.partials + kSpStatWords * b);
    row[0] = make_uint4(r[0], r[1], r[2], r[3]);
    row[1] = make_uint4(r[4], 0u, 0u, 0u);
  }
}

void launch_speckle_stage(const SpArgs& a, int stage, hipStream_t s) {
  const dim3 grid((unsigned)sp_blocks_x(a.cols), (unsigned)sp_blocks_y(a.rows));
  const int n = a.rows * a.cols;
  if (stage == 0) {
    hipLaunchKernelGGL(speckle_label_kernel, grid, dim3(kSpBlock), 0, s, a);
  } else if (stage == 1) {
    const int n_h = (sp_blocks_y(a.rows) - 1) * a.cols, n_pairs = (int)sp_seam_pairs(a.rows, a.cols);
    if (n_pairs > 0) hipLaunchKernelGGL(speckle_seam_kernel, dim3((unsigned)((n_pairs + kSpBlock - 1) / kSpBlock)), dim3(kSpBlock), 0, s, a, n_h, n_pairs);
  } else if (stage == 2) {
    hipLaunchKernelGGL(speckle_count_kernel, dim3((unsigned)((n + kSpBlock - 1) / kSpBlock)), dim3(kSpBlock), 0, s, a);
  } else {
    hipLaunchKernelGGL(speckle_apply_kernel, grid, dim3(kSpBlock), 0, s, a);
  }
}

}  // namespace odo
