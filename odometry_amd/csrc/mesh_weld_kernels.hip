// mesh_weld_kernels.hip — the mesh welder's kernels (mesh_weld.hip.h) as a translation unit of their own, plus their host-side
// launcher. The key, the hashes and the rotation are mesh_weld_math.h's; the compaction is count -> scan -> scatter with the helpers of
// volume_scan.hip.h. include/odometry_hip.h, odo_mesh_weld_create; DESIGN.md section 9.19.
#include <hip/hip_runtime.h>
#include "mesh_weld.hip.h"
#include "volume_scan.hip.h"

namespace odo {

constexpr int kWeldScope = __HIP_MEMORY_SCOPE_AGENT;

// The block's counts of N predicates: thread k < N gets the number of threads whose p[k] holds, every other thread 0. Every thread
// of the block calls it. A counter of the run then takes one atomic per block, and none for a count of 0: the counters are single
// words, and every atomic on one word is served in turn.
template <int N>
__device__ __forceinline__ uint32_t weld_block_sums(const bool (&p)[N]) {
  __shared__ uint32_t sh[N][kWeldBlock / 64];
#pragma unroll
  for (int k = 0; k < N; k++) {
    const unsigned long long b = __ballot(p[k]);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  uint32_t t = 0;
  if (threadIdx.x < N)
#pragma unroll
    for (int q = 0; q < kWeldBlock / 64; q++) t += sh[threadIdx.x][q];
  return t;
}
__device__ __forceinline__ void weld_add(unsigned long long* ctr, uint32_t n) {
  if (n) atomicAdd(ctr, (unsigned long long)n);
}

__global__ void weld_begin_kernel(WeldState* state0, unsigned long long* ctr, uint32_t n_v, uint32_t n_t) {
  if (threadIdx.x == 0) { state0->n_v = n_v; state0->n_t = n_t; }
  if (threadIdx.x < kWeldStatWords) ctr[threadIdx.x] = 0ull;
}

// ---- group 0: a vertex claims its key's slot and lowers the slot's smallest index. Every claimant of a key walks the same sequence
// and stops at the first slot that holds the key or is empty; a slot never changes its key, so all of them end in the same slot.
// A slot is read before it is written: where many vertices share a cell, only the first few claimants of its slot pay for an atomic
// (a stale read costs the atomic it would have saved, never the result).
__global__ void __launch_bounds__(kWeldBlock) weld_key_kernel(WeldArgs a) {
  const uint32_t i = blockIdx.x * kWeldBlock + threadIdx.x;
  if (i >= a.in->n_v) return;
  const float4 p = a.in_xyz0[i];
  const float o[3] = {a.ox, a.oy, a.oz};
  const unsigned long long key = weld_key(p.x, p.y, p.z, o, a.inv, a.grid);
  int32_t slot = -1;
  if (key != kWeldNoKey) {
    const uint32_t mask = a.vslots - 1u;
    uint32_t s = (uint32_t)weld_hash(key) & mask, trips = 0;
    for (;;) {
      unsigned long long cur = __hip_atomic_load(&a.vkeys[s], __ATOMIC_RELAXED, kWeldScope);
      if (cur == kWeldNoKey) {
        __hip_atomic_compare_exchange_strong(&a.vkeys[s], &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, kWeldScope);
        if (cur == kWeldNoKey) cur = key;   // claimed; otherwise cur is the key that came first
      }
      if (cur == key) { slot = (int32_t)s; break; }
      if (++trips >= a.vslots) { atomicOr(a.ctr + kWeldGuard, (unsigned long long)kWeldGuardVertexProbe); break; }
      s = (s + 1u) & mask;
    }
    if (slot >= 0 && __hip_atomic_load(&a.vmin[slot], __ATOMIC_RELAXED, kWeldScope) > i)   // (the word only ever falls)
      __hip_atomic_fetch_min(&a.vmin[slot], i, __ATOMIC_RELAXED, kWeldScope);
  }
  a.vaux[i] = slot;
}

// ---- group 1: the representatives, behind the kernel boundary that completes every atomicMin.
__global__ void __launch_bounds__(kWeldBlock) weld_rep_kernel(WeldArgs a) {
  const uint32_t i = blockIdx.x * kWeldBlock + threadIdx.x;
  const bool live = i < a.in->n_v;
  int32_t slot = -1, r = (int32_t)i;
  if (live) {
    slot = a.vaux[i];
    if (slot >= 0) r = (int32_t)a.vmin[slot];
    a.rep[i] = r;
  }
  const bool p[2] = {live && r != (int32_t)i, live && slot < 0};
  const uint32_t n = weld_block_sums<2>(p);
  if (threadIdx.x < 2) weld_add(a.ctr + (threadIdx.x == 0 ? kWeldMerged : kWeldKeyless), n);
}

// ---- group 2: the rotated triples, then the triangle table. A slot holds a triangle index; the triple behind it is read from rtri,
// which the launch before wrote. Whoever finds its own triple in a slot lowers the slot to its index if that is smaller.
__global__ void __launch_bounds__(kWeldBlock) weld_remap_kernel(WeldArgs a) {
  const uint32_t t = blockIdx.x * kWeldBlock + threadIdx.x;
  if (t >= a.in->n_t) return;
  const int32_t in[3] = {a.in_tri[3 * (size_t)t], a.in_tri[3 * (size_t)t + 1], a.in_tri[3 * (size_t)t + 2]};
  int32_t r[3];
  weld_remap(in, a.rep, (int)a.in->n_v, r);
#pragma unroll
  for (int c = 0; c < 3; c++) a.rtri[3 * (size_t)t + c] = r[c];
}

__global__ void __launch_bounds__(kWeldBlock) weld_tri_table_kernel(WeldArgs a) {
  const uint32_t t = blockIdx.x * kWeldBlock + threadIdx.x;
  if (t >= a.in->n_t) return;
  const int32_t r0 = a.rtri[3 * (size_t)t], r1 = a.rtri[3 * (size_t)t + 1], r2 = a.rtri[3 * (size_t)t + 2];
  int32_t slot = -1;
  if (r0 >= 0) {
    const uint32_t mask = a.tslots - 1u;
    uint32_t s = (uint32_t)weld_tri_hash(r0, r1, r2) & mask, trips = 0;
    for (;;) {
      int32_t cur = __hip_atomic_load(&a.ttab[s], __ATOMIC_RELAXED, kWeldScope);
      if (cur == kWeldNoTri) {
        __hip_atomic_compare_exchange_strong(&a.ttab[s], &cur, (int32_t)t, __ATOMIC_RELAXED, __ATOMIC_RELAXED, kWeldScope);
        if (cur == kWeldNoTri) { slot = (int32_t)s; break; }   // claimed; otherwise cur is the occupant that came first
      }
      const int32_t* u = a.rtri + 3 * (size_t)cur;
      if (u[0] == r0 && u[1] == r1 && u[2] == r2) {
        if (cur > (int32_t)t) __hip_atomic_fetch_min(&a.ttab[s], (int32_t)t, __ATOMIC_RELAXED, kWeldScope);   // (a slot only ever falls)
        slot = (int32_t)s;
        break;
      }
      if (++trips >= a.tslots) { atomicOr(a.ctr + kWeldGuard, (unsigned long long)kWeldGuardTriangleProbe); break; }
      s = (s + 1u) & mask;
    }
  }
  a.tslot[t] = slot;
}

// Triangle t survives iff the slot that holds its triple holds t.
__device__ __forceinline__ bool weld_tri_kept(const WeldArgs& a, uint32_t t) {
  const int32_t slot = a.tslot[t];
  return slot >= 0 && a.ttab[slot] == (int32_t)t;
}
// A vertex is kept iff it is its own representative and, when unreferenced vertices are dropped, a surviving triangle names it.
__device__ __forceinline__ bool weld_vertex_kept(const WeldArgs& a, uint32_t i, bool* unreferenced) {
  const bool own = a.rep[i] == (int32_t)i;
  *unreferenced = own && a.drop_unreferenced && !a.vref[i];
  return own && !*unreferenced;
}

// ---- group 3: the survivors and their per-block counts.
__global__ void __launch_bounds__(kWeldBlock) weld_tri_keep_kernel(WeldArgs a) {
  const uint32_t n_t = a.in->n_t, t = blockIdx.x * kWeldBlock + threadIdx.x;
  if (blockIdx.x * kWeldBlock >= n_t) return;
  bool keep = false, dup = false, deg = false, bad = false;
  if (t < n_t) {
    const int32_t r0 = a.rtri[3 * (size_t)t];
    bad = r0 == kWeldTriBad;
    deg = r0 == kWeldTriDegenerate;
    if (r0 >= 0) {
      keep = weld_tri_kept(a, t);
      dup = !keep && a.tslot[t] >= 0;
      if (keep) {
        a.vref[r0] = 1;
        a.vref[a.rtri[3 * (size_t)t + 1]] = 1;
        a.vref[a.rtri[3 * (size_t)t + 2]] = 1;
      }
    }
  }
  const bool p[4] = {keep, dup, deg, bad};
  const uint32_t n = weld_block_sums<4>(p);
  if (threadIdx.x == 0) a.tblk[blockIdx.x] = n;
  else if (threadIdx.x < 4) weld_add(a.ctr + (threadIdx.x == 1 ? kWeldDuplicate : threadIdx.x == 2 ? kWeldDegenerate : kWeldBadIndex), n);
}

__global__ void __launch_bounds__(kWeldBlock) weld_vertex_keep_kernel(WeldArgs a) {
  const uint32_t n_v = a.in->n_v, i = blockIdx.x * kWeldBlock + threadIdx.x;
  if (blockIdx.x * kWeldBlock >= n_v) return;
  bool unref = false;
  const bool keep = i < n_v && weld_vertex_kept(a, i, &unref);
  const bool p[2] = {keep, unref};
  const uint32_t n = weld_block_sums<2>(p);
  if (threadIdx.x == 0) a.vblk[blockIdx.x] = n;
  else if (threadIdx.x == 1) weld_add(a.ctr + kWeldUnreferenced, n);
}

// ---- group 4: one block: both counts' exclusive offsets (volume_scan.hip.h), the next pass's counts, the run's counters.
__global__ void __launch_bounds__(kWeldScanThreads) weld_scan_kernel(WeldArgs a) {
  const uint32_t n_v = a.in->n_v, n_t = a.in->n_t;
  const unsigned long long tv = scan_counts<kWeldScanThreads, 1>(a.vblk, a.vblk_off, (int)((n_v + kWeldBlock - 1) / kWeldBlock)).t[0];
  const unsigned long long tt = scan_counts<kWeldScanThreads, 1>(a.tblk, a.tblk_off, (int)((n_t + kWeldBlock - 1) / kWeldBlock)).t[0];
  if (threadIdx.x == 0) {
    a.out->n_v = (uint32_t)tv;
    a.out->n_t = (uint32_t)tt;
    if (a.first) { a.ctr[kWeldVerticesIn] = n_v; a.ctr[kWeldTrianglesIn] = n_t; }
    if (a.last) { a.ctr[kWeldVerticesOut] = tv; a.ctr[kWeldTrianglesOut] = tt; }
    a.ctr[kWeldPasses] += 1ull;
  }
}

// ---- group 5: the kept vertices in ascending index with their own bytes; the surviving triangles in input order, in the new indices.
__global__ void __launch_bounds__(kWeldBlock) weld_vertex_scatter_kernel(WeldArgs a) {
  __shared__ unsigned wsum[kWeldBlock / 64];
  const uint32_t n_v = a.in->n_v, i = blockIdx.x * kWeldBlock + threadIdx.x;
  if (blockIdx.x * kWeldBlock >= n_v) return;
  bool unref;
  const bool keep = i < n_v && weld_vertex_kept(a, i, &unref);
  const unsigned rank = scan_block<kWeldBlock>(keep ? 1u : 0u, wsum).rank;
  if (i >= n_v) return;
  const unsigned long long idx = a.vblk_off[blockIdx.x] + rank;
  a.vaux[i] = keep ? (int32_t)idx : -1;
  if (!keep) return;
  a.out_xyz0[idx] = a.in_xyz0[i];
  a.out_nrmw[idx] = a.in_nrmw[i];
  if (a.in_rgba) a.out_rgba[idx] = a.in_rgba[i];
}

__global__ void __launch_bounds__(kWeldBlock) weld_tri_scatter_kernel(WeldArgs a) {
  __shared__ unsigned wsum[kWeldBlock / 64];
  const uint32_t n_t = a.in->n_t, t = blockIdx.x * kWeldBlock + threadIdx.x;
  if (blockIdx.x * kWeldBlock >= n_t) return;
  const bool keep = t < n_t && a.rtri[3 * (size_t)t] >= 0 && weld_tri_kept(a, t);
  const unsigned rank = scan_block<kWeldBlock>(keep ? 1u : 0u, wsum).rank;
  if (!keep) return;
  const unsigned long long idx = a.tblk_off[blockIdx.x] + rank;
#pragma unroll
  for (int c = 0; c < 3; c++) a.out_tri[3 * idx + c] = a.vaux[a.rtri[3 * (size_t)t + c]];
}

void launch_weld_begin(WeldState* state0, unsigned long long* ctr, int n_v, int n_t, hipStream_t s) {
  hipLaunchKernelGGL(weld_begin_kernel, dim3(1), dim3(64), 0, s, state0, ctr, (uint32_t)n_v, (uint32_t)n_t);
}

int launch_weld_group(const WeldArgs& a, int group, hipStream_t s) {
  const dim3 block(kWeldBlock), vgrid((unsigned)weld_blocks(a.n_v_max)), tgrid((unsigned)weld_blocks(a.n_t_max));
  const bool v = a.n_v_max > 0, t = a.n_t_max > 0;
  hipError_t e = hipSuccess;
  if (group == 0) {
    if (v) {
      e = hipMemsetAsync(a.vkeys, 0xFF, sizeof(unsigned long long) * (size_t)a.vslots, s);
      if (e == hipSuccess) e = hipMemsetAsync(a.vmin, 0xFF, sizeof(uint32_t) * (size_t)a.vslots, s);
      hipLaunchKernelGGL(weld_key_kernel, vgrid, block, 0, s, a);
    }
  } else if (group == 1) {
    if (v) hipLaunchKernelGGL(weld_rep_kernel, vgrid, block, 0, s, a);
  } else if (group == 2) {
    if (t) {
      e = hipMemsetAsync(a.ttab, 0xFF, sizeof(int32_t) * (size_t)a.tslots, s);
      hipLaunchKernelGGL(weld_remap_kernel, tgrid, block, 0, s, a);
      hipLaunchKernelGGL(weld_tri_table_kernel, tgrid, block, 0, s, a);
    }
  } else if (group == 3) {
    if (v) e = hipMemsetAsync(a.vref, 0, (size_t)a.n_v_max, s);
    if (t) hipLaunchKernelGGL(weld_tri_keep_kernel, tgrid, block, 0, s, a);
    if (v) hipLaunchKernelGGL(weld_vertex_keep_kernel, vgrid, block, 0, s, a);
  } else if (group == 4) {
    hipLaunchKernelGGL(weld_scan_kernel, dim3(1), dim3(kWeldScanThreads), 0, s, a);
  } else {
    if (v) hipLaunchKernelGGL(weld_vertex_scatter_kernel, vgrid, block, 0, s, a);
    if (t) hipLaunchKernelGGL(weld_tri_scatter_kernel, tgrid, block, 0, s, a);
  }
  return e == hipSuccess ? 0 : -1;
}

}  // namespace odo
