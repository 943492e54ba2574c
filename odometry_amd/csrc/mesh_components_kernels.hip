// mesh_components_kernels.hip — the mesh component filter's kernels (mesh_components.hip.h) as a translation unit of their own, plus
// their host-side launcher. Validity, survival, the largest component's word and the edge key are mesh_components_math.h's; the
// union-find is the speckle filter's scheme (speckle_kernels.hip) over vertices; the compaction is count -> scan -> scatter with the
// helpers of volume_scan.hip.h. include/odometry_hip.h, odo_mesh_components_create; DESIGN.md section 9.20.
#include <hip/hip_runtime.h>
#include "mesh_components.hip.h"
#include "volume_scan.hip.h"

namespace odo {

constexpr int kMcScope = __HIP_MEMORY_SCOPE_AGENT;

// A/B builds (tools/mesh_components_cost.py): ODO_MC_SHORTEN 0 takes the path shortening out of the unions,
// ODO_MC_ELECT 0 the wave's election out of the sizes, ODO_MC_WALK_SCOPE is the scope at which a union's walk reads parent words.
// The results are the same bytes either way.
// The walk's scope is the workgroup's: the read may be served by the CU's L1, which is invalidated when the kernel starts, so it
// returns a value the word held during this launch — a vertex of the same component with a smaller index, which only makes a walk
// longer. A root that is stale is found out by the atomicMin that follows: it returns the word's present value, and the union goes
// on from there. At agent scope every walk's last read goes to the L2 channel of one hot root word (about 720 against 1 066 us).
#ifndef ODO_MC_SHORTEN
#define ODO_MC_SHORTEN 1
#endif
#ifndef ODO_MC_WALK_SCOPE
#define ODO_MC_WALK_SCOPE __HIP_MEMORY_SCOPE_WORKGROUP
#endif
#ifndef ODO_MC_ELECT
#define ODO_MC_ELECT 1
#endif

// A parent word that other threads lower with atomicMin while it is read. Any value it ever held is a vertex of the same component
// with an index no larger than the word's own, so a stale read only makes a walk longer.
template <int Scope = kMcScope>
__device__ __forceinline__ int32_t mc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, Scope); }

// The root above vertex i. Terminates because parent[i] <= i with equality only at a root: the index strictly decreases. `bound` is
// the number of vertices, which that invariant cannot exceed; a walk that does, or that meets a word breaking the invariant, sets
// kMcGuardFind in *guard and ends where it is.
template <int Scope = kMcScope>
__device__ __forceinline__ int32_t mc_find(const int32_t* parent, int32_t i, int bound, uint32_t* guard) {
  int trips = 0;
  for (;;) {
    const int32_t p = mc_load<Scope>(parent + i);
    if (p == i) break;
    if ((uint32_t)p > (uint32_t)i || ++trips > bound) { *guard |= (uint32_t)kMcGuardFind; break; }
    i = p;
  }
  return i;
}

// Unites the components of vertices a and b: the larger root is put under the smaller with atomicMin. If the word was no longer a
// root — another thread lowered it to `old` first — the link to `old` may have been replaced, so the union goes on from `old`. The
// larger of the two roots strictly decreases from trip to trip, so it ends within `bound` trips.
// On the way out both vertices are pointed at the root that was found, if that lowers their words: every word a parent ever held is
// a vertex of the same component with a smaller index, so shortening a path with atomicMin never changes a root, and later walks
// from these vertices are one step.
__device__ __forceinline__ void mc_union(int32_t* parent, int32_t a, int32_t b, int bound, uint32_t* guard) {
  const int32_t a0 = a, b0 = b;
  int trips = 0;
  for (;;) {
    a = mc_find<ODO_MC_WALK_SCOPE>(parent, a, bound, guard);
    b = mc_find<ODO_MC_WALK_SCOPE>(parent, b, bound, guard);
    if (a == b) break;
    if (a < b) { const int32_t t = a; a = b; b = t; }
    const int32_t old = atomicMin(parent + a, b);
    if (old == a) break;
    if (++trips > bound) { *guard |= (uint32_t)kMcGuardUnion; break; }
    a = old;
  }
#if ODO_MC_SHORTEN
  const int32_t r = a < b ? a : b;                                    // (the root both were under when the loop ended)
  if (mc_load(parent + a0) > r) atomicMin(parent + a0, r);
  if (mc_load(parent + b0) > r) atomicMin(parent + b0, r);
#endif
}

// The block's counts of N predicates: thread k < N gets the number of threads whose p[k] holds, every other thread 0. Every thread
// of the block calls it. A counter of the run then takes one atomic per block, and none for a count of 0.
template <int N>
__device__ __forceinline__ uint32_t mc_block_sums(const bool (&p)[N]) {
  __shared__ uint32_t sh[N][kMcBlock / 64];
#pragma unroll
  for (int k = 0; k < N; k++) {
    const unsigned long long b = __ballot(p[k]);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = (uint32_t)__popcll(b);
  }
  __syncthreads();
  uint32_t t = 0;
  if (threadIdx.x < N)
#pragma unroll
    for (int q = 0; q < kMcBlock / 64; q++) t += sh[threadIdx.x][q];
  return t;
}
__device__ __forceinline__ void mc_add(unsigned long long* ctr, uint32_t n) {
  if (n) atomicAdd(ctr, (unsigned long long)n);
}

__device__ __forceinline__ void mc_triangle(const McArgs& a, uint32_t t, int32_t (&v)[3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) v[c] = a.in_tri[3 * (size_t)t + c];
}

__device__ __forceinline__ bool mc_kept(const McArgs& a, int32_t label, unsigned long long best) {
  return mc_survives(a.size[label], label, a.min_triangles, a.keep_largest, best);
}

__global__ void mc_begin_kernel(McState* state, unsigned long long* ctr) {
  if (threadIdx.x == 0) { state->n_v = 0u; state->n_t = 0u; state->best = 0ull; }
  if (threadIdx.x < kMcStatWords) ctr[threadIdx.x] = 0ull;
}

// ---- group 0: every vertex its own root, then the unions.
__global__ void __launch_bounds__(kMcBlock) mc_init_kernel(McArgs a) {
  const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
  if (i < (uint32_t)a.n_v) a.parent[i] = (int32_t)i;
}

__global__ void __launch_bounds__(kMcBlock) mc_union_kernel(McArgs a) {
  const uint32_t t = blockIdx.x * kMcBlock + threadIdx.x;
  if (t >= (uint32_t)a.n_t) return;
  int32_t v[3];
  mc_triangle(a, t, v);
  if (!mc_valid(v, a.n_v)) return;
  uint32_t guard = 0;
  if (v[1] != v[0]) mc_union(a.parent, v[0], v[1], a.n_v, &guard);
  if (v[2] != v[0]) mc_union(a.parent, v[0], v[2], a.n_v, &guard);
  if (guard) atomicOr(a.ctr + kMcGuard, (unsigned long long)guard);
}

// ---- group 1: behind the kernel boundary that completes every union the roots are final. A vertex's word goes straight to its
// root: a walk that reads it meanwhile sees the old ancestor or the root, both of its component and no larger than itself.
__global__ void __launch_bounds__(kMcBlock) mc_flatten_kernel(McArgs a) {
  const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
  if (i >= (uint32_t)a.n_v) return;
  uint32_t guard = 0;
  const int32_t r = mc_find(a.parent, (int32_t)i, a.n_v, &guard);
  if (r != (int32_t)i) __hip_atomic_store(a.parent + i, r, __ATOMIC_RELAXED, kMcScope);
  a.size[i] = 0u;
  if (guard) atomicOr(a.ctr + kMcGuard, (unsigned long long)guard);
}

// A mesh is mostly one component: nearly every triangle of a launch adds to the same word. So a wave elects one lane per distinct
// root — a ballot against the first remaining lane's root, while lanes remain — and the wave's first root waits in LDS, where
// thread 0 merges the block's waves that agree before it goes to memory. Integer sums: the order does not matter.
__global__ void __launch_bounds__(kMcBlock) mc_label_kernel(McArgs a) {
  __shared__ int32_t s_root[kMcBlock / 64];
  __shared__ uint32_t s_cnt[kMcBlock / 64];
  const uint32_t t = blockIdx.x * kMcBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  bool valid = false, bad = false, deg = false;
  int32_t root = -1;
  if (t < (uint32_t)a.n_t) {
    int32_t v[3];
    mc_triangle(a, t, v);
    valid = mc_valid(v, a.n_v);
    bad = !valid;
    if (valid) {
      deg = mc_degenerate(v);
      root = a.parent[v[0]];
    }
    a.label[t] = valid ? root : kMcNoLabel;
  }
  if (lane == 0) s_cnt[w] = 0u;
#if !ODO_MC_ELECT
  if (valid) atomicAdd(a.size + root, 1u);
  unsigned long long left = 0ull;
#else
  unsigned long long left = __ballot(valid);
#endif
  bool first = true;
  while (left) {                                                      // (wave-uniform; at most 64 trips)
    const int leader = __ffsll((long long)left) - 1;
    const int32_t r = __shfl(root, leader);
    const unsigned long long same = __ballot(valid && root == r) & left;
    if (lane == leader) {
      const uint32_t n = (uint32_t)__popcll(same);
      if (first) { s_root[w] = r; s_cnt[w] = n; }
      else atomicAdd(a.size + r, n);
    }
    first = false;
    left &= ~same;
  }
  const bool p[2] = {bad, deg};
  const uint32_t n = mc_block_sums<2>(p);                             // (its barrier also publishes s_root / s_cnt)
  if (threadIdx.x < 2) mc_add(a.ctr + (threadIdx.x == 0 ? kMcBadIndex : kMcDegenerate), n);
  if (threadIdx.x == 2) {
#pragma unroll
    for (int q = 0; q < kMcBlock / 64; q++) {
      uint32_t c = s_cnt[q];
      if (!c) continue;
      for (int k = q + 1; k < kMcBlock / 64; k++)
        if (s_cnt[k] && s_root[k] == s_root[q]) { c += s_cnt[k]; s_cnt[k] = 0u; }
      atomicAdd(a.size + s_root[q], c);
    }
  }
}

// The components and the largest of them: the maximum of mc_best_word over the roots, a wave's maximum in one atomic.
__global__ void __launch_bounds__(kMcBlock) mc_roots_kernel(McArgs a) {
  const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
  uint32_t sz = 0u;
  if (i < (uint32_t)a.n_v && a.parent[i] == (int32_t)i) sz = a.size[i];
  unsigned long long best = sz ? mc_best_word(sz, (int32_t)i) : 0ull;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if ((threadIdx.x & 63) == 0 && best) atomicMax(&a.state->best, best);
  const bool p[1] = {sz != 0u};
  const uint32_t n = mc_block_sums<1>(p);
  if (threadIdx.x == 0) mc_add(a.ctr + kMcComponents, n);
}

// ---- group 2: the edge table. Every claimant of a key walks the same sequence and stops at the first slot that holds the key or is
// empty; a slot never changes its key, so all of them end in the same slot.
__global__ void __launch_bounds__(kMcBlock) mc_edge_kernel(McArgs a) {
  const uint32_t t = blockIdx.x * kMcBlock + threadIdx.x;
  if (t >= (uint32_t)a.n_t) return;
  int32_t v[3];
  mc_triangle(a, t, v);
  if (!mc_valid(v, a.n_v)) return;
  const uint32_t mask = a.eslots - 1u;
  uint32_t guard = 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int32_t p = v[c], q = v[c == 2 ? 0 : c + 1];
    if (p == q) continue;
    const unsigned long long key = mc_edge_key(p, q);
    uint32_t s = (uint32_t)mc_hash(key) & mask, trips = 0;
    for (;;) {
      unsigned long long cur = __hip_atomic_load(&a.ekeys[s], __ATOMIC_RELAXED, kMcScope);
      if (cur == kMcNoEdge) {
        __hip_atomic_compare_exchange_strong(&a.ekeys[s], &cur, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, kMcScope);
        if (cur == kMcNoEdge) cur = key;   // claimed; otherwise cur is the key that came first
      }
      if (cur == key) { atomicAdd(a.euse + s, 1u); break; }
      if (++trips >= a.eslots) { guard |= (uint32_t)kMcGuardEdgeProbe; break; }
      s = (s + 1u) & mask;
    }
  }
  if (guard) atomicOr(a.ctr + kMcGuard, (unsigned long long)guard);
}

// A thread per slot: the edges, those used once and those used more than twice, of the input and of what survives. An edge lies in
// one component: that of its smaller vertex.
__global__ void __launch_bounds__(kMcBlock) mc_census_kernel(McArgs a) {
  const uint32_t s = blockIdx.x * kMcBlock + threadIdx.x;
  bool edge = false, open = false, many = false, out = false;
  if (s < a.eslots) {
    const unsigned long long key = a.ekeys[s];
    if (key != kMcNoEdge) {
      const uint32_t use = a.euse[s];
      edge = true;
      open = use == 1u;
      many = use > 2u;
      out = mc_kept(a, a.parent[mc_edge_low(key)], a.state->best);
    }
  }
  const bool p[6] = {edge, open, many, edge && out, open && out, many && out};
  const uint32_t n = mc_block_sums<6>(p);
  if (threadIdx.x < 6) mc_add(a.ctr + kMcEdges + threadIdx.x, n);
}

// ---- group 3: the survivors and their per-block counts.
__global__ void __launch_bounds__(kMcBlock) mc_tri_keep_kernel(McArgs a) {
  const uint32_t t = blockIdx.x * kMcBlock + threadIdx.x;
  bool keep = false, removed = false;
  if (t < (uint32_t)a.n_t) {
    const int32_t label = a.label[t];
    if (label != kMcNoLabel) {
      keep = mc_kept(a, label, a.state->best);
      removed = !keep;
      if (keep) {
        int32_t v[3];
        mc_triangle(a, t, v);
        a.vref[v[0]] = 1; a.vref[v[1]] = 1; a.vref[v[2]] = 1;
      }
    }
  }
  const bool p[2] = {keep, removed};
  const uint32_t n = mc_block_sums<2>(p);
  if (threadIdx.x == 0) a.tblk[blockIdx.x] = n;
  else if (threadIdx.x == 1) mc_add(a.ctr + kMcRemovedTriangles, n);
}

// A vertex a valid triangle names stays or leaves with its component; one that none names stays unless unreferenced vertices are
// dropped.
__device__ __forceinline__ bool mc_vertex_kept(const McArgs& a, uint32_t i, bool* unreferenced, bool* removed, bool* removed_root) {
  const int32_t r = a.parent[i];
  const bool named = a.size[r] != 0u, keep = named ? a.vref[i] != 0 : !a.drop_unreferenced;
  *unreferenced = !named && !keep;
  *removed = named && !keep;
  *removed_root = *removed && r == (int32_t)i;
  return keep;
}

__global__ void __launch_bounds__(kMcBlock) mc_vertex_keep_kernel(McArgs a) {
  const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
  bool keep = false, unref = false, removed = false, root = false;
  if (i < (uint32_t)a.n_v) keep = mc_vertex_kept(a, i, &unref, &removed, &root);
  const bool p[4] = {keep, unref, removed, root};
  const uint32_t n = mc_block_sums<4>(p);
  if (threadIdx.x == 0) a.vblk[blockIdx.x] = n;
  else if (threadIdx.x < 4)
    mc_add(a.ctr + (threadIdx.x == 1 ? kMcUnreferenced : threadIdx.x == 2 ? kMcRemovedVertices : kMcRemovedComponents), n);
}

// ---- group 4: one block: both counts' exclusive offsets (volume_scan.hip.h), the result's counts, the run's counters.
__global__ void __launch_bounds__(kMcScanThreads) mc_scan_kernel(McArgs a) {
  const unsigned long long tv = scan_counts<kMcScanThreads, 1>(a.vblk, a.vblk_off, mc_blocks(a.n_v)).t[0];
  const unsigned long long tt = scan_counts<kMcScanThreads, 1>(a.tblk, a.tblk_off, mc_blocks(a.n_t)).t[0];
  if (threadIdx.x == 0) {
    a.state->n_v = (uint32_t)tv;
    a.state->n_t = (uint32_t)tt;
    a.ctr[kMcVerticesIn] = (unsigned long long)a.n_v;
    a.ctr[kMcTrianglesIn] = (unsigned long long)a.n_t;
    a.ctr[kMcVerticesOut] = tv;
    a.ctr[kMcTrianglesOut] = tt;
    a.ctr[kMcLargest] = mc_best_size(a.state->best);
  }
}

// ---- group 5: the kept vertices in ascending index with their own bytes; the surviving triangles in input order, in the new indices.
__global__ void __launch_bounds__(kMcBlock) mc_vertex_scatter_kernel(McArgs a) {
  __shared__ unsigned wsum[kMcBlock / 64];
  const uint32_t i = blockIdx.x * kMcBlock + threadIdx.x;
  bool u, r, q;
  const bool keep = i < (uint32_t)a.n_v && mc_vertex_kept(a, i, &u, &r, &q);
  const unsigned rank = scan_block<kMcBlock>(keep ? 1u : 0u, wsum).rank;
  if (i >= (uint32_t)a.n_v) return;
  const unsigned long long idx = a.vblk_off[blockIdx.x] + rank;
  a.vnew[i] = keep ? (int32_t)idx : -1;
  if (!keep) return;
  a.out_xyz0[idx] = a.in_xyz0[i];
  a.out_nrmw[idx] = a.in_nrmw[i];
  if (a.in_rgba) a.out_rgba[idx] = a.in_rgba[i];
}

__global__ void __launch_bounds__(kMcBlock) mc_tri_scatter_kernel(McArgs a) {
  __shared__ unsigned wsum[kMcBlock / 64];
  const uint32_t t = blockIdx.x * kMcBlock + threadIdx.x;
  bool keep = false;
  if (t < (uint32_t)a.n_t) {
    const int32_t label = a.label[t];
    keep = label != kMcNoLabel && mc_kept(a, label, a.state->best);
  }
  const unsigned rank = scan_block<kMcBlock>(keep ? 1u : 0u, wsum).rank;
  if (!keep) return;
  const unsigned long long idx = a.tblk_off[blockIdx.x] + rank;
  int32_t v[3];
  mc_triangle(a, t, v);
#pragma unroll
  for (int c = 0; c < 3; c++) a.out_tri[3 * idx + c] = a.vnew[v[c]];
}

void launch_mc_begin(McState* state, unsigned long long* ctr, hipStream_t s) {
  hipLaunchKernelGGL(mc_begin_kernel, dim3(1), dim3(64), 0, s, state, ctr);
}

int launch_mc_group(const McArgs& a, int group, hipStream_t s) {
  const dim3 block(kMcBlock), vgrid((unsigned)mc_blocks(a.n_v)), tgrid((unsigned)mc_blocks(a.n_t));
  const bool v = a.n_v > 0, t = a.n_t > 0;
  hipError_t e = hipSuccess;
  if (group == 0) {
    if (v) hipLaunchKernelGGL(mc_init_kernel, vgrid, block, 0, s, a);
    if (v && t) hipLaunchKernelGGL(mc_union_kernel, tgrid, block, 0, s, a);
  } else if (group == 1) {
    if (v) hipLaunchKernelGGL(mc_flatten_kernel, vgrid, block, 0, s, a);
    if (t) hipLaunchKernelGGL(mc_label_kernel, tgrid, block, 0, s, a);
    if (v) hipLaunchKernelGGL(mc_roots_kernel, vgrid, block, 0, s, a);
  } else if (group == 2) {
    if (a.eslots && v && t) {
      e = hipMemsetAsync(a.ekeys, 0xFF, sizeof(unsigned long long) * (size_t)a.eslots, s);
      if (e == hipSuccess) e = hipMemsetAsync(a.euse, 0, sizeof(uint32_t) * (size_t)a.eslots, s);
      hipLaunchKernelGGL(mc_edge_kernel, tgrid, block, 0, s, a);
      hipLaunchKernelGGL(mc_census_kernel, dim3((unsigned)mc_blocks((long long)a.eslots)), block, 0, s, a);
    }
  } else if (group == 3) {
    if (v) e = hipMemsetAsync(a.vref, 0, (size_t)a.n_v, s);
    if (t) hipLaunchKernelGGL(mc_tri_keep_kernel, tgrid, block, 0, s, a);
    if (v) hipLaunchKernelGGL(mc_vertex_keep_kernel, vgrid, block, 0, s, a);
  } else if (group == 4) {
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kMcScanThreads), 0, s, a);
  } else {
    if (v) hipLaunchKernelGGL(mc_vertex_scatter_kernel, vgrid, block, 0, s, a);
    if (t) hipLaunchKernelGGL(mc_tri_scatter_kernel, tgrid, block, 0, s, a);
  }
  return e == hipSuccess ? 0 : -1;
}

}  // namespace odo
