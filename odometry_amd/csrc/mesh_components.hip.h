// mesh_components.hip.h — what the mesh component filter's kernels (mesh_components_kernels.hip, a translation unit of its own) and its
// host object (mesh_components_api.hip.h, in the main unit) share: the launch constants, the launch arguments and the launcher.
// include/odometry_hip.h, odo_mesh_components_create / DESIGN.md section 9.20; the rule is mesh_components_math.h's.
//
// One run = six groups of launches on one stream; a kernel boundary is the only barrier between them:
//   0  union                 mc_init_kernel: parent[i] = i; mc_union_kernel: a thread per valid triangle unites v0 - v1 and
//                            v0 - v2: the larger root goes under the smaller with atomicMin, a lost race goes on from the word it read
//                            (the speckle filter's scheme, speckle_kernels.hip); both vertices are then pointed at that root
//   1  flatten + sizes       mc_flatten_kernel: parent[i] = root(i), size[i] = 0; mc_label_kernel: a valid triangle's label = parent[v0], 1 added
//                            to its root's size — a wave elects one lane per distinct root, a block merges its waves' first roots —
//                            and bad_index / degenerate counted; mc_roots_kernel: the components counted, the largest found with a
//                            64-bit atomicMax of size << 32 | ~label, one per wave
//   2  edge table + census   (only with edge statistics) the table cleared; mc_edge_kernel: a valid triangle's edges a != b claim the
//                            slot of min << 32 | max with a 64-bit atomicCAS (linear probing from the splitmix64 finaliser) and add 1
//                            to its use count; mc_census_kernel: a thread per slot, six counts per block, one atomicAdd per block and
//                            counter
//   3  survivors             vref cleared; mc_tri_keep_kernel: a triangle survives with its component, marks its three vertices
//                            (plain byte stores) and counts; mc_vertex_keep_kernel counts the kept vertices, the removed ones and
//                            the removed components
//   4  scans                 mc_scan_kernel, one block: the offsets of both per-block counts (volume_scan.hip.h), the result's
//                            counts, the run's counters
//   5  scatters              mc_vertex_scatter_kernel copies the kept vertices and leaves their new indices in vnew;
//                            mc_tri_scatter_kernel writes the surviving triangles in those indices
// Every data-dependent loop carries a hard trip bound — n_v for a walk to a root and for a union, the table's size for a probe;
// hitting it ORs a bit of kMcGuard* into the guard counter and leaves the loop. No loop waits for another thread.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mesh_components_math.h"

namespace odo {

constexpr int kMcBlock = 256;                         // threads per workgroup of every per-vertex, per-triangle and per-slot launch
constexpr int kMcScanThreads = 1024;                  // the one block of the scan
constexpr int kMcGroups = 6;                          // timed groups of a run

struct McState {
  uint32_t n_v, n_t;               // the last run's result counts
  unsigned long long best;         // mc_best_word of the largest component, 0 without one
};

struct McArgs {
  const float4* in_xyz0;
  const float4* in_nrmw;
  const uint32_t* in_rgba;         // NULL without colour
  const int32_t* in_tri;
  float4* out_xyz0;
  float4* out_nrmw;
  uint32_t* out_rgba;
  int32_t* out_tri;
  int32_t* parent;                 // [vertex_capacity]
  uint32_t* size;                  // [vertex_capacity] at a root: its component's valid triangles
  int32_t* vnew;                   // [vertex_capacity] a vertex's index in the output, -1: none
  uint8_t* vref;                   // [vertex_capacity] 1: named by a surviving triangle
  int32_t* label;                  // [triangle_capacity]
  unsigned long long* ekeys;       // [eslots] NULL without edge statistics
  uint32_t* euse;                  // [eslots]
  uint32_t* vblk;                  // per-block counts of kept vertices, of surviving triangles
  uint32_t* tblk;
  unsigned long long* vblk_off;    // their exclusive offsets
  unsigned long long* tblk_off;
  McState* state;
  unsigned long long* ctr;         // [kMcStatWords]
  uint32_t eslots;                 // a power of two; 0 without edge statistics
  int n_v, n_t;                    // the run's input counts: the launches' sizes
  int min_triangles, keep_largest, drop_unreferenced;
};

__host__ __device__ inline int mc_blocks(long long n) { return (int)((n + kMcBlock - 1) / kMcBlock); }

// One block: the result's counts, the largest and the counters zeroed.
void launch_mc_begin(McState* state, unsigned long long* ctr, hipStream_t s);
// group: 0 .. kMcGroups - 1 as above, memsets included. Nothing is launched for a count of 0. 0, or -1 if a clear failed.
int launch_mc_group(const McArgs& a, int group, hipStream_t s);

}  // namespace odo
