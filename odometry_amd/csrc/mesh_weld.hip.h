// mesh_weld.hip.h — what the mesh welder's kernels (mesh_weld_kernels.hip, a translation unit of its own) and its host object
// (mesh_weld_api.hip.h, in the main unit) share: the launch constants, the launch arguments and the launcher.
// include/odometry_hip.h, odo_mesh_weld_create / DESIGN.md section 9.19; the rule is mesh_weld_math.h's.
//
// One pass = six groups of launches on one stream; a kernel boundary is the only barrier between them:
//   0  keys + vertex table   the vertex table cleared; weld_key_kernel: a thread per vertex computes its key, claims the key's slot
//                            with a 64-bit atomicCAS (linear probing from the splitmix64 finaliser) and lowers the slot's
//                            smallest-index word with atomicMin; the slot goes to vaux
//   1  representatives       weld_rep_kernel: rep[i] = the smallest index of vertex i's slot (i itself for a keyless vertex)
//   2  triangle remap+table  the triangle table cleared; weld_remap_kernel writes every triangle's rotated triple of representatives
//                            (or why it is dropped) to rtri; weld_tri_table_kernel claims an empty slot with atomicCAS(-1 -> t) or
//                            lowers a slot that holds the same triple with atomicMin; the slot goes to tslot
//   3  survivors             vref cleared; weld_tri_keep_kernel: triangle t survives iff its slot holds t, marks its three vertices
//                            and counts; weld_vertex_keep_kernel counts the kept vertices
//   4  scans                 weld_scan_kernel, one block: the offsets of both per-block counts (volume_scan.hip.h), the output's
//                            counts for the next pass, the run's counters
//   5  scatters              weld_vertex_scatter_kernel copies the kept vertices and leaves their new indices in vaux;
//                            weld_tri_scatter_kernel writes the surviving triangles in those indices
// A pass's vertex and triangle counts live on the device (WeldState): pass k + 1 is enqueued behind pass k without a host wait, with
// grids sized for the run's input, and blocks beyond the counts leave at once.
// Both probe loops carry a hard trip bound, the table's size; hitting it ORs a bit of kWeldGuard* into the guard counter and leaves
// the loop. No loop waits for another thread.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mesh_weld_math.h"

namespace odo {

constexpr int kWeldBlock = 256;                       // threads per workgroup of every per-vertex and per-triangle launch
constexpr int kWeldScanThreads = 1024;                // the one block of the scan
constexpr int kWeldGroups = 6;                        // timed groups of a pass
constexpr int kWeldMaxPasses = 8;

struct WeldState {
  uint32_t n_v, n_t;      // the counts a pass reads (state[k]) and writes (state[k + 1])
};

struct WeldArgs {
  // this pass's input (the caller's for pass 0, the previous pass's output otherwise) and output
  const float4* in_xyz0;
  const float4* in_nrmw;
  const uint32_t* in_rgba;        // NULL without colour
  const int32_t* in_tri;
  float4* out_xyz0;
  float4* out_nrmw;
  uint32_t* out_rgba;
  int32_t* out_tri;
  // tables
  unsigned long long* vkeys;      // [vslots]
  uint32_t* vmin;                 // [vslots]
  int32_t* ttab;                  // [tslots]
  // scratch
  int32_t* vaux;                  // [vertex_capacity] a vertex's slot (-1: none), later its index in the output
  int32_t* rep;                   // [vertex_capacity]
  uint8_t* vref;                  // [vertex_capacity] 1: named by a surviving triangle
  int32_t* rtri;                  // [3 triangle_capacity]
  int32_t* tslot;                 // [triangle_capacity]
  uint32_t* vblk;                 // per-block counts of kept vertices, of surviving triangles
  uint32_t* tblk;
  unsigned long long* vblk_off;   // their exclusive offsets
  unsigned long long* tblk_off;
  const WeldState* in;            // state[k]
  WeldState* out;                 // state[k + 1]
  unsigned long long* ctr;        // [kWeldStatWords]
  uint32_t vslots, tslots;        // powers of two
  float inv, ox, oy, oz;
  int grid, drop_unreferenced;
  int first, last;                // the run's first / last pass: vertices_in and triangles_in, vertices_out and triangles_out
  int n_v_max, n_t_max;           // the run's input counts: the launches' sizes
};

inline int weld_blocks(int n) { return (n + kWeldBlock - 1) / kWeldBlock; }

// One thread: state[0] = the run's counts, the counters zeroed.
void launch_weld_begin(WeldState* state0, unsigned long long* ctr, int n_v, int n_t, hipStream_t s);
// group: 0 .. kWeldGroups - 1 as above, memsets included. Nothing is launched for a count of 0.
int launch_weld_group(const WeldArgs& a, int group, hipStream_t s);

}  // namespace odo
