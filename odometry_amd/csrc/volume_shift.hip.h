// volume_shift.hip.h — what the moving TSDF volume's kernels (volume_shift_kernels.hip, a translation unit of their own) and the host
// object (volume_shift_api.hip.h, in the main unit) share: the launch arguments, the spill store's counters and the launchers.
// include/odometry_hip.h, odo_volume_shift / DESIGN.md section 9.9; the rules are volume_shift_math.h's.
//
// One shift = one launch: a thread per four x-consecutive voxels of the NEW grid writes their words (and colour words) into a second
// pair of buffers, the old voxels d away or 0. The stores are the aligned side — a wave stores 1 KiB of a row — and the loads are off by
// dx words; j, k and the quad come from the launch geometry (64 lanes along the row, 4 rows per block, planes in y), no division;
// no atomics: a destination word is a pure function of the old grid. The host swaps the buffers when it enqueues.
// One spill, in front of the shift when the volume has a store = four launches, the extraction's shape over the PRE-shift grid: count
// (the extraction's three ballots per wave, each edge ANDed with "a or b leaves"), scan (one block: the blocks' exclusive offsets and
// the sum), scatter (points, normals and colours at the store's `written` + block offset + rank, clamped at capacity), advance (one
// thread: written and total move on). Whole grid, not only the leaving slabs: the output order (voxel a in raster order, axis) and
// the extraction's scratch and index arithmetic come for free, and a count over voxels that stay is one coalesced read of the grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "volume.hip.h"
#include "volume_mesh.hip.h"

namespace odo {

constexpr int kVolShiftLanes = 64;    // the shift's block: one wave along a row (four voxels per thread) ...
constexpr int kVolShiftRows = 4;      // ... by four rows
constexpr int kVolShiftBlock = kVolShiftLanes * kVolShiftRows;

// Device-resident counters of one spill store.
struct VolSpillCounters {
  unsigned long long written;   // points in the store (<= capacity)
  unsigned long long total;     // points that qualified since enable / clear; total - written were dropped
  unsigned long long pending;   // the points of the last spill enqueued (scan -> advance)
};

struct VolShiftArgs {
  const uint32_t* src;       // [n]: the old grid
  uint32_t* dst;             // [n]: the new one
  const uint32_t* src_col;   // the colour grids likewise, nullptr: no colour
  uint32_t* dst_col;
  int nx, ny, nz, n;
  int dx, dy, dz;
};

struct VolSpillArgs {
  VolExtractArgs a;          // the pre-shift grid and the extraction's scratch; capacity, xyz0, nrmw = the store's; ctr unused
  int dx, dy, dz;
  const uint32_t* col;       // the pre-shift colour grid, nullptr: no colour
  uint32_t* rgba;            // [capacity], nullptr: no colour
  VolSpillCounters* sc;
};

// ---- the mesh of the leaving slab -----------------------------------------------------------------------------
// One mesh spill, in front of the shift when the volume has a mesh store = five launches (six with colour), the mesh's shape over the
// PRE-shift grid with volume_shift_math.h's two predicates ANDed in: count (edge mask & "edge spilled", triangle count * "cell spilled"),
// scan (both block sums; the spill's two counts are left in the store's counters), vertices and triangles (both take their base from
// the store's `written` counters, so a triangle's indices are the store's), colour, advance (one thread). No host wait.
// Work follows the slab: a thread whose voxel is more than one voxel from every leaving voxel (shift_near) loads nothing, and a block
// without such a voxel returns after writing its two zero counts; block order and output order stay the mesh's.
// A spill is appended whole or not at all: every emitting block reads the same four counters and writes nothing unless both of the
// spill's counts fit what is left, so the store is a complete mesh of every spill it holds. (odo_volume_mesh differs: it never remaps
// indices and its triangles may name vertices beyond the vertex capacity.)
struct VolSpillMeshCounters {
  unsigned long long v_written, t_written;   // vertices / triangles in the store (<= the capacities)
  unsigned long long v_total, t_total;       // those that qualified since enable / clear; total - written were dropped
  unsigned long long v_pending, t_pending;   // the counts of the last spill enqueued (scan -> emit, advance)
};

struct VolSpillMeshArgs {
  VolMeshArgs a;             // the pre-shift grid and the mesh's scratch; capacities, xyz0, nrmw, tri = the store's; ctr unused
  int dx, dy, dz;
  const uint32_t* col;       // the pre-shift colour grid, nullptr: no colour
  uint32_t* rgba;            // [vertex_capacity], nullptr: no colour
  VolSpillMeshCounters* sc;
};

void launch_volume_spill_mesh(const VolSpillMeshArgs& a, hipStream_t s);   // count, scan, vertices, triangles, colour, advance
void launch_volume_spill_mesh_stage(const VolSpillMeshArgs& a, int stage, hipStream_t s);   // count (0) .. colour (4): timing

void launch_volume_shift(const VolShiftArgs& a, hipStream_t s);
void launch_volume_spill(const VolSpillArgs& a, hipStream_t s);   // count, scan, scatter, advance
void launch_volume_spill_stage(const VolSpillArgs& a, int stage, hipStream_t s);   // one of count (0), scan (1), scatter (2): timing

}  // namespace odo
