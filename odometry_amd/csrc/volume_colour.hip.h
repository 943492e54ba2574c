// volume_colour.hip.h — what the TSDF volume's colour kernels (volume_colour_kernels.hip, a translation unit of their own) and the
// host object (volume_api.hip.h, in the main unit) share: the launch arguments and the launchers.
//
// The colour grid is a second array beside the voxel grid, one 32-bit word per voxel in the same raster order: uint8 R, G, B (bytes
// 0, 1, 2) and uint8 wc (byte 3: the colour weight, 0 = never coloured). include/odometry_hip.h / DESIGN.md section 9.6.
//
// The coloured integration is volume_kernels.hip's (volume.hip.h: one body for the plain and the coloured kernel).
// Colours of extracted points / mesh vertices = one launch behind the unchanged extraction / mesh launches, on the volume's stream: a
// thread per voxel rebuilds the index of its first point (the extraction's wave ballots and block offsets; the mesh's per-voxel
// vertex base and edge mask) and writes one dword per point. No atomics; the order does not depend on timing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "volume.hip.h"
#include "volume_mesh.hip.h"

namespace odo {

struct VolExtractColourArgs {
  VolExtractArgs a;       // what launch_volume_extract was given: wave_mask and blk_off are read, xyz0 / nrmw are not
  const uint32_t* col;
  uint32_t* rgba;         // [capacity]
};

struct VolMeshColourArgs {
  VolMeshArgs a;          // what launch_volume_mesh_emit was given: edge_mask and vertex_base are read
  const uint32_t* col;
  uint32_t* rgba;         // [vertex_capacity]
};

void launch_volume_extract_colour(const VolExtractColourArgs& a, hipStream_t s);
void launch_volume_mesh_colour(const VolMeshColourArgs& a, hipStream_t s);

}  // namespace odo
