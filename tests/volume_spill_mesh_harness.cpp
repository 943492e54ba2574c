// tests/volume_spill_mesh_harness.cpp — the mesh spill's predicates of odometry_amd/csrc/volume_shift_math.h (which cells and which
// edges a shift spills, which voxels are near the slab) compiled on their own with g++, the lines the device and the library compile.
//   IN OUT    IN: {int32 nx, ny, nz, dx, dy, dz}; OUT, all in raster order: uint8 near[n] per voxel; uint8 edge[n][7] per voxel and
//             direction e (2: the far end lies outside the grid and the predicate is not asked); uint8 cell[(nz-1)(ny-1)(nx-1)].
// Prints OK at the end.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../odometry_amd/csrc/volume_mesh_table.h"
#include "../odometry_amd/csrc/volume_shift_math.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t h[6];
  if (std::fread(h, sizeof(h), 1, in) != 1) return 2;
  const int nx = h[0], ny = h[1], nz = h[2], dx = h[3], dy = h[4], dz = h[5];
  std::vector<uint8_t> near, edge, cell;
  for (int k = 0; k < nz; k++)
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        near.push_back(odo::shift_near(i, j, k, dx, dy, dz, nx, ny, nz));
        for (int e = 0; e < 7; e++) {
          const int c = odo::mtet_dir_offset(e);   // c = dx + 2 dy + 4 dz of direction e
          const bool inside = i + (c & 1) < nx && j + ((c >> 1) & 1) < ny && k + ((c >> 2) & 1) < nz;
          edge.push_back(inside ? (uint8_t)odo::shift_edge_spilled(i, j, k, c, dx, dy, dz, nx, ny, nz) : (uint8_t)2);
        }
      }
  for (int k = 0; k + 1 < nz; k++)
    for (int j = 0; j + 1 < ny; j++)
      for (int i = 0; i + 1 < nx; i++) cell.push_back(odo::shift_cell_spilled(i, j, k, dx, dy, dz, nx, ny, nz));
  for (const auto* v : {&near, &edge, &cell})
    if (!v->empty() && std::fwrite(v->data(), 1, v->size(), out) != v->size()) return 2;
  std::fclose(in);
  if (std::fclose(out) != 0) return 2;
  std::puts("OK");
  return 0;
}
