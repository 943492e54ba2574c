// tests/volume_mesh_table_harness.cpp — odometry_amd/csrc/volume_mesh_table.h (the marching-tetrahedra table of odo_volume_mesh)
// compiled on its own with g++: prints the paths, the direction codes and, for all 6 x 16 (tetrahedron, pattern) entries, the
// triangles as the lookup returns them; then the triangle count of every one of the 256 cell patterns.
//   path t c0 c1 c2 c3
//   dir e offset
//   entry t m n  (corner e) x 3 n
//   cell pos8 n
#include <cstdio>
#include "../odometry_amd/csrc/volume_mesh_table.h"

int main() {
  static constexpr odo::MtetTable T = odo::make_mtet_table();
  for (int t = 0; t < 6; t++)
    std::printf("path %d %d %d %d %d\n", t, odo::mtet_corner(t, 0), odo::mtet_corner(t, 1), odo::mtet_corner(t, 2), odo::mtet_corner(t, 3));
  for (int e = 0; e < 7; e++) {
    if (odo::mtet_offset_dir(odo::mtet_dir_offset(e)) != e) return 1;
    std::printf("dir %d %d\n", e, odo::mtet_dir_offset(e));
  }
  for (int t = 0; t < 6; t++)
    for (int m = 0; m < 16; m++) {
      const int n = odo::mtet_count(m);
      if (n != (int)T.e[t][m].n) return 1;
      std::printf("entry %d %d %d", t, m, n);
      for (int r = 0; r < n; r++)
        for (int x = 0; x < 3; x++) {
          int c, e;
          odo::mtet_lookup(T, t, m, r, x, &c, &e);
          std::printf(" %d %d", c, e);
        }
      std::printf("\n");
    }
  for (unsigned pos8 = 0; pos8 < 256; pos8++) std::printf("cell %u %d\n", pos8, odo::mtet_cell_count(pos8));
  std::printf("OK\n");
  return 0;
}
