// tests/volume_shift_harness.cpp — odometry_amd/csrc/volume_shift_math.h (where a shifted voxel comes from, which voxels leave, how far
// the window may travel, the shift that follows a pose) and host_fp.h's window_origin compiled on their own with g++, the lines the
// device and the library compile.
//   shift IN OUT    IN: {int32 nx, ny, nz, dx, dy, dz, has_col; uint32 vox[n]; uint32 col[n] if has_col}; OUT: uint32 vox'[n], uint32
//                   col'[n] if has_col, uint8 leaves[n]: the shifted grids and the predicate per OLD voxel, in raster order.
//   follow IN OUT   IN: {int32 count; count x Row}; OUT: count x Out: the window's origin for (origin0, off), the follow rule's
//                   shift for the pose in that window, the new cumulative shift off + d_try and its origin.
// Every mode prints OK at the end. The grids are plain arrays on the heap: a read outside them is AddressSanitizer's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../odometry_amd/csrc/host_fp.h"
#include "../odometry_amd/csrc/volume_shift_math.h"

struct Row {
  float pose[16];   // column-major
  float origin0[3];
  int32_t off[3], n[3];
  float vs, focus;
  int32_t threshold, d_try[3];
};
struct Out {
  float origin[3];
  int32_t follow_ok, d[3];
  int32_t offset_ok, off_new[3];
  float origin_new[3];
};

template <class T>
static bool read_n(std::FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}

static int shift(std::FILE* in, std::FILE* out) {
  int32_t h[7];
  if (std::fread(h, sizeof(h), 1, in) != 1) return 2;
  const int nx = h[0], ny = h[1], nz = h[2], d[3] = {h[3], h[4], h[5]};
  const size_t n = (size_t)nx * ny * nz;
  std::vector<uint32_t> src[2], dst[2];
  for (int g = 0; g < (h[6] ? 2 : 1); g++) {
    if (!read_n(in, &src[g], n)) return 2;
    dst[g].assign(n, 0xABABABABu);
  }
  std::vector<uint8_t> leaves(n);
  for (int k = 0; k < nz; k++)
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        const size_t v = ((size_t)k * ny + j) * nx + i;
        int si, sj, sk;
        const bool inside = odo::shift_source(i, d[0], nx, &si) & odo::shift_source(j, d[1], ny, &sj) & odo::shift_source(k, d[2], nz, &sk);
        for (int g = 0; g < (h[6] ? 2 : 1); g++) dst[g].at(v) = inside ? src[g].at(((size_t)sk * ny + sj) * nx + si) : 0u;
        leaves.at(v) = odo::shift_leaves(i, d[0], nx) || odo::shift_leaves(j, d[1], ny) || odo::shift_leaves(k, d[2], nz);
      }
  for (int g = 0; g < (h[6] ? 2 : 1); g++)
    if (std::fwrite(dst[g].data(), sizeof(uint32_t), n, out) != n) return 2;
  return std::fwrite(leaves.data(), 1, n, out) == n ? 0 : 2;
}

static int follow(std::FILE* in, std::FILE* out) {
  int32_t count;
  std::vector<Row> rows;
  if (std::fread(&count, sizeof(count), 1, in) != 1 || count < 0 || !read_n(in, &rows, (size_t)count)) return 2;
  for (const Row& r : rows) {
    Out o;
    std::memset(&o, 0, sizeof(o));
    hostfp::window_origin(r.origin0, r.off, r.vs, o.origin);
    o.follow_ok = odo::follow_shift(r.pose, o.origin, r.n, r.vs, r.focus, r.threshold, o.d);
    o.offset_ok = 1;
    for (int c = 0; c < 3; c++) o.offset_ok &= (int32_t)odo::shift_offset(r.off[c], r.d_try[c], &o.off_new[c]);
    if (o.offset_ok) hostfp::window_origin(r.origin0, o.off_new, r.vs, o.origin_new);
    else std::memset(o.off_new, 0, sizeof(o.off_new));
    if (std::fwrite(&o, sizeof(o), 1, out) != 1) return 2;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 3;
  std::FILE* in = std::fopen(argv[2], "rb");
  std::FILE* out = std::fopen(argv[3], "wb");
  if (!in || !out) return 2;
  int rc = 3;
  if (!std::strcmp(argv[1], "shift")) rc = shift(in, out);
  else if (!std::strcmp(argv[1], "follow")) rc = follow(in, out);
  std::fclose(in);
  if (std::fclose(out)) rc = 2;
  if (rc == 0) std::printf("OK\n");
  return rc;
}
