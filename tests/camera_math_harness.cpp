// tests/camera_math_harness.cpp — odometry_amd/csrc/camera_math.h (the map entry, the remapped pixel and the host-side coefficients of
// the camera model) compiled on its own with g++, the lines the device compiles. tests/test_camera_cases_cpu.py builds it with
// -fsanitize=address,undefined,float-cast-overflow and, from mutated copies of the header (-DCAMERA_MATH_H=...), the mutants.
//   maps IN OUT    IN: records {double raw[5], dist[4], R[9], P[12]; int32 rows, cols}; OUT per record: int32 status (0, or -1 for a
//                  singular P[:, :3] * R) and, for status 0, mapx then mapy (rows x cols float each).
//   remap IN OUT   IN: records {int32 srows, scols, drows, dcols; float border; float src[srows * scols], mapx[drows * dcols],
//                  mapy[drows * dcols]}; OUT per record: float dst[drows * dcols].
// The loader reads the source through a bounds check of its own, so a tap that reached outside the source would abort here (and under
// AddressSanitizer in any case: the source is on the heap).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#ifndef CAMERA_MATH_H
#define CAMERA_MATH_H "../odometry_amd/csrc/camera_math.h"
#endif
#include CAMERA_MATH_H

struct MapRec {
  double raw[5], dist[4], R[9], P[12];
  int32_t rows, cols;
};
struct RemapHead {
  int32_t srows, scols, drows, dcols;
  float border;
};

struct HostLoad {
  const float* p;
  size_t n;
  float operator()(size_t i) const {
    if (i >= n) std::abort();
    return p[i];
  }
};

static bool read_floats(std::FILE* f, std::vector<float>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(float), n, f) == n;
}

static int maps(std::FILE* in, std::FILE* out) {
  MapRec r;
  while (std::fread(&r, sizeof(r), 1, in) == 1) {
    if (r.rows < 1 || r.cols < 1) return 4;
    odo::CamCoef k;
    const int32_t status = odo::cam_coef(r.raw, r.dist, r.R, r.P, &k) ? 0 : -1;
    if (std::fwrite(&status, sizeof(status), 1, out) != 1) return 2;
    if (status) continue;
    const size_t n = (size_t)r.rows * r.cols;
    std::vector<float> mx(n), my(n);
    for (int v = 0; v < r.rows; v++)
      for (int u = 0; u < r.cols; u++) odo::undistort_map_entry(k, u, v, &mx[(size_t)v * r.cols + u], &my[(size_t)v * r.cols + u]);
    if (std::fwrite(mx.data(), sizeof(float), n, out) != n || std::fwrite(my.data(), sizeof(float), n, out) != n) return 2;
  }
  return 0;
}

static int remap(std::FILE* in, std::FILE* out) {
  RemapHead h;
  std::vector<float> src, mx, my, dst;
  while (std::fread(&h, sizeof(h), 1, in) == 1) {
    if (h.srows < 1 || h.scols < 1 || h.drows < 1 || h.dcols < 1) return 4;
    const size_t ns = (size_t)h.srows * h.scols, nd = (size_t)h.drows * h.dcols;
    if (!read_floats(in, src, ns) || !read_floats(in, mx, nd) || !read_floats(in, my, nd)) return 4;
    const HostLoad load = {src.data(), src.size()};
    dst.resize(nd);
    for (size_t o = 0; o < nd; o++) dst[o] = odo::remap_bilinear_pixel(load, h.srows, h.scols, mx[o], my[o], h.border);
    if (std::fwrite(dst.data(), sizeof(float), nd, out) != nd) return 2;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 3;
  std::FILE* in = std::fopen(argv[2], "rb");
  std::FILE* out = std::fopen(argv[3], "wb");
  if (!in || !out) return 2;
  int st = 3;
  if (!std::strcmp(argv[1], "maps")) st = maps(in, out);
  else if (!std::strcmp(argv[1], "remap")) st = remap(in, out);
  std::fclose(in);
  if (std::fclose(out)) return 2;
  if (st == 0) std::printf("OK\n");
  return st;
}
