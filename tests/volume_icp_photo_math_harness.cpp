// tests/volume_icp_photo_math_harness.cpp — odometry_amd/csrc/volume_icp_photo_math.h (the photometric row of the TSDF volume's
// frame-to-model alignment and the 31 sums) over volume_icp_math.h, compiled on its own with g++: the lines the device and the
// library compile. Two builds of this one file (tests/test_volume_icp_photo_cpu.py), as tests/volume_icp_math_harness.cpp has:
//   a shared library (icp_photo_host_rows, icp_photo_host_step) for ctypes, and
//   a stand-alone program with AddressSanitizer and UBSan that runs the same functions over files:
//     rows IN OUT    IN: {int32 rows, cols, stride; float f, cx, cy, depth_scale, max_depth, dist_max, huber_delta, photo_weight,
//                    photo_huber; float M[16], C[16] (column-major)} then raw uint16[rows cols], grey float[rows cols], depth
//                    float[rows cols], nrmw float[rows cols 4], rgba uint8[rows cols 4];
//                    OUT: float[rows cols 16] then double acc[31] (over the stride's pixels in raster order, per pixel the
//                    geometric row and then the photometric one)
//     step IN OUT    IN: records {double acc[31]; float C[16]; int32 min_pairs; float eps_t, eps_r; int32 pad};
//                    OUT: per record {int32 failed, converged; float delta[6]; float C[16]} of icp_step on the first 29
// The frames are copied to the heap at their exact size, so a row that read outside one would be AddressSanitizer's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../odometry_amd/csrc/volume_icp_photo_math.h"

struct PhotoHead {
  int32_t rows, cols, stride;
  float f, cx, cy, depth_scale, max_depth, dist_max, huber_delta, photo_weight, photo_huber;
  float M[16], C[16];
};
struct PhotoStepRec {
  double acc[odo::kIcpPhotoAcc];
  float C[16];
  int32_t min_pairs;
  float eps_t, eps_r;
  int32_t pad;
};
struct PhotoStepOut {
  int32_t failed, converged;
  float delta[6];
  float C[16];
};

extern "C" void icp_photo_host_rows(const PhotoHead* h, const uint16_t* raw, const float* grey, const float* depth, const float* nrmw,
                                    const uint32_t* rgba, float* rows16, double* acc) {
  odo::IcpView v;
  v.rows = h->rows; v.cols = h->cols; v.f = h->f; v.cx = h->cx; v.cy = h->cy;
  v.depth_scale = h->depth_scale; v.max_depth = h->max_depth; v.dist_max = h->dist_max; v.huber_delta = h->huber_delta;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) v.m[3 * r + c] = h->M[4 * c + r];
  odo::IcpPhotoView ph;
  ph.weight = h->photo_weight; ph.huber_delta = h->photo_huber;
  for (int i = 0; i < odo::kIcpPhotoAcc; i++) acc[i] = 0.0;
  std::memset(rows16, 0, sizeof(float) * 16 * (size_t)h->rows * h->cols);
  for (int y = 0; y < h->rows; y += h->stride)
    for (int x = 0; x < h->cols; x += h->stride) {
      float* o = rows16 + 16 * ((size_t)y * h->cols + x);
      float J[6], res, w;
      if (odo::icp_row(v, h->C, raw, depth, nrmw, x, y, J, &res, &w)) {
        for (int i = 0; i < 6; i++) o[i] = J[i];
        o[6] = res; o[7] = w;
        odo::icp_photo_accumulate(acc, o, false);
        // accumulate_row's form of the same terms
        double one[ODO_NACC] = {0.0}, two[odo::kIcpPhotoAcc] = {0.0};
        odo::accumulate_row(one, res, w, J);
        odo::icp_photo_accumulate(two, o, false);
        for (int q = 0; q < ODO_NACC; q++)
          if (two[q] != one[q] && !(two[q] != two[q] && one[q] != one[q])) std::abort();   // (equal, or both NaN)
      }
      if (odo::icp_photo_row(v, ph, h->C, raw, grey, depth, rgba, x, y, J, &res, &w)) {
        for (int i = 0; i < 6; i++) o[8 + i] = J[i];
        o[14] = res; o[15] = w;
        odo::icp_photo_accumulate(acc, o + 8, true);
      }
    }
}

extern "C" void icp_photo_host_step(const PhotoStepRec* r, PhotoStepOut* o) {
  std::memcpy(o->C, r->C, sizeof(o->C));
  int converged = 0;
  o->failed = odo::icp_step(r->acc, r->min_pairs, r->eps_t, r->eps_r, o->C, o->delta, &converged);
  o->converged = converged;
}

#ifndef ICP_HARNESS_LIBRARY
static int rows_mode(const char* in, const char* out_path) {
  std::FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  PhotoHead h;
  if (std::fread(&h, sizeof(h), 1, f) != 1 || h.rows < 1 || h.cols < 1 || h.stride < 1) return 2;
  const size_t n = (size_t)h.rows * h.cols;
  std::vector<uint16_t> raw(n);
  std::vector<float> grey(n), depth(n), nrmw(4 * n), rows16(16 * n);
  std::vector<uint32_t> rgba(n);
  if (std::fread(raw.data(), 2, n, f) != n || std::fread(grey.data(), 4, n, f) != n || std::fread(depth.data(), 4, n, f) != n ||
      std::fread(nrmw.data(), 4, 4 * n, f) != 4 * n || std::fread(rgba.data(), 4, n, f) != n)
    return 2;
  std::fclose(f);
  double acc[odo::kIcpPhotoAcc];
  icp_photo_host_rows(&h, raw.data(), grey.data(), depth.data(), nrmw.data(), rgba.data(), rows16.data(), acc);
  f = std::fopen(out_path, "wb");
  if (!f || std::fwrite(rows16.data(), 4, 16 * n, f) != 16 * n || std::fwrite(acc, 8, odo::kIcpPhotoAcc, f) != (size_t)odo::kIcpPhotoAcc ||
      std::fclose(f))
    return 2;
  std::printf("OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 3;
  if (!std::strcmp(argv[1], "rows")) return rows_mode(argv[2], argv[3]);
  if (!std::strcmp(argv[1], "step")) {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<PhotoStepRec> in;
    PhotoStepRec t;
    while (std::fread(&t, sizeof(t), 1, f) == 1) in.push_back(t);
    std::fclose(f);
    std::vector<PhotoStepOut> out(in.size());
    for (size_t i = 0; i < in.size(); i++) icp_photo_host_step(&in[i], &out[i]);
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), sizeof(PhotoStepOut), out.size(), f) != out.size() || std::fclose(f)) return 2;
    std::printf("OK\n");
    return 0;
  }
  return 3;
}
#endif
