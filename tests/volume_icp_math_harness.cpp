// tests/volume_icp_math_harness.cpp — odometry_amd/csrc/volume_icp_math.h (the row, the step and the eigenvalues of the TSDF volume's
// frame-to-model alignment) and the host part hostfp::icp_frame / hostfp::mul4 of odometry_amd/csrc/host_fp.h compiled on their own
// with g++, the lines the device and the library compile. Two builds of this one file (tests/test_volume_icp_cpu.py):
//   a shared library (icp_host_rows, icp_host_step, icp_host_eigenvalues, icp_host_frame) for ctypes, and
//   a stand-alone program with AddressSanitizer and UBSan that runs the same four functions over files:
//     rows IN OUT    IN: {int32 rows, cols, stride; float f, cx, cy, depth_scale, max_depth, dist_max, huber_delta; float M[16], C[16]
//                    (column-major)} then raw uint16[rows cols], depth float[rows cols], nrmw float[rows cols 4];
//                    OUT: float[rows cols 8] then double acc[29] (accumulate_row over the stride's pixels in raster order)
//     step IN OUT    IN: records {double acc[29]; float C[16]; int32 min_pairs; float eps_t, eps_r; int32 pad};
//                    OUT: per record {int32 failed, converged; float delta[6]; float C[16]}
//     eig IN OUT     IN: records double acc[29]; OUT: per record double ev[6]
//     frame IN OUT   IN: records {float P_m[16], P_init[16]}; OUT: per record {float M[16], C0[16], back[16]}, back = mul4(P_m, C0)
// The frames are copied to the heap at their exact size, so a row that read outside one would be AddressSanitizer's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../odometry_amd/csrc/host_fp.h"
#include "../odometry_amd/csrc/volume_icp_math.h"

struct RowsHead {
  int32_t rows, cols, stride;
  float f, cx, cy, depth_scale, max_depth, dist_max, huber_delta;
  float M[16], C[16];
};
struct StepRec {
  double acc[ODO_NACC];
  float C[16];
  int32_t min_pairs;
  float eps_t, eps_r;
  int32_t pad;
};
struct StepOut {
  int32_t failed, converged;
  float delta[6];
  float C[16];
};

extern "C" void icp_host_rows(const RowsHead* h, const uint16_t* raw, const float* depth, const float* nrmw, float* rows8, double* acc) {
  odo::IcpView v;
  v.rows = h->rows; v.cols = h->cols; v.f = h->f; v.cx = h->cx; v.cy = h->cy;
  v.depth_scale = h->depth_scale; v.max_depth = h->max_depth; v.dist_max = h->dist_max; v.huber_delta = h->huber_delta;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) v.m[3 * r + c] = h->M[4 * c + r];
  for (int i = 0; i < ODO_NACC; i++) acc[i] = 0.0;
  std::memset(rows8, 0, sizeof(float) * 8 * (size_t)h->rows * h->cols);
  for (int y = 0; y < h->rows; y += h->stride)
    for (int x = 0; x < h->cols; x += h->stride) {
      float J[6], res, w;
      if (!odo::icp_row(v, h->C, raw, depth, nrmw, x, y, J, &res, &w)) continue;
      float* o = rows8 + 8 * ((size_t)y * h->cols + x);
      for (int i = 0; i < 6; i++) o[i] = J[i];
      o[6] = res; o[7] = w;
      odo::accumulate_row(acc, res, w, J);
      // the kernels' form of the same terms
      double one[ODO_NACC] = {0.0};
      odo::accumulate_row(one, res, w, J);
      for (int q = 0; q < ODO_NACC - 1; q++) {
        int ia, ib;
        odo::icp_term_operands(q, &ia, &ib);
        const double term = odo::icp_term(o, ia, ib);
        if (term != one[q] && !(term != term && one[q] != one[q])) std::abort();   // (equal, or both NaN)
      }
    }
}

extern "C" void icp_host_step(const StepRec* r, StepOut* o) {
  std::memcpy(o->C, r->C, sizeof(o->C));
  int converged = 0;
  o->failed = odo::icp_step(r->acc, r->min_pairs, r->eps_t, r->eps_r, o->C, o->delta, &converged);
  o->converged = converged;
}

extern "C" void icp_host_eigenvalues(const double* acc, double* ev) { odo::icp_eigenvalues(acc, ev); }

extern "C" void icp_host_frame(const float* P_m, const float* P_init, float* out48) {
  hostfp::icp_frame(P_m, P_init, out48, out48 + 16);
  hostfp::mul4(P_m, out48 + 16, out48 + 32);
}

#ifndef ICP_HARNESS_LIBRARY
template <class T>
static bool read_all(const char* path, std::vector<T>* v) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  T t;
  while (std::fread(&t, sizeof(T), 1, f) == 1) v->push_back(t);
  std::fclose(f);
  return true;
}
template <class T>
static int write_all(const char* path, const std::vector<T>& v) {
  std::FILE* f = std::fopen(path, "wb");
  if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size() || std::fclose(f)) return 2;
  std::printf("OK\n");
  return 0;
}

static int rows_mode(const char* in, const char* out_path) {
  std::FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  RowsHead h;
  if (std::fread(&h, sizeof(h), 1, f) != 1 || h.rows < 1 || h.cols < 1 || h.stride < 1) return 2;
  const size_t n = (size_t)h.rows * h.cols;
  std::vector<uint16_t> raw(n);
  std::vector<float> depth(n), nrmw(4 * n), rows8(8 * n);
  if (std::fread(raw.data(), 2, n, f) != n || std::fread(depth.data(), 4, n, f) != n || std::fread(nrmw.data(), 4, 4 * n, f) != 4 * n) return 2;
  std::fclose(f);
  double acc[ODO_NACC];
  icp_host_rows(&h, raw.data(), depth.data(), nrmw.data(), rows8.data(), acc);
  f = std::fopen(out_path, "wb");
  if (!f || std::fwrite(rows8.data(), 4, 8 * n, f) != 8 * n || std::fwrite(acc, 8, ODO_NACC, f) != ODO_NACC || std::fclose(f)) return 2;
  std::printf("OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 3;
  if (!std::strcmp(argv[1], "rows")) return rows_mode(argv[2], argv[3]);
  if (!std::strcmp(argv[1], "step")) {
    std::vector<StepRec> in;
    if (!read_all(argv[2], &in)) return 2;
    std::vector<StepOut> out(in.size());
    for (size_t i = 0; i < in.size(); i++) icp_host_step(&in[i], &out[i]);
    return write_all(argv[3], out);
  }
  if (!std::strcmp(argv[1], "eig")) {
    struct Acc { double a[ODO_NACC]; };
    struct Ev { double e[6]; };
    std::vector<Acc> in;
    if (!read_all(argv[2], &in)) return 2;
    std::vector<Ev> out(in.size());
    for (size_t i = 0; i < in.size(); i++) icp_host_eigenvalues(in[i].a, out[i].e);
    return write_all(argv[3], out);
  }
  if (!std::strcmp(argv[1], "frame")) {
    struct In { float P_m[16], P_init[16]; };
    struct Out { float o[48]; };
    std::vector<In> in;
    if (!read_all(argv[2], &in)) return 2;
    std::vector<Out> out(in.size());
    for (size_t i = 0; i < in.size(); i++) icp_host_frame(in[i].P_m, in[i].P_init, out[i].o);
    return write_all(argv[3], out);
  }
  return 3;
}
#endif
