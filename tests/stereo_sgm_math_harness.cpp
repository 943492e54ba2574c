// The semi-global mode's host + device header (odometry_amd/csrc/stereo_sgm_math.h, over stereo_depth_math.h) as a stand-alone
// program for g++, built with -fsanitize=address,undefined by tests/test_stereo_sgm_cpu.py: every frame, plane and volume lives in a
// heap block of exactly its size, so an entry read or written outside a volume is reported.
//   stereo_sgm_math_harness <in> <out>
// in:  records of int32 rows, cols, dmin, dmax, A, uniq, lr_max, max_raw, p1, p2, paths; double fx, baseline, depth_scale; then, if
//      sgm_check_params passes, float left[rows * cols], right[rows * cols]
// out: per record int32 sgm_check_params(...), then for a pair that passes: uint16 depth[rows * cols], uint16 q[rows * cols], int64
//      interior, matched, rej_unique, rej_lr, rej_range, sum_q, the largest admissible S, the largest admissible C; uint16
//      S[rows * cols * D]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../odometry_amd/csrc/stereo_sgm_math.h"

template <typename T>
static T* block(size_t n) { return static_cast<T*>(malloc(n * sizeof(T) + (n == 0))); }

template <typename T>
static T* read_block(FILE* f, size_t n) {
  T* p = block<T>(n);
  if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[11];
  int records = 0;
  while (fread(head, sizeof(int32_t), 11, in) == 11) {
    double cam[3];
    if (fread(cam, sizeof(double), 3, in) != 3) return 2;
    const int rows = head[0], cols = head[1], p1 = head[8], p2 = head[9], paths = head[10];
    records++;
    const int32_t check = odo::sgm_check_params(rows, cols, head[2], head[3], head[4], p1, p2, paths);
    fwrite(&check, sizeof(check), 1, out);
    if (check != 0) continue;
    if (odo::sd_check_params(rows, cols, head[2], head[3], head[4], head[5], head[6], head[7], cam[0], cam[1], cam[2]) != 0) return 3;
    odo::SdRule r;
    r.dmin = head[2]; r.dmax = head[3]; r.A = head[4]; r.uniq = head[5]; r.lr_max = head[6]; r.max_raw = head[7];
    r.k = odo::sd_k(cam[0], cam[1], cam[2]);
    const size_t n = (size_t)rows * cols, D = (size_t)(r.dmax - r.dmin + 1);
    float* left = read_block<float>(in, n);
    float* right = read_block<float>(in, n);
    // the census planes hold the census domain only, as in stereo_depth_math_harness.cpp
    const bool domain = rows > 2 * odo::kSdCensusRy && cols > 2 * odo::kSdCensusRx;
    const size_t lead = (size_t)odo::kSdCensusRy * cols + odo::kSdCensusRx;
    const size_t words = domain ? (size_t)(rows - 2 * odo::kSdCensusRy - 1) * cols + (cols - 2 * odo::kSdCensusRx) : 0;
    uint64_t* pl = block<uint64_t>(words);
    uint64_t* pr = block<uint64_t>(words);
    for (size_t i = 0; i < words; i++) pl[i] = pr[i] = 0;
    if (domain)
      for (int y = odo::kSdCensusRy; y < rows - odo::kSdCensusRy; y++)
        for (int x = odo::kSdCensusRx; x < cols - odo::kSdCensusRx; x++) {
          pl[(size_t)y * cols + x - lead] = odo::sd_census(left + (size_t)y * cols + x, cols);
          pr[(size_t)y * cols + x - lead] = odo::sd_census(right + (size_t)y * cols + x, cols);
        }
    const uint64_t* cl = reinterpret_cast<const uint64_t*>(reinterpret_cast<uintptr_t>(pl) - lead * sizeof(uint64_t));
    const uint64_t* cr = reinterpret_cast<const uint64_t*>(reinterpret_cast<uintptr_t>(pr) - lead * sizeof(uint64_t));
    uint16_t* C = block<uint16_t>(n * D);
    uint16_t* S = block<uint16_t>(n * D);
    odo::sgm_cost_volume(cl, cr, rows, cols, r, C);
    odo::sgm_aggregate(C, rows, cols, r, p1, p2, paths, S);
    int64_t count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < n * D; i++)
      if (C[i] != odo::kSgmNone) {
        if (S[i] == odo::kSgmNone) return 4;
        count[6] = S[i] > count[6] ? S[i] : count[6];
        count[7] = C[i] > count[7] ? C[i] : count[7];
      } else if (S[i] != odo::kSgmNone) return 4;
    std::vector<uint8_t> dr(n, (uint8_t)odo::kSdNoRight);
    std::vector<uint16_t> depth(n, 0), q(n, 0);
    for (int y = 0; y < rows; y++)
      for (int x = 0; x < cols; x++) dr[(size_t)y * cols + x] = odo::sgm_right_pixel(S, rows, cols, y, x, r);
    for (int y = 0; y < rows; y++)
      for (int x = 0; x < cols; x++) {
        const size_t i = (size_t)y * cols + x;
        const int o = odo::sgm_left_pixel(S, dr.data(), rows, cols, y, x, r, &depth[i], &q[i]);
        count[0] += o != odo::kSdNotInterior;
        if (o != odo::kSdNotInterior) count[o] += 1;
        count[5] += q[i];
      }
    fwrite(depth.data(), sizeof(uint16_t), n, out);
    fwrite(q.data(), sizeof(uint16_t), n, out);
    fwrite(count, sizeof(int64_t), 8, out);
    fwrite(S, sizeof(uint16_t), n * D, out);
    free(left); free(right); free(pl); free(pr); free(C); free(S);
  }
  fclose(in);
  fclose(out);
  printf("%d records\n", records);
  return 0;
}
