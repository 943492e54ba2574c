// The dense stereo matcher's host + device header (odometry_amd/csrc/stereo_depth_math.h) as a stand-alone program for g++, built
// with -fsanitize=address,undefined by tests/test_stereo_depth_cpu.py: every frame and plane lives in a heap block of exactly its
// size, so a tap read outside the frame or outside the census domain's plane is reported.
//   stereo_depth_math_harness <in> <out>
// in:  records of int32 rows, cols, dmin, dmax, A, uniq, lr_max, max_raw; double fx, baseline, depth_scale; then
//        rows >= 1: float left[rows * cols], right[rows * cols]
//        rows == -7777: `cols` triples of int32 cm, c0, cp (sd_subpixel on its own)
// out: per record int32 sd_check_params(...), then for a pair that passes: uint16 depth[rows * cols], uint16 q[rows * cols], int64
//      interior, matched, rej_unique, rej_lr, rej_range, sum_q; for triples (no check): int32 f[cols]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../odometry_amd/csrc/stereo_depth_math.h"

template <typename T>
static T* read_block(FILE* f, size_t n) {
  T* p = static_cast<T*>(malloc(n * sizeof(T) + (n == 0)));
  if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[8];
  int records = 0;
  while (fread(head, sizeof(int32_t), 8, in) == 8) {
    double cam[3];
    if (fread(cam, sizeof(double), 3, in) != 3) return 2;
    const int rows = head[0], cols = head[1];
    records++;
    if (rows == -7777) {
      int32_t* t = read_block<int32_t>(in, 3 * (size_t)cols);
      for (int i = 0; i < cols; i++) {
        const int32_t f = odo::sd_subpixel(t[3 * i], t[3 * i + 1], t[3 * i + 2]);
        fwrite(&f, sizeof(f), 1, out);
      }
      free(t);
      continue;
    }
    const int32_t check = odo::sd_check_params(rows, cols, head[2], head[3], head[4], head[5], head[6], head[7], cam[0], cam[1], cam[2]);
    fwrite(&check, sizeof(check), 1, out);
    if (check != 0) continue;
    odo::SdRule r;
    r.dmin = head[2]; r.dmax = head[3]; r.A = head[4]; r.uniq = head[5]; r.lr_max = head[6]; r.max_raw = head[7];
    r.k = odo::sd_k(cam[0], cam[1], cam[2]);
    const size_t n = (size_t)rows * cols;
    float* left = read_block<float>(in, n);
    float* right = read_block<float>(in, n);
    // the census planes hold the census domain only ((rows - 6) x (cols - 8) words): reaching outside it is a heap overflow. The
    // walk's plane pointers are offset so that (y, x) of the frame lands on (y - 3, x - 4) of the block with the frame's stride.
    const bool domain = rows > 2 * odo::kSdCensusRy && cols > 2 * odo::kSdCensusRx;
    const size_t lead = (size_t)odo::kSdCensusRy * cols + odo::kSdCensusRx;
    const size_t words = domain ? (size_t)(rows - 2 * odo::kSdCensusRy - 1) * cols + (cols - 2 * odo::kSdCensusRx) : 0;
    uint64_t* pl = static_cast<uint64_t*>(malloc(words * sizeof(uint64_t) + (words == 0)));
    uint64_t* pr = static_cast<uint64_t*>(malloc(words * sizeof(uint64_t) + (words == 0)));
    for (size_t i = 0; i < words; i++) pl[i] = pr[i] = 0;
    if (domain)
      for (int y = odo::kSdCensusRy; y < rows - odo::kSdCensusRy; y++)
        for (int x = odo::kSdCensusRx; x < cols - odo::kSdCensusRx; x++) {
          pl[(size_t)y * cols + x - lead] = odo::sd_census(left + (size_t)y * cols + x, cols);
          pr[(size_t)y * cols + x - lead] = odo::sd_census(right + (size_t)y * cols + x, cols);
        }
    std::vector<uint8_t> dr(n, (uint8_t)odo::kSdNoRight);
    std::vector<uint16_t> depth(n, 0), q(n, 0);
    int64_t count[6] = {0, 0, 0, 0, 0, 0};
    if (domain) {
      // (the offset pointers are formed as integers: nothing is dereferenced outside the blocks)
      const uint64_t* cl = reinterpret_cast<const uint64_t*>(reinterpret_cast<uintptr_t>(pl) - lead * sizeof(uint64_t));
      const uint64_t* cr = reinterpret_cast<const uint64_t*>(reinterpret_cast<uintptr_t>(pr) - lead * sizeof(uint64_t));
      for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) dr[(size_t)y * cols + x] = odo::sd_right_pixel(cl, cr, rows, cols, y, x, r);
      for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
          const size_t i = (size_t)y * cols + x;
          const int o = odo::sd_left_pixel(cl, cr, dr.data(), rows, cols, y, x, r, &depth[i], &q[i]);
          count[0] += o != odo::kSdNotInterior;
          if (o != odo::kSdNotInterior) count[o] += 1;
          count[5] += q[i];
        }
    }
    fwrite(depth.data(), sizeof(uint16_t), n, out);
    fwrite(q.data(), sizeof(uint16_t), n, out);
    fwrite(count, sizeof(int64_t), 6, out);
    free(left); free(right); free(pl); free(pr);
  }
  fclose(in);
  fclose(out);
  printf("%d records\n", records);
  return 0;
}
