// The bilateral depth filter's host + device header (odometry_amd/csrc/depth_filter_math.h) as a stand-alone program for g++, built
// with -fsanitize=address,undefined by tests/test_depth_filter_cpu.py: every table and frame lives in a heap block of exactly its
// size, so a tap read outside the frame or a table index past its end is reported.
//   depth_filter_harness <in> <out>
// in:  records of int32 rows, cols, R; uint8 ws[(2R + 1)^2], wr[256], shift[256]; uint16 raw[rows * cols]
// out: per record int32 df_check_tables(...), then uint16 out[rows * cols] (df_pixel of every pixel)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../odometry_amd/csrc/depth_filter_math.h"

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
  int32_t head[3];
  int records = 0;
  while (fread(head, sizeof(int32_t), 3, in) == 3) {
    const int rows = head[0], cols = head[1], R = head[2], n = 2 * R + 1;
    uint8_t* ws = read_block<uint8_t>(in, (size_t)n * n);
    uint8_t* wr = read_block<uint8_t>(in, 256);
    uint8_t* shift = read_block<uint8_t>(in, 256);
    uint16_t* raw = read_block<uint16_t>(in, (size_t)rows * cols);
    uint8_t* wr0 = static_cast<uint8_t*>(malloc(odo::kDfRangePadded));
    odo::df_pad_range(wr, wr0);
    const int32_t check = odo::df_check_tables(R, ws, wr, shift);
    fwrite(&check, sizeof(check), 1, out);
    std::vector<uint16_t> o((size_t)rows * cols);
    if (check == 0)
      for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) o[(size_t)y * cols + x] = odo::df_pixel(raw, rows, cols, y, x, R, ws, wr0, shift);
    fwrite(o.data(), sizeof(uint16_t), o.size(), out);
    free(ws); free(wr); free(wr0); free(shift); free(raw);
    records++;
  }
  fclose(in);
  fclose(out);
  printf("%d records\n", records);
  return 0;
}
