// The speckle filter's host + device header (odometry_amd/csrc/speckle_math.h) as a stand-alone program for g++, built with
// -fsanitize=address,undefined by tests/test_speckle_cpu.py: the key frame, both targets and both planes live in heap blocks of
// exactly the frame's size, so a neighbour read outside the frame is a reported overflow.
//   speckle_math_harness <in> <out>
// in:  records of int32 rows, cols, max_diff, min_size; for a set that passes sp_check_params then uint16 key[rows * cols]
// out: per record int32 sp_check_params(...), then for a set that passes: uint16 a[rows * cols] (the key frame filtered in place),
//      uint16 b[rows * cols] (a frame of 0xABAB filtered), int32 parent[rows * cols], int32 size[rows * cols], int64 counters[8]
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../odometry_amd/csrc/speckle_math.h"

template <typename T>
static T* block(size_t n) {
  T* p = static_cast<T*>(malloc(n * sizeof(T)));
  if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[4];
  int records = 0;
  while (fread(head, sizeof(int32_t), 4, in) == 4) {
    records++;
    const int rows = head[0], cols = head[1], max_diff = head[2], min_size = head[3];
    const int32_t check = odo::sp_check_params(rows, cols, max_diff, min_size);
    fwrite(&check, sizeof(check), 1, out);
    if (check != 0) continue;
    const size_t n = (size_t)rows * cols;
    uint16_t* key = block<uint16_t>(n);
    if (fread(key, sizeof(uint16_t), n, in) != n) { fprintf(stderr, "short read\n"); return 2; }
    uint16_t* b = block<uint16_t>(n);
    for (size_t i = 0; i < n; i++) b[i] = 0xABAB;
    int32_t* parent = block<int32_t>(n);
    int32_t* size = block<int32_t>(n);
    int64_t count[odo::kSpStatWords];
    odo::sp_ref_label(key, rows, cols, max_diff, parent, size);
    odo::sp_ref_apply(parent, size, rows, cols, min_size, key, b, count);   // the key frame is its own first target
    fwrite(key, sizeof(uint16_t), n, out);
    fwrite(b, sizeof(uint16_t), n, out);
    fwrite(parent, sizeof(int32_t), n, out);
    fwrite(size, sizeof(int32_t), n, out);
    fwrite(count, sizeof(int64_t), odo::kSpStatWords, out);
    free(key); free(b); free(parent); free(size);
  }
  fclose(in);
  fclose(out);
  printf("%d records\n", records);
  return 0;
}
