// Host harness for read_png_gray16 (include/odometry_io.hpp), loaded through ctypes by tests/test_rgbd_cpu.py.
#include <cstring>
#include <vector>

#include "../include/odometry_io.hpp"

extern "C" int io_read_png16(const char* path, unsigned short* out, int cap, int* w, int* h) {
  std::vector<uint16_t> px;
  if (!odometry::io::read_png_gray16(path, px, *w, *h)) return -1;
  if ((long)px.size() > (long)cap) return -2;
  std::memcpy(out, px.data(), px.size() * sizeof(uint16_t));
  return 0;
}
