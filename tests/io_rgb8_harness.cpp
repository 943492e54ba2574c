// Host harness for read_png_rgb8 (include/odometry_io.hpp), loaded through ctypes by tests/test_rgbd_frontend_cpu.py.
#include <cstring>
#include <vector>

#include "../include/odometry_io.hpp"

extern "C" int io_read_png_rgb8(const char* path, unsigned char* out, int cap, int* w, int* h, int* channels) {
  std::vector<uint8_t> px;
  if (!odometry::io::read_png_rgb8(path, px, *w, *h, *channels)) return -1;
  if ((long)px.size() > (long)cap) return -2;
  std::memcpy(out, px.data(), px.size());
  return 0;
}
