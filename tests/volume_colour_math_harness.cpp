// tests/volume_colour_math_harness.cpp — odometry_amd/csrc/volume_colour_math.h (the colour update and the colour interpolation of
// the TSDF volume's colour grid) compiled on its own with g++, the lines the device compiles.
//   update OUT          writes c' of colour_update for every (c, wc, s), c, wc, s = 0 .. 255, as 2^24 bytes at index (c * 256 + wc) * 256
//                       + s (max_weight 255; the three channels carry c, 255 - c and c ^ 0x5a with the samples s, 255 - s and s ^ 0xa5 and
//                       are checked against each other here), then the new weights for max_weight 1, 3 and 255 on stdout
//   interp IN OUT       IN: records {uint32 ca, uint32 cb, float alpha}; OUT: one uint32 of colour_interpolate per record
#include <cstdio>
#include <cstring>
#include <vector>
#include "../odometry_amd/csrc/volume_colour_math.h"

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "update")) {
    std::vector<unsigned char> out(1u << 24);
    for (uint32_t c = 0; c < 256; c++)
      for (uint32_t wc = 0; wc < 256; wc++)
        for (uint32_t s = 0; s < 256; s++) {
          const uint32_t c1 = 255u - c, c2 = c ^ 0x5au, s1 = 255u - s, s2 = s ^ 0xa5u;
          const uint32_t word = c | (c1 << 8) | (c2 << 16) | (wc << 24);
          const uint32_t got = odo::colour_update(word, s, s1, s2, 255u);
          // the other two channels through the rule itself: every byte lane is held to it, not only the first
          const uint32_t d = wc + 1u;
          const uint32_t w1 = (c1 * wc + s1 + (d >> 1)) / d, w2 = (c2 * wc + s2 + (d >> 1)) / d;
          if (((got >> 8) & 0xffu) != w1 || ((got >> 16) & 0xffu) != w2 || (got >> 24) != (wc + 1u < 255u ? wc + 1u : 255u)) {
            std::printf("mismatch c %u wc %u s %u: %08x\n", c, wc, s, got);
            return 1;
          }
          out[(c * 256u + wc) * 256u + s] = (unsigned char)(got & 0xffu);
        }
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size() || std::fclose(f)) return 2;
    for (uint32_t mw : {1u, 3u, 255u})
      for (uint32_t wc = 0; wc < 256; wc++) std::printf("weight %u %u %u\n", mw, wc, odo::colour_update(wc << 24, 7u, 8u, 9u, mw) >> 24);
    std::printf("OK\n");
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "interp")) {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    struct Rec { uint32_t ca, cb; float alpha; } r;
    std::vector<uint32_t> out;
    while (std::fread(&r, sizeof(r), 1, f) == 1) out.push_back(odo::colour_interpolate(r.ca, r.cb, r.alpha));
    std::fclose(f);
    f = std::fopen(argv[3], "wb");
    if (!f || std::fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size() || std::fclose(f)) return 2;
    std::printf("OK\n");
    return 0;
  }
  return 3;
}
