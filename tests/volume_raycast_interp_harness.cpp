// tests/volume_raycast_interp_harness.cpp — rc_colour_interp of odometry_amd/csrc/volume_raycast_math.h (the trilinear colour sampling
// of the TSDF volume's ray-cast) compiled on its own with g++, the lines the device compiles, behind the march and the cell evaluation
// of the same header.
//   IN OUT      IN: records {uint32 vox[8], uint32 col[8] (2 x 2 x 2 grids, voxel (i, j, k) at i + 2 j + 4 k; a colour word is R, G, B,
//               wc from the low byte up), float e[3], float g[3], float t_min, float step, int32 n_steps, float depth_scale}; OUT: per
//               record {int32 hit, float z, uint8 rgba[4]}: one ray marched through the grid, then the cell evaluation at t = z with
//               the corners' colour words and the rule.
// Both grids are read through a loader with a bounds check of its own, as the kernel's loader reads them: the voxel pair and the
// colour pair at the same index, the colour pairs kept in the order of rc_cell's calls. A cell evaluation that reached outside either
// grid would abort here (and under AddressSanitizer in any case).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../odometry_amd/csrc/volume_raycast_math.h"

struct Rec {
  uint32_t vox[8], col[8];
  float e[3], g[3];
  float t_min, step;
  int32_t n_steps;
  float scale;
};
struct Out {
  int32_t hit;
  float z;
  uint8_t rgba[4];
};

static uint64_t pair_at(const std::vector<uint32_t>& grid, size_t word) {
  if (word + 1 >= grid.size()) std::abort();
  return (uint64_t)grid[word] | ((uint64_t)grid[word + 1] << 32);
}

struct HostLoad2 {
  const std::vector<uint32_t>* vox;
  uint64_t operator()(size_t word) const { return pair_at(*vox, word); }
};

struct HostLoad2Colour {
  const std::vector<uint32_t>* vox;
  const std::vector<uint32_t>* col;
  uint64_t* cp;   // [4]
  int* n;
  uint64_t operator()(size_t word) const {
    if (*n >= 4) std::abort();
    cp[(*n)++] = pair_at(*col, word);
    return pair_at(*vox, word);
  }
};

int main(int argc, char** argv) {
  if (argc != 3) return 3;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<Out> out;
  Rec r;
  while (std::fread(&r, sizeof(r), 1, f) == 1) {
    const std::vector<uint32_t> vox(r.vox, r.vox + 8), col(r.col, r.col + 8);   // on the heap: a read past the eighth word is AddressSanitizer's
    const HostLoad2 load = {&vox};
    odo::RcRay ray;
    ray.nx = ray.ny = ray.nz = 2;
    ray.ex = r.e[0]; ray.ey = r.e[1]; ray.ez = r.e[2];
    ray.gx = r.g[0]; ray.gy = r.g[1]; ray.gz = r.g[2];
    Out o;
    std::memset(&o, 0, sizeof(o));
    float z = 0.0f;
    if (odo::rc_march(load, ray, r.t_min, r.step, r.n_steps, &z)) {
      o.hit = 1;
      o.z = z;
      uint64_t cp[4] = {0, 0, 0, 0};
      int calls = 0;
      const HostLoad2Colour both = {&vox, &col, cp, &calls};
      odo::RcCell cell;
      if (odo::rc_cell(both, ray, z, &cell)) {
        if (calls != 4) std::abort();
        const uint32_t c = odo::rc_colour_interp(cell, cp);
        std::memcpy(o.rgba, &c, 4);
      }
    }
    out.push_back(o);
  }
  std::fclose(f);
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(Out), out.size(), f) != out.size() || std::fclose(f)) return 2;
  std::printf("OK\n");
  return 0;
}
