// tests/volume_raycast_math_harness.cpp — odometry_amd/csrc/volume_raycast_math.h (the sample, interpolation, gradient, hit and march
// of the TSDF volume's ray-cast) compiled on its own with g++, the lines the device compiles.
//   IN OUT      IN: records {uint32 vox[8] (a 2 x 2 x 2 grid, voxel (i, j, k) at i + 2 j + 4 k), float e[3], float g[3], float t_min,
//               float step, int32 n_steps, float depth_scale}; OUT: per record {int32 hit, float z, uint32 raw, float nrmw[4]}: one ray
//               marched through the grid, then the cell evaluation at t = z.
//   frame IN OUT   IN: records {float A[16] (column-major pose), float origin[3], float vs}; OUT: {float e[3], float G[9]} of
//               hostfp::raycast_frame (odometry_amd/csrc/host_fp.h): the host part of the specification.
// The loader reads the pair of voxels through a bounds check of its own, so a cell evaluation that reached outside the grid would
// abort here (and under AddressSanitizer in any case).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../odometry_amd/csrc/host_fp.h"
#include "../odometry_amd/csrc/volume_raycast_math.h"

struct Rec {
  uint32_t vox[8];
  float e[3], g[3];
  float t_min, step;
  int32_t n_steps;
  float scale;
};
struct Out {
  int32_t hit;
  float z;
  uint32_t raw;
  float nrmw[4];
};

struct HostLoad2 {
  const uint32_t* vox;
  size_t n;
  uint64_t operator()(size_t word) const {
    if (word + 1 >= n) std::abort();
    return (uint64_t)vox[word] | ((uint64_t)vox[word + 1] << 32);
  }
};

static int frames(const char* in, const char* out_path) {
  std::FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  struct { float A[16], origin[3], vs; } r;
  std::vector<float> out;
  while (std::fread(&r, sizeof(r), 1, f) == 1) {
    float eG[12];
    hostfp::raycast_frame(r.A, r.origin, r.vs, eG, eG + 3);
    out.insert(out.end(), eG, eG + 12);
  }
  std::fclose(f);
  f = std::fopen(out_path, "wb");
  if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size() || std::fclose(f)) return 2;
  std::printf("OK\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "frame")) return frames(argv[2], argv[3]);
  if (argc != 3) return 3;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<Out> out;
  Rec r;
  while (std::fread(&r, sizeof(r), 1, f) == 1) {
    std::vector<uint32_t> grid(r.vox, r.vox + 8);   // on the heap: a read past the eighth word is AddressSanitizer's
    const HostLoad2 load = {grid.data(), grid.size()};
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
      o.raw = odo::rc_raw(z, r.scale);
      odo::RcCell cell;
      if (odo::rc_cell(load, ray, z, &cell) && odo::rc_normal(cell, &o.nrmw[0], &o.nrmw[1], &o.nrmw[2])) o.nrmw[3] = (float)cell.wmin;
      else o.nrmw[0] = o.nrmw[1] = o.nrmw[2] = 0.0f;
    }
    out.push_back(o);
  }
  std::fclose(f);
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(Out), out.size(), f) != out.size() || std::fclose(f)) return 2;
  std::printf("OK\n");
  return 0;
}
