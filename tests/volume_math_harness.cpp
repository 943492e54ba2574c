// tests/volume_math_harness.cpp — odometry_amd/csrc/volume_math.h (the voxel word, the gradient, the point of an edge and the
// integration of one voxel of the TSDF volume) compiled on its own with g++, the lines the device compiles.
//   integrate IN OUT   IN: {Head, Frame, uint32 vox[n], uint16 raw[rows * cols]}; OUT: uint32 vox[n] after the frame was integrated
//                      into every voxel, in raster order.
//   extract IN OUT     IN: {Head, uint32 vox[n]}; OUT: per point {float xyz0[4], float nrmw[4]} in (voxel, axis) order: the +x, +y, +z
//                      edges of the point extraction.
//   mesh IN OUT        the same over the seven edge directions of volume_mesh_table.h, xyz0[3] = the direction's number.
// Every mode prints its tallies, one `name count` per line, then OK. The grid is a plain array on the heap: a neighbour read outside
// it is AddressSanitizer's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../odometry_amd/csrc/volume_math.h"
#include "../odometry_amd/csrc/volume_mesh_table.h"

struct Head {
  int32_t nx, ny, nz;
  float vs, o[3];
};
struct Frame {
  int32_t rows, cols, max_weight;
  float f0, cx0, cy0, depth_scale, max_depth, mu;
  float m[12];   // m0 m1 m2 m4 m5 m6 m8 m9 m10 m12 m13 m14
  float zc_far;
};

template <class T>
static bool read_n(std::FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return std::fread(v->data(), sizeof(T), n, f) == n;
}

static int write_all(const char* path, const void* p, size_t bytes) {
  std::FILE* f = std::fopen(path, "wb");
  if (!f || (bytes && std::fwrite(p, 1, bytes, f) != bytes) || std::fclose(f)) return 2;   // (no point at all: p is null)
  std::printf("OK\n");
  return 0;
}

static odo::VolGrid grid_of(const Head& h, std::vector<uint32_t>* vox) {
  odo::VolGrid g;
  g.vox = vox->data(); g.nx = h.nx; g.ny = h.ny; g.nz = h.nz;
  g.vs = h.vs; g.ox = h.o[0]; g.oy = h.o[1]; g.oz = h.o[2];
  return g;
}

static int integrate(std::FILE* in, const char* out) {
  Head h;
  Frame r;
  std::vector<uint32_t> vox;
  std::vector<uint16_t> raw;
  if (std::fread(&h, sizeof(h), 1, in) != 1 || std::fread(&r, sizeof(r), 1, in) != 1 || !read_n(in, &vox, (size_t)h.nx * h.ny * h.nz) ||
      !read_n(in, &raw, (size_t)r.rows * r.cols)) return 2;
  const odo::VolGrid g = grid_of(h, &vox);
  odo::VolFrame f;
  f.rows = r.rows; f.cols = r.cols; f.max_weight = r.max_weight;
  f.f0 = r.f0; f.cx0 = r.cx0; f.cy0 = r.cy0; f.depth_scale = r.depth_scale; f.max_depth = r.max_depth; f.mu = r.mu;
  f.m0 = r.m[0]; f.m1 = r.m[1]; f.m2 = r.m[2]; f.m4 = r.m[3]; f.m5 = r.m[4]; f.m6 = r.m[5];
  f.m8 = r.m[6]; f.m9 = r.m[7]; f.m10 = r.m[8]; f.m12 = r.m[9]; f.m13 = r.m[10]; f.m14 = r.m[11];
  f.zc_far = r.zc_far;
  long skip[7] = {0, 0, 0, 0, 0, 0, 0}, band = 0, saturated = 0;
  for (int k = 0; k < g.nz; k++)
    for (int j = 0; j < g.ny; j++)
      for (int i = 0; i < g.nx; i++) {
        skip[odo::vox_visit(g, f, raw.data(), i, j, k, [&](int, float sdf, float s) {
          uint32_t* p = &vox.at(((size_t)k * g.ny + j) * g.nx + i);
          saturated += odo::vox_w(*p) + 1 > f.max_weight;
          *p = odo::vox_update(*p, s, f.max_weight);
          band += odo::vox_in_band(sdf, f.mu);
        })]++;
      }
  std::printf("updated %ld\nbehind %ld\npast %ld\noutside %ld\nhole %ld\nfar %ld\nbeyond %ld\nband %ld\nsaturated %ld\n", skip[odo::kVoxKept],
              skip[odo::kVoxBehind], skip[odo::kVoxPast], skip[odo::kVoxOutside], skip[odo::kVoxHole], skip[odo::kVoxFar], skip[odo::kVoxBeyond],
              band, saturated);
  return write_all(out, vox.data(), sizeof(uint32_t) * vox.size());
}

// vox_gradient, and which rule each of its axes took (the loads of vox_gradient, the rule itself out of the header).
static bool gradient(const odo::VolGrid& g, long long v, int i, int j, int k, uint32_t vc, float* grad, long* met) {
  const int pos[3] = {i, j, k}, dim[3] = {g.nx, g.ny, g.nz};
  const long long stride[3] = {1, g.nx, (long long)g.nx * g.ny};
  for (int c = 0; c < 3; c++) {
    float d;
    met[odo::vox_difference((float)odo::vox_q(vc), pos[c] + 1 < dim[c] ? g.vox[v + stride[c]] : 0u, pos[c] > 0 ? g.vox[v - stride[c]] : 0u, &d)]++;
  }
  return odo::vox_gradient(g, v, i, j, k, vc, grad);
}

static int points(std::FILE* in, const char* out, bool mesh) {
  Head h;
  std::vector<uint32_t> vox;
  if (std::fread(&h, sizeof(h), 1, in) != 1 || !read_n(in, &vox, (size_t)h.nx * h.ny * h.nz)) return 2;
  const odo::VolGrid g = grid_of(h, &vox);
  std::vector<float> rec;
  long met[4] = {0, 0, 0, 0};
  for (int v = 0; v < (int)vox.size(); v++) {
    int i, j, k;
    odo::vox_ijk(g, v, &i, &j, &k);
    const uint32_t va = vox[(size_t)v];
    const float cx = odo::vox_centre(g.ox, i, g.vs), cy = odo::vox_centre(g.oy, j, g.vs), cz = odo::vox_centre(g.oz, k, g.vs);
    for (int e = 0; e < (mesh ? 7 : 3); e++) {
      const int c = mesh ? odo::mtet_dir_offset(e) : 1 << e;
      const int dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
      if (i + dx >= g.nx || j + dy >= g.ny || k + dz >= g.nz) continue;
      const long long b = odo::vox_corner_word(g, v, c);
      const uint32_t vb = vox.at((size_t)b);
      if (!odo::vox_edge(va, vb)) continue;
      float ga[3], gb[3];
      const bool has_a = gradient(g, v, i, j, k, va, ga, met), has_b = gradient(g, b, i + dx, j + dy, k + dz, vb, gb, met);
      const odo::VoxEdgePoint p = odo::vox_edge_point(va, vb, has_a, ga, has_b, gb, cx, cy, cz, g.vs, dx, dy, dz);
      const float r[8] = {p.x, p.y, p.z, mesh ? (float)e : 0.0f, p.nx, p.ny, p.nz, p.w};
      rec.insert(rec.end(), r, r + 8);
    }
  }
  std::printf("both %ld\nplus %ld\nminus %ld\nneither %ld\n", met[odo::kVoxBoth], met[odo::kVoxPlus], met[odo::kVoxMinus], met[odo::kVoxNeither]);
  return write_all(out, rec.data(), sizeof(float) * rec.size());
}

int main(int argc, char** argv) {
  if (argc != 4) return 3;
  std::FILE* in = std::fopen(argv[2], "rb");
  if (!in) return 2;
  int rc = 3;
  if (!std::strcmp(argv[1], "integrate")) rc = integrate(in, argv[3]);
  else if (!std::strcmp(argv[1], "extract")) rc = points(in, argv[3], false);
  else if (!std::strcmp(argv[1], "mesh")) rc = points(in, argv[3], true);
  std::fclose(in);
  return rc;
}
