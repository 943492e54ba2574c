// The mesh welder's host + device header (odometry_amd/csrc/mesh_weld_math.h) as a stand-alone program for g++, built with
// -fsanitize=address,undefined by tests/test_mesh_weld_cpu.py: both tables, every scratch array and every pass's outputs live in heap
// blocks of exactly their sizes, so a probe past a table's end or an index outside a mesh is a reported overflow.
//   mesh_weld_math_harness <in> <out>
// in:  records of int32 n_v, n_t, grids, drop_unreferenced, colour, vertex_capacity, triangle_capacity, 0 and float eps, origin[3];
//      for a set that passes the three checks then float xyz0[4 n_v], float nrmw[4 n_v], uint8 rgba[4 n_v] (with colour),
//      int32 tri[3 n_t]
// out: per record int32 weld_check_create(...), weld_check_rule(...), weld_check_counts(...), then for a set that passes all three:
//      int32 vertices, triangles of the result, its arrays in the input's order, int64 counters[12]
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../odometry_amd/csrc/mesh_weld_math.h"

template <typename T>
static T* block(size_t n) {
  T* p = static_cast<T*>(malloc(n * sizeof(T)));
  if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
  return p;
}

template <typename T>
static T* read_block(FILE* in, size_t n) {
  T* p = block<T>(n);
  if (fread(p, sizeof(T), n, in) != n) { fprintf(stderr, "short read\n"); exit(2); }
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int32_t head[8];
  float rule[4];
  int records = 0;
  while (fread(head, sizeof(int32_t), 8, in) == 8 && fread(rule, sizeof(float), 4, in) == 4) {
    records++;
    int n_v = head[0], n_t = head[1];
    const int grids = head[2], drop = head[3], colour = head[4], vcap = head[5], tcap = head[6];
    const int32_t check[3] = {odo::weld_check_create(vcap, tcap, colour), odo::weld_check_rule(rule[0], rule + 1, grids, drop),
                              odo::weld_check_counts(n_v, n_t, vcap, tcap)};
    fwrite(check, sizeof(int32_t), 3, out);
    if (check[0] || check[1] || check[2]) continue;
    float* xyz0 = read_block<float>(in, 4 * (size_t)n_v);
    float* nrmw = read_block<float>(in, 4 * (size_t)n_v);
    uint8_t* rgba = colour ? read_block<uint8_t>(in, 4 * (size_t)n_v) : nullptr;
    int32_t* tri = read_block<int32_t>(in, 3 * (size_t)n_t);
    const uint32_t vslots = odo::weld_slots(vcap), tslots = odo::weld_slots(tcap);
    unsigned long long* vkeys = block<unsigned long long>(vslots);
    uint32_t* vmin = block<uint32_t>(vslots);
    int32_t* ttab = block<int32_t>(tslots);
    int64_t st[odo::kWeldStatWords] = {0};
    st[odo::kWeldVerticesIn] = n_v;
    st[odo::kWeldTrianglesIn] = n_t;
    const float inv = odo::weld_inv(rule[0]);
    for (int k = 0; k < grids; k++) {
      int32_t* rep = block<int32_t>(n_v);
      int32_t* vnew = block<int32_t>(n_v);
      uint8_t* vref = block<uint8_t>(n_v);
      int32_t* rtri = block<int32_t>(3 * (size_t)n_t);
      uint8_t* tkeep = block<uint8_t>(n_t);
      int nv = 0, nt = 0;
      odo::weld_ref_plan(xyz0, tri, n_v, n_t, inv, rule + 1, k, drop, vkeys, vmin, vslots, ttab, tslots, rep, vnew, vref, rtri, tkeep, st,
                         &nv, &nt);
      float* o_xyz0 = block<float>(4 * (size_t)nv);
      float* o_nrmw = block<float>(4 * (size_t)nv);
      uint8_t* o_rgba = colour ? block<uint8_t>(4 * (size_t)nv) : nullptr;
      int32_t* o_tri = block<int32_t>(3 * (size_t)nt);
      odo::weld_ref_emit(xyz0, nrmw, rgba, n_v, n_t, vnew, rtri, tkeep, o_xyz0, o_nrmw, o_rgba, o_tri);
      free(rep); free(vnew); free(vref); free(rtri); free(tkeep);
      free(xyz0); free(nrmw); free(rgba); free(tri);
      xyz0 = o_xyz0; nrmw = o_nrmw; rgba = o_rgba; tri = o_tri;
      n_v = nv; n_t = nt;
      st[odo::kWeldPasses] += 1;
    }
    st[odo::kWeldVerticesOut] = n_v;
    st[odo::kWeldTrianglesOut] = n_t;
    const int32_t counts[2] = {n_v, n_t};
    fwrite(counts, sizeof(int32_t), 2, out);
    fwrite(xyz0, sizeof(float), 4 * (size_t)n_v, out);
    fwrite(nrmw, sizeof(float), 4 * (size_t)n_v, out);
    if (colour) fwrite(rgba, 1, 4 * (size_t)n_v, out);
    fwrite(tri, sizeof(int32_t), 3 * (size_t)n_t, out);
    fwrite(st, sizeof(int64_t), odo::kWeldStatWords, out);
    free(xyz0); free(nrmw); free(rgba); free(tri); free(vkeys); free(vmin); free(ttab);
  }
  fclose(in);
  fclose(out);
  printf("%d records\n", records);
  return 0;
}
