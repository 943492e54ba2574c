// The mesh component filter's host + device header (odometry_amd/csrc/mesh_components_math.h) as a stand-alone program for g++, built
// with -fsanitize=address,undefined by tests/test_mesh_components_cpu.py: the parent, size and label arrays, the edge table and the
// outputs live in heap blocks of exactly their sizes, so a probe past the table's end or an index outside a mesh is a reported
// overflow.
//   mesh_components_math_harness <in> <out>
// in:  records of int32 n_v, n_t, min_triangles, keep_largest, drop_unreferenced, colour, edge_stats, vertex_capacity,
//      triangle_capacity, 0; for a set that passes the three checks then float xyz0[4 n_v], float nrmw[4 n_v], uint8 rgba[4 n_v]
//      (with colour), int32 tri[3 n_t]
// out: per record int32 mc_check_create(...), mc_check_rule(...), mc_check_counts(...), then for a set that passes all three:
//      int32 vertices, triangles of the result, its arrays in the input's order, int32 label[n_t], int64 counters[19]
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../odometry_amd/csrc/mesh_components_math.h"

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
  int32_t head[10];
  int records = 0;
  while (fread(head, sizeof(int32_t), 10, in) == 10) {
    records++;
    const int n_v = head[0], n_t = head[1], min_triangles = head[2], keep_largest = head[3], drop = head[4], colour = head[5];
    const int edge_stats = head[6], vcap = head[7], tcap = head[8];
    const int32_t check[3] = {odo::mc_check_create(vcap, tcap, colour, edge_stats), odo::mc_check_rule(min_triangles, keep_largest, drop),
                              odo::mc_check_counts(n_v, n_t, vcap, tcap)};
    fwrite(check, sizeof(int32_t), 3, out);
    if (check[0] || check[1] || check[2]) continue;
    float* xyz0 = read_block<float>(in, 4 * (size_t)n_v);
    float* nrmw = read_block<float>(in, 4 * (size_t)n_v);
    uint8_t* rgba = colour ? read_block<uint8_t>(in, 4 * (size_t)n_v) : nullptr;
    int32_t* tri = read_block<int32_t>(in, 3 * (size_t)n_t);
    const uint32_t eslots = edge_stats ? odo::mc_edge_slots(tcap) : 0u;
    unsigned long long* ekeys = eslots ? block<unsigned long long>(eslots) : nullptr;
    uint32_t* euse = eslots ? block<uint32_t>(eslots) : nullptr;
    int32_t* parent = block<int32_t>(n_v);
    uint32_t* size = block<uint32_t>(n_v);
    int32_t* vnew = block<int32_t>(n_v);
    uint8_t* vref = block<uint8_t>(n_v);
    int32_t* label = block<int32_t>(n_t);
    int64_t st[odo::kMcStatWords];
    int nv = 0, nt = 0;
    odo::mc_ref_plan(tri, n_v, n_t, min_triangles, keep_largest, drop, parent, size, vnew, vref, label, ekeys, euse, eslots, st, &nv, &nt);
    float* o_xyz0 = block<float>(4 * (size_t)nv);
    float* o_nrmw = block<float>(4 * (size_t)nv);
    uint8_t* o_rgba = colour ? block<uint8_t>(4 * (size_t)nv) : nullptr;
    int32_t* o_tri = block<int32_t>(3 * (size_t)nt);
    odo::mc_ref_emit(xyz0, nrmw, rgba, tri, n_v, n_t, vnew, label, o_xyz0, o_nrmw, o_rgba, o_tri);
    const int32_t counts[2] = {nv, nt};
    fwrite(counts, sizeof(int32_t), 2, out);
    fwrite(o_xyz0, sizeof(float), 4 * (size_t)nv, out);
    fwrite(o_nrmw, sizeof(float), 4 * (size_t)nv, out);
    if (colour) fwrite(o_rgba, 1, 4 * (size_t)nv, out);
    fwrite(o_tri, sizeof(int32_t), 3 * (size_t)nt, out);
    fwrite(label, sizeof(int32_t), (size_t)n_t, out);
    fwrite(st, sizeof(int64_t), odo::kMcStatWords, out);
    free(xyz0); free(nrmw); free(rgba); free(tri); free(ekeys); free(euse); free(parent); free(size); free(vnew); free(vref); free(label);
    free(o_xyz0); free(o_nrmw); free(o_rgba); free(o_tri);
  }
  fclose(in);
  fclose(out);
  printf("%d records\n", records);
  return 0;
}
