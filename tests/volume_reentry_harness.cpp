// volume_reentry_harness.cpp — odometry_amd/csrc/volume_shift_math.h's re-entry rules (global index, inside-the-window test, destination
// word, the saved-voxel predicate) as a stand-alone host program, built by tests/test_volume_reentry_cpu.py with AddressSanitizer and
// UBSan: the lines the kernels of volume_reentry_kernels.hip compile, walked serially.
//   step IN OUT   int32 nx ny nz dx dy dz ox oy oz capacity m vol_colour store_colour; uint32 words[n]; uint32 colour[n] (vol_colour);
//                 int32 g[m][3]; uint32 vox[m]; uint32 col[m] (store_colour)
//                 -> uint32 words[n]; uint32 colour[n] (vol_colour); int32 m2 restored saved dropped; g[m2][3]; vox[m2]; col[m2]
//   keys IN OUT   int32 count; count x int32 {off, i, g, off2, n} -> count x {int64 global; int32 inside; int32 t (0 when outside)}
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../odometry_amd/csrc/volume_shift_math.h"

using namespace odo;

static std::vector<uint8_t> slurp(const char* path) {
  std::vector<uint8_t> b;
  FILE* f = fopen(path, "rb");
  if (!f) return b;
  uint8_t tmp[1 << 16];
  size_t r;
  while ((r = fread(tmp, 1, sizeof(tmp), f)) > 0) b.insert(b.end(), tmp, tmp + r);
  fclose(f);
  return b;
}

template <class T>
static void put(std::vector<uint8_t>& out, const T* p, size_t count) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
  out.insert(out.end(), b, b + sizeof(T) * count);
}

static int step(const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
  int32_t h[13];
  if (in.size() < sizeof(h)) return 1;
  memcpy(h, in.data(), sizeof(h));
  const int nx = h[0], ny = h[1], nz = h[2], d[3] = {h[3], h[4], h[5]}, off[3] = {h[6], h[7], h[8]};
  const long long capacity = h[9];
  const size_t m = (size_t)h[10], n = (size_t)nx * ny * nz;
  const bool vcol = h[11] != 0, scol = h[12] != 0;
  const size_t need = sizeof(h) + 4 * n * (vcol ? 2 : 1) + m * (12 + 4 + (scol ? 4 : 0));
  if (in.size() != need) return 2;
  std::vector<uint32_t> W(n), C(vcol ? n : 0), vox(m), col(scol ? m : 0);
  std::vector<int32_t> g(3 * m);
  const uint8_t* at = in.data() + sizeof(h);
  memcpy(W.data(), at, 4 * n); at += 4 * n;
  if (vcol) { memcpy(C.data(), at, 4 * n); at += 4 * n; }
  if (m) { memcpy(g.data(), at, 12 * m); at += 12 * m; memcpy(vox.data(), at, 4 * m); at += 4 * m; }
  if (scol && m) memcpy(col.data(), at, 4 * m);
  int off2[3];
  for (int c = 0; c < 3; c++) if (!shift_offset(off[c], d[c], &off2[c])) return 3;
  // the shift
  std::vector<uint32_t> W2(n, 0u), C2(vcol ? n : 0, 0u);
  for (int k = 0; k < nz; k++)
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        int si, sj, sk;
        if (!(shift_source(i, d[0], nx, &si) & shift_source(j, d[1], ny, &sj) & shift_source(k, d[2], nz, &sk))) continue;
        const size_t to = ((size_t)k * ny + j) * nx + i, from = ((size_t)sk * ny + sj) * nx + si;
        W2[to] = W[from];
        if (vcol) C2[to] = C[from];
      }
  // restore and keep
  std::vector<int32_t> g2;
  std::vector<uint32_t> vox2, col2;
  int32_t restored = 0, saved = 0, dropped = 0;
  for (size_t e = 0; e < m; e++) {
    long long word;
    if (reentry_dest(&g[3 * e], off2, nx, ny, nz, &word)) {
      W2[(size_t)word] = vox[e];
      if (scol && vcol) C2[(size_t)word] = col[e];
      restored++;
    } else {
      g2.insert(g2.end(), &g[3 * e], &g[3 * e] + 3);
      vox2.push_back(vox[e]);
      if (scol) col2.push_back(col[e]);
    }
  }
  // save
  for (int k = 0; k < nz; k++)
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx; i++) {
        if (!(shift_leaves(i, d[0], nx) || shift_leaves(j, d[1], ny) || shift_leaves(k, d[2], nz))) continue;
        const size_t v = ((size_t)k * ny + j) * nx + i;
        if (!reentry_saved(W[v], vcol ? C[v] : 0u)) continue;
        if ((long long)vox2.size() >= capacity) { dropped++; continue; }
        g2.push_back((int32_t)reentry_global(off[0], i));
        g2.push_back((int32_t)reentry_global(off[1], j));
        g2.push_back((int32_t)reentry_global(off[2], k));
        vox2.push_back(W[v]);
        if (scol) col2.push_back(C[v]);
        saved++;
      }
  put(out, W2.data(), n);
  if (vcol) put(out, C2.data(), n);
  const int32_t tail[4] = {(int32_t)vox2.size(), restored, saved, dropped};
  put(out, tail, 4);
  put(out, g2.data(), g2.size());
  put(out, vox2.data(), vox2.size());
  if (scol) put(out, col2.data(), col2.size());
  return 0;
}

static int keys(const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
  int32_t count;
  if (in.size() < 4) return 1;
  memcpy(&count, in.data(), 4);
  if (in.size() != 4 + (size_t)count * 20) return 2;
  for (int r = 0; r < count; r++) {
    int32_t x[5];
    memcpy(x, in.data() + 4 + (size_t)r * 20, 20);
    const int64_t glob = reentry_global(x[0], x[1]);
    int t = 0;
    const int32_t inside = reentry_inside(x[2], x[3], x[4], &t) ? 1 : 0;
    const int32_t tt = inside ? t : 0;
    put(out, &glob, 1);
    put(out, &inside, 1);
    put(out, &tt, 1);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) { printf("usage: %s step|keys IN OUT\n", argv[0]); return 2; }
  const std::string mode = argv[1];
  const std::vector<uint8_t> in = slurp(argv[2]);
  std::vector<uint8_t> out;
  const int rc = mode == "step" ? step(in, out) : mode == "keys" ? keys(in, out) : 9;
  if (rc) { printf("bad input (%d)\n", rc); return 1; }
  FILE* f = fopen(argv[3], "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { printf("cannot write\n"); return 1; }
  fclose(f);
  printf("OK\n");
  return 0;
}
