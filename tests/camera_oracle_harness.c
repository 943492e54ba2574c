/* tests/camera_oracle_harness.c — orc_camera_init_maps and orc_camera_remap of oracle/odo_oracle.c as a stand-alone program, the
 * record formats of tests/camera_math_harness.cpp. tests/test_camera_cases_cpu.py compiles the two files together with
 * -fsanitize=address,undefined,float-cast-overflow: the oracle's camera model converts nothing that an int cannot hold.
 *   maps IN OUT    IN: records {double raw[5], dist[4], R[9], P[12]; int32 rows, cols}; OUT per record: int32 status and, for
 *                  status 0, mapx then mapy.
 *   remap IN OUT   IN: records {int32 srows, scols, drows, dcols; float border; src, mapx, mapy}; OUT per record: dst. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int orc_camera_init_maps(const double raw[5], const double dist[4], const double R[9], const double P[12], int rows, int cols,
                         float* mapx, float* mapy);
void orc_camera_remap(const float* src, int srows, int scols, const float* mapx, const float* mapy, int drows, int dcols,
                      float border_value, float* dst);

struct map_rec {
  double raw[5], dist[4], R[9], P[12];
  int32_t rows, cols;
};
struct remap_head {
  int32_t srows, scols, drows, dcols;
  float border;
};

static float* read_floats(FILE* f, size_t n) {
  float* p = (float*)malloc(n * sizeof(float));
  if (p && fread(p, sizeof(float), n, f) != n) {
    free(p);
    p = NULL;
  }
  return p;
}

static int maps(FILE* in, FILE* out) {
  struct map_rec r;
  while (fread(&r, sizeof(r), 1, in) == 1) {
    if (r.rows < 1 || r.cols < 1) return 4;
    const size_t n = (size_t)r.rows * r.cols;
    float* mx = (float*)malloc(n * sizeof(float));
    float* my = (float*)malloc(n * sizeof(float));
    if (!mx || !my) return 2;
    const int32_t status = orc_camera_init_maps(r.raw, r.dist, r.R, r.P, r.rows, r.cols, mx, my);
    int bad = fwrite(&status, sizeof(status), 1, out) != 1;
    if (!bad && status == 0) bad = fwrite(mx, sizeof(float), n, out) != n || fwrite(my, sizeof(float), n, out) != n;
    free(mx);
    free(my);
    if (bad) return 2;
  }
  return 0;
}

static int remap(FILE* in, FILE* out) {
  struct remap_head h;
  while (fread(&h, sizeof(h), 1, in) == 1) {
    if (h.srows < 1 || h.scols < 1 || h.drows < 1 || h.dcols < 1) return 4;
    const size_t ns = (size_t)h.srows * h.scols, nd = (size_t)h.drows * h.dcols;
    float* src = read_floats(in, ns);
    float* mx = read_floats(in, nd);
    float* my = read_floats(in, nd);
    float* dst = (float*)malloc(nd * sizeof(float));
    if (!src || !mx || !my || !dst) return 4;
    orc_camera_remap(src, h.srows, h.scols, mx, my, h.drows, h.dcols, h.border, dst);
    const int bad = fwrite(dst, sizeof(float), nd, out) != nd;
    free(src);
    free(mx);
    free(my);
    free(dst);
    if (bad) return 2;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 3;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 2;
  int st = 3;
  if (!strcmp(argv[1], "maps")) st = maps(in, out);
  else if (!strcmp(argv[1], "remap")) st = remap(in, out);
  fclose(in);
  if (fclose(out)) return 2;
  if (st == 0) printf("OK\n");
  return st;
}
