// volume_colour_kernels.hip — the TSDF volume's colour kernels (volume_colour.hip.h) as a translation unit of their own, plus their
// host-side launchers. The arithmetic is the table of include/odometry_hip.h (odo_volume_integrate_colour_dev) / DESIGN.md section
// 9.6: the geometry half is volume_integrate_kernel's (volume_kernels.hip) line for line — fp32, one rounding per operation, the unit
// is built with -ffp-contract=off and correctly rounded divide — and the colour half is integer arithmetic out of
// volume_colour_math.h. Nothing is combined across threads but counts.
#include <hip/hip_runtime.h>
#include "volume_colour.hip.h"
#include "volume_colour_math.h"
#include "volume_mesh_table.h"

namespace odo {

__device__ __forceinline__ int vcol_q(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }
__device__ __forceinline__ int vcol_w(uint32_t v) { return (int)(v >> 16); }
__device__ __forceinline__ float vcol_centre(float o, int i, float vs) { return o + ((float)i + 0.5f) * vs; }

__device__ __forceinline__ void vcol_next_tile(const VolIntegrateArgs& a, int* tx, int* ty, int* k) {
  *tx += a.step_x;
  if (*tx >= a.tiles_x) { *tx -= a.tiles_x; ++*ty; }
  *ty += a.step_y;
  if (*ty >= a.tiles_y) { *ty -= a.tiles_y; ++*k; }
  *k += a.step_k;
}

// volume_integrate_kernel with the colour update inside the band: the same tiles, the same digit-wise grid-stride walk, the same
// early-out, the depth pixel first and the voxel only after every test, the same per-block counter rows. Only a voxel with
// |sdf| <= mu reads a colour pixel or touches the colour grid, so the colour updates of a frame equal its in-band count.
__global__ void __launch_bounds__(kVolBlock) volume_integrate_colour_kernel(VolIntegrateColourArgs ac) {
  __shared__ unsigned sh[2][kVolBlock / 64];
  const VolIntegrateArgs& a = ac.a;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned n_upd = 0, n_band = 0;
  int tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
  const unsigned r0 = blockIdx.x / (unsigned)a.tiles_x;
  int ty = (int)(r0 % (unsigned)a.tiles_y), k = (int)(r0 / (unsigned)a.tiles_y);
  for (; k < a.g.nz; vcol_next_tile(a, &tx, &ty, &k)) {
    const int i = tx * kVolTileX + lane, j = ty * kVolTileY + w;
    if (i >= a.g.nx || j >= a.g.ny) continue;
    const float X = vcol_centre(a.g.ox, i, a.g.vs), Y = vcol_centre(a.g.oy, j, a.g.vs), Z = vcol_centre(a.g.oz, k, a.g.vs);
    const float zc = ((a.m2 * X + a.m6 * Y) + a.m10 * Z) + a.m14;
    if (!(zc > 0.0f)) continue;
    if (zc > a.zc_far) continue;   // (volume_integrate_kernel: it only ever skips what the tests below skip)
    const float xc = ((a.m0 * X + a.m4 * Y) + a.m8 * Z) + a.m12;
    const float yc = ((a.m1 * X + a.m5 * Y) + a.m9 * Z) + a.m13;
    const float u = a.f0 * (xc / zc) + a.cx0, v = a.f0 * (yc / zc) + a.cy0;
    const float xf = floorf(u + 0.5f), yf = floorf(v + 0.5f);
    if (!(xf >= 0.0f && xf < (float)a.cols && yf >= 0.0f && yf < (float)a.rows)) continue;   // (NaN fails too)
    const int pixel = (int)yf * a.cols + (int)xf;   // (< rows * cols <= 2^28)
    const unsigned raw = a.raw[pixel];
    if (raw == 0) continue;
    const float D = (float)raw / a.depth_scale;
    if (D > a.max_depth) continue;
    const float sdf = D - zc;
    if (sdf < -a.mu) continue;
    const float s = fminf(1.0f, sdf / a.mu) * 32767.0f;
    const size_t word = ((size_t)k * a.g.ny + j) * a.g.nx + i;
    // The band's loads are issued in front of the voxel's and nothing is computed from them before the voxel's update: the pixel, the
    // colour word and the voxel word are in flight together instead of one latency behind the other. lo = the pixel's first two
    // bytes (3 channels: one 16-bit load at any alignment) or all four, hi = its third byte (3 channels).
    const bool band = fabsf(sdf) <= a.mu;
    uint32_t lo = 0, hi = 0, cw = 0;
    uint32_t* cp = ac.c.col + word;
    if (band) {
      if (ac.c.channels == 4) {
        lo = ((const uint32_t*)ac.c.pix)[pixel];   // (the frame is 4-byte aligned: checked by the host)
      } else {
        const uint8_t* px = ac.c.pix + 3 * (size_t)pixel;
        uint16_t two;
        __builtin_memcpy(&two, px, 2);
        lo = two;
        hi = px[2];
      }
      cw = *cp;
    }
    uint32_t* p = a.g.vox + word;
    const uint32_t old = *p;
    const int wo = vcol_w(old);
    const float W = (float)wo;
    const float F = ((float)vcol_q(old) * W + s) / (W + 1.0f);
    const int qn = (int)rintf(F);
    const int wn = min(wo + 1, a.max_weight);
    *p = ((uint32_t)wn << 16) | ((uint32_t)qn & 0xffffu);
    n_upd++;
    if (band) {
      n_band++;
      const uint32_t c0 = lo & 0xffu, c1 = (lo >> 8) & 0xffu, c2 = ac.c.channels == 4 ? (lo >> 16) & 0xffu : hi;   // in memory order
      *cp = colour_update(cw, ac.c.bgr ? c2 : c0, c1, ac.c.bgr ? c0 : c2, (uint32_t)ac.c.max_weight);
    }
  }
  for (int o = 32; o > 0; o >>= 1) { n_upd += __shfl_xor(n_upd, o, 64); n_band += __shfl_xor(n_band, o, 64); }
  if (lane == 0) { sh[0][w] = n_upd; sh[1][w] = n_band; }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned long long t = 0;
    for (int q = 0; q < kVolBlock / 64; q++) t += sh[threadIdx.x][q];
    a.blk[2 * blockIdx.x + threadIdx.x] = t;
  }
}

void launch_volume_integrate_colour(const VolIntegrateColourArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_integrate_colour_kernel, dim3(a.a.nblk), dim3(kVolBlock), 0, s, a);
}

// ---- colours of the extraction's points -------------------------------------------------------------------------------------------
// The extraction's alpha of the edge a -> b (volume_scatter_kernel): both observed, exactly one of them positive.
__device__ __forceinline__ float vcol_alpha(uint32_t va, uint32_t vb) {
  const float qa = (float)vcol_q(va);
  return qa / (qa - (float)vcol_q(vb));
}

// A thread per voxel, volume_scatter_kernel's index arithmetic: block offset + the points of the waves before + the points of the
// lanes before; one dword per point.
__global__ void __launch_bounds__(kVolExtBlock) volume_extract_colour_kernel(VolExtractColourArgs ac) {
  const VolExtractArgs& a = ac.a;
  const int v = blockIdx.x * kVolExtBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long* wm = a.wave_mask + 3 * (size_t)blockIdx.x * (kVolExtBlock / 64);
  const unsigned long long bx = wm[3 * w], by = wm[3 * w + 1], bz = wm[3 * w + 2];
  const unsigned long long bit = 1ull << lane;
  if (v >= a.n || !((bx | by | bz) & bit)) return;
  int pre = 0;
  for (int q = 0; q < 3 * w; q++) pre += __popcll(wm[q]);
  const unsigned long long below = bit - 1ull;
  unsigned long long idx = a.blk_off[blockIdx.x] + (unsigned long long)(pre + __popcll(bx & below) + __popcll(by & below) + __popcll(bz & below));
  const unsigned long long cap = (unsigned long long)a.capacity;
  if (idx >= cap) return;
  const uint32_t va = a.g.vox[v], ca = ac.col[v];
  const size_t sy = (size_t)a.g.nx, sz = (size_t)a.g.nx * a.g.ny;
  if (bx & bit) {
    ac.rgba[idx++] = colour_interpolate(ca, ac.col[v + 1], vcol_alpha(va, a.g.vox[v + 1]));
    if (idx >= cap) return;
  }
  if (by & bit) {
    ac.rgba[idx++] = colour_interpolate(ca, ac.col[v + sy], vcol_alpha(va, a.g.vox[v + sy]));
    if (idx >= cap) return;
  }
  if (bz & bit) ac.rgba[idx] = colour_interpolate(ca, ac.col[v + sz], vcol_alpha(va, a.g.vox[v + sz]));
}

void launch_volume_extract_colour(const VolExtractColourArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_extract_colour_kernel, dim3(a.a.nblk), dim3(kVolExtBlock), 0, s, a);
}

// ---- colours of the mesh's vertices -----------------------------------------------------------------------------------------------
// A thread per voxel: the vertex kernel left the voxel's first index (vertex_base) beside its edge mask.
__global__ void __launch_bounds__(kMeshBlock) volume_mesh_colour_kernel(VolMeshColourArgs ac) {
  const VolMeshArgs& a = ac.a;
  const int v = blockIdx.x * kMeshBlock + threadIdx.x;
  if (v >= a.n) return;
  const unsigned mask = (unsigned)a.edge_mask[v];
  if (!mask) return;
  unsigned long long idx = a.vertex_base[v];
  const unsigned long long cap = (unsigned long long)a.vertex_capacity;
  if (idx >= cap) return;
  const uint32_t va = a.g.vox[v], ca = ac.col[v];
#pragma unroll
  for (int e = 0; e < 7; e++) {
    if (!((mask >> e) & 1u)) continue;
    if (idx >= cap) return;
    const int c = mtet_dir_offset(e);
    const long long vb = (long long)v + (c & 1) + (long long)((c >> 1) & 1) * a.g.nx + (long long)((c >> 2) & 1) * a.g.nx * a.g.ny;
    ac.rgba[idx] = colour_interpolate(ca, ac.col[vb], vcol_alpha(va, a.g.vox[vb]));
    idx++;
  }
}

void launch_volume_mesh_colour(const VolMeshColourArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_mesh_colour_kernel, dim3(a.a.nblk), dim3(kMeshBlock), 0, s, a);
}

}  // namespace odo
