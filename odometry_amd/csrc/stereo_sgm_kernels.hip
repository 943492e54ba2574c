// stereo_sgm_kernels.hip — the kernels of the dense stereo matcher's semi-global mode (stereo_sgm.hip.h) as a translation unit of its
// own, plus their host-side launchers. The step of a path, the lines and the bounds are stereo_sgm_math.h's; the staging, the taps,
// the candidate walk and a left pixel's outputs are the match kernel's (stereo_depth.hip.h, stereo_depth_math.h).
// include/odometry_hip.h, odo_stereo_depth_enable_sgm; DESIGN.md section 9.18.
#include <hip/hip_runtime.h>
#include "stereo_sgm.hip.h"

namespace odo {

// ---- cost: the left match kernel's tile. A thread makes its pixel's costs kSgmCostChunk candidates at a time into the wave's block
// of LDS; the wave then stores the block pixel by pixel, half a wave per pixel: every store is 32 consecutive entries of C (and of
// S where they are kSgmNone), not 64 entries D apart.
template <int A>
__global__ void __launch_bounds__(kSdBlock) sgm_cost_kernel(SgmArgs g) {
  using T = SdTile<A>;
  __shared__ __attribute__((aligned(16))) uint64_t s_own[T::kRows * T::kOwnStride];
  __shared__ __attribute__((aligned(16))) uint64_t s_other[T::kRows * T::kOtherStride];
  __shared__ uint16_t s_out[kSdTileH][kSdTileW * kSgmCostStride];
  const SdArgs& a = g.sd;
  const int rows = a.rows, cols = a.cols, dmin = a.r.dmin, dmax = a.r.dmax, D = dmax - dmin + 1;
  sd_stage_tile<A, false>(a, s_own, s_other);
  const int tid = (int)threadIdx.x, tx = tid & (kSdTileW - 1), ty = tid / kSdTileW;
  const int gx0 = (int)blockIdx.x * kSdTileW, x = gx0 + tx, y = (int)blockIdx.y * kSdTileH + ty;
  uint64_t win[T::kN][T::kN];
  sd_window<A>(s_own, tx, ty, win);
  const int last = sd_last<A, false>(a, x, y);                  // (dmin - 1 outside the frame)
  const uint64_t* base = s_other + ty * T::kOtherStride + tx;
  uint16_t* mine = s_out[ty];
  const int half = tx / kSgmCostChunk, i = tx % kSgmCostChunk;   // on the way out: the pixel of a pair, the candidate of the chunk
  const size_t row = (size_t)(y < rows ? y : 0) * cols;
#pragma unroll 1
  for (int k0 = 0; k0 < D; k0 += kSgmCostChunk) {
#pragma unroll 1
    for (int j = 0; j < kSgmCostChunk; j++) {
      const int d = dmin + k0 + j;
      mine[tx * kSgmCostStride + j] = (uint16_t)(d <= last ? sd_tap_cost<A, false>(win, base, d, dmin, dmax) : kSgmNone);
    }
    __syncthreads();
    for (int t = half; t < kSdTileW; t += kSdTileW / kSgmCostChunk) {
      const int px = gx0 + t;
      if (px < cols && y < rows && k0 + i < D) {
        const uint16_t v = mine[t * kSgmCostStride + i];
        const size_t at = (row + px) * (size_t)D + k0 + i;
        g.C[at] = v;
        if (v == kSgmNone) g.S[at] = v;
      }
    }
    __syncthreads();
  }
}

// The cross-lane steps of a path, as DPP operands of the VALU (no trip through the LDS crossbar, which a __shfl takes): the minimum
// over the wave's 64 lanes as a scalar, and a register moved one lane up or down with `edge` entering at the open end.
__device__ __forceinline__ int sgm_min2(int a, int b) { return b < a ? b : a; }
__device__ __forceinline__ int sgm_wave_min(int v) {
  v = sgm_min2(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));    // quad_perm [1, 0, 3, 2]: pairs
  v = sgm_min2(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));    // quad_perm [2, 3, 0, 1]: quads
  v = sgm_min2(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));   // row_half_mirror: eights
  v = sgm_min2(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));   // row_mirror: rows of 16
  v = sgm_min2(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));   // row_bcast:15 into rows 1 and 3
  v = sgm_min2(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));   // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int sgm_from_lane_below(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xf, 0xf, false); }   // wave_shr:1
__device__ __forceinline__ int sgm_from_lane_above(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x130, 0xf, 0xf, false); }   // wave_shl:1

// ---- paths: a wave per line of direction (DX, DY). NS = the slots in use, ceil(D / 64). First: the launch stores S; otherwise it
// adds to it. Every load is issued by every lane at an index clamped into the pixel's admissible entries (the value is dropped where
// the lane has no candidate) and at a step clamped into the line: nothing about a load depends on a branch, so the wave waits for
// exactly the ring entry it is about to use and leaves the younger loads in flight.
template <int DX, int DY, int NS, bool First>
__global__ void __launch_bounds__(kSgmBlock) sgm_path_kernel(SgmArgs g) {
  const int cols = g.sd.cols, dmin = g.sd.r.dmin, dmax = g.sd.r.dmax, A = g.sd.r.A;
  const int D = dmax - dmin + 1, p1 = g.p1, p2 = g.p2;
  const SgmRect rc = sgm_rect(g.sd.rows, cols, dmin, A);
  const int lane = (int)threadIdx.x & 63;
  const int line = (int)blockIdx.x * kSgmLinesPerBlock + ((int)threadIdx.x >> 6);
  if (line >= sgm_lines(rc, DX, DY)) return;                    // (the whole wave)
  int x, y, len;
  sgm_line(rc, DX, DY, line, &x, &y, &len);

  // Step t's pixel: its costs and, unless this launch stores S, the sums so far, into ring entry k — asked for kSgmAhead steps
  // before they are used. Within a launch an entry of S is read and written by this wave alone, at its own step.
  int cb[kSgmAhead][NS], sb[kSgmAhead][NS];
  const auto fetch = [&](int k, int t) {
    const int tt = t < len ? t : len - 1;                        // (past the line's end: its last pixel again, unused)
    const int px = x + tt * DX, py = y + tt * DY, n = sgm_count(px, dmin, dmax, A);
    const size_t at = ((size_t)py * cols + px) * (size_t)D;
#pragma unroll
    for (int j = 0; j < NS; j++) {
      const int i = lane + 64 * j, ic = i < n ? i : n - 1;       // n >= 1: the pixel is active
      const int c = g.C[at + ic];
      cb[k][j] = i < n ? c : kSgmInf;
      sb[k][j] = First ? 0 : (int)g.S[at + ic];
    }
  };
  int lprev[NS];
#pragma unroll
  for (int j = 0; j < NS; j++) lprev[j] = kSgmInf;
#pragma unroll
  for (int k = 0; k < kSgmAhead; k++) fetch(k, k);
#pragma unroll 1
  for (int t0 = 0; t0 < len; t0 += kSgmAhead) {
#pragma unroll
    for (int k = 0; k < kSgmAhead; k++) {
      const int t = t0 + k;
      if (t >= len) break;                                       // (the whole wave)
      const int px = x + t * DX, py = y + t * DY, nc = sgm_count(px, dmin, dmax, A);
      uint16_t* s = g.S + ((size_t)py * cols + px) * (size_t)D;
      int c[NS], sold[NS];
#pragma unroll
      for (int j = 0; j < NS; j++) { c[j] = cb[k][j]; sold[j] = sb[k][j]; }
      fetch(k, t + kSgmAhead);
      int m = lprev[0];
#pragma unroll
      for (int j = 1; j < NS; j++) m = sgm_min2(m, lprev[j]);
      m = sgm_wave_min(m);
      int l[NS];
#pragma unroll
      for (int j = 0; j < NS; j++) {
        // across a slot seam the neighbour is the other end of the neighbouring slot
        const int below = j > 0 ? __builtin_amdgcn_readlane(lprev[j > 0 ? j - 1 : 0], 63) : kSgmInf;
        const int above = j + 1 < NS ? __builtin_amdgcn_readlane(lprev[j + 1 < NS ? j + 1 : j], 0) : kSgmInf;
        const int lm = sgm_from_lane_below(lprev[j], below), lp = sgm_from_lane_above(lprev[j], above);
        l[j] = t == 0 ? c[j] : sgm_step(c[j], lprev[j], lm, lp, m, p1, p2);
      }
#pragma unroll
      for (int j = 0; j < NS; j++) {
        const bool in = lane + 64 * j < nc;
        if (in) s[lane + 64 * j] = (uint16_t)(sold[j] + l[j]);
        lprev[j] = in ? l[j] : kSgmInf;
      }
    }
  }
}

// ---- selection: the match kernel's walk and end over S. The largest admissible candidate as in sd_last, A at run time.
template <bool Right>
__global__ void __launch_bounds__(kSdBlock) sgm_select_kernel(SgmArgs g) {
  __shared__ uint16_t s_s[kSdTileH][kSgmChunk * kSgmChunkStride];
  __shared__ uint32_t s_red[kSdBlock / 64][6];
  const SdArgs& a = g.sd;
  const int rows = a.rows, cols = a.cols, dmin = a.r.dmin, dmax = a.r.dmax, A = a.r.A, D = dmax - dmin + 1;
  const int tid = (int)threadIdx.x, tx = tid & (kSdTileW - 1), ty = tid / kSdTileW;
  const int gx0 = (int)blockIdx.x * kSdTileW, x = gx0 + tx, y = (int)blockIdx.y * kSdTileH + ty;
  int last = dmin - 1;
  if (sd_interior_row(y, rows, A)) {
    if (Right) { if (x >= A + kSdCensusRx) last = sd_right_last(x, cols, dmax, A); }
    else if (sd_interior_col(x, cols, A)) last = sd_left_last(x, dmax, A);
  }
  SdWalk w;
  sd_walk_init(&w);
  uint16_t* mine = s_s[ty];                                      // the wave's own block: [pixel of the tile row][candidate of the chunk]
  const uint16_t* srow = g.S + (size_t)(y < rows ? y : 0) * cols * (size_t)D;
  for (int k0 = 0; k0 < D; k0 += kSgmChunk) {
    const int idx = k0 + tx;                                     // the candidate this lane stages: a wave loads 64 in a row
    if (!Right) {
      for (int t = 0; t < kSgmChunk; t++) {
        const int px = gx0 + t;
        uint16_t v = (uint16_t)kSgmNone;
        if (px < cols && y < rows && idx < D) v = srow[(size_t)px * D + idx];
        mine[t * kSgmChunkStride + tx] = v;
      }
    } else {
      for (int u = 0; u < 2 * kSgmChunk - 1; u++) {              // left pixel gx0 + dmin + k0 + u serves right pixel t = u - i at candidate i
        const int t = u - tx, px = gx0 + dmin + k0 + u;
        if (t < 0 || t >= kSgmChunk) continue;
        uint16_t v = (uint16_t)kSgmNone;
        if (px < cols && y < rows && idx < D) v = srow[(size_t)px * D + idx];
        mine[t * kSgmChunkStride + tx] = v;
      }
    }
    __syncthreads();
    const int hi = last - dmin - k0 < kSgmChunk - 1 ? last - dmin - k0 : kSgmChunk - 1;
#pragma unroll 1
    for (int i = 0; i <= hi; i++) sd_walk_step(&w, dmin + k0 + i, (int)mine[tx * kSgmChunkStride + i]);
    __syncthreads();
  }
  if (Right) {
    if (x < cols && y < rows) a.dr[(size_t)y * cols + x] = w.c0 == kSdNone ? (uint8_t)kSdNoRight : (uint8_t)w.dl;
    return;
  }
  sd_left_outputs<false>(a, w, A, x, y, s_red);
}

// ---- launchers
void launch_sgm_cost(const SgmArgs& g, hipStream_t s) {
  const dim3 grid((unsigned)sd_blocks_x(g.sd.cols), (unsigned)sd_blocks_y(g.sd.rows));
  switch (g.sd.r.A) {
    case 0: hipLaunchKernelGGL(sgm_cost_kernel<0>, grid, dim3(kSdBlock), 0, s, g); break;
    case 1: hipLaunchKernelGGL(sgm_cost_kernel<1>, grid, dim3(kSdBlock), 0, s, g); break;
    case 2: hipLaunchKernelGGL(sgm_cost_kernel<2>, grid, dim3(kSdBlock), 0, s, g); break;
    default: hipLaunchKernelGGL(sgm_cost_kernel<3>, grid, dim3(kSdBlock), 0, s, g); break;
  }
}

template <int DX, int DY, bool First>
static void launch_path(const SgmArgs& g, const SgmRect& rc, hipStream_t s) {
  const int lines = sgm_lines(rc, DX, DY);
  const dim3 grid((unsigned)((lines + kSgmLinesPerBlock - 1) / kSgmLinesPerBlock)), block(kSgmBlock);
  switch ((g.sd.r.dmax - g.sd.r.dmin + 64) / 64) {              // the slots in use
    case 1: hipLaunchKernelGGL((sgm_path_kernel<DX, DY, 1, First>), grid, block, 0, s, g); break;
    case 2: hipLaunchKernelGGL((sgm_path_kernel<DX, DY, 2, First>), grid, block, 0, s, g); break;
    case 3: hipLaunchKernelGGL((sgm_path_kernel<DX, DY, 3, First>), grid, block, 0, s, g); break;
    default: hipLaunchKernelGGL((sgm_path_kernel<DX, DY, kSgmSlots, First>), grid, block, 0, s, g); break;
  }
}

void launch_sgm_paths(const SgmArgs& g, hipStream_t s) {
  const SgmRect rc = sgm_rect(g.sd.rows, g.sd.cols, g.sd.r.dmin, g.sd.r.A);
  if (sgm_empty(rc)) return;
  for (int k = 0; k < g.paths; k++)                              // in sgm_direction's order; the first one stores S
    switch (k) {
      case 0: launch_path<1, 0, true>(g, rc, s); break;
      case 1: launch_path<-1, 0, false>(g, rc, s); break;
      case 2: launch_path<0, 1, false>(g, rc, s); break;
      case 3: launch_path<0, -1, false>(g, rc, s); break;
      case 4: launch_path<1, 1, false>(g, rc, s); break;
      case 5: launch_path<-1, -1, false>(g, rc, s); break;
      case 6: launch_path<1, -1, false>(g, rc, s); break;
      default: launch_path<-1, 1, false>(g, rc, s); break;
    }
}

void launch_sgm_select(const SgmArgs& g, bool right, hipStream_t s) {
  const dim3 grid((unsigned)sd_blocks_x(g.sd.cols), (unsigned)sd_blocks_y(g.sd.rows));
  if (right) hipLaunchKernelGGL(sgm_select_kernel<true>, grid, dim3(kSdBlock), 0, s, g);
  else hipLaunchKernelGGL(sgm_select_kernel<false>, grid, dim3(kSdBlock), 0, s, g);
}

}  // namespace odo
