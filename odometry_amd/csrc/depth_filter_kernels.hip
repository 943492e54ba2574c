// depth_filter_kernels.hip — the bilateral depth filter's kernel (depth_filter.hip.h) as a translation unit of its own, plus its
// host-side launcher. Integer arithmetic only; the tap rule and the rounded division are depth_filter_math.h's.
// include/odometry_hip.h, odo_depth_filter_create; DESIGN.md section 9.12.
#include <hip/hip_runtime.h>
#include "depth_filter.hip.h"

namespace odo {

// Vec: cols % 4 == 0 and both frames 8-byte aligned. Then every group of four pixels at a column that is a multiple of four is one
// aligned 8-byte word that lies wholly inside or wholly outside its row: the tile and its halo are staged with 8-byte loads and the
// outputs leave as 8-byte stores. Otherwise (any cols, 2-byte alignment) the same walk goes pixel by pixel, each one guarded.
// amdgpu_waves_per_eu(1, 2): a frame has about one wave per SIMD whatever the tiling (480 x 640: 1 200 waves on 1 024 SIMDs), so the
// registers that keep a window row's lookups in flight cost nothing; left to the unit's occupancy-first scheduler the R = 4 build
// kept itself to 44 VGPRs and took 19.0 us for a 480 x 640 frame against 16.0 us.
template <int R, bool Vec>
__global__ void __launch_bounds__(kDfBlock) __attribute__((amdgpu_waves_per_eu(1, 2))) depth_filter_kernel(DfArgs a) {
  constexpr int kRows = kDfTileH + 2 * R;            // staged rows
  constexpr int kGroups = kDfLdsStride / 4;          // groups of four pixels per staged row
  constexpr int kN = 2 * R + 1;
  __shared__ __attribute__((aligned(16))) uint16_t tile[kRows * kDfLdsStride];
  __shared__ __attribute__((aligned(16))) uint8_t s_wr[4 * kDfRangeWords];   // the padded range table (df_pad_range): entry 256 is 0
  __shared__ __attribute__((aligned(16))) uint8_t s_shift[kDfRange];
  __shared__ uint32_t s_red[kDfBlock / 64][3];

  const int tid = (int)threadIdx.x;
  const int gx0 = (int)blockIdx.x * kDfTileW, gy0 = (int)blockIdx.y * kDfTileH;

  // ---- stage: the tables (one dword per thread of the first 129), then the tile with its halo, zero outside the frame
  if (tid < kDfRangeWords) reinterpret_cast<uint32_t*>(s_wr)[tid] = reinterpret_cast<const uint32_t*>(a.wr0)[tid];
  else if (tid < kDfRangeWords + kDfRange / 4)
    reinterpret_cast<uint32_t*>(s_shift)[tid - kDfRangeWords] = reinterpret_cast<const uint32_t*>(a.shift)[tid - kDfRangeWords];
  if (Vec) {
    for (int i = tid; i < kRows * kGroups; i += kDfBlock) {
      const int r = i / kGroups, g = i - r * kGroups;
      const int gy = gy0 - R + r, gx = gx0 - kDfPad + 4 * g;      // (gx is a multiple of 4: the group is inside iff its first pixel is)
      uint2 v = make_uint2(0u, 0u);
      if (gy >= 0 && gy < a.rows && gx >= 0 && gx < a.cols) v = *reinterpret_cast<const uint2*>(a.in + (size_t)gy * a.cols + gx);
      *reinterpret_cast<uint2*>(tile + r * kDfLdsStride + 4 * g) = v;
    }
  } else {
    for (int i = tid; i < kRows * kDfLdsStride; i += kDfBlock) {
      const int r = i / kDfLdsStride, c = i - r * kDfLdsStride;
      const int gy = gy0 - R + r, gx = gx0 - kDfPad + c;
      uint16_t v = 0;
      if (gy >= 0 && gy < a.rows && gx >= 0 && gx < a.cols) v = a.in[(size_t)gy * a.cols + gx];
      tile[i] = v;
    }
  }
  __syncthreads();

  // ---- the window: kDfPerThread outputs at tile columns 4 tx .. 4 tx + 3 of tile row ty. Staged column of tile column x: x + kDfPad,
  // so the taps of all four lie in the staged columns 4 tx + kDfPad - R .. 4 tx + kDfPad + 3 + R, inside the twelve from 4 tx on.
  const int tx = tid & (kDfTileW / kDfPerThread - 1), ty = tid / (kDfTileW / kDfPerThread);
  const uint32_t* row0 = reinterpret_cast<const uint32_t*>(tile + ty * kDfLdsStride + 4 * tx);   // staged row of dy = -R, as dwords
  constexpr int kLo = (kDfPad - R) / 2, kHi = (kDfPad + 3 + R) / 2;                              // the dwords of the twelve that hold taps
  int c[kDfPerThread], s[kDfPerThread], S[kDfPerThread], W[kDfPerThread];
  {
    const uint32_t* rc = row0 + R * (kDfLdsStride / 2);
    const uint32_t c01 = rc[kDfPad / 2], c23 = rc[kDfPad / 2 + 1];
    c[0] = (int)(c01 & 0xffffu); c[1] = (int)(c01 >> 16); c[2] = (int)(c23 & 0xffffu); c[3] = (int)(c23 >> 16);
  }
#pragma unroll
  for (int j = 0; j < kDfPerThread; j++) { s[j] = s_shift[c[j] >> 8]; S[j] = 0; W[j] = 0; }
  // One window row per trip, not unrolled: unrolled over the rows the scheduler lifts every table lookup of the window to the front
  // (R = 4: 324 of them) and the kernel spills. dy is wave-uniform, so the row's weights are scalar loads of the argument words.
#pragma unroll 1
  for (int dy = 0; dy < kN; dy++) {
    uint32_t w32[6];
#pragma unroll
    for (int q = kLo; q <= kHi; q++) w32[q] = row0[dy * (kDfLdsStride / 2) + q];
    const uint32_t wsw[kDfWsRowWords] = {a.ws[dy][0], a.ws[dy][1], a.ws[dy][2]};
#pragma unroll
    for (int dx = 0; dx < kN; dx++) {
      const int ws = (int)((wsw[dx >> 2] >> (8 * (dx & 3))) & 0xffu);   // (dx is a constant: a scalar field extract)
#pragma unroll
      for (int j = 0; j < kDfPerThread; j++) {
        const int col = kDfPad - R + j + dx;                             // staged column relative to 4 tx, a constant
        const int t = (int)((col & 1) ? (w32[col >> 1] >> 16) : (w32[col >> 1] & 0xffffu));
        df_tap(t, c[j], s[j], ws, s_wr, &S[j], &W[j]);
      }
    }
  }

  // ---- outputs and the workgroup's statistics. Pixels of the tile outside the frame were staged as 0: they give 0 and count nowhere.
  uint16_t o[kDfPerThread];
  uint32_t n_valid = 0, n_changed = 0, sum_abs = 0;
#pragma unroll
  for (int j = 0; j < kDfPerThread; j++) {
    o[j] = df_output(c[j], S[j], W[j]);
    const int d = (int)o[j] - c[j];
    n_valid += c[j] != 0;
    n_changed += d != 0;
    sum_abs += (uint32_t)(d < 0 ? -d : d);
  }
  const int x = gx0 + 4 * tx, y = gy0 + ty;
  if (y < a.rows) {
    if (Vec) {
      if (x < a.cols)
        *reinterpret_cast<uint2*>(a.out + (size_t)y * a.cols + x) = make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16));
    } else {
#pragma unroll
      for (int j = 0; j < kDfPerThread; j++)
        if (x + j < a.cols) a.out[(size_t)y * a.cols + x + j] = o[j];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_valid += __shfl_down(n_valid, off);
    n_changed += __shfl_down(n_changed, off);
    sum_abs += __shfl_down(sum_abs, off);
  }
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = n_valid; s_red[tid >> 6][1] = n_changed; s_red[tid >> 6][2] = sum_abs; }
  __syncthreads();
  if (tid == 0) {
    uint32_t r[3] = {0u, 0u, 0u};
#pragma unroll
    for (int w = 0; w < kDfBlock / 64; w++) { r[0] += s_red[w][0]; r[1] += s_red[w][1]; r[2] += s_red[w][2]; }
    const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    *reinterpret_cast<uint4*>(a.partials + kDfStatWords * b) = make_uint4(r[0], r[1], r[2], 0u);
  }
}

template <int R>
static void launch_depth_filter_r(const DfArgs& a, const dim3& grid, bool vec, hipStream_t s) {
  if (vec) hipLaunchKernelGGL((depth_filter_kernel<R, true>), grid, dim3(kDfBlock), 0, s, a);
  else hipLaunchKernelGGL((depth_filter_kernel<R, false>), grid, dim3(kDfBlock), 0, s, a);
}

void launch_depth_filter(const DfArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)df_blocks_x(a.cols), (unsigned)df_blocks_y(a.rows));
  const bool vec = (a.cols & 3) == 0 && (((uintptr_t)a.in | (uintptr_t)a.out) & 7) == 0;
  switch (a.radius) {
    case 1: launch_depth_filter_r<1>(a, grid, vec, s); break;
    case 2: launch_depth_filter_r<2>(a, grid, vec, s); break;
    case 3: launch_depth_filter_r<3>(a, grid, vec, s); break;
    default: launch_depth_filter_r<4>(a, grid, vec, s); break;
  }
}

}  // namespace odo
