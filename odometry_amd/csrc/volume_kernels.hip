// volume_kernels.hip — the TSDF volume's kernels (volume.hip.h) as a translation unit of their own, plus their host-side launchers.
// The arithmetic is the table of include/odometry_hip.h (odo_volume_*) / DESIGN.md sections 9.4 and 9.6 and lives in volume_math.h
// and volume_colour_math.h: fp32, one rounding per operation (the unit is built with -ffp-contract=off and correctly rounded
// divide / sqrt), nothing combined across threads but counts. The kernels add the walk over the voxels, the loads and the stores.
#include <hip/hip_runtime.h>
#include "volume.hip.h"
#include "volume_colour_math.h"
#include "volume_scan.hip.h"

namespace odo {

__device__ __forceinline__ void vol_next_tile(const VolIntegrateArgs& a, int* tx, int* ty, int* k) {
  *tx += a.step_x;
  if (*tx >= a.tiles_x) { *tx -= a.tiles_x; ++*ty; }
  *ty += a.step_y;
  if (*ty >= a.tiles_y) { *ty -= a.tiles_y; ++*k; }
  *k += a.step_k;
}

// Tiles of 64 x 4 voxels in raster order (x tiles fastest, then y tiles, then k), walked grid-stride. The projection is computed
// from (i, j, k) for every voxel; a voxel that fails any test is neither loaded nor stored, so a wave whose 64 voxels all fail
// leaves without a voxel access: the tests are vox_visit's, which calls back for a voxel that passed them all. Colour: the colour
// update inside the band. Only a voxel with |sdf| <= mu reads a colour pixel or touches the colour grid, so the colour updates of a
// frame equal its in-band count.
template <bool Colour>
__device__ __forceinline__ void volume_integrate_body(const VolIntegrateArgs& a, const VolColourFrame& c) {
  __shared__ unsigned sh[2][kVolBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned n_upd = 0, n_band = 0;   // per thread: at most tiles / nblk + 1 voxels, far below 2^32
  // (tx, ty, k) = the tile's digits; the stride of nblk tiles is added digit by digit (step_x / _y / _k are its digits): no division
  // in the loop
  int tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
  const unsigned r0 = blockIdx.x / (unsigned)a.tiles_x;
  int ty = (int)(r0 % (unsigned)a.tiles_y), k = (int)(r0 / (unsigned)a.tiles_y);
  for (; k < a.g.nz; vol_next_tile(a, &tx, &ty, &k)) {
    const int i = tx * kVolTileX + lane, j = ty * kVolTileY + w;
    if (i >= a.g.nx || j >= a.g.ny) continue;
    vox_visit(a.g, a.f, a.raw, i, j, k, [&](int pixel, float sdf, float s) {
      const size_t word = ((size_t)k * a.g.ny + j) * a.g.nx + i;
      const bool band = vox_in_band(sdf, a.f.mu);
      // The band's loads are issued in front of the voxel's and nothing is computed from them before the voxel's update: the pixel, the
      // colour word and the voxel word are in flight together instead of one latency behind the other. lo = the pixel's first two
      // bytes (3 channels: one 16-bit load at any alignment) or all four, hi = its third byte (3 channels).
      uint32_t lo = 0, hi = 0, cw = 0;
      uint32_t* cp = Colour ? c.col + word : nullptr;
      if constexpr (Colour) {
        if (band) {
          if (c.channels == 4) {
            lo = ((const uint32_t*)c.pix)[pixel];   // (the frame is 4-byte aligned: checked by the host)
          } else {
            const uint8_t* px = c.pix + 3 * (size_t)pixel;
            uint16_t two;
            __builtin_memcpy(&two, px, 2);
            lo = two;
            hi = px[2];
          }
          cw = *cp;
        }
      }
      uint32_t* p = a.g.vox + word;
      *p = vox_update(*p, s, a.f.max_weight);
      n_upd++;
      if constexpr (!Colour) {
        n_band += band ? 1u : 0u;
      } else if (band) {
        n_band++;
        const uint32_t c0 = lo & 0xffu, c1 = (lo >> 8) & 0xffu, c2 = c.channels == 4 ? (lo >> 16) & 0xffu : hi;   // in memory order
        *cp = colour_update(cw, c.bgr ? c2 : c0, c1, c.bgr ? c0 : c2, (uint32_t)c.max_weight);
      }
    });
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

__global__ void __launch_bounds__(kVolBlock) volume_integrate_kernel(VolIntegrateArgs a) { volume_integrate_body<false>(a, VolColourFrame{}); }
__global__ void __launch_bounds__(kVolBlock) volume_integrate_colour_kernel(VolIntegrateColourArgs ac) { volume_integrate_body<true>(ac.a, ac.c); }

// One block: the blocks' rows into the counters.
__global__ void __launch_bounds__(kVolBlock) volume_sum_kernel(VolIntegrateArgs a) {
  __shared__ unsigned long long sh[2][kVolBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long u = 0, b = 0;
  for (int r = threadIdx.x; r < a.nblk; r += kVolBlock) { u += a.blk[2 * r]; b += a.blk[2 * r + 1]; }
  for (int o = 32; o > 0; o >>= 1) { u += __shfl_xor(u, o, 64); b += __shfl_xor(b, o, 64); }
  if (lane == 0) { sh[0][w] = u; sh[1][w] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    u = b = 0;
    for (int q = 0; q < kVolBlock / 64; q++) { u += sh[0][q]; b += sh[1][q]; }
    a.ctr->updated = u;
    a.ctr->band = b;
    a.ctr->cumulative += u;
  }
}

void launch_volume_integrate(const VolIntegrateArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_integrate_kernel, dim3(a.nblk), dim3(kVolBlock), 0, s, a);
  hipLaunchKernelGGL(volume_sum_kernel, dim3(1), dim3(kVolBlock), 0, s, a);
}

void launch_volume_integrate_colour(const VolIntegrateColourArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_integrate_colour_kernel, dim3(a.a.nblk), dim3(kVolBlock), 0, s, a);
  hipLaunchKernelGGL(volume_sum_kernel, dim3(1), dim3(kVolBlock), 0, s, a.a);
}

// ---- extraction ----------------------------------------------------------------------------------------------------------------
// The passes are volume_scan.hip.h's: the three ballots per wave and the block's count, the scan of the counts, a thread's rank and
// its voxel's points.
__global__ void __launch_bounds__(kVolExtBlock) volume_count_kernel(VolExtractArgs a) {
  const int v = blockIdx.x * kVolExtBlock + threadIdx.x;
  bool ex = false, ey = false, ez = false;
  if (v < a.n) {
    const uint32_t va = a.g.vox[v];
    if (vox_w(va) > 0) {
      int i, j, k;
      vox_ijk(a.g, v, &i, &j, &k);
      const size_t sy = (size_t)a.g.nx, sz = (size_t)a.g.nx * a.g.ny;
      ex = i + 1 < a.g.nx && vox_edge(va, a.g.vox[v + 1]);
      ey = j + 1 < a.g.ny && vox_edge(va, a.g.vox[v + sy]);
      ez = k + 1 < a.g.nz && vox_edge(va, a.g.vox[v + sz]);
    }
  }
  const unsigned long long b[3] = {__ballot(ex), __ballot(ey), __ballot(ez)};
  ballot_counts(b, a.wave_mask, a.blk);
}

// One block: the blocks' exclusive offsets, the total, the clamp at capacity.
__global__ void __launch_bounds__(kVolScanThreads) volume_scan_kernel(VolExtractArgs a) {
  const unsigned long long total = scan_counts<kVolScanThreads, 1>(a.blk, a.blk_off, a.nblk).t[0];
  if (threadIdx.x == 0) {
    a.ctr->ext_total = total;
    a.ctr->ext_written = total < (unsigned long long)a.capacity ? total : (unsigned long long)a.capacity;
  }
}

__global__ void __launch_bounds__(kVolExtBlock) volume_scatter_kernel(VolExtractArgs a) {
  const int v = blockIdx.x * kVolExtBlock + threadIdx.x;
  const unsigned long long bit = 1ull << (threadIdx.x & 63);
  unsigned long long e[3];
  ballot_wave(a.wave_mask, e);
  if (v >= a.n || !((e[0] | e[1] | e[2]) & bit)) return;
  const int rank = ballot_rank<3, int>(a.wave_mask, e);
  const unsigned long long idx = a.blk_off[blockIdx.x] + (unsigned long long)rank;
  extract_points(a.g, v, e, bit, idx, (unsigned long long)a.capacity, a.xyz0, a.nrmw, nullptr, nullptr);
}

void launch_volume_extract(const VolExtractArgs& a, hipStream_t s) {
  const dim3 grid(a.nblk), block(kVolExtBlock);
  hipLaunchKernelGGL(volume_count_kernel, grid, block, 0, s, a);
  hipLaunchKernelGGL(volume_scan_kernel, dim3(1), dim3(kVolScanThreads), 0, s, a);
  hipLaunchKernelGGL(volume_scatter_kernel, grid, block, 0, s, a);
}

}  // namespace odo
