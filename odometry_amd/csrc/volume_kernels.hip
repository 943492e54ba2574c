// volume_kernels.hip — the TSDF volume's kernels (volume.hip.h) as a translation unit of their own, plus their host-side launchers.
// The arithmetic is the table of include/odometry_hip.h (odo_volume_*) / DESIGN.md section 9.4: fp32, one rounding per operation
// (the unit is built with -ffp-contract=off and correctly rounded divide / sqrt), nothing combined across threads.
#include <hip/hip_runtime.h>
#include "volume.hip.h"

namespace odo {

__device__ __forceinline__ int vol_q(uint32_t v) { return (int)(int16_t)(v & 0xffffu); }
__device__ __forceinline__ int vol_w(uint32_t v) { return (int)(v >> 16); }
__device__ __forceinline__ float vol_centre(float o, int i, float vs) { return o + ((float)i + 0.5f) * vs; }

__device__ __forceinline__ void vol_next_tile(const VolIntegrateArgs& a, int* tx, int* ty, int* k) {
  *tx += a.step_x;
  if (*tx >= a.tiles_x) { *tx -= a.tiles_x; ++*ty; }
  *ty += a.step_y;
  if (*ty >= a.tiles_y) { *ty -= a.tiles_y; ++*k; }
  *k += a.step_k;
}

// Tiles of 64 x 4 voxels in raster order (x tiles fastest, then y tiles, then k), walked grid-stride. The projection is computed
// from (i, j, k) for every voxel; a voxel that fails any test is neither loaded nor stored, so a wave whose 64 voxels all fail
// leaves without a voxel access.
__global__ void __launch_bounds__(kVolBlock) volume_integrate_kernel(VolIntegrateArgs a) {
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
    const float X = vol_centre(a.g.ox, i, a.g.vs), Y = vol_centre(a.g.oy, j, a.g.vs), Z = vol_centre(a.g.oz, k, a.g.vs);
    const float zc = ((a.m2 * X + a.m6 * Y) + a.m10 * Z) + a.m14;
    if (!(zc > 0.0f)) continue;
    // Early-out in front of the two divides and the depth pixel; it only ever skips what the tests below skip: a reading that passes
    // D <= max_depth has D - zc <= max_depth - zc (fp32 subtraction is monotonic), and beyond zc_far = 1.001 (max_depth + mu) that
    // is below -mu by 0.1 %, ten thousand roundings. (The same for the four sides of the image was measured and dropped)
    if (zc > a.zc_far) continue;
    const float xc = ((a.m0 * X + a.m4 * Y) + a.m8 * Z) + a.m12;
    const float yc = ((a.m1 * X + a.m5 * Y) + a.m9 * Z) + a.m13;
    const float u = a.f0 * (xc / zc) + a.cx0, v = a.f0 * (yc / zc) + a.cy0;
    const float xf = floorf(u + 0.5f), yf = floorf(v + 0.5f);
    if (!(xf >= 0.0f && xf < (float)a.cols && yf >= 0.0f && yf < (float)a.rows)) continue;   // (NaN fails too)
    const unsigned raw = a.raw[(int)yf * a.cols + (int)xf];
    if (raw == 0) continue;
    const float D = (float)raw / a.depth_scale;
    if (D > a.max_depth) continue;
    const float sdf = D - zc;
    if (sdf < -a.mu) continue;
    const float s = fminf(1.0f, sdf / a.mu) * 32767.0f;
    uint32_t* p = a.g.vox + ((size_t)k * a.g.ny + j) * a.g.nx + i;
    const uint32_t old = *p;
    const int wo = vol_w(old);
    const float W = (float)wo;
    const float F = ((float)vol_q(old) * W + s) / (W + 1.0f);
    const int qn = (int)rintf(F);
    const int wn = min(wo + 1, a.max_weight);
    *p = ((uint32_t)wn << 16) | ((uint32_t)qn & 0xffffu);
    n_upd++;
    n_band += fabsf(sdf) <= a.mu ? 1u : 0u;
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

void launch_volume_sum(const VolIntegrateArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_sum_kernel, dim3(1), dim3(kVolBlock), 0, s, a);
}

// ---- extraction ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void vol_ijk(const VolGrid& g, int v, int* i, int* j, int* k) {
  const int row = v / g.nx;
  *i = v - row * g.nx;
  *k = row / g.ny;
  *j = row - *k * g.ny;
}

// An edge a -> b carries a point iff both voxels were observed and exactly one of them has q > 0.
__device__ __forceinline__ bool vol_edge(uint32_t va, uint32_t vb) {
  return vol_w(va) > 0 && vol_w(vb) > 0 && (vol_q(va) > 0) != (vol_q(vb) > 0);
}

__global__ void __launch_bounds__(kVolExtBlock) volume_count_kernel(VolExtractArgs a) {
  __shared__ int sh[kVolExtBlock / 64];
  const int v = blockIdx.x * kVolExtBlock + threadIdx.x;
  bool ex = false, ey = false, ez = false;
  if (v < a.n) {
    const uint32_t va = a.g.vox[v];
    if (vol_w(va) > 0) {
      int i, j, k;
      vol_ijk(a.g, v, &i, &j, &k);
      const size_t sy = (size_t)a.g.nx, sz = (size_t)a.g.nx * a.g.ny;
      ex = i + 1 < a.g.nx && vol_edge(va, a.g.vox[v + 1]);
      ey = j + 1 < a.g.ny && vol_edge(va, a.g.vox[v + sy]);
      ez = k + 1 < a.g.nz && vol_edge(va, a.g.vox[v + sz]);
    }
  }
  const unsigned long long bx = __ballot(ex), by = __ballot(ey), bz = __ballot(ez);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* wm = a.wave_mask + 3 * ((size_t)blockIdx.x * (kVolExtBlock / 64) + w);
    wm[0] = bx; wm[1] = by; wm[2] = bz;
    sh[w] = __popcll(bx) + __popcll(by) + __popcll(bz);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int q = 0; q < kVolExtBlock / 64; q++) t += sh[q];
    a.blk[blockIdx.x] = t;
  }
}

// One block: exclusive scan of the per-block counts, 1024 at a time (coalesced loads and stores, a running base), the total, the
// clamp at capacity.
__global__ void __launch_bounds__(kVolScanThreads) volume_scan_kernel(VolExtractArgs a) {
  __shared__ unsigned wsum[kVolScanThreads / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned long long base = 0;
  for (int c0 = 0; c0 < a.nblk; c0 += kVolScanThreads) {
    const int b = c0 + t;
    const unsigned s = b < a.nblk ? (unsigned)a.blk[b] : 0u;   // (<= 3 072 per block: a chunk's sum stays far below 2^32)
    unsigned inc = s;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned before = 0, total = 0;
    for (int q = 0; q < kVolScanThreads / 64; q++) {
      if (q < w) before += wsum[q];
      total += wsum[q];
    }
    if (b < a.nblk) a.blk_off[b] = base + (unsigned long long)(before + inc - s);
    base += total;
    __syncthreads();   // wsum is written again
  }
  if (t == 0) {
    a.ctr->ext_total = base;
    a.ctr->ext_written = base < (unsigned long long)a.capacity ? base : (unsigned long long)a.capacity;
  }
}

// The gradient of Q = (float)q at voxel (i, j, k), whose own word is vc: per axis the central difference over observed neighbours,
// else twice the one-sided difference towards the one that is; false when an axis has neither.
__device__ __forceinline__ bool vol_gradient(const VolGrid& g, int v, int i, int j, int k, uint32_t vc, float* gx, float* gy, float* gz) {
  const float Q = (float)vol_q(vc);
  const int pos[3] = {i, j, k}, dim[3] = {g.nx, g.ny, g.nz};
  const long long stride[3] = {1, g.nx, (long long)g.nx * g.ny};
  float out[3];
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    uint32_t vp = 0, vm = 0;
    if (pos[c] + 1 < dim[c]) vp = g.vox[v + stride[c]];
    if (pos[c] > 0) vm = g.vox[v - stride[c]];
    const bool up = vol_w(vp) > 0, um = vol_w(vm) > 0;   // (a neighbour outside the grid stays 0: w = 0, not usable)
    const float Qp = (float)vol_q(vp), Qm = (float)vol_q(vm);
    float d = 0.0f;
    if (up && um) d = Qp - Qm;
    else if (up) d = 2.0f * (Qp - Q);
    else if (um) d = 2.0f * (Q - Qm);
    else ok = false;
    out[c] = d;
  }
  *gx = out[0]; *gy = out[1]; *gz = out[2];
  return ok;
}

__global__ void __launch_bounds__(kVolExtBlock) volume_scatter_kernel(VolExtractArgs a) {
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
  if (idx >= (unsigned long long)a.capacity) return;   // (so are this voxel's later edges)
  int i, j, k;
  vol_ijk(a.g, v, &i, &j, &k);
  const uint32_t va = a.g.vox[v];
  const float qa = (float)vol_q(va);
  float gax, gay, gaz;
  const bool has_a = vol_gradient(a.g, v, i, j, k, va, &gax, &gay, &gaz);
  const float cx = vol_centre(a.g.ox, i, a.g.vs), cy = vol_centre(a.g.oy, j, a.g.vs), cz = vol_centre(a.g.oz, k, a.g.vs);
  const unsigned long long bits[3] = {bx, by, bz};
  const long long stride[3] = {1, a.g.nx, (long long)a.g.nx * a.g.ny};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (!(bits[c] & bit)) continue;
    if (idx >= (unsigned long long)a.capacity) return;
    const int vb_i = (int)(v + stride[c]);
    const uint32_t vb = a.g.vox[vb_i];
    const float alpha = qa / (qa - (float)vol_q(vb));
    const float step = alpha * a.g.vs;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, gbx, gby, gbz;
    const bool has_b = vol_gradient(a.g, vb_i, i + (c == 0), j + (c == 1), k + (c == 2), vb, &gbx, &gby, &gbz);
    if (has_a && has_b) {
      const float mx = gax + alpha * (gbx - gax), my = gay + alpha * (gby - gay), mz = gaz + alpha * (gbz - gaz);
      const float len = sqrtf((mx * mx + my * my) + mz * mz);
      if (len > 0.0f) { nx = mx / len; ny = my / len; nz = mz / len; }
    }
    a.xyz0[idx] = make_float4(c == 0 ? cx + step : cx, c == 1 ? cy + step : cy, c == 2 ? cz + step : cz, 0.0f);
    a.nrmw[idx] = make_float4(nx, ny, nz, (float)min(vol_w(va), vol_w(vb)));
    idx++;
  }
}

void launch_volume_extract(const VolExtractArgs& a, hipStream_t s) {
  const dim3 grid(a.nblk), block(kVolExtBlock);
  hipLaunchKernelGGL(volume_count_kernel, grid, block, 0, s, a);
  hipLaunchKernelGGL(volume_scan_kernel, dim3(1), dim3(kVolScanThreads), 0, s, a);
  hipLaunchKernelGGL(volume_scatter_kernel, grid, block, 0, s, a);
}

}  // namespace odo
