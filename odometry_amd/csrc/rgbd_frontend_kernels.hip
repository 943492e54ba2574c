// rgbd_frontend_kernels.hip — the RGB-D front end's kernels (rgbd_frontend.hip.h) as a translation unit of their own, plus their
// host-side launcher. Compiled with the library's flags: -ffp-contract=off and IEEE fp32 divides, so every operation below rounds once.
#include <hip/hip_runtime.h>
#include "rgbd_frontend.hip.h"

namespace odo {

// The 8-bit BT.601 fixed-point rule (weights sum to 2^14: R = G = B = v gives v).
__device__ __forceinline__ float fe_grey(unsigned r, unsigned g, unsigned b) {
  return (float)((r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14);
}
// c0 / c2: the first / third byte of the pixel in memory.
__device__ __forceinline__ float fe_grey_mem(unsigned c0, unsigned c1, unsigned c2, int bgr) {
  return bgr ? fe_grey(c2, c1, c0) : fe_grey(c0, c1, c2);
}

__global__ void __launch_bounds__(kFeBlock) rgbd_fe_grey_kernel(FeArgs a) {
  const long long n = (long long)a.rows * a.cols;
  const long long g = (long long)blockIdx.x * kFeBlock + threadIdx.x;   // group of four pixels
  const long long p0 = 4 * g;
  if (g == 0) a.ctr->fill_ticket = 0ull;
  if (p0 >= n) return;
  if (p0 + 4 <= n) {
    float4 o;
    if (a.channels == 4) {
      const uint4 w = *reinterpret_cast<const uint4*>(a.colour + 16 * g);
      o.x = fe_grey_mem(w.x & 255u, (w.x >> 8) & 255u, (w.x >> 16) & 255u, a.bgr);
      o.y = fe_grey_mem(w.y & 255u, (w.y >> 8) & 255u, (w.y >> 16) & 255u, a.bgr);
      o.z = fe_grey_mem(w.z & 255u, (w.z >> 8) & 255u, (w.z >> 16) & 255u, a.bgr);
      o.w = fe_grey_mem(w.w & 255u, (w.w >> 8) & 255u, (w.w >> 16) & 255u, a.bgr);
    } else {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(a.colour + 12 * g);   // four pixels = three dwords
      const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
      o.x = fe_grey_mem(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u, a.bgr);
      o.y = fe_grey_mem(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u, a.bgr);
      o.z = fe_grey_mem((w1 >> 16) & 255u, w1 >> 24, w2 & 255u, a.bgr);
      o.w = fe_grey_mem((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24, a.bgr);
    }
    *reinterpret_cast<float4*>(a.gray + p0) = o;
    *reinterpret_cast<uint4*>(a.zbuf + p0) = make_uint4(kFeEmpty, kFeEmpty, kFeEmpty, kFeEmpty);
  } else {
    for (long long p = p0; p < n; p++) {   // the frame's last one to three pixels
      const uint8_t* px = a.colour + p * a.channels;
      a.gray[p] = fe_grey_mem(px[0], px[1], px[2], a.bgr);
      a.zbuf[p] = kFeEmpty;
    }
  }
}

// Row i of P_c = R P_d + t in the operand order of world_point (odo_math.h).
#define FE_ROW(i, X, Y, Z) (((a.e[4 * (i)] * (X) + a.e[4 * (i) + 1] * (Y)) + a.e[4 * (i) + 2] * (Z)) + a.e[4 * (i) + 3])

__global__ void __launch_bounds__(kFeBlock) rgbd_fe_register_kernel(FeArgs a) {
  __shared__ unsigned sh[kFeBlock / 64][4];
  const long long nd = (long long)a.depth_rows * a.depth_cols;
  const long long stride = (long long)gridDim.x * kFeBlock;
  unsigned n_has = 0u, n_behind = 0u, n_range = 0u, n_splat = 0u;   // the same in every lane of a wave
  // (base is the same for the whole block, so every lane of a wave takes part in every ballot)
  for (long long base = (long long)blockIdx.x * kFeBlock; base < nd; base += stride) {
    const long long i = base + threadIdx.x;
    const int r = i < nd ? (int)a.depth[i] : 0;
    const bool has = r != 0;
    bool behind = false, range = false, splat = false;
    if (has) {
      const int y = (int)(i / a.depth_cols), x = (int)(i - (long long)y * a.depth_cols);
      const float z = (float)r / a.scale_in;
      const float xf = (float)x, yf = (float)y;
      const float Xa = ((xf + -0.5f) - a.cxd) / a.fxd * z, Ya = ((yf + -0.5f) - a.cyd) / a.fyd * z;
      const float Xm = ((xf + 0.0f) - a.cxd) / a.fxd * z, Ym = ((yf + 0.0f) - a.cyd) / a.fyd * z;
      const float Xb = ((xf + 0.5f) - a.cxd) / a.fxd * z, Yb = ((yf + 0.5f) - a.cyd) / a.fyd * z;
      const float X0 = FE_ROW(0, Xa, Ya, z), Y0 = FE_ROW(1, Xa, Ya, z), Z0 = FE_ROW(2, Xa, Ya, z);
      const float X1 = FE_ROW(0, Xb, Yb, z), Y1 = FE_ROW(1, Xb, Yb, z), Z1 = FE_ROW(2, Xb, Yb, z);
      const float Zm = FE_ROW(2, Xm, Ym, z);
      if (!(Z0 > 0.0f && Z1 > 0.0f && Zm > 0.0f)) {
        behind = true;
      } else {
        const float q = rintf(Zm * a.scale_out);
        const float u0 = a.f * (X0 / Z0) + a.cx, u1 = a.f * (X1 / Z1) + a.cx;
        const float v0 = a.f * (Y0 / Z0) + a.cy, v1 = a.f * (Y1 / Z1) + a.cy;
        if (!(q >= 1.0f && q <= 65535.0f) || !(isfinite(u0) && isfinite(u1) && isfinite(v0) && isfinite(v1))) {
          range = true;
        } else {
          // target pixels whose centres lie in the half-open footprint: columns ua .. ub, rows va .. vb (fp32 throughout: the
          // values may be far outside any integer type)
          const float ua = ceilf(fminf(u0, u1)), ub = ceilf(fmaxf(u0, u1)) - 1.0f;
          const float va = ceilf(fminf(v0, v1)), vb = ceilf(fmaxf(v0, v1)) - 1.0f;
          if ((ub - ua) + 1.0f > (float)kFeMaxSplat || (vb - va) + 1.0f > (float)kFeMaxSplat) {
            splat = true;
          } else {
            const float ulo = fmaxf(ua, 0.0f), uhi = fminf(ub, (float)(a.cols - 1));
            const float vlo = fmaxf(va, 0.0f), vhi = fminf(vb, (float)(a.rows - 1));
            if (ulo <= uhi && vlo <= vhi) {   // inside the image, hence inside int: at most 4 x 4 pixels
              const int iu0 = (int)ulo, iu1 = (int)uhi, iv0 = (int)vlo, iv1 = (int)vhi;
              const uint32_t qi = (uint32_t)q;
              for (int v = iv0; v <= iv1; v++)
                for (int u = iu0; u <= iu1; u++)
                  (void)__hip_atomic_fetch_min(a.zbuf + (size_t)v * a.cols + u, qi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
        }
      }
    }
    n_has += (unsigned)__popcll(__ballot(has));
    n_behind += (unsigned)__popcll(__ballot(behind));
    n_range += (unsigned)__popcll(__ballot(range));
    n_splat += (unsigned)__popcll(__ballot(splat));
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) { sh[t >> 6][0] = n_has; sh[t >> 6][1] = n_behind; sh[t >> 6][2] = n_range; sh[t >> 6][3] = n_splat; }
  __syncthreads();
  if (t < 4) {
    unsigned n = 0u;
    for (int k = 0; k < kFeBlock / 64; k++) n += sh[k][t];
    a.ctr->reg[blockIdx.x][t] = n;   // read by the resolve kernel's last block
  }
}
#undef FE_ROW

__global__ void __launch_bounds__(kFeBlock) rgbd_fe_resolve_kernel(FeArgs a, int reg_blocks) {
  __shared__ unsigned sh[kFeBlock / 64];
  __shared__ unsigned long long red[4][kFeBlock / 64];
  __shared__ unsigned long long last_total;   // ~0: this block is not the last one
  const long long n = (long long)a.rows * a.cols;
  const long long stride = 4ll * gridDim.x * kFeBlock;
  unsigned cnt = 0u;   // the same in every lane of a wave
  for (long long base = 4ll * blockIdx.x * kFeBlock; base < n; base += stride) {
    const long long p0 = base + 4 * threadIdx.x;
    bool f0 = false, f1 = false, f2 = false, f3 = false;
    if (p0 + 4 <= n) {
      const uint4 w = *reinterpret_cast<const uint4*>(a.zbuf + p0);
      f0 = w.x != kFeEmpty; f1 = w.y != kFeEmpty; f2 = w.z != kFeEmpty; f3 = w.w != kFeEmpty;
      uint2 o;   // values written by the register kernel are 1 .. 65535
      o.x = (f0 ? w.x : 0u) | ((f1 ? w.y : 0u) << 16);
      o.y = (f2 ? w.z : 0u) | ((f3 ? w.w : 0u) << 16);
      *reinterpret_cast<uint2*>(a.out + p0) = o;
    } else if (p0 < n) {   // the frame's last one to three pixels
      for (long long p = p0; p < n; p++) {
        const uint32_t w = a.zbuf[p];
        const bool f = w != kFeEmpty;
        a.out[p] = f ? (uint16_t)w : (uint16_t)0;
        if (p == p0) f0 = f; else if (p == p0 + 1) f1 = f; else f2 = f;
      }
    }
    cnt += (unsigned)(__popcll(__ballot(f0)) + __popcll(__ballot(f1)) + __popcll(__ballot(f2)) + __popcll(__ballot(f3)));
  }
  const int t = threadIdx.x;
  if ((t & 63) == 0) sh[t >> 6] = cnt;
  __syncthreads();
  if (t == 0) {
    unsigned tot = 0u;
    for (int k = 0; k < kFeBlock / 64; k++) tot += sh[k];
    // one atomic per block: its ticket in the high half, its count in the low half; the block whose ticket is the last one reads
    // the others' sum off the value the add returns. Release / acquire at agent scope: the completion word below is seen by the
    // host before this launch has ended, so every block's depth values must have left its XCD's L2 before its ticket counts
    const unsigned long long old = __hip_atomic_fetch_add(&a.ctr->fill_ticket, (1ull << 32) | tot, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    last_total = (unsigned)(old >> 32) == gridDim.x - 1 ? (old & 0xffffffffull) + tot : ~0ull;
  }
  __syncthreads();
  if (last_total == ~0ull) return;
  // the last block: the register kernel's rows (an earlier launch on the same stream), summed
  unsigned long long s0 = 0ull, s1 = 0ull, s2 = 0ull, s3 = 0ull;
  for (int b = t; b < reg_blocks; b += kFeBlock) { s0 += a.ctr->reg[b][0]; s1 += a.ctr->reg[b][1]; s2 += a.ctr->reg[b][2]; s3 += a.ctr->reg[b][3]; }
  for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_down(s0, o); s1 += __shfl_down(s1, o); s2 += __shfl_down(s2, o); s3 += __shfl_down(s3, o); }
  if ((t & 63) == 0) { red[0][t >> 6] = s0; red[1][t >> 6] = s1; red[2][t >> 6] = s2; red[3][t >> 6] = s3; }
  __syncthreads();
  if (t == 0) {
    long long tot[4];
    for (int q = 0; q < 4; q++) {
      unsigned long long v = 0ull;
      for (int k = 0; k < kFeBlock / 64; k++) v += red[q][k];
      tot[q] = (long long)v;
    }
    a.stats[0] = tot[0];
    a.stats[1] = (long long)last_total;
    a.stats[2] = tot[1];
    a.stats[3] = tot[2];
    a.stats[4] = tot[3];
    a.stats[5] = a.frame;
    __hip_atomic_store(a.done_flag, a.token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

void launch_rgbd_frontend(const FeArgs& a, hipStream_t s) {
  const long long n = (long long)a.rows * a.cols, nd = (long long)a.depth_rows * a.depth_cols;
  const long long groups = ((n + 3) / 4 + kFeBlock - 1) / kFeBlock, dblocks = (nd + kFeBlock - 1) / kFeBlock;
  const unsigned gb = (unsigned)groups;
  const unsigned rb = (unsigned)(dblocks < kFeRegBlocksMax ? dblocks : kFeRegBlocksMax);
  const unsigned sb = (unsigned)(groups < kFeResBlocksMax ? groups : kFeResBlocksMax);
  hipLaunchKernelGGL(rgbd_fe_grey_kernel, dim3(gb), dim3(kFeBlock), 0, s, a);
  hipLaunchKernelGGL(rgbd_fe_register_kernel, dim3(rb), dim3(kFeBlock), 0, s, a);
  hipLaunchKernelGGL(rgbd_fe_resolve_kernel, dim3(sb), dim3(kFeBlock), 0, s, a, (int)rb);
}

}  // namespace odo
