// volume_icp_photo_kernels.hip — the kernels of the TSDF volume's frame-to-model alignment with a photometric term
// (volume_icp_photo.hip.h) as a translation unit of their own, plus their host-side launchers. The arithmetic is the table of
// include/odometry_hip.h (odo_volume_icp_photo_align_dev) / DESIGN.md section 9.10 and lives in volume_icp_photo_math.h over
// volume_icp_math.h — fp32, one rounding per operation, the unit is built with -ffp-contract=off and correctly rounded divide and
// sqrt; the sums are fp64 over exact products. The kernels add the pixel of a thread, the loads, the fixed order of the sums and the
// stores, as volume_icp_kernels.hip does for the geometric rows alone.
#include <hip/hip_runtime.h>
#include "volume_icp_photo.hip.h"

namespace odo {

__global__ void __launch_bounds__(64) volume_icp_photo_init_kernel(IcpPhotoState* st, IcpInit init) {
  const int t = threadIdx.x;
  if (t < kIcpPhotoAcc) st->acc[t] = 0.0;
  if (t < 6) st->delta[t] = 0.0f;
  if (t < kIcpMaxLevels) st->done[t] = 0;
  if (t == 0) {
#pragma unroll
    for (int i = 0; i < 16; i++) st->C[i] = init.C[i];
    st->status = 0; st->iterations = 0; st->trace_n = 0; st->evaluated = 0; st->pad_ = 0;
  }
}

// The eight lanes that share a sum, folded as volume_icp_kernels.hip folds them: ((0 + 4) + (2 + 6)) + ((1 + 5) + (3 + 7)).
static __device__ __forceinline__ double icp_fold8(double v) {
  v += __shfl_xor(v, 4, kIcpFoldLanes);
  v += __shfl_xor(v, 2, kIcpFoldLanes);
  v += __shfl_xor(v, 1, kIcpFoldLanes);
  return v;
}

static __device__ __forceinline__ void icp_publish(float* row, const float J[6], float res, float w, bool pair) {
  row[0] = J[0]; row[1] = J[1]; row[2] = J[2]; row[3] = J[3]; row[4] = J[4]; row[5] = J[5];
  row[6] = res; row[7] = w; row[8] = pair ? 1.0f : 0.0f;
}

// A thread per lattice point of the stride. Every thread publishes its two rows (zeros without a pair) in LDS: row t the geometric
// one, row 256 + t the photometric one, kIcpRow floats apart (odd, so that the eight rows eight lanes read at once lie in eight
// different groups of banks, in either half). Thread 8 q + s then adds the exact fp64 terms of sum q over the rows s, s + 8,
// s + 16, ... in that order — sums 0 .. 27 over all 512, the geometric count over the first 256, the photometric count and cost
// over the last 256 — and the eight lanes of a sum are folded by icp_fold8: one 31-double partial per block, plain stores.
__global__ void __launch_bounds__(kIcpBlock) volume_icp_photo_rows_kernel(VolIcpPhotoRowsArgs a) {
  const IcpPhotoState* st = a.state;
  if (st->status != 0 || st->done[a.level] != 0) return;   // (uniform over the grid: no thread reaches the barrier)
  __shared__ float sh[kIcpPhotoRows * kIcpRow];
  const int t = threadIdx.x;
  const int x = (blockIdx.x * kIcpTile + t % kIcpTile) * a.stride;
  const int y = (blockIdx.y * kIcpTile + t / kIcpTile) * a.stride;
  float Jg[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rg = 0.0f, wg = 0.0f;
  float Jp[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rp = 0.0f, wp = 0.0f;
  bool geo = false, photo = false;
  if (x < a.cols && y < a.rows) {
    float C[16];
#pragma unroll
    for (int i = 0; i < 16; i++) C[i] = st->C[i];
    IcpView v;
    v.rows = a.rows; v.cols = a.cols; v.f = a.f; v.cx = a.cx; v.cy = a.cy;
    v.depth_scale = a.depth_scale; v.max_depth = a.max_depth; v.dist_max = a.dist_max; v.huber_delta = a.huber_delta;
    v.m[0] = a.m0; v.m[1] = a.m1; v.m[2] = a.m2; v.m[3] = a.m3; v.m[4] = a.m4; v.m[5] = a.m5; v.m[6] = a.m6; v.m[7] = a.m7; v.m[8] = a.m8;
    IcpPhotoView ph;
    ph.weight = a.photo_weight; ph.huber_delta = a.photo_huber;
    geo = icp_row(v, C, a.raw, a.depth_m, a.nrmw_m, x, y, Jg, &rg, &wg);
    photo = icp_photo_row(v, ph, C, a.raw, a.grey, a.depth_m, a.rgba_m, x, y, Jp, &rp, &wp);
  }
  icp_publish(sh + t * kIcpRow, Jg, rg, wg, geo);
  icp_publish(sh + (kIcpBlock + t) * kIcpRow, Jp, rp, wp, photo);
  if (a.rows_dev) {   // the thread's stride x stride cell of the frame: its own pixel first, zeros for the others
    for (int dy = 0; dy < a.stride; dy++)
      for (int dx = 0; dx < a.stride; dx++) {
        const int px = x + dx, py = y + dy;
        if (px >= a.cols || py >= a.rows) continue;
        const bool me = (dx == 0 && dy == 0);
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4* o = reinterpret_cast<float4*>(a.rows_dev + ((size_t)py * a.cols + px) * 16);
        o[0] = me ? make_float4(Jg[0], Jg[1], Jg[2], Jg[3]) : zero;
        o[1] = me ? make_float4(Jg[4], Jg[5], rg, wg) : zero;
        o[2] = me ? make_float4(Jp[0], Jp[1], Jp[2], Jp[3]) : zero;
        o[3] = me ? make_float4(Jp[4], Jp[5], rp, wp) : zero;
      }
  }
  __syncthreads();
  if (t < kIcpPhotoAcc * kIcpFoldLanes) {
    const int q = t / kIcpFoldLanes, s = t % kIcpFoldLanes;
    // One loop for every lane, so that the wave which holds sums 24 .. 30 does not walk the rows once per kind of sum: a lane's sum
    // is described by its operands, whether it counts, and the half of the rows it covers; a row outside that half is not added.
    int ia, ib;
    icp_term_operands(q < ODO_NACC - 1 ? q : ODO_NACC - 2, &ia, &ib);   // (sum 30 is sum 27's term; the counts read row[8])
    const bool count = (q == ODO_NACC - 1 || q == ODO_NACC);
    const int lo = q < ODO_NACC ? 0 : kIcpBlock, hi = q == ODO_NACC - 1 ? kIcpBlock : kIcpPhotoRows;
    double v = 0.0;
#pragma unroll 8
    for (int i = s; i < kIcpPhotoRows; i += kIcpFoldLanes) {   // (unrolled: the LDS reads of eight rows in flight, the adds in order)
      const float* row = sh + i * kIcpRow;
      const double term = count ? (double)row[8] : icp_term(row, ia, ib);
      if (i >= lo && i < hi) v += term;
    }
    v = icp_fold8(v);
    if (s == 0) a.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kIcpPhotoAcc + q] = v;
  }
}

// One block. Thread 8 q + s adds sum q of the partials s, s + 8, s + 16, ... in that order, icp_fold8 folds the eight lanes, and
// thread 0 takes the step (icp_step on the first 29 sums) on the state, or with take_step == 0 only leaves the folded sums in it.
__global__ void __launch_bounds__(kIcpBlock) volume_icp_photo_step_kernel(VolIcpPhotoStepArgs a) {
  IcpPhotoState* st = a.state;
  if (st->status != 0 || st->done[a.level] != 0) return;
  __shared__ double sum[kIcpPhotoAcc];
  const int t = threadIdx.x;
  if (t < kIcpPhotoAcc * kIcpFoldLanes) {
    const int q = t / kIcpFoldLanes, s = t % kIcpFoldLanes;
    double v = 0.0;
#pragma unroll 8
    for (int b = s; b < a.nblk; b += kIcpFoldLanes) v += a.partials[(size_t)b * kIcpPhotoAcc + q];   // (unrolled: the loads of eight partials in flight, the adds in order)
    v = icp_fold8(v);
    if (s == 0) sum[q] = v;
  }
  __syncthreads();
  if (t < kIcpPhotoAcc) st->acc[t] = sum[t];
  if (t != 0) return;
  st->evaluated = 1;
  if (!a.take_step) return;
  float C[16], delta[6];
#pragma unroll
  for (int i = 0; i < 16; i++) C[i] = st->C[i];
  int converged = 0;
  const int failed = icp_step(sum, a.min_pairs, a.eps_t, a.eps_r, C, delta, &converged);
  const int n = st->iterations;
#pragma unroll
  for (int i = 0; i < 16; i++) st->C[i] = C[i];
#pragma unroll
  for (int i = 0; i < 6; i++) st->delta[i] = delta[i];
  if (a.trace && n < a.trace_capacity) {
    IcpPhotoTraceRow* r = a.trace + n;
    r->level = a.level; r->iteration = n;
    for (int i = 0; i < kIcpPhotoAcc; i++) r->acc[i] = sum[i];
#pragma unroll
    for (int i = 0; i < 6; i++) r->delta[i] = delta[i];
#pragma unroll
    for (int i = 0; i < 16; i++) r->C[i] = C[i];
    st->trace_n = n + 1;
  }
  st->iterations = n + 1;
  if (failed) st->status = 1;
  else if (converged) st->done[a.level] = 1;
}

void launch_volume_icp_photo_init(IcpPhotoState* state, const IcpInit& init, hipStream_t s) {
  hipLaunchKernelGGL(volume_icp_photo_init_kernel, dim3(1), dim3(64), 0, s, state, init);
}
void launch_volume_icp_photo_rows(const VolIcpPhotoRowsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_icp_photo_rows_kernel, volume_icp_grid(a.rows, a.cols, a.stride), dim3(kIcpBlock), 0, s, a);
}
void launch_volume_icp_photo_step(const VolIcpPhotoStepArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_icp_photo_step_kernel, dim3(1), dim3(kIcpBlock), 0, s, a);
}

}  // namespace odo
