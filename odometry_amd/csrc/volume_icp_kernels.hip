// volume_icp_kernels.hip — the kernels of the TSDF volume's frame-to-model alignment (volume_icp.hip.h) as a translation unit of their
// own, plus their host-side launchers: kernel templates over the number of sums N, instantiated for the geometric rows alone
// (N = ODO_NACC = 29) and for the geometric and the photometric rows (N = kIcpPhotoAcc = 31). The arithmetic is the table of
// include/odometry_hip.h (odo_volume_icp_align_dev, odo_volume_icp_photo_align_dev) / DESIGN.md sections 9.8 and 9.10 and lives in
// volume_icp_math.h and volume_icp_photo_math.h over odo_math.h — fp32, one rounding per operation, the unit is built with
// -ffp-contract=off and correctly rounded divide and sqrt; the sums are fp64 over exact products. The kernels add the pixel of a
// thread, the loads, the fixed order of the sums and the stores.
#include <hip/hip_runtime.h>
#include "volume_icp.hip.h"

namespace odo {

template <int N>
__global__ void __launch_bounds__(64) volume_icp_init_kernel(IcpStateT<N>* st, IcpInit init) {
  const int t = threadIdx.x;
  if (t < N) st->acc[t] = 0.0;
  if (t < 6) st->delta[t] = 0.0f;
  if (t < kIcpMaxLevels) st->done[t] = 0;
  if (t == 0) {
#pragma unroll
    for (int i = 0; i < 16; i++) st->C[i] = init.C[i];   // (constant indices: the by-value argument stays in registers)
    st->status = 0; st->iterations = 0; st->trace_n = 0; st->evaluated = 0; st->pad_ = 0;
  }
}

// The eight lanes that share a sum: lane s has added its terms in ascending order; the tree adds the lanes as ((0 + 4) + (2 + 6)) +
// ((1 + 5) + (3 + 7)).
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

// A thread per lattice point of the stride. Every thread publishes its row (zeros without a pair) in LDS — with the photometric
// term its two rows: row t the geometric one, row 256 + t the photometric one — kIcpRow floats apart (odd, so that the eight rows
// eight lanes read at once lie in eight different groups of banks, in either half). Thread 8 q + s then adds the exact fp64 terms
// of sum q over the rows s, s + 8, s + 16, ... in that order — sums 0 .. 27 over all the rows, the geometric count over the first
// 256, the photometric count and cost over the last 256 — and the eight lanes of a sum are folded by icp_fold8: one N-double partial
// per block, plain stores.
template <int N>
__global__ void __launch_bounds__(kIcpBlock) volume_icp_rows_kernel(VolIcpRowsArgs<N> a) {
  constexpr bool kPhoto = N == kIcpPhotoAcc;
  constexpr int kRows = kPhoto ? kIcpPhotoRows : kIcpBlock;   // rows in LDS
  constexpr int kOut = kPhoto ? 16 : 8;                       // floats per pixel of rows_dev
  const IcpStateT<N>* st = a.state;
  if (st->status != 0 || st->done[a.level] != 0) return;   // (uniform over the grid: no thread reaches the barrier)
  __shared__ float sh[kRows * kIcpRow];
  const int t = threadIdx.x;
  const int x = (blockIdx.x * kIcpTile + t % kIcpTile) * a.stride;
  const int y = (blockIdx.y * kIcpTile + t / kIcpTile) * a.stride;
  float Jg[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rg = 0.0f, wg = 0.0f;
  [[maybe_unused]] float Jp[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, rp = 0.0f, wp = 0.0f;
  bool geo = false;
  [[maybe_unused]] bool photo = false;
  if (x < a.cols && y < a.rows) {
    float C[16];
#pragma unroll
    for (int i = 0; i < 16; i++) C[i] = st->C[i];
    IcpView v;
    v.rows = a.rows; v.cols = a.cols; v.f = a.f; v.cx = a.cx; v.cy = a.cy;
    v.depth_scale = a.depth_scale; v.max_depth = a.max_depth; v.dist_max = a.dist_max; v.huber_delta = a.huber_delta;
    v.m[0] = a.m0; v.m[1] = a.m1; v.m[2] = a.m2; v.m[3] = a.m3; v.m[4] = a.m4; v.m[5] = a.m5; v.m[6] = a.m6; v.m[7] = a.m7; v.m[8] = a.m8;
    geo = icp_row(v, C, a.raw, a.depth_m, a.nrmw_m, x, y, Jg, &rg, &wg);
    if constexpr (kPhoto) {
      IcpPhotoView ph;
      ph.weight = a.photo_weight; ph.huber_delta = a.photo_huber;
      photo = icp_photo_row(v, ph, C, a.raw, a.grey, a.depth_m, a.rgba_m, x, y, Jp, &rp, &wp);
    }
  }
  icp_publish(sh + t * kIcpRow, Jg, rg, wg, geo);
  if constexpr (kPhoto) icp_publish(sh + (kIcpBlock + t) * kIcpRow, Jp, rp, wp, photo);
  if (a.rows_dev) {   // the thread's stride x stride cell of the frame: its own pixel first, zeros for the others
    for (int dy = 0; dy < a.stride; dy++)
      for (int dx = 0; dx < a.stride; dx++) {
        const int px = x + dx, py = y + dy;
        if (px >= a.cols || py >= a.rows) continue;
        const bool me = (dx == 0 && dy == 0);
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float4* o = reinterpret_cast<float4*>(a.rows_dev + ((size_t)py * a.cols + px) * kOut);
        o[0] = me ? make_float4(Jg[0], Jg[1], Jg[2], Jg[3]) : zero;
        o[1] = me ? make_float4(Jg[4], Jg[5], rg, wg) : zero;
        if constexpr (kPhoto) {
          o[2] = me ? make_float4(Jp[0], Jp[1], Jp[2], Jp[3]) : zero;
          o[3] = me ? make_float4(Jp[4], Jp[5], rp, wp) : zero;
        }
      }
  }
  __syncthreads();
  if (t < N * kIcpFoldLanes) {
    const int q = t / kIcpFoldLanes, s = t % kIcpFoldLanes;
    double v = 0.0;
    if constexpr (kPhoto) {
      // One loop for every lane, so that the wave which holds sums 24 .. 30 does not walk the rows once per kind of sum: a lane's sum
      // is described by its operands, whether it counts, and the half of the rows it covers; a row outside that half is not added.
      int ia, ib;
      icp_term_operands(q < ODO_NACC - 1 ? q : ODO_NACC - 2, &ia, &ib);   // (sum 30 is sum 27's term; the counts read row[8])
      const bool count = (q == ODO_NACC - 1 || q == ODO_NACC);
      const int lo = q < ODO_NACC ? 0 : kIcpBlock, hi = q == ODO_NACC - 1 ? kIcpBlock : kRows;
#pragma unroll 8
      for (int i = s; i < kRows; i += kIcpFoldLanes) {   // (unrolled: the LDS reads of eight rows in flight, the adds in order)
        const float* row = sh + i * kIcpRow;
        const double term = count ? (double)row[8] : icp_term(row, ia, ib);
        if (i >= lo && i < hi) v += term;
      }
    } else {
      // The same additions in the same order with lo = 0, hi = 256. Kept as two loops, a lane's kind of sum chosen outside them:
      // instantiated for 256 rows the single loop above took 6.96 / 7.29 / 8.79 us at strides 4 / 2 / 1 against these loops' 6.32 /
      // 6.60 / 8.41.
      int ia, ib;
      icp_term_operands(q, &ia, &ib);
      if (q < ODO_NACC - 1) {
        for (int i = s; i < kRows; i += kIcpFoldLanes) v += icp_term(sh + i * kIcpRow, ia, ib);
      } else {
        for (int i = s; i < kRows; i += kIcpFoldLanes) v += (double)sh[i * kIcpRow + 8];
      }
    }
    v = icp_fold8(v);
    if (s == 0) a.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * N + q] = v;
  }
}

// One block. Thread 8 q + s adds sum q of the partials s, s + 8, s + 16, ... in that order, icp_fold8 folds the eight lanes, and
// thread 0 takes the step (icp_step, on the first 29 sums) on the state, or with take_step == 0 only leaves the folded sums in it.
template <int N>
__global__ void __launch_bounds__(kIcpBlock) volume_icp_step_kernel(VolIcpStepArgs<N> a) {
  IcpStateT<N>* st = a.state;
  if (st->status != 0 || st->done[a.level] != 0) return;
  __shared__ double sum[N];
  const int t = threadIdx.x;
  if (t < N * kIcpFoldLanes) {
    const int q = t / kIcpFoldLanes, s = t % kIcpFoldLanes;
    double v = 0.0;
#pragma unroll 8
    for (int b = s; b < a.nblk; b += kIcpFoldLanes) v += a.partials[(size_t)b * N + q];   // (unrolled: the loads of eight partials in flight, the adds in order)
    v = icp_fold8(v);
    if (s == 0) sum[q] = v;
  }
  __syncthreads();
  if (t < N) st->acc[t] = sum[t];
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
    IcpTraceRowT<N>* r = a.trace + n;
    r->level = a.level; r->iteration = n;
    for (int i = 0; i < N; i++) r->acc[i] = sum[i];
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

template <int N> void launch_volume_icp_init(IcpStateT<N>* state, const IcpInit& init, hipStream_t s) {
  hipLaunchKernelGGL(volume_icp_init_kernel<N>, dim3(1), dim3(64), 0, s, state, init);
}
template <int N> void launch_volume_icp_rows(const VolIcpRowsArgs<N>& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_icp_rows_kernel<N>, volume_icp_grid(a.rows, a.cols, a.stride), dim3(kIcpBlock), 0, s, a);
}
template <int N> void launch_volume_icp_step(const VolIcpStepArgs<N>& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_icp_step_kernel<N>, dim3(1), dim3(kIcpBlock), 0, s, a);
}

template void launch_volume_icp_init<ODO_NACC>(IcpState*, const IcpInit&, hipStream_t);
template void launch_volume_icp_rows<ODO_NACC>(const VolIcpRowsArgs<ODO_NACC>&, hipStream_t);
template void launch_volume_icp_step<ODO_NACC>(const VolIcpStepArgs<ODO_NACC>&, hipStream_t);
template void launch_volume_icp_init<kIcpPhotoAcc>(IcpPhotoState*, const IcpInit&, hipStream_t);
template void launch_volume_icp_rows<kIcpPhotoAcc>(const VolIcpRowsArgs<kIcpPhotoAcc>&, hipStream_t);
template void launch_volume_icp_step<kIcpPhotoAcc>(const VolIcpStepArgs<kIcpPhotoAcc>&, hipStream_t);

}  // namespace odo
