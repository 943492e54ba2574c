// volume_icp_kernels.hip — the kernels of the TSDF volume's frame-to-model alignment (volume_icp.hip.h) as a translation unit of their
// own, plus their host-side launchers. The arithmetic is the table of include/odometry_hip.h (odo_volume_icp_align_dev) / DESIGN.md
// section 9.8 and lives in volume_icp_math.h over odo_math.h — fp32, one rounding per operation, the unit is built with
// -ffp-contract=off and correctly rounded divide and sqrt; the sums are fp64 over exact products. The kernels add the pixel of a
// thread, the loads, the fixed order of the sums and the stores.
#include <hip/hip_runtime.h>
#include "volume_icp.hip.h"
#include "volume_icp_math.h"

namespace odo {

__global__ void __launch_bounds__(64) volume_icp_init_kernel(IcpState* st, IcpInit init) {
  const int t = threadIdx.x;
  if (t < ODO_NACC) st->acc[t] = 0.0;
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
__device__ __forceinline__ double icp_fold8(double v) {
  v += __shfl_xor(v, 4, kIcpFoldLanes);
  v += __shfl_xor(v, 2, kIcpFoldLanes);
  v += __shfl_xor(v, 1, kIcpFoldLanes);
  return v;
}

// A thread per lattice point of the stride. Every thread publishes its row (zeros without a pair) in LDS; thread 8 q + s then adds
// the exact fp64 terms of sum q over the rows s, s + 8, s + 16, ... of the block in that order, and the eight lanes of a sum are
// folded by icp_fold8: one 29-double partial per block, plain stores.
__global__ void __launch_bounds__(kIcpBlock) volume_icp_rows_kernel(VolIcpRowsArgs a) {
  const IcpState* st = a.state;
  if (st->status != 0 || st->done[a.level] != 0) return;   // (uniform over the grid: no thread reaches the barrier)
  __shared__ float sh[kIcpBlock * kIcpRow];
  const int t = threadIdx.x;
  const int x = (blockIdx.x * kIcpTile + t % kIcpTile) * a.stride;
  const int y = (blockIdx.y * kIcpTile + t / kIcpTile) * a.stride;
  float J[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, res = 0.0f, w = 0.0f;
  bool pair = false;
  if (x < a.cols && y < a.rows) {
    float C[16];
#pragma unroll
    for (int i = 0; i < 16; i++) C[i] = st->C[i];
    IcpView v;
    v.rows = a.rows; v.cols = a.cols; v.f = a.f; v.cx = a.cx; v.cy = a.cy;
    v.depth_scale = a.depth_scale; v.max_depth = a.max_depth; v.dist_max = a.dist_max; v.huber_delta = a.huber_delta;
    v.m[0] = a.m0; v.m[1] = a.m1; v.m[2] = a.m2; v.m[3] = a.m3; v.m[4] = a.m4; v.m[5] = a.m5; v.m[6] = a.m6; v.m[7] = a.m7; v.m[8] = a.m8;
    pair = icp_row(v, C, a.raw, a.depth_m, a.nrmw_m, x, y, J, &res, &w);
  }
  float* mine = sh + t * kIcpRow;
  mine[0] = J[0]; mine[1] = J[1]; mine[2] = J[2]; mine[3] = J[3]; mine[4] = J[4]; mine[5] = J[5];
  mine[6] = res; mine[7] = w; mine[8] = pair ? 1.0f : 0.0f;
  if (a.rows_dev) {   // the thread's stride x stride cell of the frame: its own pixel first, zeros for the others
    for (int dy = 0; dy < a.stride; dy++)
      for (int dx = 0; dx < a.stride; dx++) {
        const int px = x + dx, py = y + dy;
        if (px >= a.cols || py >= a.rows) continue;
        const bool me = (dx == 0 && dy == 0);
        float4* o = reinterpret_cast<float4*>(a.rows_dev + ((size_t)py * a.cols + px) * 8);
        o[0] = me ? make_float4(J[0], J[1], J[2], J[3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        o[1] = me ? make_float4(J[4], J[5], res, w) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      }
  }
  __syncthreads();
  if (t < ODO_NACC * kIcpFoldLanes) {
    const int q = t / kIcpFoldLanes, s = t % kIcpFoldLanes;
    int ia, ib;
    icp_term_operands(q, &ia, &ib);
    double v = 0.0;
    if (q < ODO_NACC - 1) {
      for (int i = s; i < kIcpBlock; i += kIcpFoldLanes) v += icp_term(sh + i * kIcpRow, ia, ib);
    } else {
      for (int i = s; i < kIcpBlock; i += kIcpFoldLanes) v += (double)sh[i * kIcpRow + 8];
    }
    v = icp_fold8(v);
    if (s == 0) a.partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ODO_NACC + q] = v;
  }
}

// One block. Thread 8 q + s adds sum q of the partials s, s + 8, s + 16, ... in that order, icp_fold8 folds the eight lanes, and
// thread 0 takes the step (icp_step) on the state, or with take_step == 0 only leaves the folded sums in it.
__global__ void __launch_bounds__(kIcpBlock) volume_icp_step_kernel(VolIcpStepArgs a) {
  IcpState* st = a.state;
  if (st->status != 0 || st->done[a.level] != 0) return;
  __shared__ double sum[ODO_NACC];
  const int t = threadIdx.x;
  if (t < ODO_NACC * kIcpFoldLanes) {
    const int q = t / kIcpFoldLanes, s = t % kIcpFoldLanes;
    double v = 0.0;
#pragma unroll 8
    for (int b = s; b < a.nblk; b += kIcpFoldLanes) v += a.partials[(size_t)b * ODO_NACC + q];   // (unrolled: the loads of eight partials in flight, the adds in order)
    v = icp_fold8(v);
    if (s == 0) sum[q] = v;
  }
  __syncthreads();
  if (t < ODO_NACC) st->acc[t] = sum[t];
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
    IcpTraceRow* r = a.trace + n;
    r->level = a.level; r->iteration = n;
    for (int i = 0; i < ODO_NACC; i++) r->acc[i] = sum[i];
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

void launch_volume_icp_init(IcpState* state, const IcpInit& init, hipStream_t s) {
  hipLaunchKernelGGL(volume_icp_init_kernel, dim3(1), dim3(64), 0, s, state, init);
}
void launch_volume_icp_rows(const VolIcpRowsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_icp_rows_kernel, volume_icp_grid(a.rows, a.cols, a.stride), dim3(kIcpBlock), 0, s, a);
}
void launch_volume_icp_step(const VolIcpStepArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(volume_icp_step_kernel, dim3(1), dim3(kIcpBlock), 0, s, a);
}

}  // namespace odo
