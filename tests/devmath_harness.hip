// tests/devmath_harness.hip — TEST INFRASTRUCTURE. The arithmetic that decides the pose, as hipcc compiles it for gfx950, reachable
// call by call: odo_math.h's functions one case per thread, the wave-wide rewrites of kernels.hip.h (sincos_pair_lanes, se3_exp_wave,
// solve_damped_wave_regs, lm_apply_step_wave) one case per wavefront, the two block-level LM state machines driven through scripted
// accumulator sets, the per-pixel chain of a level pixel by pixel, and dense.hip.h's shared-reciprocal divisions against the plain `/`.
// Includes kernels.hip.h the way lm_chain_kernels.hip does (every ODO_KERNEL is a template nobody instantiates, device variables are
// static), plus dense.hip.h's device forms. A shared library of its own (tests/_build_devmath_<scheduler>.so, built by
// tests/devmath.py with the product's flags); never linked into libodometry_hip.so.
//
// Every entry point takes HOST pointers, allocates, copies, launches on the null stream, synchronises, copies back and frees, and
// returns the first HIP error code (0 = hipSuccess). Every kernel is a bounded loop over its cases: no waiting on memory, nothing of
// the persistent kernels' hand-over paths, no inline assembly.
//
// For tests/test_gpu_dense_cases.py it also launches product kernels as they are: lm_dense_eval_kernel and lm_dense_eval_batch_kernel (dense.hip.h)
// block by block with the grid cap chosen by the test, dense_block_run of every block, and the t-distribution scale kernels over a
// residual vector (dm_tdist_scale). The only waiting among them is lm_tdist_scale_multi_kernel's own bounded exchange (4 ms a wait),
// launched exactly as lm_launch_scale launches it, with its fall-back queued behind it.
//
// For tests/test_gpu_kf_list_cases.py: make_point per pixel (dm_make_points), kf_count_kernel + kf_fill_kernel over levels of any
// shapes as lm_enqueue_lists launches them, and the by-reference instantiation of their bodies from a table (dm_kf_lists), and
// lm_residual_only_list_kernel / lm_residual_list_kernel on a list those kernels built (dm_list_eval). Every output buffer starts as
// 0xAB bytes and has spare room behind what may be written.
#include <hip/hip_runtime.h>
#define ODO_LM_CHAIN_TU 1
#define ODO_DENSE_KERNELS 1
#define ODO_KERNEL template <int kNotInThisUnit = 0> static __global__
#define ODO_KERNEL_T static __global__
#include "../odometry_amd/csrc/kernels.hip.h"
#include "devmath_ops.h"

#include <stddef.h>
#include <vector>

using namespace odo;

namespace {

// Device buffers of one entry point: freed when it returns, whichever way.
struct Pool {
  std::vector<void*> bufs;
  hipError_t err = hipSuccess;
  ~Pool() { for (void* p : bufs) (void)hipFree(p); }
  void* raw(size_t bytes) {
    if (err != hipSuccess) return nullptr;
    void* p = nullptr;
    err = hipMalloc(&p, bytes ? bytes : 4);
    if (err != hipSuccess) return nullptr;
    bufs.push_back(p);
    return p;
  }
  template <class T> T* up(const T* host, size_t count) {   // a device copy of host[0 .. count)
    T* p = (T*)raw(count * sizeof(T));
    if (p && count) err = hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice);
    return p;
  }
  template <class T> T* zeros(size_t count) {
    T* p = (T*)raw(count * sizeof(T));
    if (p) err = hipMemset(p, 0, count ? count * sizeof(T) : 4);
    return p;
  }
  template <class T> void fill(T* dev, size_t count) {   // every byte 0xAB: what a kernel did not write shows
    if (dev && err == hipSuccess) err = hipMemset(dev, 0xAB, count ? count * sizeof(T) : 4);
  }
  template <class T> T* filled(size_t count) {
    T* p = (T*)raw(count * sizeof(T));
    fill(p, count);
    return p;
  }
  template <class T> void down(T* host, const T* dev, size_t count) {
    if (err == hipSuccess && count) err = hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  void ran() {   // after a launch
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
  }
  int done() {   // frees; the first error of the whole entry
    for (void* p : bufs) { const hipError_t e = hipFree(p); if (err == hipSuccess) err = e; }
    bufs.clear();
    return (int)err;
  }
};

constexpr int kEachBlock = 256;
inline int each_grid(long n) {
  long g = (n + kEachBlock - 1) / kEachBlock;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}
inline int wave_grid(long n) { return (int)(n < 1 ? 1 : (n > 8192 ? 8192 : n)); }

// ---- one case per thread ----------------------------------------------------------------------------------------------------------
template <class F>
__global__ void __launch_bounds__(kEachBlock) each_kernel(int n, F f) {
  for (int i = (int)(blockIdx.x * kEachBlock + threadIdx.x); i < n; i += (int)(gridDim.x * kEachBlock)) f(i);
}
#define DM_EACH(pool, n, ...)                                                                   \
  do {                                                                                          \
    if ((pool).err == hipSuccess) {                                                             \
      auto f_ = __VA_ARGS__;                                                                    \
      hipLaunchKernelGGL(each_kernel<decltype(f_)>, dim3(each_grid(n)), dim3(kEachBlock), 0, nullptr, (int)(n), f_); \
      (pool).ran();                                                                             \
    }                                                                                           \
  } while (0)

// ---- one case per wavefront -------------------------------------------------------------------------------------------------------
// The number of lanes whose 32-bit pattern differs from lane 0's (all 64 lanes must be active).
__device__ __forceinline__ int lanes_off(unsigned v) {
  const unsigned v0 = (unsigned)__builtin_amdgcn_readfirstlane((int)v);
  return __popcll(__ballot(v != v0));
}
__device__ __forceinline__ int lanes_off(float v) { return lanes_off(__float_as_uint(v)); }

__global__ void __launch_bounds__(64) sincos_pair_kernel(int n, const float* __restrict__ xa, const float* __restrict__ xb,
                                                         float* __restrict__ out, int* __restrict__ off) {
  for (int c = (int)blockIdx.x; c < n; c += (int)gridDim.x) {
    float sa, ca, sb, cb;
    sincos_pair_lanes(xa[c], xb[c], &sa, &ca, &sb, &cb);
    const int bad = lanes_off(sa) + lanes_off(ca) + lanes_off(sb) + lanes_off(cb);
    if (threadIdx.x == 0) { out[4 * c + 0] = sa; out[4 * c + 1] = ca; out[4 * c + 2] = sb; out[4 * c + 3] = cb; off[c] = bad; }
  }
}
__global__ void __launch_bounds__(64) se3_exp_wave_kernel(int n, const float* __restrict__ a, float* __restrict__ q, float* __restrict__ M,
                                                          int* __restrict__ off) {
  for (int c = (int)blockIdx.x; c < n; c += (int)gridDim.x) {
    float a6[6];
#pragma unroll
    for (int i = 0; i < 6; i++) a6[i] = a[6 * c + i];
    Se3 s;
    se3_exp_wave(a6, &s);
    float qq[7];
    dm::put_se3(s, qq);
    int bad = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) bad += lanes_off(qq[i]);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < 7; i++) q[7 * c + i] = qq[i];
      se3_to_colmajor(s, M + 16 * c);
      off[c] = bad;
    }
  }
}
__global__ void __launch_bounds__(64) solve_wave_kernel(int n, const double* __restrict__ acc, const float* __restrict__ lambda,
                                                        float* __restrict__ delta, int* __restrict__ off) {
  __shared__ double acc_sh[32];   // (the product's solve reads its sums from LDS)
  for (int c = (int)blockIdx.x; c < n; c += (int)gridDim.x) {
    if (threadIdx.x < ODO_NACC) acc_sh[threadIdx.x] = acc[(size_t)c * ODO_NACC + threadIdx.x];
    __syncthreads();
    float d[6];
    solve_damped_wave_regs(acc_sh, lambda[c], d);
    int bad = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) bad += lanes_off(d[i]);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 0; i < 6; i++) delta[6 * c + i] = d[i];
      off[c] = bad;
    }
    __syncthreads();
  }
}
__global__ void __launch_bounds__(64) apply_step_wave_kernel(int n, const LmState* __restrict__ in, LmState* __restrict__ out,
                                                             int* __restrict__ off) {
  for (int c = (int)blockIdx.x; c < n; c += (int)gridDim.x) {
    LmState s = in[c];
    lm_apply_step_wave(&s, s.max_iters);
    // all 64 dwords of the state, lane against lane 0 — through a fixed-size unrolled walk, so the state stays in registers
    int bad = 0;
    unsigned w[64];
    memcpy(w, &s, sizeof(w));
#pragma unroll
    for (int i = 0; i < 64; i++) bad += lanes_off(w[i]);
    if (threadIdx.x == 0) { out[c] = s; off[c] = bad; }
  }
}

// ---- the block-level state machines over a script -------------------------------------------------------------------------------
// One script per block. Block sizes 64 and kCoarseBlock. The state starts as lm_fused_prologue starts a Solve, the first walk down the
// pyramid is lm_state_machine(pending = false) as in the prologue, and the LmHot is loaded once and carried from evaluation to
// evaluation exactly as lm_coarse_body carries it. out = the full 64-dword state after every evaluation (the hot form: s_sh with
// lm_hot_store applied to a copy, which is what the coarse kernel publishes when it leaves).
template <bool kHot>
__global__ void __launch_bounds__(kCoarseBlock) script_block_kernel(const dm::LmScript* __restrict__ scripts, const double* __restrict__ acc,
                                                                    LmState* __restrict__ out, int* __restrict__ count) {
  __shared__ LmState s_sh;
  __shared__ double acc_sh[32];
  __shared__ StepLevel lv_sh[ODO_MAX_LEVELS_K];
  __shared__ dm::LmScript sc_sh;
  const int t = (int)threadIdx.x;
  {
    constexpr int kLvWords = (int)(sizeof(StepLevel) * ODO_MAX_LEVELS_K / (sizeof(unsigned))), kScWords = (int)(sizeof(dm::LmScript) / sizeof(unsigned));
    for (int i = t; i < kLvWords; i += (int)blockDim.x) ((unsigned*)lv_sh)[i] = 0u;
    for (int i = t; i < kScWords; i += (int)blockDim.x) ((unsigned*)&sc_sh)[i] = ((const unsigned*)&scripts[blockIdx.x])[i];
  }
  __syncthreads();
  if (t < ODO_MAX_LEVELS_K) lv_sh[t].max_iters = sc_sh.max_iters[t];
  if (t == 0) dm::script_begin(&s_sh, sc_sh.init);
  __syncthreads();
  const int n_levels = sc_sh.n_levels, stop_level = sc_sh.stop_level, n_evals = sc_sh.n_evals, first = sc_sh.acc_first;
  const float lambda0 = sc_sh.lambda0, precision = sc_sh.precision;
  lm_state_machine(false, lv_sh, n_levels, lambda0, precision, s_sh, acc_sh, nullptr, nullptr, false, nullptr, stop_level);
  LmHot hot;
  if (kHot) lm_hot_load(hot, s_sh);
  int e = 0;
  for (; e < n_evals; e++) {
    if (!dm::script_live(s_sh)) break;   // block-uniform: read behind the barrier that ends the state machine
    if (t < ODO_NACC) acc_sh[t] = acc[(size_t)(first + e) * ODO_NACC + t];
    __syncthreads();
    if (kHot) lm_state_machine_hot(hot, lv_sh, n_levels, lambda0, precision, s_sh, acc_sh, nullptr, nullptr, false, nullptr, stop_level);
    else lm_state_machine(true, lv_sh, n_levels, lambda0, precision, s_sh, acc_sh, nullptr, nullptr, false, nullptr, stop_level);
    if (t == 0) {
      LmState o = s_sh;
      if (kHot) lm_hot_store(hot, o);
      out[first + e] = o;
    }
    __syncthreads();   // acc_sh is rewritten by the next trip
  }
  if (t == 0) count[blockIdx.x] = e;
}

// ---- one pixel of a level per thread --------------------------------------------------------------------------------------------
// mode 0 / 1 / 3: dm::op_pixel; 2: make_point + point_residual_g<false>.
__global__ void __launch_bounds__(kEachBlock) pixel_kernel(dm::PixLevel L, int mode, int* __restrict__ hit, float* __restrict__ r,
                                                           float* __restrict__ w, float* __restrict__ J) {
  const int iw = L.cols - 8, ih = L.rows - 8;
  const int n = iw * ih;
  for (int i = (int)(blockIdx.x * kEachBlock + threadIdx.x); i < n; i += (int)(gridDim.x * kEachBlock)) {
    const int x = 4 + i % iw, y = 4 + i / iw;
    if (mode != 2) { dm::op_pixel(L, mode, x, y, hit, r, w, J); continue; }
    const int o = y * L.cols + x;
    float rr = 0.0f, JJ[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool h = false;
    const float d = L.D1[o];
    if (depth_valid(d)) {
      const PointK p = make_point(x, y, d, L.I1[o], L.k);
      h = point_residual_g<false>(p, L.T, L.k, lm_uniform_ptr(L.I2), L.rows, L.cols, &rr, JJ);
    }
    dm::pix_store(L, o, h, rr, JJ, hit, r, w, J);
  }
}
// dense_stage_a + dense_stage_b of one pixel from a zeroed accumulator: hit and the 29 products of the pixel's own row.
struct DenseArgs { float T[16]; int robust; float huber_delta, scale_sqr; int fast; };
__global__ void __launch_bounds__(kEachBlock) dense_pixel_kernel(DenseLevel L, DenseArgs a, int* __restrict__ hit, double* __restrict__ acc_out) {
  const int iw = L.cols - 8, ih = L.rows - 8;
  const int n = iw * ih;
  const float flf = (float)L.k.fl;
  const float yfl = rcp_refined(flf);
  const bool fast = a.fast != 0;
  for (int i = (int)(blockIdx.x * kEachBlock + threadIdx.x); i < n; i += (int)(gridDim.x * kEachBlock)) {
    const int x = 4 + i % iw, y = 4 + i / iw;
    const int o = y * L.cols + x;
    DensePix q;
    dense_stage_a<0>(x, y, L.D1[o], L.I1[o], fast, L, flf, yfl, a.T, &q);
    double acc[ODO_NACC];
#pragma unroll
    for (int k = 0; k < ODO_NACC; k++) acc[k] = 0.0;
    dense_stage_b<0>(q, fast, L, flf, a.robust, a.huber_delta, a.scale_sqr, acc);
    hit[o] = q.hit ? 1 : 0;
#pragma unroll
    for (int k = 0; k < ODO_NACC; k++) acc_out[(size_t)o * ODO_NACC + k] = acc[k];
  }
}

// ---- the dense scan's decomposition: dense_block_run of every block of a level ----------------------------------------------------
__global__ void __launch_bounds__(64) dense_runs_kernel(DenseLevel L, int* __restrict__ out5) {
  const DenseRun r = dense_block_run(L, (int)blockIdx.x);
  if (threadIdx.x == 0) {
    int* o = out5 + 5 * (size_t)blockIdx.x;
    o[0] = r.strip; o[1] = r.rg; o[2] = r.rg0; o[3] = r.rg1; o[4] = r.count;
  }
}
// A state as the evaluation kernels read it: the pose, `active`, `level`.
__global__ void __launch_bounds__(64) dense_state_kernel(LmState* __restrict__ st, const float* __restrict__ T, int n, const int* __restrict__ active,
                                                         int level) {
  for (int i = (int)threadIdx.x; i < n * 16; i += 64) st[i / 16].T[i % 16] = T[i];
  for (int i = (int)threadIdx.x; i < n; i += 64) { st[i].active = active[i]; st[i].level = level; }
}

// ---- the keyframe point lists from a table in global memory ------------------------------------------------------------------------
// The `const KfLevels&` instantiation of both bodies, shaped like kf_count_batch_kernel / kf_fill_batch_kernel (batch.hip.h): one table
// entry per blockIdx.y. (The product's batch launch passes no dense_above; here it is an argument, so that every case can be compared
// with its by-value launch.)
struct KfTab {
  KfLevels kl;
  int* rowcnt;
  int* npts;
  PointList pl[ODO_MAX_LEVELS_K];
};
__global__ void __launch_bounds__(256) kf_count_ref_kernel(const KfTab* __restrict__ tab) {
  const KfTab& q = tab[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x < ODO_MAX_LEVELS_K) q.npts[threadIdx.x] = 0;
  kf_count_kernel_body<const KfLevels&>(q.kl, q.rowcnt);
}
__global__ void __launch_bounds__(256) kf_fill_ref_kernel(const KfTab* __restrict__ tab, float f0, float cx0, float cy0, int dense_above) {
  const KfTab& q = tab[blockIdx.y];
  const int l = kf_find_level(q.kl, blockIdx.x);
  kf_fill_kernel_body<const KfLevels&>(q.kl, l, q.pl[l], f0, cx0, cy0, q.rowcnt, q.npts, dense_above);
}

// ---- the shared-reciprocal divisions against the plain `/` of the same unit -------------------------------------------------------
constexpr int kFirstCap = 16;   // mismatches returned with their index
__device__ __forceinline__ void note_mismatch(bool bad, int i, unsigned long long* __restrict__ n_bad, int* __restrict__ first) {
  if (bad) {
    const unsigned long long k = atomicAdd(n_bad, 1ull);
    if (k < (unsigned long long)kFirstCap) first[k] = i;
  }
}
// form 0: div_shared(a, b, rcp_refined(b)) against a / b; form 1: recip_shared(b, rcp_refined(b)) against 1.0f / b; form 2: div_shared_z
// (numerators that may be a zero of either sign) against a / b.
// The first n_out results of both forms are written out (shared: q_out[i], plain: q_out[n_out + i]).
__global__ void __launch_bounds__(kEachBlock) div32_kernel(int n, int form, const float* __restrict__ a, const float* __restrict__ b,
                                                           unsigned long long* __restrict__ n_bad, int* __restrict__ first, int n_out,
                                                           float* __restrict__ q_out) {
  for (int i = (int)(blockIdx.x * kEachBlock + threadIdx.x); i < n; i += (int)(gridDim.x * kEachBlock)) {
    const float bb = b[i], aa = form == 1 ? 1.0f : a[i];
    const float y = rcp_refined(bb);
    const float qs = form == 1 ? recip_shared(bb, y) : (form == 2 ? div_shared_z(aa, bb, y) : div_shared(aa, bb, y));
    const float qp = aa / bb;
    note_mismatch(__float_as_uint(qs) != __float_as_uint(qp), i, n_bad, first);
    if (i < n_out) { q_out[i] = qs; q_out[n_out + i] = qp; }
  }
}
__global__ void __launch_bounds__(kEachBlock) div64_kernel(int n, const double* __restrict__ a, const double* __restrict__ b,
                                                           unsigned long long* __restrict__ n_bad, int* __restrict__ first, int n_out,
                                                           double* __restrict__ q_out) {
  for (int i = (int)(blockIdx.x * kEachBlock + threadIdx.x); i < n; i += (int)(gridDim.x * kEachBlock)) {
    const double aa = a[i], bb = b[i];
    const double qs = div_shared_d(aa, bb, rcp_refined_d(bb));
    const double qp = aa / bb;
    note_mismatch(__double_as_longlong(qs) != __double_as_longlong(qp), i, n_bad, first);
    if (i < n_out) { q_out[i] = qs; q_out[n_out + i] = qp; }
  }
}
// The call sites: point_xyz_shared against point_xyz, point_jacobian_shared against point_jacobian (both on point_xyz's result),
// warp_uv_shared against warp_point_uv. Case i: pixel (x[i], y[i]), inverse depth d[i], level (fl[i], cx[i], cy[i]), pose T[16 (i % n_T)].
// n_bad[0..2] / first[0..2][kFirstCap]: one counter per call site.
__global__ void __launch_bounds__(kEachBlock) callsite_kernel(int n, const int* __restrict__ x, const int* __restrict__ y, const float* __restrict__ d,
                                                              const double* __restrict__ fl, const float* __restrict__ cx, const float* __restrict__ cy,
                                                              int n_T, const float* __restrict__ T, unsigned long long* __restrict__ n_bad,
                                                              int* __restrict__ first) {
  for (int i = (int)(blockIdx.x * kEachBlock + threadIdx.x); i < n; i += (int)(gridDim.x * kEachBlock)) {
    LevelK k;
    k.fl = fl[i]; k.cx = cx[i]; k.cy = cy[i]; k.bilinear = 0;
    const float flf = (float)k.fl, yfl = rcp_refined(flf);
    PointK p, ps;
    point_xyz(x[i], y[i], d[i], k, &p.X, &p.Y, &p.Z);
    point_xyz_shared(x[i], y[i], d[i], k, flf, yfl, &ps.X, &ps.Y, &ps.Z);
    note_mismatch(__float_as_uint(p.X) != __float_as_uint(ps.X) || __float_as_uint(p.Y) != __float_as_uint(ps.Y) ||
                  __float_as_uint(p.Z) != __float_as_uint(ps.Z), i, n_bad + 0, first + 0 * kFirstCap);
    p.i1 = 0.0f;
    ps = p;
    point_jacobian(&p, k);
    point_jacobian_shared(&ps, k, flf);
    const float ja[9] = {p.fx_z, p.jw02, p.jw03, p.jw04, p.jw05, p.jw12, p.jw13, p.jw14, p.jw15};
    const float jb[9] = {ps.fx_z, ps.jw02, ps.jw03, ps.jw04, ps.jw05, ps.jw12, ps.jw13, ps.jw14, ps.jw15};
    bool bad = false;
#pragma unroll
    for (int q = 0; q < 9; q++) bad = bad || (__float_as_uint(ja[q]) != __float_as_uint(jb[q]));
    note_mismatch(bad, i, n_bad + 1, first + 1 * kFirstCap);
    const float* Ti = T + 16 * (i % n_T);
    float u0 = 0.0f, v0 = 0.0f, u1 = 0.0f, v1 = 0.0f;
    const bool h0 = warp_point_uv(p, Ti, k, &u0, &v0), h1 = warp_uv_shared(p, Ti, k, &u1, &v1);
    note_mismatch(h0 != h1 || (h0 && (__float_as_uint(u0) != __float_as_uint(u1) || __float_as_uint(v0) != __float_as_uint(v1))), i,
                  n_bad + 2, first + 2 * kFirstCap);
  }
}

}  // namespace

#define DM_LAUNCH(pool, kernel, grid, block, ...)                                          \
  do {                                                                                     \
    if ((pool).err == hipSuccess) {                                                        \
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, nullptr, __VA_ARGS__);        \
      (pool).ran();                                                                        \
    }                                                                                      \
  } while (0)

extern "C" {

// sizeof / offsetof of the structures tests/devmath.py mirrors: out[0 .. dm_layout_count())
int dm_layout_count() { return 40; }
void dm_layout(int* out) {
  int k = 0;
  out[k++] = (int)sizeof(LmState);
  out[k++] = (int)offsetof(LmState, cur); out[k++] = (int)offsetof(LmState, inc); out[k++] = (int)offsetof(LmState, last);
  out[k++] = (int)offsetof(LmState, T); out[k++] = (int)offsetof(LmState, lambda); out[k++] = (int)offsetof(LmState, err_last);
  out[k++] = (int)offsetof(LmState, err_now); out[k++] = (int)offsetof(LmState, level); out[k++] = (int)offsetof(LmState, iter);
  out[k++] = (int)offsetof(LmState, active); out[k++] = (int)offsetof(LmState, status); out[k++] = (int)offsetof(LmState, n_evals);
  out[k++] = (int)offsetof(LmState, stop_reason); out[k++] = (int)offsetof(LmState, iters_level); out[k++] = (int)offsetof(LmState, delta);
  out[k++] = (int)offsetof(LmState, pending); out[k++] = (int)offsetof(LmState, pending_nblk); out[k++] = (int)offsetof(LmState, max_iters);
  out[k++] = (int)offsetof(LmState, finished);                                                                      // 20
  out[k++] = (int)sizeof(DenseLevel);
  out[k++] = (int)offsetof(DenseLevel, I1); out[k++] = (int)offsetof(DenseLevel, I2); out[k++] = (int)offsetof(DenseLevel, D1);
  out[k++] = (int)offsetof(DenseLevel, rows); out[k++] = (int)offsetof(DenseLevel, cols);
  out[k++] = (int)(offsetof(DenseLevel, k) + offsetof(LevelK, fl)); out[k++] = (int)(offsetof(DenseLevel, k) + offsetof(LevelK, cx));
  out[k++] = (int)(offsetof(DenseLevel, k) + offsetof(LevelK, cy)); out[k++] = (int)(offsetof(DenseLevel, k) + offsetof(LevelK, bilinear));
  out[k++] = (int)offsetof(DenseLevel, nblk); out[k++] = (int)offsetof(DenseLevel, n_strips); out[k++] = (int)offsetof(DenseLevel, n_rg);
  out[k++] = (int)offsetof(DenseLevel, fast_ok); out[k++] = (int)offsetof(DenseLevel, max_iters);                      // 35
  out[k++] = (int)sizeof(dm::LmScript); out[k++] = (int)sizeof(dm::PixLevel); out[k++] = (int)sizeof(LevelK);
  out[k++] = kCoarseBlock; out[k++] = kFirstCap;                                                                     // 40
}
int dm_dense_fast_ok(double fl, float cx, float cy, int rows, int cols) { return dense_fast_ok(fl, cx, cy, rows, cols); }

// ---- per-thread ----
int dm_level_k(int n, const float* f0, const float* cx0, const float* cy0, const int* level, double* fl, float* cxy) {
  Pool P;
  const float *df = P.up(f0, n), *dx = P.up(cx0, n), *dy = P.up(cy0, n);
  const int* dl = P.up(level, n);
  double* dfl = P.zeros<double>(n);
  float* dc = P.zeros<float>(3 * (size_t)n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_level_k(i, df, dx, dy, dl, dfl, dc); });
  P.down(fl, dfl, n); P.down(cxy, dc, 3 * (size_t)n);
  return P.done();
}
int dm_sincos(int n, const float* x, float* s, float* c) {
  Pool P;
  const float* dx = P.up(x, n);
  float *ds = P.zeros<float>(n), *dc = P.zeros<float>(n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_sincos(i, dx, ds, dc); });
  P.down(s, ds, n); P.down(c, dc, n);
  return P.done();
}
int dm_se3_exp(int n, const float* a, float* q, float* M) {
  Pool P;
  const float* da = P.up(a, 6 * (size_t)n);
  float *dq = P.zeros<float>(7 * (size_t)n), *dM = P.zeros<float>(16 * (size_t)n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_se3_exp(i, da, dq, dM); });
  P.down(q, dq, 7 * (size_t)n); P.down(M, dM, 16 * (size_t)n);
  return P.done();
}
int dm_se3_roundtrip(int n, const float* Min, float* q, float* M) {
  Pool P;
  const float* di = P.up(Min, 16 * (size_t)n);
  float *dq = P.zeros<float>(7 * (size_t)n), *dM = P.zeros<float>(16 * (size_t)n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_se3_roundtrip(i, di, dq, dM); });
  P.down(q, dq, 7 * (size_t)n); P.down(M, dM, 16 * (size_t)n);
  return P.done();
}
int dm_se3_left_update(int n, const float* d6, const float* cur, int variant, float* q, float* M) {
  Pool P;
  const float *dd = P.up(d6, 6 * (size_t)n), *dc = P.up(cur, 16 * (size_t)n);
  float *dq = P.zeros<float>(7 * (size_t)n), *dM = P.zeros<float>(16 * (size_t)n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_se3_left_update(i, dd, dc, variant, dq, dM); });
  P.down(q, dq, 7 * (size_t)n); P.down(M, dM, 16 * (size_t)n);
  return P.done();
}
int dm_solve_damped(int n, const double* acc, const float* lambda, float* delta) {
  Pool P;
  const double* da = P.up(acc, ODO_NACC * (size_t)n);
  const float* dl = P.up(lambda, n);
  float* dd = P.zeros<float>(6 * (size_t)n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_solve_damped(i, da, dl, dd); });
  P.down(delta, dd, 6 * (size_t)n);
  return P.done();
}
int dm_robust_weight(int n, const float* r, const int* robust, const float* huber, const float* scale, float* w) {
  Pool P;
  const float *dr = P.up(r, n), *dh = P.up(huber, n), *dsc = P.up(scale, n);
  const int* dmode = P.up(robust, n);
  float* dw = P.zeros<float>(n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_robust_weight(i, dr, dmode, dh, dsc, dw); });
  P.down(w, dw, n);
  return P.done();
}
int dm_apply_step(int n, const LmState* in, LmState* out) {
  Pool P;
  const LmState* di = P.up(in, n);
  LmState* dout = P.zeros<LmState>(n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_apply_step(i, di, dout); });
  P.down(out, dout, n);
  return P.done();
}
int dm_depth_schedule(int n, int cap, const float* errs, const int* n_errs, const float* lambda0, const float* precision,
                      const int* max_iters, int* rec, int* fin) {
  Pool P;
  const float *de = P.up(errs, (size_t)n * cap), *dl = P.up(lambda0, n), *dp = P.up(precision, n);
  const int *dn = P.up(n_errs, n), *dmi = P.up(max_iters, n);
  int *dr = P.zeros<int>((size_t)n * cap * 5), *df = P.zeros<int>(3 * (size_t)n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_depth_schedule(i, cap, de, dn, dl, dp, dmi, dr, df); });
  P.down(rec, dr, (size_t)n * cap * 5); P.down(fin, df, 3 * (size_t)n);
  return P.done();
}
// n scripts over n_acc accumulator sets in all (script i owns [acc_first, acc_first + n_evals)); out: n_acc states, count: n ints.
// form 0: lm_consume, one script per thread; 1: lm_state_machine, 2: lm_state_machine_hot, one script per block of `block` threads.
int dm_lm_script(int n, const dm::LmScript* scripts, int n_acc, const double* acc, int form, int block, LmState* out, int* count) {
  if (form != 0 && block != 64 && block != kCoarseBlock) return (int)hipErrorInvalidValue;
  for (int i = 0; i < n; i++) {   // every script stays inside the buffers
    const dm::LmScript& s = scripts[i];
    if (s.n_levels < 1 || s.n_levels > ODO_MAX_LEVELS_K || s.stop_level < 0 || s.n_evals < 0 || s.acc_first < 0 ||
        (long)s.acc_first + s.n_evals > (long)n_acc)
      return (int)hipErrorInvalidValue;
  }
  Pool P;
  const dm::LmScript* ds = P.up(scripts, n);
  const double* da = P.up(acc, ODO_NACC * (size_t)n_acc);
  LmState* dout = P.zeros<LmState>(n_acc);
  int* dc = P.zeros<int>(n);
  if (form == 0) DM_EACH(P, n, [=] __device__(int i) { dc[i] = dm::script_run(ds[i], da, dout); });
  else if (form == 1) DM_LAUNCH(P, script_block_kernel<false>, n, block, ds, da, dout, dc);
  else DM_LAUNCH(P, script_block_kernel<true>, n, block, ds, da, dout, dc);
  P.down(out, dout, n_acc); P.down(count, dc, n);
  return P.done();
}

// ---- per-wave ----
int dm_sincos_pair_wave(int n, const float* xa, const float* xb, float* out4, int* off) {
  Pool P;
  const float *da = P.up(xa, n), *db = P.up(xb, n);
  float* dout = P.zeros<float>(4 * (size_t)n);
  int* doff = P.zeros<int>(n);
  DM_LAUNCH(P, sincos_pair_kernel, wave_grid(n), 64, n, da, db, dout, doff);
  P.down(out4, dout, 4 * (size_t)n); P.down(off, doff, n);
  return P.done();
}
int dm_se3_exp_wave(int n, const float* a, float* q, float* M, int* off) {
  Pool P;
  const float* da = P.up(a, 6 * (size_t)n);
  float *dq = P.zeros<float>(7 * (size_t)n), *dM = P.zeros<float>(16 * (size_t)n);
  int* doff = P.zeros<int>(n);
  DM_LAUNCH(P, se3_exp_wave_kernel, wave_grid(n), 64, n, da, dq, dM, doff);
  P.down(q, dq, 7 * (size_t)n); P.down(M, dM, 16 * (size_t)n); P.down(off, doff, n);
  return P.done();
}
int dm_solve_damped_wave(int n, const double* acc, const float* lambda, float* delta, int* off) {
  Pool P;
  const double* da = P.up(acc, ODO_NACC * (size_t)n);
  const float* dl = P.up(lambda, n);
  float* dd = P.zeros<float>(6 * (size_t)n);
  int* doff = P.zeros<int>(n);
  DM_LAUNCH(P, solve_wave_kernel, wave_grid(n), 64, n, da, dl, dd, doff);
  P.down(delta, dd, 6 * (size_t)n); P.down(off, doff, n);
  return P.done();
}
int dm_apply_step_wave(int n, const LmState* in, LmState* out, int* off) {
  Pool P;
  const LmState* di = P.up(in, n);
  LmState* dout = P.zeros<LmState>(n);
  int* doff = P.zeros<int>(n);
  DM_LAUNCH(P, apply_step_wave_kernel, wave_grid(n), 64, n, di, dout, doff);
  P.down(out, dout, n); P.down(off, doff, n);
  return P.done();
}

// ---- per-pixel ----
// L: host pointers in I1 / I2 / D1 (rows x cols each). hit / r / w: rows x cols, J: rows x cols x 6; the border of 4 stays 0.
int dm_pixels(const dm::PixLevel* L, int mode, int* hit, float* r, float* w, float* J) {
  if (L->rows < 2 || L->cols < 2 || L->rows > 65535 || L->cols > 65535 || mode < 0 || mode > 3) return (int)hipErrorInvalidValue;
  const size_t npx = (size_t)L->rows * L->cols;
  Pool P;
  dm::PixLevel D = *L;
  D.I1 = P.up(L->I1, npx); D.I2 = P.up(L->I2, npx); D.D1 = P.up(L->D1, npx);
  int* dh = P.zeros<int>(npx);
  float *dr = P.zeros<float>(npx), *dw = P.zeros<float>(npx), *dJ = P.zeros<float>(6 * npx);
  const long n = (long)(L->cols - 8) * (L->rows - 8);
  if (L->cols > 8 && L->rows > 8) DM_LAUNCH(P, pixel_kernel, each_grid(n), kEachBlock, D, mode, dh, dr, dw, dJ);
  P.down(hit, dh, npx); P.down(r, dr, npx); P.down(w, dw, npx); P.down(J, dJ, 6 * npx);
  return P.done();
}
// L: a DenseLevel with host pointers (geometry fields unused). acc: rows x cols x 29 doubles.
int dm_dense_pixels(const DenseLevel* L, const float* T, int robust, float huber_delta, float scale_sqr, int fast, int* hit, double* acc) {
  if (L->rows < 2 || L->cols < 2 || L->rows > 65535 || L->cols > 65535) return (int)hipErrorInvalidValue;
  const size_t npx = (size_t)L->rows * L->cols;
  Pool P;
  DenseLevel D = *L;
  D.I1 = P.up(L->I1, npx); D.I2 = P.up(L->I2, npx); D.D1 = P.up(L->D1, npx);
  DenseArgs a;
  for (int i = 0; i < 16; i++) a.T[i] = T[i];
  a.robust = robust; a.huber_delta = huber_delta; a.scale_sqr = scale_sqr; a.fast = fast;
  int* dh = P.zeros<int>(npx);
  double* dacc = P.zeros<double>(ODO_NACC * npx);
  const long n = (long)(L->cols - 8) * (L->rows - 8);
  if (L->cols > 8 && L->rows > 8) DM_LAUNCH(P, dense_pixel_kernel, each_grid(n), kEachBlock, D, a, dh, dacc);
  P.down(hit, dh, npx); P.down(acc, dacc, ODO_NACC * npx);
  return P.done();
}

// ---- the dense scan block by block ----
// A level as lm_dense_level describes it, with the grid cap given by the caller (the product's is kDenseGridCap; a small cap gives a
// small frame the runs of several units the product builds above 1024 units): images uploaded, geometry and fast_ok filled in.
static bool dense_device_level(Pool& P, const DenseLevel& H, int cap, DenseLevel* D) {
  if (H.rows < 2 || H.cols < 2 || H.rows > 65535 || H.cols > 65535 || cap < 1 || cap > kDenseMaxBlocks) return false;
  const size_t npx = (size_t)H.rows * H.cols;
  memset(D, 0, sizeof(*D));
  D->I1 = P.up(H.I1, npx); D->I2 = P.up(H.I2, npx); D->D1 = P.up(H.D1, npx);
  D->rows = H.rows; D->cols = H.cols; D->k = H.k;
  D->fast_ok = dense_fast_ok(H.k.fl, H.k.cx, H.k.cy, H.rows, H.cols);
  dense_level_geometry(D, kDenseBlock, cap);
  return true;
}
constexpr int kDmExpectLevel = 2;   // the level the states below sit on (any value: the kernels compare it with their argument)
static LmState* dense_device_states(Pool& P, int n, const float* T, const int* active) {
  LmState* st = P.zeros<LmState>(n);
  const float* dT = P.up(T, 16 * (size_t)n);
  const int* da = P.up(active, n);
  DM_LAUNCH(P, dense_state_kernel, 1, 64, st, dT, n, da, kDmExpectLevel);
  return st;
}
static double* dense_device_partials(Pool& P, int nblk) {   // every byte 0xAB: a row the kernel did not write shows
  double* p = (double*)P.raw(sizeof(double) * ODO_NACC * (size_t)nblk);
  if (p && P.err == hipSuccess) P.err = hipMemset(p, 0xAB, sizeof(double) * ODO_NACC * (size_t)nblk);
  return p;
}
// geom3 = {n_strips, n_rg, nblk}; out5 = dense_block_run of blocks 0 .. nblk - 1 (n_rows: the rows out5 has room for).
int dm_dense_runs(const DenseLevel* L, int cap, int n_rows, int* geom3, int* out5) {
  DenseLevel D;
  memset(&D, 0, sizeof(D));
  D.rows = L->rows; D.cols = L->cols;
  if (cap < 1 || cap > kDenseMaxBlocks) return (int)hipErrorInvalidValue;
  dense_level_geometry(&D, kDenseBlock, cap);
  geom3[0] = D.n_strips; geom3[1] = D.n_rg; geom3[2] = D.nblk;
  if (D.nblk > n_rows) return (int)hipErrorInvalidValue;
  Pool P;
  int* d = P.zeros<int>(5 * (size_t)D.nblk);
  DM_LAUNCH(P, dense_runs_kernel, D.nblk, 64, D, d);
  P.down(out5, d, 5 * (size_t)D.nblk);
  return P.done();
}
// lm_dense_eval_kernel launched as launch_dense_eval launches it (grid = nblk blocks of kDenseBlock threads) on a state with
// active = 1 at pose T. partials: n_rows x 29, n_rows >= the level's nblk; rows past nblk come back as 0xAB bytes.
int dm_dense_eval(const DenseLevel* L, int cap, const float* T, int robust, float huber_delta, float scale_sqr, int plain_div, int n_rows,
                  double* partials) {
  Pool P;
  DenseLevel D;
  if (!dense_device_level(P, *L, cap, &D) || D.nblk > n_rows) return (int)hipErrorInvalidValue;
  const int one = 1;
  const LmState* st = dense_device_states(P, 1, T, &one);
  const float* dscale = P.up(&scale_sqr, 1);
  double* dp = dense_device_partials(P, n_rows);
  if (plain_div) DM_LAUNCH(P, (lm_dense_eval_kernel<kDenseBlock, 1, kDenseWaves>), D.nblk, kDenseBlock, D, st, kDmExpectLevel, robust, huber_delta, dscale, dp);
  else DM_LAUNCH(P, (lm_dense_eval_kernel<kDenseBlock, 0, kDenseWaves>), D.nblk, kDenseBlock, D, st, kDmExpectLevel, robust, huber_delta, dscale, dp);
  P.down(partials, dp, ODO_NACC * (size_t)n_rows);
  return P.done();
}
// lm_dense_eval_batch_kernel over n items of different sizes, launched as launch_dense_eval_batch launches it: grid = (largest nblk
// rounded up to a multiple of 8, n). Item i: level Ls[i] with cap caps[i], pose T + 16 i, state active[i]; its partial rows are
// partials + 29 row_off[i] .. 29 row_off[i + 1] (row_off[i + 1] - row_off[i] >= its nblk).
int dm_dense_eval_batch(int n, const DenseLevel* Ls, const int* caps, const float* T, const int* robust, const float* huber_delta,
                        const float* scale_sqr, const int* active, int plain_div, const int* row_off, double* partials) {
  if (n < 1 || n > 64) return (int)hipErrorInvalidValue;
  Pool P;
  std::vector<DenseBatchItem> items((size_t)n);
  std::vector<double*> dps((size_t)n);
  LmState* st = dense_device_states(P, n, T, active);
  const float* dscale = P.up(scale_sqr, n);
  int max_nblk = 1;
  for (int i = 0; i < n; i++) {
    DenseBatchItem& it = items[i];
    memset(&it, 0, sizeof(it));
    const int rows = row_off[i + 1] - row_off[i];
    if (!dense_device_level(P, Ls[i], caps[i], &it.L) || it.L.nblk > rows) return (int)hipErrorInvalidValue;
    dps[i] = dense_device_partials(P, rows);
    it.st = st + i; it.scale_sqr = dscale + i; it.partials = dps[i];
    it.expect_level = kDmExpectLevel; it.robust = robust[i]; it.huber_delta = huber_delta[i];
    if (it.L.nblk > max_nblk) max_nblk = it.L.nblk;
  }
  const DenseBatchItem* dit = P.up(items.data(), (size_t)n);
  const dim3 grid((unsigned)((max_nblk + 7) / 8 * 8), (unsigned)n);
  if (plain_div) DM_LAUNCH(P, (lm_dense_eval_batch_kernel<kDenseBlock, 1, kDenseWaves>), grid, kDenseBlock, dit);
  else DM_LAUNCH(P, (lm_dense_eval_batch_kernel<kDenseBlock, 0, kDenseWaves>), grid, kDenseBlock, dit);
  for (int i = 0; i < n; i++) P.down(partials + ODO_NACC * (size_t)row_off[i], dps[i], ODO_NACC * (size_t)(row_off[i + 1] - row_off[i]));
  return P.done();
}

// ---- the t-distribution scale over stored residuals ----
// order 0: lm_tdist_scale_kernel in list order (n <= 64 kTdistChunksMax); 1: the same kernel's strided order; 2: what lm_launch_scale
// queues for n residuals (tdist_scale_plan: the list order, or the multi-workgroup kernel with the single-workgroup kernel behind it
// on only_if, or the single-workgroup kernel alone when n does not fit), `reps` times in a row on ONE exchange buffer with the
// launch epoch counting up as the library's does. The multi-workgroup kernel's waits are bounded (its default: 4 ms), and its test
// hook stays off. scale_sqr[reps]; info[4 reps] = {G (0: no multi launch), gave up, writer (0 list order, 1 strided, 2 multi), 0}.
int dm_tdist_scale(const float* res, int n, int order, int reps, float* scale_sqr, int* info) {
  if (n < 0 || reps < 1 || reps > 16 || order < 0 || order > 2 || (order == 0 && n > 64 * kTdistChunksMax)) return (int)hipErrorInvalidValue;
  Pool P;
  const float* dres = P.up(res, (size_t)n);
  const int one = 1;
  float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const LmState* st = dense_device_states(P, 1, eye, &one);
  float* dscale = (float*)P.raw(sizeof(float));
  unsigned long long* xbuf = P.zeros<unsigned long long>(kTsXbufWords);
  int* gave_up = P.zeros<int>(2);   // {flag, passes redone by the fall-back}
  const TdistScalePlan plan = tdist_scale_plan(n);
  unsigned epoch = 0;
  for (int r = 0; r < reps; r++) {
    int* o = info + 4 * r;
    o[0] = o[1] = o[2] = o[3] = 0;
    if (dscale && P.err == hipSuccess) P.err = hipMemset(dscale, 0xff, sizeof(float));   // (a NaN: a launch that writes nothing shows)
    if (order != 2 || plan.list) {
      const int list_order = (order == 1) ? 0 : 1;
      DM_LAUNCH(P, lm_tdist_scale_kernel<0>, 1, 1024, dres, n, st, kDmExpectLevel, dscale, list_order, (int*)nullptr);
      o[2] = list_order ? 0 : 1;
    } else if (!plan.fits) {
      DM_LAUNCH(P, lm_tdist_scale_kernel<0>, 1, 1024, dres, n, st, kDmExpectLevel, dscale, plan.single_order, (int*)nullptr);
      o[2] = plan.single_order ? 0 : 1;
    } else if (P.err == hipSuccess) {
      epoch++;
      int before[2] = {0, 0}, after[2] = {0, 0};
      P.down(before, gave_up, 2);
      hipLaunchKernelGGL(lm_tdist_scale_multi_kernel<0>, dim3((unsigned)plan.G), dim3(kTsThreads), 0, nullptr, dres, n, st, kDmExpectLevel,
                         dscale, xbuf, epoch, 0u, gave_up, 0);
      hipLaunchKernelGGL(lm_tdist_scale_kernel<0>, dim3(1), dim3(1024), 0, nullptr, dres, n, st, kDmExpectLevel, dscale, plan.single_order,
                         gave_up);
      P.ran();
      P.down(after, gave_up, 2);
      o[0] = plan.G;
      o[1] = (after[1] != before[1]) ? 1 : 0;
      o[2] = o[1] ? (plan.single_order ? 0 : 1) : 2;
    }
    P.down(scale_sqr + r, dscale, 1);
  }
  return P.done();
}

// ---- the keyframe point lists ----
int dm_make_points(int n, const float* I1, const float* D1, int cols, float f0, float cx0, float cy0, int level, float* out13) {
  if (cols < 1 || level < 0 || level >= ODO_MAX_LEVELS_K) return (int)hipErrorInvalidValue;
  Pool P;
  const float *dI = P.up(I1, n), *dD = P.up(D1, n);
  float* dout = P.zeros<float>(13 * (size_t)n);
  DM_EACH(P, n, [=] __device__(int i) { dm::op_make_point(i, dI, dD, cols, f0, cx0, cy0, level, dout); });
  P.down(out13, dout, 13 * (size_t)n);
  return P.done();
}
// The buffers of one list build, laid out as lm_lists_layout lays them out: levels[l] = rows x cols floats of I1 and of D1 at pixel
// offset sum(rows cols) of the levels before it (levels need not be a pyramid). Every level 0 .. ODO_MAX_LEVELS_K - 1 gets a list
// of (its interior + spare) entries, rowcnt has one spare entry; all of it, and npts, starts as 0xAB bytes.
struct KfSet {
  KfLevels kl;
  int rows_total;
  int *rowcnt, *npts;
  PointList pl[ODO_MAX_LEVELS_K];
  size_t cap[ODO_MAX_LEVELS_K], cap_total;
};
static bool kf_device_set(Pool& P, int n_levels, const int* rows, const int* cols, const float* I1, const float* D1, int spare, KfSet* S) {
  if (n_levels < 1 || n_levels > ODO_MAX_LEVELS_K || spare < 0 || spare > 4096) return false;
  memset(S, 0, sizeof(*S));
  size_t npx = 0;
  for (int l = 0; l < n_levels; l++) {
    if (rows[l] < 1 || cols[l] < 1 || rows[l] > 65535 || cols[l] > 65535) return false;
    npx += (size_t)rows[l] * cols[l];
  }
  const float *dI = P.up(I1, npx), *dD = P.up(D1, npx);
  KfLevels& kl = S->kl;
  kl.n_levels = n_levels;
  size_t off = 0;
  int rows_total = 0;
  for (int l = 0; l < ODO_MAX_LEVELS_K; l++) {
    size_t interior = 0;
    if (l < n_levels) {
      kl.I1[l] = dI + off; kl.D1[l] = dD + off;
      kl.rows[l] = rows[l]; kl.cols[l] = cols[l];
      kl.row_base[l] = rows_total;
      const int ir = rows[l] - 8, ic = cols[l] - 8;
      rows_total += (ir > 0 && ic > 0) ? ir : 0;
      interior = (ir > 0 && ic > 0) ? (size_t)ir * ic : 0;
      off += (size_t)rows[l] * cols[l];
    }
    S->cap[l] = interior + (size_t)spare;
    S->cap_total += S->cap[l];
    S->pl[l].a = P.filled<float4>(S->cap[l]); S->pl[l].b = P.filled<float4>(S->cap[l]);
    S->pl[l].c = P.filled<float4>(S->cap[l]); S->pl[l].d = P.filled<float>(S->cap[l]);
  }
  for (int l = n_levels; l <= ODO_MAX_LEVELS_K; l++) kl.row_base[l] = rows_total;
  S->rows_total = rows_total;
  S->rowcnt = P.filled<int>((size_t)rows_total + 1);
  S->npts = P.filled<int>(ODO_MAX_LEVELS_K);
  return rows_total > 0;
}
static void kf_launch_by_value(Pool& P, const KfSet& S, float f0, float cx0, float cy0, int dense_above) {   // lm_enqueue_lists' pair
  DM_LAUNCH(P, kf_count_kernel<0>, S.rows_total, 256, S.kl, S.rowcnt, S.npts);
  DM_LAUNCH(P, kf_fill_kernel<0>, S.rows_total, 256, S.kl, f0, cx0, cy0, (const int*)S.rowcnt, S.npts, S.pl[0], S.pl[1], S.pl[2], S.pl[3],
            S.pl[4], S.pl[5], S.pl[6], S.pl[7], dense_above);
}
// n_sets list builds of the same level shapes with contents of their own (I1 / D1: n_sets x sum(rows cols)), twice in a row into the
// same buffers. form 0: kf_count_kernel + kf_fill_kernel as lm_enqueue_lists launches them (rows_total blocks of 256), one pair per
// set; form 1: the by-reference bodies over a table of n_sets entries, grid (rows_total, n_sets). Outputs, [run 2][set n_sets][...]:
// rowcnt rows_total + 1, npts ODO_MAX_LEVELS_K, a / b / c 4 x cap_total floats and d cap_total floats, level l's entries at offset
// sum of (interior + spare) of the levels before it.
int dm_kf_lists(int n_sets, int form, int n_levels, const int* rows, const int* cols, const float* I1, const float* D1, float f0, float cx0,
                float cy0, int dense_above, int spare, int* rowcnt, int* npts, float* a, float* b, float* c, float* d) {
  if (n_sets < 1 || n_sets > 4 || form < 0 || form > 1) return (int)hipErrorInvalidValue;
  Pool P;
  std::vector<KfSet> S((size_t)n_sets);
  size_t npx = 0;
  for (int l = 0; l < n_levels && l < ODO_MAX_LEVELS_K; l++) npx += (size_t)(rows[l] > 0 ? rows[l] : 0) * (cols[l] > 0 ? cols[l] : 0);
  for (int i = 0; i < n_sets; i++)
    if (!kf_device_set(P, n_levels, rows, cols, I1 + npx * i, D1 + npx * i, spare, &S[i])) return (int)hipErrorInvalidValue;
  const KfTab* dtab = nullptr;
  if (form == 1) {
    std::vector<KfTab> tab((size_t)n_sets);
    for (int i = 0; i < n_sets; i++) {
      memset(&tab[i], 0, sizeof(KfTab));
      tab[i].kl = S[i].kl; tab[i].rowcnt = S[i].rowcnt; tab[i].npts = S[i].npts;
      for (int l = 0; l < ODO_MAX_LEVELS_K; l++) tab[i].pl[l] = S[i].pl[l];
    }
    dtab = P.up(tab.data(), (size_t)n_sets);
  }
  const int rt = S[0].rows_total;
  const size_t ct = S[0].cap_total;
  for (int run = 0; run < 2; run++) {
    if (form == 1) {
      DM_LAUNCH(P, kf_count_ref_kernel, dim3((unsigned)rt, (unsigned)n_sets), 256, dtab);
      DM_LAUNCH(P, kf_fill_ref_kernel, dim3((unsigned)rt, (unsigned)n_sets), 256, dtab, f0, cx0, cy0, dense_above);
    } else {
      for (int i = 0; i < n_sets; i++) kf_launch_by_value(P, S[i], f0, cx0, cy0, dense_above);
    }
    for (int i = 0; i < n_sets; i++) {
      const size_t s = (size_t)run * n_sets + i;
      P.down(rowcnt + s * ((size_t)rt + 1), S[i].rowcnt, (size_t)rt + 1);
      P.down(npts + s * ODO_MAX_LEVELS_K, S[i].npts, ODO_MAX_LEVELS_K);
      size_t at = 0;
      for (int l = 0; l < ODO_MAX_LEVELS_K; l++) {
        const size_t n = S[i].cap[l];
        P.down(a + 4 * (s * ct + at), (const float*)S[i].pl[l].a, 4 * n); P.down(b + 4 * (s * ct + at), (const float*)S[i].pl[l].b, 4 * n);
        P.down(c + 4 * (s * ct + at), (const float*)S[i].pl[l].c, 4 * n); P.down(d + (s * ct + at), (const float*)S[i].pl[l].d, n);
        at += n;
      }
    }
  }
  return P.done();
}
// What reads a list: the level's list built by the two kernels above (one level, level 0: its intrinsics are make_level_k(fl, cx, cy,
// 0)), then lm_residual_only_list_kernel and lm_residual_list_kernel launched as lm_launch_eval launches them — nblk blocks of
// kLmBlock over the n points kf_fill_kernel counted — on a state with `active` at pose L->T, twice. level_ok = 0: the launches'
// expect_level is not the state's level. found[0] = n. partials: [2][nblk + 1][29], res: [2][n_cap]; both start every launch as 0xAB
// bytes.
int dm_list_eval(const dm::PixLevel* L, int nblk, int active, int level_ok, int n_cap, int* found, double* partials, float* res) {
  const float f0 = (float)L->k.fl;
  if ((double)f0 != L->k.fl || nblk < 1 || nblk > 4096 || n_cap < 1) return (int)hipErrorInvalidValue;
  Pool P;
  KfSet S;
  if (!kf_device_set(P, 1, &L->rows, &L->cols, L->I1, L->D1, 1, &S)) return (int)hipErrorInvalidValue;
  kf_launch_by_value(P, S, f0, L->k.cx, L->k.cy, 0);
  int n = -1;
  P.down(&n, S.npts, 1);
  found[0] = n;
  if (P.err != hipSuccess || n < 0 || n > n_cap || (size_t)n + 1 > S.cap[0]) { const int e = P.done(); return e ? e : (int)hipErrorInvalidValue; }
  LevelK k = make_level_k(f0, L->k.cx, L->k.cy, 0);
  k.bilinear = L->k.bilinear;
  const float* dI2 = P.up(L->I2, (size_t)L->rows * L->cols);
  const LmState* st = dense_device_states(P, 1, L->T, &active);
  const float* dscale = P.up(&L->scale_sqr, 1);
  const size_t np = ODO_NACC * ((size_t)nblk + 1);
  double* dp = P.filled<double>(np);
  float* dres = P.filled<float>((size_t)n_cap);
  const int expect = level_ok ? kDmExpectLevel : kDmExpectLevel + 1;
  for (int run = 0; run < 2; run++) {
    P.fill(dp, np); P.fill(dres, (size_t)n_cap);
    DM_LAUNCH(P, lm_residual_only_list_kernel<0>, nblk, kLmBlock, S.pl[0], n, dI2, L->rows, L->cols, k, st, expect, dres);
    DM_LAUNCH(P, lm_residual_list_kernel<0>, nblk, kLmBlock, S.pl[0], n, dI2, L->rows, L->cols, k, st, expect, L->robust, L->huber_delta, dscale,
              dp);
    P.down(partials + run * np, dp, np); P.down(res + (size_t)run * n_cap, dres, (size_t)n_cap);
  }
  return P.done();
}

// ---- divisions ----
// n_bad: one count; first: kFirstCap indices (-1 = unused); q: 2 n_out results (shared form, then plain).
int dm_div32(int n, int form, const float* a, const float* b, unsigned long long* n_bad, int* first, int n_out, float* q) {
  if (n_out > n) return (int)hipErrorInvalidValue;
  Pool P;
  const float *da = P.up(a, n), *db = P.up(b, n);
  unsigned long long* dn = P.zeros<unsigned long long>(1);
  int* df = (int*)P.raw(sizeof(int) * kFirstCap);
  if (df && P.err == hipSuccess) P.err = hipMemset(df, 0xff, sizeof(int) * kFirstCap);
  float* dq = P.zeros<float>(2 * (size_t)n_out);
  DM_LAUNCH(P, div32_kernel, each_grid(n), kEachBlock, n, form, da, db, dn, df, n_out, dq);
  P.down(n_bad, dn, 1); P.down(first, df, kFirstCap); P.down(q, dq, 2 * (size_t)n_out);
  return P.done();
}
int dm_div64(int n, const double* a, const double* b, unsigned long long* n_bad, int* first, int n_out, double* q) {
  if (n_out > n) return (int)hipErrorInvalidValue;
  Pool P;
  const double *da = P.up(a, n), *db = P.up(b, n);
  unsigned long long* dn = P.zeros<unsigned long long>(1);
  int* df = (int*)P.raw(sizeof(int) * kFirstCap);
  if (df && P.err == hipSuccess) P.err = hipMemset(df, 0xff, sizeof(int) * kFirstCap);
  double* dq = P.zeros<double>(2 * (size_t)n_out);
  DM_LAUNCH(P, div64_kernel, each_grid(n), kEachBlock, n, da, db, dn, df, n_out, dq);
  P.down(n_bad, dn, 1); P.down(first, df, kFirstCap); P.down(q, dq, 2 * (size_t)n_out);
  return P.done();
}
// n_bad[3], first[3 * kFirstCap]: point_xyz, point_jacobian, warp.
int dm_callsites(int n, const int* x, const int* y, const float* d, const double* fl, const float* cx, const float* cy, int n_T,
                 const float* T, unsigned long long* n_bad, int* first) {
  if (n_T < 1) return (int)hipErrorInvalidValue;
  Pool P;
  const int *dx = P.up(x, n), *dy = P.up(y, n);
  const float *dd = P.up(d, n), *dcx = P.up(cx, n), *dcy = P.up(cy, n), *dT = P.up(T, 16 * (size_t)n_T);
  const double* dfl = P.up(fl, n);
  unsigned long long* dn = P.zeros<unsigned long long>(3);
  int* df = (int*)P.raw(sizeof(int) * 3 * kFirstCap);
  if (df && P.err == hipSuccess) P.err = hipMemset(df, 0xff, sizeof(int) * 3 * kFirstCap);
  DM_LAUNCH(P, callsite_kernel, each_grid(n), kEachBlock, n, dx, dy, dd, dfl, dcx, dcy, n_T, dT, dn, df);
  P.down(n_bad, dn, 3); P.down(first, df, 3 * kFirstCap);
  return P.done();
}

}  // extern "C"
