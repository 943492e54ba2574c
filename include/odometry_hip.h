/*
 * odometry_hip.h — C ABI of the MI355X-native photometric-LM tracking hot path.
 *
 * The reference (WangYuTum/odometry) has no FFI layer; its boundary is the public C++ surface the
 * runner uses (run_odometry_kitti_offline.cpp:68-70,88,102,130-131,205,215,229,251-252,261,268).
 * Each entry point below names the reference interface it replaces. The C++ shim classes in
 * include/odometry_shim.hpp keep the reference's class names and signatures over this ABI.
 *
 * Conventions: plain C, no exceptions; every call returns 0 on success and -1 on failure
 * (OptimizerStatus / GlobalStatus, ref: include/data_types.h:27-28) and odo_last_error() describes
 * the last failure of the calling thread. Poses are 16 fp32 COLUMN-major (Eigen Affine4f,
 * ref: include/data_types.h:24). Images are single-channel fp32 row-major (CV_32F, ref: data_types.h:10-12).
 * The caller owns all host buffers; the library owns device memory behind the opaque handles.
 * One odo_ctx = one HIP stream on one device; handles are not thread-safe (the reference is strictly
 * single-threaded, ref: run_odometry_kitti_offline.cpp:3).
 * There is NO CPU fallback: without a HIP device odo_ctx_create fails.
 */
#ifndef ODOMETRY_HIP_H
#define ODOMETRY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct odo_ctx odo_ctx;
typedef struct odo_pyr odo_pyr;
typedef struct odo_lm odo_lm;
typedef struct odo_depth odo_depth;
typedef struct odo_tracker odo_tracker;
typedef struct odo_camera odo_camera;
typedef struct odo_map odo_map;
typedef struct odo_volume odo_volume;
typedef struct odo_rgbd_frontend odo_rgbd_frontend;

/* Level-0 pinhole intrinsics (fy = fx). NULL wherever accepted = the KITTI-00 constants the reference
 * hard-codes (ref: include/image_processing_global.h:35-36: 718.856f, 607.1928, 185.2157). */
typedef struct {
  float f0, cx0, cy0;
} odo_intrinsics;

enum { ODO_PYR_IMAGE = 0, ODO_PYR_DEPTH = 1 };
enum { ODO_MAX_LEVELS = 8, ODO_NACC = 29 };

const char* odo_last_error(void);
int odo_version(void);

/* ---- context ------------------------------------------------------------------------------
 * One HIP stream + its bookkeeping. A context is meant for one host thread (the reference is single-threaded, ref:
 * run_odometry_kitti_offline.cpp:3): launches of two threads on the same context would interleave on its stream. Its device-block
 * free list, pinned staging ring and upload tickets are mutex-guarded, so allocation / upload / release from a second thread
 * (e.g. a Mat destroyed elsewhere) is safe. */
int odo_ctx_create(int device, odo_ctx** out);
/* Same, on a high-priority HIP stream (its hardware queue comes from a pool of its own): for a latency-critical chain of
 * dependent launches that must not queue behind other streams' work. Used by odo_tracker for the LM stream. */
int odo_ctx_create_high_priority(int device, odo_ctx** out);
int odo_ctx_destroy(odo_ctx* ctx);
int odo_ctx_synchronize(odo_ctx* ctx);
/* HIP-event timing on the context's own stream (bench.py): record start / stop around a region,
 * then read the elapsed milliseconds (synchronises on the stop event). */
int odo_ctx_timer_start(odo_ctx* ctx);
int odo_ctx_timer_stop(odo_ctx* ctx, float* elapsed_ms);
/* Device scratch for callers that keep inputs resident in HBM (bench.py, tracker). */
int odo_dev_alloc(odo_ctx* ctx, size_t bytes, void** out_dev);
int odo_dev_free(odo_ctx* ctx, void* dev);
int odo_dev_upload(odo_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int odo_dev_download(odo_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* The drop-in path (include/odometry_shim.hpp) without stalls: page-locked host blocks (an upload from one is a plain
 * asynchronous DMA; uploads from other host memory are copied once into the context's pinned staging ring), uploads that
 * return as soon as the caller may reuse its buffer instead of waiting for the device, and device blocks recycled through a
 * free list of the context, whose release neither synchronises the stream nor calls the driver (is_async, as returned by
 * the allocation, and the size go back into the matching free). Recycled blocks are for work on the context's own stream
 * only: a block may be handed out again while work that used it is still queued on that stream. A block from
 * odo_host_alloc must not be freed while uploads from it may be pending (odo_ctx_synchronize first). */
void* odo_host_alloc(size_t bytes);
void odo_host_free(void* host);
int odo_dev_upload_async(odo_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
/* The same for an image whose rows lie src_pitch bytes apart on the host (a cv::Mat view: step > cols * elemSize): `rows` rows of
 * row_bytes bytes land densely packed at dst_dev. */
int odo_dev_upload_2d_async(odo_ctx* ctx, void* dst_dev, const void* src_host, size_t src_pitch, size_t row_bytes, int rows);
/* Upload tickets: odo_dev_upload_async from a page-locked block (odo_host_alloc) is a DMA that reads the block in place after
 * the call has returned. odo_ctx_upload_ticket returns the ticket of the most recent such upload (monotonic, 0 = none);
 * odo_ctx_upload_wait(ticket) returns once that upload and all earlier ones no longer read host memory — the moment the block
 * may be rewritten or released. Waiting for a retired ticket costs nothing. */
unsigned long odo_ctx_upload_ticket(odo_ctx* ctx);
int odo_ctx_upload_wait(odo_ctx* ctx, unsigned long ticket);
/* Orders `waiter`'s stream behind everything queued on `signaller`'s stream so far (an event, no host wait): two contexts of one
 * host thread — the drop-in classes keep a second one for work that need not wait for the pose LM (an upload started early). */
int odo_ctx_stream_wait(odo_ctx* waiter, odo_ctx* signaller);
/* The same in two halves: odo_ctx_mark names the point `ctx`'s stream has been filled up to (returns a non-zero mark), and
 * odo_ctx_stream_wait_mark orders `waiter` behind that point — not behind what was queued on `signaller` since (a mark older
 * than the last 32 falls back to "everything queued so far"). */
unsigned long odo_ctx_mark(odo_ctx* ctx);
int odo_ctx_stream_wait_mark(odo_ctx* waiter, odo_ctx* signaller, unsigned long mark);
/* Host waits until `ctx`'s stream has passed `mark` (odo_ctx_mark). */
int odo_ctx_wait_mark(odo_ctx* ctx, unsigned long mark);
/* Has the stream passed that mark? 1 yes, 0 not yet (never blocks), -1 on error. */
int odo_ctx_mark_reached(odo_ctx* ctx, unsigned long mark);
/* Images in host memory the library cannot watch — a cv::Mat (ref: run_odometry_kitti_offline.cpp:200,334-359 refills the same two
 * Mats every frame; the classes of include/odometry_shim.hpp see them three times per frame, :205 / :229 / :251). A device mirror
 * of such an image may be reused only if the bytes are still the ones that were uploaded:
 *   odo_host_fingerprint       64-bit fingerprint of all pixels (rows of row_bytes bytes, src_pitch apart; one read of the image);
 *   odo_dev_upload_fp_async    odo_dev_upload_2d_async through the pinned staging ring, *fp = the fingerprint of exactly the bytes
 *                              that were staged (fused with the copy; the caller may rewrite the image once the call has returned);
 *   odo_dev_download_async     device -> a block from odo_host_alloc, asynchronous on ctx's stream (ComputeDepth's outputs are staged
 *                              on the host beside the pose LM, ref: src/depth_estimate.cpp:33-78 fills left_val / left_disp / left_dep);
 *   odo_host_copy_fingerprint  host -> host copy (staging block -> the caller's cv::Mat), returns the fingerprint of what was written.
 * Not cryptographic: it guards against a caller rewriting its buffer, not against an adversary. No device needed for the two
 * host-only calls. */
unsigned long long odo_host_fingerprint(const void* src_host, size_t src_pitch, size_t row_bytes, int rows);
unsigned long long odo_host_copy_fingerprint(void* dst_host, size_t dst_pitch, const void* src_host, size_t src_pitch, size_t row_bytes,
                                             int rows);
int odo_dev_upload_fp_async(odo_ctx* ctx, void* dst_dev, const void* src_host, size_t src_pitch, size_t row_bytes, int rows,
                            unsigned long long* fp);
int odo_dev_download_async(odo_ctx* ctx, void* dst_pinned_host, const void* src_dev, size_t bytes);
int odo_dev_alloc_async(odo_ctx* ctx, size_t bytes, void** out_dev, int* is_async);
int odo_dev_free_async(odo_ctx* ctx, void* dev, size_t bytes, int is_async);

/* ---- pyramids ------------------------------------------------------------------------------
 * Replaces ImagePyramid::ImagePyramid / DepthPyramid::DepthPyramid
 * (ref: include/image_pyramid.h:24,51; src/image_pyramid.cpp:13-19,30-37;
 *  src/image_processing_global.cpp:12-56,58-113).
 * kind IMAGE: L0 = 3x3 Gaussian blur if smooth else copy; L1 = pyrDown(input); Lk = pyrDown(L(k-1)).
 * kind DEPTH: L0 = copy, or cv::medianBlur 3x3 (replicated border) if smooth (ref: src/image_processing_global.cpp:76-80; no
 * reference caller passes 1); Lk(y,x) = L(k-1)(2y+1,2x+1).
 * `img` is a host pointer with row pitch stride_bytes (0 = cols*4). */
int odo_pyramid_create(odo_ctx* ctx, const float* img, int rows, int cols, size_t stride_bytes, int levels,
                       int smooth, int kind, odo_pyr** out);
/* Same, input already resident in device memory (dense, row pitch = cols*4). */
int odo_pyramid_create_dev(odo_ctx* ctx, const float* img_dev, int rows, int cols, int levels, int smooth,
                           int kind, odo_pyr** out);
/* Rebuild an existing pyramid in place from a new device-resident image of the same size. */
int odo_pyramid_rebuild_dev(odo_pyr* pyr, const float* img_dev, int smooth);
/* GetNumberLevels / GetPyramidImage / GetPyramidDepth (ref: include/image_pyramid.h:33,36,60,63). */
int odo_pyramid_levels(const odo_pyr* pyr);
int odo_pyramid_level_dims(const odo_pyr* pyr, int level, int* rows, int* cols);
int odo_pyramid_download(const odo_pyr* pyr, int level, float* dst_host);
const float* odo_pyramid_level_dev(const odo_pyr* pyr, int level);
int odo_pyramid_destroy(odo_pyr* pyr);

/* ---- pose optimiser --------------------------------------------------------------------------
 * Replaces LevenbergMarquardtOptimizer (ref: include/lm_optimizer.h:32,44,47,54;
 * src/lm_optimizer.cpp:19-41,54-69,73-160,163-264,364-405).
 * max_iters is indexed by pyramid level (ref: src/lm_optimizer.cpp:117). robust: 0 none, 1 Huber, 2 t-dist. */
int odo_lm_create(odo_ctx* ctx, float lambda, float precision, const int* max_iters, int n_levels,
                  const float init_colmajor[16], int robust, float huber_delta, const odo_intrinsics* K,
                  odo_lm** out);
/* Solve (ref: src/lm_optimizer.cpp:54-69): returns 0 and the keyframe->current pose, or -1 and the
 * pseudo-identity whose (3,3) element is 0 (ref: src/lm_optimizer.cpp:48-52,60-65). */
int odo_lm_solve(odo_lm* lm, const odo_pyr* kf_img, const odo_pyr* kf_dep, const odo_pyr* cur_img,
                 float out_colmajor[16]);
/* Optional: starts the Solve that the next odo_lm_solve(lm, kf_img, kf_dep, cur_img) with the SAME pyramids will collect, and
 * returns without waiting (a caller that knows the inputs early — the next frame's pyramid, the initial pose set by Reset —
 * overlaps the head of the Solve with its own bookkeeping). Same launches, earlier: results are unchanged. Reset, or a Solve on
 * other pyramids, abandons it. Returns 0 started, 1 nothing started (this Solve does not use the fused pipeline), -1 error.
 * While a started Solve is in flight the optimiser's trace / report of the previous Solve are being overwritten. */
int odo_lm_solve_begin(odo_lm* lm, const odo_pyr* kf_img, const odo_pyr* kf_dep, const odo_pyr* cur_img);
/* Host work for the time a Solve leaves the calling thread idle (ref: src/lm_optimizer.cpp:73-160 keeps the CPU busy for the whole
 * Solve; here the thread inside odo_lm_solve spins on the device's completion word for ~0.25 ms): `fn(arg)` is called over and over
 * from that wait loop, on the caller's thread, until the result is there — keep each call short (~10 us: the result is noticed between
 * calls). NULL removes it. Not for an optimiser owned by odo_tracker / odo_tracker_batch (they feed their depth stream from there). */
int odo_lm_set_idle_callback(odo_lm* lm, void (*fn)(void*), void* arg);
/* Keyframe-candidate point lists built ahead of the Solve that may need them (the point lists are what the validity test of
 * ComputeResidualJacobianNaive selects, ref: src/lm_optimizer.cpp:190-198; the runner promotes a frame to keyframe AFTER its Solve,
 * run_odometry_kitti_offline.cpp:258-260, so the first Solve against a new keyframe would build them in front of its first launch):
 * img / dep are the pyramids of a frame that may become the keyframe. The launches go to `side`'s stream behind `mark` of the
 * optimiser's stream (odo_ctx_mark; 0: behind everything queued there); the call returns at once. A later Solve on exactly these
 * pyramids adopts the lists by a buffer swap; any other Solve ignores them. One candidate at a time. Not for an optimiser owned
 * by a tracker. */
int odo_lm_candidate_begin(odo_lm* lm, odo_ctx* side, const odo_pyr* img, const odo_pyr* dep, unsigned long mark);
/* n independent Solves (n sequences, each with its own optimiser and pyramids) in the SAME launches: a single Solve is a
 * serial chain of short launches that leaves most of the chip idle, n chains side by side take the time of the longest.
 * Per-sequence arithmetic and launch order are those of odo_lm_solve: results are bit-identical to n separate calls. The
 * optimisers must share one context. out_colmajor: n x 16 floats; status[i] = 0 / -1 per sequence (a failed sequence gets
 * the pseudo-identity, like odo_lm_solve). Sequences that cannot take the fused point-list pipeline make the call fall back
 * to one Solve after the other. */
int odo_lm_solve_batch(int n, odo_lm* const* lms, const odo_pyr* const* kf_img, const odo_pyr* const* kf_dep,
                       const odo_pyr* const* cur_img, float* out_colmajor, int* status);
/* Reset (ref: src/lm_optimizer.cpp:373-382): new initial pose and lambda, statistics cleared. */
int odo_lm_reset(odo_lm* lm, const float init_colmajor[16], float lambda);
/* ShowReport data (ref: src/lm_optimizer.cpp:364-371). The reference never writes its statistics, so
 * `iters`/`cost` are always 0 there; here iters[l] = evaluations spent on level l in the last Solve and
 * cost[l][0..1] = mean weighted error at the first / last evaluation of level l. */
int odo_lm_report(const odo_lm* lm, int iters[4], float cost[4][2]);
int odo_lm_destroy(odo_lm* lm);

/* One ComputeResidualJacobianNaive + normal-equation pass (ref: src/lm_optimizer.cpp:163-264,129,145-149)
 * at pose T on `level`: acc[0..20] upper triangle of JtWJ (row-major), acc[21..26] JtWr, acc[27] sum w r^2,
 * acc[28] N. Parity-test entry for the dominant kernel. */
int odo_lm_accumulate(odo_lm* lm, const odo_pyr* kf_img, const odo_pyr* kf_dep, const odo_pyr* cur_img, int level,
                      const float T_colmajor[16], double acc[ODO_NACC]);
/* Per-evaluation trace of the last Solve (level, iteration, residual count, accept / stop decision, error, lambda, step; see
 * DESIGN.md). Optimisers created with odo_lm_create record it (and the per-level cost statistics of odo_lm_report); the
 * optimisers inside odo_tracker / odo_tracker_batch do not — nobody reads them, and the row costs ~600 cycles per evaluation on
 * the critical wave — unless ODO_LM_TRACE=1 is set when the tracker is created; odo_lm_trace then returns -1. */
typedef struct {
  int level, iter, n_res, accepted, stop;
  float err, lambda_after;
  float delta[6];
} odo_lm_trace_row;
int odo_lm_trace(const odo_lm* lm, odo_lm_trace_row* rows, int cap, int* n_rows);
/* Recording on (1, the default of odo_lm_create) / off (0). Off: the optimiser's Solves run the lean builds of the LM kernels —
 * no per-evaluation trace rows, no per-level cost statistics (odo_lm_trace returns -1, odo_lm_report's costs read 0; its
 * evaluation counts stay) —, ~2 % less time per Solve. The drop-in LevenbergMarquardtOptimizer switches it off: the reference's
 * ShowReport prints statistics nobody ever wrote (ref: src/lm_optimizer.cpp:364-371). Not while a Solve is in flight. */
int odo_lm_set_record(odo_lm* lm, int on);
/* Roofline leg of bench.py (any size / intrinsics, e.g. the dense 1920x1080 config): `reps` event-bracketed launches of
 * the evaluation kernel on `level` at pose T; mean / min launch time, algorithmic bytes of one launch, residual count. */
int odo_lm_time_eval(odo_lm* lm, const odo_pyr* kf_img, const odo_pyr* kf_dep, const odo_pyr* cur_img, int level,
                     const float T_colmajor[16], int reps, float* mean_us, float* min_us, double* algorithmic_bytes,
                     int* n_points);
/* The same for n optimisers of one context in ONE launch (blockIdx.y = stream): the batched dense evaluation of odo_lm_solve_batch.
 * `level` must be dense (not a point-list level) for every optimiser; algorithmic_bytes / n_points_total are totals over the streams. */
int odo_lm_time_eval_batch(int n, odo_lm* const* lms, const odo_pyr* const* kf_img, const odo_pyr* const* kf_dep,
                           const odo_pyr* const* cur_img, int level, const float T_colmajor[16], int reps, float* mean_us,
                           float* min_us, double* algorithmic_bytes, int* n_points_total);
/* Roofline leg of bench.py: execution spans of the LM kernels' launches (lm_coarse_kernel, lm_step_kernel and their batched
 * twins). A sampled launch records the device wall clock (100 MHz) at the entry of its earliest block and at the exit of its latest
 * one — the kernel's own execution time, free of queueing and dispatch effects — into a slot of device memory; the statistics
 * calls drain the stream and read the slots. on = 0: off; 1: every launch; N > 1: every N-th launch of a Solve (rotating residue:
 * cheap enough to stay on inside a timed region). For a batched Solve the statistics live with the first optimiser. */
int odo_lm_event_timing(odo_lm* lm, int on);
int odo_lm_event_stats(odo_lm* lm, double* total_us, long* launches, long* active_launches,
                       double* algorithmic_bytes);
/* Share of the above spent in the single-workgroup coarse-level kernel (one launch per Solve). */
int odo_lm_event_stats2(odo_lm* lm, double* coarse_us, long* coarse_launches);
/* out[0] sampled step-kernel time (us), [1] sampled step launches, [2] sampled coarse-kernel time (us), [3] sampled coarse
 * launches, [4] all launches issued, [5] all coarse launches, [6] evaluations, [7] algorithmic bytes, [8] / [9] summed
 * start-to-start periods of consecutive sampled step launches (us) and their number — execution plus the dependent-kernel
 * boundary: what an evaluation costs the serial chain —, [10] / [11] the same from a coarse launch to the step launch behind it. */
int odo_lm_event_stats_ex(odo_lm* lm, double out[12]);
/* Sampling of the current image at the warped point. ODO_SAMPLE_FLOOR (default, parity mode) is what the reference does:
 * I2 at floor(u), floor(v), central-difference gradient at that pixel (ref: src/lm_optimizer.cpp:208-217,
 * include/image_processing_global.h:62-69). ODO_SAMPLE_BILINEAR is a NON-PARITY option (BASELINE.json north_star: "bilinear
 * sample"): I2 interpolated in the 2x2 cell around (u, v), gradient = derivative of that interpolant, points whose cell
 * leaves the image skipped; everything else (geometric Jacobian at the un-warped point, weights, LM schedule) unchanged. It
 * has its own oracle mode (orc_set_sampling) and its own parity tests. */
enum { ODO_SAMPLE_FLOOR = 0, ODO_SAMPLE_BILINEAR = 1 };
int odo_lm_set_sampling(odo_lm* lm, int sampling);
/* Iteration space of the residual kernel: 0 = automatic (per keyframe and level: a compacted point list when at most
 * half of the interior pixels carry depth, the dense scan of the reference otherwise), 1 = always the dense scan,
 * 2 = always the point list. All three evaluate the same per-point arithmetic. */
int odo_lm_set_mode(odo_lm* lm, int mode);
/* Points per level of the cached keyframe lists and which levels use them (after a Solve / accumulate). */
int odo_lm_points(const odo_lm* lm, int npts[ODO_MAX_LEVELS], int use_list[ODO_MAX_LEVELS]);
/* Launch statistics of the last Solve (bench.py roofline): number of residual-kernel launches that did
 * work, and the algorithmic bytes they touched (dense scan 12 B per interior
 * pixel, point list 32 B per point, plus the fp64 partials written). */
int odo_lm_launch_stats(const odo_lm* lm, int* n_active_launches, int* n_total_launches, double* algorithmic_bytes);
/* The persistent launch of the fine levels (lm_fine_kernel: every evaluation the coarse launch leaves in ONE launch whose
 * workgroups exchange partial sums through L2): *workgroups = how many cooperate (0: off — this optimiser
 * issues a step launch per evaluation, by choice (ODO_LM_NO_FINE) or after three fall-backs), *fallbacks = Solves whose persistent
 * launch gave up waiting for one of its workgroups and that were redone on the step launches (results unaffected): this
 * optimiser's own Solves plus the batched Solves (odo_lm_solve_batch, odo_tracker_batch) of its context. */
int odo_lm_persistent_stats(const odo_lm* lm, int* workgroups, int* fallbacks);
/* Which path the optimiser's last odo_lm_solve / odo_lm_solve_batch took (read-only, host values, no synchronisation):
 * out[0] the number of sequences of the batched Solve it ran in — 0: a Solve of its own, which is also what every optimiser reports
 *        after odo_lm_solve_batch fell back to one Solve after the other (more than 64 sequences, t-distribution weights, ...);
 * out[1] min_level: the coarse launch took the levels >= min_level (n_levels: there was none);
 * out[2] fine_lo: the persistent launch took the levels [fine_lo, min_level), step launches what lies below (fine_lo >= min_level:
 *        the sequence took no part in a persistent launch);
 * out[3] workgroups per sequence of the persistent launch that was issued for the Solve (0: none was issued) — in a batched Solve
 *        the launch's number, the same for every sequence, also for one that only has its state carried by it;
 * out[4] launches issued (of the whole batch; after a redo: of the redo);
 * out[5] 1 if the persistent launch gave up and the Solve was redone on the step launches (out[1 .. 3] then describe the redo). */
int odo_lm_last_plan(const odo_lm* lm, int out[6]);
/* Its give-up policy. A wait inside the launch is bounded by the device wall clock (4 ms; ODO_LM_FINE_WAIT_US) — stretched while the
 * shader clock runs below nominal (process start, power cap), but never beyond 4 x the bound (16 ms) —, so a give-up costs that + one
 * redo of the Solve on the step launches. Three give-ups switch the launch off; it is tried again after *retry_after
 * Solves — 4 096, doubling with every further switch-off up to 2^20 — and 1 024 clean Solves with the launch on forget all of it.
 * *strikes = give-ups that count at the moment (3: switched off), *solves_until_retry = Solves left on the step launches before the
 * next try (0 while the launch is on). */
int odo_lm_persistent_backoff(const odo_lm* lm, int* strikes, int* retry_after, int* solves_until_retry);
/* ComputeScaleNaive over levels too large for one workgroup (ref: src/lm_optimizer.cpp:338-358; dense levels, robust mode 2):
 * *multi_launches = scale iterations issued on the multi-workgroup kernel, *fallbacks = those redone by the single-workgroup kernel
 * queued behind it because the launch gave up waiting for a workgroup. The two kernels add in different orders: a Solve with a
 * fall-back may differ from one without in the last bits of sigma (and so of the pose). Synchronises the optimiser's stream. */
int odo_lm_tdist_stats(odo_lm* lm, long* multi_launches, int* fallbacks);

/* Diagnostic: cycle-counter stamps at the phase boundaries of one LM update launch ("update kernel"). */
int odo_debug_update_stamps(odo_lm* lm, const odo_pyr* kf_img, const odo_pyr* kf_dep, const odo_pyr* cur_img, int level,
                            const float T_colmajor[16], unsigned long long stamps[8]);
/* Test entry: the wave-parallel damped 6x6 solve used by the LM update kernel (ref: src/lm_optimizer.cpp:145-151)
 * on caller-supplied accumulators. */
int odo_debug_solve(odo_ctx* ctx, const double acc[ODO_NACC], float lambda, float delta[6]);

/* ---- depth estimator ---------------------------------------------------------------------------
 * Replaces DepthEstimator (ref: include/depth_estimate.h:31-33,51,54; src/depth_estimate.cpp:9-26,33-78,
 * 80-198,200-242,244-401,435-453,465-468). Camera pointers are replaced by K (NULL = KITTI-00).
 * max_disparity: 0 = the reference search range [boundary, x) (ref: src/depth_estimate.cpp:382), else
 * [max(boundary, x - max_disparity), x). any_size: 0 keeps the 376x1241 guard (ref: :46-49). */
int odo_depth_create(odo_ctx* ctx, float grad_th, float ssd_th, float photo_th, float min_depth, float max_depth,
                     float lambda, float huber_delta, float precision, int max_iters, int boundary,
                     const odo_intrinsics* K, float baseline, int max_residuals, int max_disparity, int any_size,
                     odo_depth** out);
/* ComputeDepth (ref: src/depth_estimate.cpp:33-78). Host buffers; val/disp/dep are overwritten
 * (zero-filled first: SURVEY appendix B #14). Returns -1 when fewer than 500 points survive (ref: :192-197). */
int odo_depth_compute(odo_depth* d, const float* left, const float* right, int rows, int cols, uint8_t* val,
                      float* disp, float* dep);
/* Same with device-resident inputs and outputs (no PCIe in the timed region). */
int odo_depth_compute_dev(odo_depth* d, const float* left_dev, const float* right_dev, int rows, int cols,
                          uint8_t* val_dev, float* disp_dev, float* dep_dev);
/* The front half of ComputeDepth that needs the LEFT image only — its 3x3 blur and the block-median point selection (ref:
 * src/depth_estimate.cpp:255-256,300-342) — enqueued ahead of the call, on `side`'s stream, so that it runs beside whatever the
 * estimator's own stream is busy with (the drop-in classes issue it from ImagePyramid's constructor, ref:
 * run_odometry_kitti_offline.cpp:205: the pose LM's Solve of :215 then hides it). `stamp` (non-zero) names the image's content:
 * odo_depth_compute_dev_stamped(.., the same left_dev, the same stamp) picks the prepared half up (same launches, earlier: results
 * identical); any other call drops it. Work queued on the estimator's stream before this call is ordered in front of it. */
int odo_depth_prepare_left_dev(odo_depth* d, odo_ctx* side, const float* left_dev, int rows, int cols, unsigned long long stamp);
/* ... ordered behind `mark` of the estimator's stream (odo_ctx_mark, taken once left_dev was complete) instead of behind everything
 * queued there by now — for a caller that has meanwhile queued work the prepared half is meant to run BESIDE (the pose LM's Solve).
 * The estimator's previous ComputeDepth must have returned before the mark was taken. */
int odo_depth_prepare_left_dev_marked(odo_depth* d, odo_ctx* side, const float* left_dev, int rows, int cols, unsigned long long stamp,
                                      unsigned long mark);
int odo_depth_compute_dev_stamped(odo_depth* d, const float* left_dev, const float* right_dev, int rows, int cols,
                                  uint8_t* val_dev, float* disp_dev, float* dep_dev, unsigned long long left_stamp);
/* The WHOLE of ComputeDepth(left, right) (ref: src/depth_estimate.cpp:31-78) started ahead of the call: every launch of it goes to
 * `side`'s stream — behind `mark` of the estimator's stream (0: behind everything queued there), i.e. behind whatever produced the
 * two images and recycled the three output blocks — and the function returns without waiting. ComputeDepth does not depend on the
 * pose: the drop-in classes start it once the Solve of :215 has been queued, and the runner's ComputeDepth of :229 only collects it.
 * Returns 0: started; 1: not started (the inverse-depth LM would need host-paced step launches: its persistent launch is off or
 * switched off) — nothing was queued; -1: error. Stamps (non-zero) name the two images' contents.
 * odo_depth_compute_end_dev: ComputeDepth proper with both stamps. The job started ahead with exactly these arguments is waited for
 * (bounded spin on its completion word; the estimator's stream is ordered behind it), a job started ahead with other arguments is
 * waited for and dropped, and without a matching job everything is computed now: the same launches either way, results identical.
 * Every other entry point of the estimator drops a job started ahead the same way. odo_depth_early_pending: 1 while one is out. */
int odo_depth_compute_begin_dev(odo_depth* d, odo_ctx* side, const float* left_dev, const float* right_dev, int rows, int cols,
                                uint8_t* val_dev, float* disp_dev, float* dep_dev, unsigned long long left_stamp,
                                unsigned long long right_stamp, unsigned long mark);
int odo_depth_compute_end_dev(odo_depth* d, const float* left_dev, const float* right_dev, int rows, int cols, uint8_t* val_dev,
                              float* disp_dev, float* dep_dev, unsigned long long left_stamp, unsigned long long right_stamp);
int odo_depth_early_pending(const odo_depth* d);
/* The three output images handed over SPARSELY, for callers whose images live in host memory they own (cv::Mat): the images are zero
 * everywhere but at the selected points (ref: src/depth_estimate.cpp:388-397,176-191 write at the points only; the zero fill is forced
 * deviation #14), so {pixel index, val, disp, dep} per point slot — odo_depth_compact_bytes() = 532 KB instead of 4.2 MB at KITTI size —
 * crosses PCIe, and the host rebuilds the images: odo_depth_compact_outputs_async queues the gather and the copy into `dst_pinned`
 * (an odo_host_alloc block) on `on`'s stream, behind the job that wrote val_dev / disp_dev / dep_dev there (the estimator's point list of
 * that job must still be current: call it before the estimator's next ComputeDepth); odo_host_scatter_outputs, once the copy has
 * completed (odo_ctx_mark / odo_ctx_wait_mark), zero-fills the caller's three images and writes the points, and returns the
 * fingerprint (odo_host_fingerprint) of the inverse-depth image it wrote — the one output the runner hands back in (DepthPyramid,
 * ref: run_odometry_kitti_offline.cpp:252). Host-only, no device needed for the second call. */
size_t odo_depth_compact_bytes(void);
int odo_depth_compact_outputs_async(odo_depth* d, odo_ctx* on, const uint8_t* val_dev, const float* disp_dev, const float* dep_dev, int cols,
                                    void* dst_pinned);
int odo_host_scatter_outputs(const void* compact, int rows, int cols, uint8_t* val, size_t val_pitch, float* disp, size_t disp_pitch,
                             float* dep, size_t dep_pitch, unsigned long long* dep_fingerprint);
/* The same into images the caller has ALREADY zero-filled (the fill needs nothing from the device: a caller with idle time before the
 * compact block arrives does it then, odo_lm_set_idle_callback). */
int odo_host_scatter_outputs_prezeroed(const void* compact, int rows, int cols, uint8_t* val, size_t val_pitch, float* disp,
                                       size_t disp_pitch, float* dep, size_t dep_pitch, unsigned long long* dep_fingerprint);
/* Disparity stage only (DisparityDepthEstimate, ref: src/depth_estimate.cpp:244-401). */
int odo_depth_disparity(odo_depth* d, const float* left, const float* right, int rows, int cols, uint8_t* val,
                        float* disp, float* dep);
/* bench.py config-5 leg: event-timed blur / point selection / epipolar SSD scan on device-resident images (mean of
 * `reps`, microseconds), the number of SSD candidates one scan evaluates and the number of selected points. */
int odo_depth_time_stages(odo_depth* d, const float* left_dev, const float* right_dev, int rows, int cols, int reps,
                          float us[3], double* candidates, int* n_selected);
/* ReportStatus data (ref: src/depth_estimate.cpp:465-468) + counts printed by ComputeDepth (:62,74). */
int odo_depth_report(const odo_depth* d, int* iters, float* cost, int* n_selected, int* n_matched, int* n_valid);
/* DepthOptimization (ref: src/depth_estimate.cpp:141-191) runs as ONE persistent launch (depth_lm_persistent_kernel: 80 workgroups of
 * 512 threads on one XCD, one point slot per thread with its state in registers, one tagged 16-byte pair {error sum, count} per
 * workgroup and iteration through L2) instead of a launch
 * per iteration; the step launches are its fall-back, bit-identical. *on = 1 while the persistent launch is in use (0: off, by
 * choice — ODO_DEPTH_NO_PERSIST — or after three give-ups, with the pose LM's back-off: odo_lm_persistent_backoff), *fallbacks =
 * ComputeDepth calls whose launch gave up waiting for one of its workgroups and that were run again on the step launches. */
int odo_depth_persistent_stats(const odo_depth* d, int* on, int* fallbacks);
int odo_depth_destroy(odo_depth* d);

/* ---- tracker: the runner's frame loop ---------------------------------------------------------------
 * Replaces the body of main() in run_odometry_kitti_offline.cpp:58-145 (set-up, frame 0) and :198-271 (per
 * frame): ImagePyramid(cur) -> Solve against the current keyframe -> cur_pose = KF * T^-1 -> ComputeDepth ->
 * rebuild the frame's image / depth pyramids -> keyframe test on the weighted motion -> Reset(T, 0.01).
 * Inputs are device-resident fp32 images (rows x cols, dense). ComputeDepth runs on a second HIP stream
 * concurrently with Solve when overlap_depth != 0 (the two are independent in the reference's loop):
 * 1 = both streams fed by the calling thread, 2 = stream B fed by a helper host thread (default). */
typedef struct {
  int rows, cols, levels;
  float lm_lambda, lm_precision;          /* ref: run_odometry_kitti_offline.cpp:88 (0.01f, 0.995f) */
  int lm_max_iters[ODO_MAX_LEVELS];       /* ref: :76 {10,20,30,30} */
  int lm_robust;                          /* ref: :86 (1 = Huber) */
  float lm_huber_delta;                   /* ref: :87 (28) */
  float grad_th, ssd_th, photo_th;        /* ref: :62-64 (8, 900, 15) */
  float min_depth, max_depth;             /* ref: :59-60 (0.1, 30) */
  float depth_lambda, depth_huber_delta, depth_precision; /* ref: :65-67 (0.01, 28, 0.995) */
  int depth_max_iters, boundary, max_residuals;            /* ref: :68,:69 (50, 4), :61 (80000) */
  int max_disparity, any_size;            /* deviations from the reference, both 0 in parity mode */
  odo_intrinsics K;
  float baseline;                         /* ref: :41 */
  float keyframe_weight[6];               /* ref: :144-145 */
  float keyframe_motion_th;               /* ref: :258 (1.1) */
  int smooth_image;                       /* ref: :130,:205,:251 (true) */
  int overlap_depth;
} odo_tracker_params;

int odo_tracker_default_params(odo_tracker_params* p); /* the runner's constants for KITTI 1241x376 */
/* Frame sizes: with any_size = 0 only 376 x 1241 (the reference's own check, ref: src/depth_estimate.cpp:46-49). With any_size = 1
 * every rows x cols whose point-selection tile — the 16 x 32 grid inside `boundary` = b — holds
 *   1 <= ((cols - 2b) / 32) * ((rows - 2b) / 16) <= 4096 pixels (integer divisions), and rows, cols <= 65535.
 * Odd sizes are supported (every pyramid level halves, rounding down); 3, 4 and 5 levels are tested. The rule is checked when a
 * frame arrives — odo_tracker_init returns -1 with the message, before anything is launched — not at create; the batched tracker
 * checks it at create. tests/shape_cases.py lists the sizes the whole trackers are tested at. */
int odo_tracker_create(int device, const odo_tracker_params* p, odo_tracker** out);
/* Frame 0 (ref: :95-145): ComputeDepth, pyramids, first keyframe with absolute pose abs_pose0. May be called again at
 * any time to start a new sequence on the same tracker: it drains both streams first and the tracker then behaves
 * exactly like a freshly created one. */
int odo_tracker_init(odo_tracker* t, const float* left_dev, const float* right_dev, const float abs_pose0_colmajor[16]);
/* One iteration of the frame loop (ref: :198-271). Returns 0, or -1 when ComputeDepth failed (the runner
 * breaks out of its loop there, ref: :230-232); like the runner, which stores the frame's pose before it computes the depth
 * (ref: :215-232), pose_to_keyframe / abs_pose / solve_status of that last frame are still written. A failed Solve is NOT an
 * error (the runner carries on with the pseudo-identity); solve_status reports it, and abs_pose is then NaN (the inverse of
 * the singular pseudo-identity, ref: :218), not zeros. */
int odo_tracker_track(odo_tracker* t, const float* left_dev, const float* right_dev, float pose_to_keyframe[16],
                      float abs_pose[16], int* is_new_keyframe, float* motion_mag, int* solve_status);
/* Optional pipelining for callers that already hold the next frame (offline runs): announce its left image before
 * tracking the current frame; its image pyramid (ref: :205 of the NEXT iteration) is then built during this call on a stream
 * of its own, and the next frame's Solve is started (odo_lm_solve_begin: initial pose = this frame's result, ref: :261 / :268)
 * as soon as this frame's Solve has returned, while the depth stream finishes this frame. Same work, earlier; results are
 * unchanged (the LM's per-evaluation trace of the frame just tracked may already be overwritten when the call returns;
 * ODO_NO_EARLY_SOLVE=1 keeps the pyramid prefetch only). The hinted buffer is identified by its device
 * address: its contents must not change between the hint and the odo_tracker_track call that consumes it (a caller that
 * recycles one buffer for every frame must not hint). odo_tracker_init drops a pending hint / prefetched pyramid. */
int odo_tracker_hint_next(odo_tracker* t, const float* next_left_dev);
/* The same with the next frame's right image as well: its ComputeDepth + candidate pyramids (ref: :226-252 of the NEXT
 * iteration; they depend on the images only) are then enqueued on the depth stream a frame early too, behind this frame's, so
 * the depth stream works a frame ahead of the pose LM and a short Solve no longer waits for it (overlap_depth == 2;
 * ODO_NO_DEPTH_AHEAD=1 turns it off). Both buffers must stay unchanged until the odo_tracker_track call that consumes them.
 * Results are unchanged. odo_tracker_outputs stays valid until the next odo_tracker_track call, as before. */
int odo_tracker_hint_next_pair(odo_tracker* t, const float* next_left_dev, const float* next_right_dev);
/* Runs to completion (or drops) everything still in flight on behalf of frames the caller handed over — the stream-B job of an
 * announced pair, the prefetched pyramid of an announced image, an early-started Solve — and leaves all streams idle. After it
 * returns nothing, queued or yet to be issued by the helper thread, reads a caller-owned frame buffer: call it before freeing or
 * overwriting frames that were announced but never tracked (odo_tracker_destroy / odo_tracker_init do it themselves). */
int odo_tracker_quiesce(odo_tracker* t);
/* Keyframe point-cloud map (replaces GlobalMap, ref: include/global_map.h, and the keyframe export of save_to_vis,
 * ref: run_odometry_kitti_offline.cpp:259-265,432-471, which writes every keyframe's images, depth and mask as PNGs for another
 * program to build the cloud from). Points are {x, y, z, intensity} fp32 in world coordinates plus {keyframe, pixel} int32;
 * keyframe = the map's own 0-based insertion counter, pixel = y * cols + x. One insertion takes the pixels with
 * (val == NULL || val != 0) && inverse depth valid (|d| >= 0.01) && d > 0, in row-major order; camera point = the LM's
 * back-projection at level 0 (odo_math.h point_xyz); world point = A * camera point, fp32 in the order ((a0 X + a4 Y) + a8 Z) + a12.
 * voxel_size > 0: key k = floor(world / voxel_size) per axis; a point with any |k| >= 2^20 is dropped (dropped_range); a point is
 * kept iff no earlier point of this or an earlier insertion had its key (dropped_voxel); points already in the map are never
 * replaced. voxel_size = 0: every candidate is kept. Kept points are appended in (insertion, pixel) order; once the map holds
 * `capacity` points the rest are dropped (dropped_capacity), and an insertion into a full map changes nothing but the insertion
 * counter. The result is a pure function of the inputs. */
/* rows x cols: the frames' size; capacity: points (1 .. 2^28). Device memory: 24 B per point + 32 B per hash slot (a power of two
 * >= 2 (capacity + rows * cols), voxel filter on only) + ~17 B per pixel. */
int odo_map_create(odo_ctx* ctx, int rows, int cols, long capacity, float voxel_size, odo_map** out);
/* One keyframe into the map (GlobalMap::InsertKeyFrame): device buffers of rows x cols; val_dev NULL = no mask, img_dev NULL =
 * intensity 0, K NULL = the KITTI-00 constants. abs_pose: camera-to-world, the convention of odo_tracker_track's abs_pose.
 * Asynchronous on ctx's stream (four launches, no host synchronisation); ordered after every earlier insertion. */
int odo_map_insert_dev(odo_map* m, const uint8_t* val_dev, const float* dep_dev, const float* img_dev, const odo_intrinsics* K,
                       const float abs_pose_colmajor[16]);
/* Points in the map; waits for pending insertions. -1 on error. */
long odo_map_size(odo_map* m);
/* Points first .. first + count - 1 to the host (save_to_vis' export): 4 floats each, and 2 ints each when kf_pixel != NULL. */
int odo_map_download(odo_map* m, long first, long count, float* xyzi, int* kf_pixel);
/* out: size, insertions, candidates, dropped_voxel, dropped_range, dropped_capacity (waits for pending insertions). */
int odo_map_stats(odo_map* m, long out[6]);
/* The camera-to-world pose insertion `keyframe` was made with (GlobalMap's keyframe poses). */
int odo_map_keyframe_pose(const odo_map* m, int keyframe, float abs_pose_colmajor[16]);
/* Empty map: points, voxels, counters and the insertion counter start from nothing. */
int odo_map_clear(odo_map* m);
/* TEST ONLY, for the project's own suite; not part of the interface an integrator uses and free to change. The voxel filter's hash
 * table as it stands (waits for pending insertions): *n_slots = its slot count, stored whenever m and the pointers are not NULL; with
 * n_slots_cap >= that count, keys[slot] and payload[slot] of every slot (an unclaimed slot holds all ones in both; a claimed one
 * its 63-bit voxel key and the least (insertion << 32 | pixel) of its claimants). -1, nothing copied: a NULL argument, a map without
 * a filter (voxel_size == 0), n_slots_cap too small. */
int odo_debug_map_table(odo_map* m, unsigned long long n_slots_cap, unsigned long long* keys, unsigned long long* payload,
                        unsigned long long* n_slots);
/* -1 while the map is attached to a tracker. */
int odo_map_destroy(odo_map* m);
/* The tracker inserts every keyframe into m (GlobalMap::InsertKeyFrame where the runner keeps its keyframes, ref:
 * run_odometry_kitti_offline.cpp:259-265): frame 0 in odo_tracker_init, each promotion in odo_tracker_track, with the frame's
 * mask, inverse depth, level-0 image and abs_pose. The insertions run on a stream of the map's own and are never waited for by
 * the host while tracking; odo_tracker_quiesce / init / destroy drain them. Poses are unchanged. Same device and frame size as
 * the tracker; one tracker per map. NULL detaches (pending insertions complete first). */
int odo_tracker_attach_map(odo_tracker* t, odo_map* m);
/* ---- RGB-D tracking: a sensor depth frame in place of the stereo pair's ComputeDepth ----
 * The reference's plan (README: "RGB-D odometry using the existing code blocks ... monocular RGB as well as Depth outputs from
 * the sensor (TUM RGB-D dataset or Intel Realsense)"): the frame loop of odo_tracker_track with the depth of each frame taken from
 * a sensor. Inputs per frame: a grey image (fp32 rows x cols, as the stereo tracker's left image) and a depth frame (uint16 rows x
 * cols, dense row-major, device-resident; raw 0 = no reading). The depth job of a frame:
 *   1. selection: the point selection of ComputeDepth (ref: src/depth_estimate.cpp:300-342) on the 3x3-blurred grey image — the
 *      16 x 32 block grid inside `boundary`, block median + grad_th, the first <= 80 pixels per block in raster order;
 *   2. each selected pixel p, r = raw[p]: r == 0 -> invalid; else d = depth_scale / (float)r (one IEEE fp32 divide), invalid if
 *      1.0f / d > max_depth || 1.0f / d < min_depth (the write-back filter, ref: src/depth_estimate.cpp:183, stated on d); invalid
 *      if a 4-neighbour q inside the image with raw[q] != 0 has (float)|raw[q] - r| > max_depth_step * (float)r (one fp32
 *      rounding; neighbours outside the image are skipped; INFINITY turns the guard off). Valid: val = 1, dep = d; otherwise
 *      val = 0, dep = 0. Unselected pixels: val = 0, dep = 0; disp = 0 everywhere;
 *   3. statistics (odo_depth_report on odo_tracker_depth): n_selected, n_matched = selected with r != 0, n_valid; iters = 0,
 *      cost = 0; status -1 ("depth failed") when n_valid < 500 (ref: src/depth_estimate.cpp:192), with the stereo tracker's
 *      consequences in init and track.
 * Everything behind the depth job — depth pyramid, keyframe-candidate lists, the helper thread, announced frames, the keyframe
 * policy, attached maps — is the stereo tracker's. */
/* Uses p's size, levels, lm_*, grad_th, boundary (>= 1: the selection's gradient reads the pixels next to its grid), min_depth /
 * max_depth, K, keyframe weights / threshold, smooth_image and overlap_depth; ignores the stereo and depth-LM fields and implies
 * any_size. depth_scale: raw units per metre (TUM 5000, RealSense 1000), finite and > 0; max_depth_step >= 0 (INFINITY: off).
 * Frame sizes: the tile rule of odo_tracker_create, 1 <= ((cols - 2b) / 32) * ((rows - 2b) / 16) <= 4096 and rows, cols <= 65535,
 * checked by odo_tracker_init_rgbd (-1 with the message, nothing launched), not here. */
int odo_tracker_create_rgbd(int device, const odo_tracker_params* p, float depth_scale, float max_depth_step, odo_tracker** out);
/* odo_tracker_init / odo_tracker_track / odo_tracker_hint_next_pair for an RGB-D tracker (same contracts; the depth frame takes
 * the right image's place). odo_tracker_hint_next (grey only), outputs, stats, timing, quiesce and attach_map work on either
 * tracker; the stereo entries refuse an RGB-D tracker and these refuse a stereo one, without enqueueing anything. */
int odo_tracker_init_rgbd(odo_tracker* t, const float* gray_dev, const uint16_t* depth_dev, const float abs_pose0_colmajor[16]);
int odo_tracker_track_rgbd(odo_tracker* t, const float* gray_dev, const uint16_t* depth_dev, float pose_to_keyframe[16],
                           float abs_pose[16], int* is_new_keyframe, float* motion_mag, int* solve_status);
int odo_tracker_hint_next_rgbd(odo_tracker* t, const float* next_gray_dev, const uint16_t* next_depth_dev);
/* Counters of the last tracked frame: LM evaluations, depth-LM iterations, valid depth points, keyframes so far. */
int odo_tracker_stats(const odo_tracker* t, int* lm_evals, int* depth_iters, int* n_valid_depth, int* n_keyframes);
/* Device pointers to the last frame's outputs (rows x cols): validity mask (u8), disparity, inverse depth. */
int odo_tracker_outputs(const odo_tracker* t, const uint8_t** val_dev, const float** disp_dev, const float** dep_dev);
/* Roofline leg of bench.py: `reps` event-bracketed launches of the dominant kernel (residual / normal-equation
 * pass) on `level` of the tracker's current pyramids; mean / min launch time, algorithmic bytes of one launch
 * (12 B per interior pixel + the fp64 partials written) and the number of residuals it produced. */
int odo_tracker_time_residual(odo_tracker* t, int level, int reps, float* mean_us, float* min_us,
                              double* algorithmic_bytes, int* n_points);
/* Diagnostics: host-clock averages per tracked frame since the last call, microseconds:
 * {track() call, Solve on stream A, stream-B job on the helper thread, wait for the helper}. */
int odo_tracker_timing(odo_tracker* t, double out[4]);
/* Chained Solves: with the next frame announced, its Solve is queued BEHIND this frame's before this frame's result exists —
 * same keyframe, initial pose = this Solve's result taken on the device (what Reset hands it, ref: run_odometry_kitti_offline.cpp:
 * 261,268), guarded on the device by the runner's keyframe test (ref: :253-258: a promoted or failed frame makes every launch of
 * the chained Solve return at once). The host's own test decides what counts; results are those of the unchained order.
 * Opt-in (ODO_CHAIN_SOLVE=1): it closes the GPU's idle gap between two Solves and does not change the frame rate. *adopted = chained Solves that became the next Solve, *wasted = chained Solves that ran for
 * nothing because the two keyframe tests disagreed (an ulp of atan2f: expected never). */
int odo_tracker_chain_stats(const odo_tracker* t, long* adopted, long* wasted);
/* Armed Solves (round 6; the default with the next pair announced, ODO_NO_ARM=1 turns them off): the next frame's Solve has its
 * coarse launch queued behind this frame's before this frame's result exists and starts on a word the host writes after the runner's
 * keyframe test (ref: run_odometry_kitti_offline.cpp:253-268) — same launches, same arithmetic, no launch call and no dispatch between
 * two Solves. started: Solves that began that way; returned: armed launches told to return (new keyframe, failed Solve). */
int odo_tracker_arm_stats(const odo_tracker* t, long* started, long* returned);
odo_lm* odo_tracker_lm(odo_tracker* t);
odo_depth* odo_tracker_depth(odo_tracker* t);   /* its depth estimator (odo_depth_persistent_stats, odo_depth_report) */
odo_ctx* odo_tracker_ctx(odo_tracker* t);

/* ---- TSDF volume: tracked RGB-D depth frames fused into dense geometry ------------------------------------------------------------
 * The second half of the reference's plan (README: an RGB-D odometry that "outputs camera trajectories as well as reconstructed 3D
 * geometry"): every depth frame with a known pose is integrated into a dense truncated signed distance grid (Curless & Levoy;
 * KinectFusion's map), and the surface is read back as an oriented point cloud. All floating point is fp32, one rounding per
 * operation; a voxel's new value depends on its old value and the frame only (no atomics, no order dependence inside a frame;
 * frames are ordered by the stream), and a voxel that is skipped is neither loaded nor stored.
 * Grid. nx x ny x nz voxels, x fastest; voxel (i, j, k) has centre o + ((float)i + 0.5f) * vs per axis. A voxel is 4 bytes: int16 q
 * (truncated signed distance * 32767) and uint16 w (weight; 0 = never observed); cleared: q = 0, w = 0.
 * Integration of one frame (raw uint16 rows x cols in the grey camera's grid, camera-to-world abs_pose). The host forms the
 * world-to-camera M = [R^T | -R^T t] in fp64 from the fp32 entries (the translation as -((r0 t0 + r1 t1) + r2 t2)) and rounds each
 * entry to fp32 once; R is taken as given. Per voxel centre (X, Y, Z):
 *   1. xc = ((m0 X + m4 Y) + m8 Z) + m12, yc and zc likewise; skipped unless zc > 0;
 *   2. u = f0 * (xc / zc) + cx0, v = f0 * (yc / zc) + cy0; xi = floorf(u + 0.5f), yi = floorf(v + 0.5f), compared AS FLOATS against
 *      [0, cols), [0, rows) (NaN: skipped);
 *   3. r = raw[yi * cols + xi]; skipped if r == 0; D = (float)r / depth_scale; skipped if D > max_depth;
 *   4. sdf = D - zc (projective, along the optical axis); skipped if sdf < -mu; s = fminf(1.0f, sdf / mu) * 32767.0f;
 *   5. W = (float)w; F = ((float)q * W + s) / (W + 1.0f); q' = (int16)rintf(F) (ties to even); w' = min(w + 1, max_weight).
 * Counters of an integration: voxels updated, and of those the ones with |sdf| <= mu.
 * Extraction. For every voxel a in raster order (k, then j, then i) and its +x, +y, +z neighbour b, in that order, inside the grid:
 * the edge carries a point iff w_a > 0 && w_b > 0 && (q_a > 0) != (q_b > 0). alpha = (float)q_a / ((float)q_a - (float)q_b); the
 * point is a's centre with alpha * vs added on the edge's axis. Normal: with Q = (float)q and "usable" = inside the grid and
 * w > 0, g(v) per axis = Q[v + e] - Q[v - e] if both neighbours are usable, else 2.0f * (Q[v + e] - Q[v]) if only v + e is, else
 * 2.0f * (Q[v] - Q[v - e]) if only v - e is; a voxel with an axis on which neither is usable has no gradient. If a and b both have
 * one: n = g_a + alpha * (g_b - g_a) per component, len = sqrtf((nx nx + ny ny) + nz nz), n / len if len > 0; otherwise
 * (0, 0, 0). The normal points from the surface into observed free space. Output per point: {x, y, z, 0} and
 * {nx, ny, nz, (float)min(w_a, w_b)}, in (voxel, axis) order; points beyond `capacity` are counted as dropped, not written. The
 * result is a pure function of the volume. */
typedef struct {
  int nx, ny, nz;          /* every dimension >= 2, nx * ny * nz <= 2^30; device memory: 4 B per voxel */
  float voxel_size;        /* metres, finite > 0 */
  float origin[3];         /* world position of the grid's minimum corner */
  float mu;                /* truncation distance, metres, > 0 */
  float max_depth;         /* metres: readings beyond it are ignored */
  int max_weight;          /* 1 .. 65535 */
  int rows, cols;          /* the depth frames' size */
  odo_intrinsics K;        /* of the grey camera (the depth frames are registered to it) */
  float depth_scale;       /* raw units per metre */
} odo_volume_params;
/* Validates everything before it touches the device. */
int odo_volume_create(odo_ctx* ctx, const odo_volume_params* p, odo_volume** out);
/* One depth frame (device-resident) into the volume. Asynchronous on ctx's stream (two launches, no host synchronisation), ordered
 * after every earlier operation on the volume; the depth buffer must stay unchanged until odo_volume_sync or the next call that
 * waits. A pose with a non-finite entry (the abs_pose of a failed Solve) is refused: -1, nothing enqueued, counters unchanged. */
int odo_volume_integrate_dev(odo_volume* v, const uint16_t* depth_dev, const float abs_pose_colmajor[16]);
/* Waits for every pending integration. */
int odo_volume_sync(odo_volume* v);
/* The surface as oriented points (waits; three launches into buffers the volume owns, then the copy): xyz0 / nrmw receive 4 floats
 * per point, at most `capacity` (0 .. 2^28) points; *n_points = points written, *n_dropped (may be NULL) = points beyond capacity.
 * The volume is not modified. */
int odo_volume_extract(odo_volume* v, long capacity, float* xyz0, float* nrmw, long* n_points, long* n_dropped);
/* The whole grid to the host, nx * ny * nz values each in raster order (either may be NULL); waits for pending integrations. */
int odo_volume_download(odo_volume* v, int16_t* q, uint16_t* w);
/* The counterpart of odo_volume_download: the whole grid from the host, nx * ny * nz values each in raster order, both arrays
 * required. Ordered after everything pending and marked like any operation that changes the volume; the frame and update counters
 * stay as they are. Refused (-1) while the volume is attached to a tracker. Restores a saved reconstruction. */
int odo_volume_upload(odo_volume* v, const int16_t* q, const uint16_t* w);
/* The surface as a triangle mesh: marching tetrahedra on the Kuhn split of every cell. A table of 6 x 16
 * entries derived by rule (odometry_amd/csrc/volume_mesh_table.h), no ambiguous cases, watertight by construction.
 * Lattice. Nodes are voxel centres. Voxel a = (i, j, k) owns up to seven edges (a, e), e = 0 .. 6 with the directions d_e =
 * (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1), b = a + d_e inside the grid.
 * Vertex. (a, e) carries one iff w_a > 0 && w_b > 0 && (q_a > 0) != (q_b > 0): the extraction's rule on seven directions.
 * alpha = Q_a / (Q_a - Q_b) in fp32 (Q = (float)q); position: on every axis with d_e = 1 centre + alpha * vs (the product rounded,
 * then the sum), the centre itself on the others; normal: g_a + alpha * (g_b - g_a) with the extraction's gradient and
 * normalisation unchanged, (0, 0, 0) if a gradient is missing. Output xyz0 = {x, y, z, (float)e}, nrmw = {nx, ny, nz,
 * (float)min(w_a, w_b)}, in (voxel in raster order, e ascending) order; a vertex's index is its position in that order. A vertex
 * that no triangle references is still emitted. The rows with e < 3, in order, are odo_volume_extract's points bit for bit.
 * Cell (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, has the corners c = dx + 2 dy + 4 dz; it is live iff all eight have w > 0, and
 * only live cells produce triangles. Six tetrahedra per cell, with the corner paths (0,1,3,7) (0,1,5,7) (0,2,3,7) (0,2,6,7)
 * (0,4,5,7) (0,4,6,7): every edge of every tetrahedron is one of the seven directions from its lower corner, so it has exactly one
 * owner (voxel, e), whose vertex exists whenever the cell is live and the edge changes sign.
 * Triangles of a tetrahedron with path positions p0 .. p3, "positive" = q > 0: none for 0 or 4 positive corners; one isolated corner
 * s (1 or 3 positive), the others r0 < r1 < r2: one triangle on the edges (s,r0) (s,r1) (s,r2); two and two (positives a < b, the
 * others c < d): the quad V0 = (a,c) V1 = (a,d) V2 = (b,d) V3 = (b,c) as (V0,V1,V2) and (V0,V2,V3). Winding: counter-clockwise seen
 * from the positive side (observed free space, where the normals point); it depends on the tetrahedron and the sign pattern only
 * (the sign of a 3 x 3 determinant of corner offsets, part of the table). Each triangle is then rotated so that its smallest vertex
 * index comes first. Output int32[3] per triangle in (cell in raster order, tetrahedron 0 .. 5, triangle) order.
 * q == 0 counts as not positive and gives alpha = -+0: coincident vertices and zero-area triangles are kept.
 * The call waits for pending integrations and modifies neither the volume nor its integration counters. Capacities 0 .. 2^28; with
 * a capacity of 0 its buffers may be NULL, and (0, 0) returns the totals. counts = {vertices written, vertices beyond
 * vertex_capacity, triangles written, triangles beyond triangle_capacity}; written items are the first min(total, capacity) in
 * the order above. Indices are NEVER remapped: a triangle may name a vertex beyond vertex_capacity, and the mesh is complete iff
 * counts[1] == 0 && counts[3] == 0. A volume with more than 2^31 - 1 vertices is refused once anything is to be written. Arguments
 * are validated before any device work. Four launches on the volume's stream, no atomics; scratch of 5 B per voxel (31 MB for
 * 240 x 128 x 200) from the first call until the volume is destroyed. */
int odo_volume_mesh(odo_volume* v, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw, int32_t* tri,
                    long counts[4]);
/* out: frames integrated since create / clear, voxels updated by the last integration, of those the ones in the band
 * (|sdf| <= mu), voxel updates since create / clear (waits for pending integrations). */
int odo_volume_stats(odo_volume* v, long out[4]);
/* Empty volume: every voxel and every counter start from nothing. */
int odo_volume_clear(odo_volume* v);
/* -1 while the volume is attached to a tracker. */
int odo_volume_destroy(odo_volume* v);
/* RGB-D trackers only (a stereo tracker is refused, nothing enqueued); same device and frame size; one tracker per volume; NULL
 * detaches after the pending integrations complete. With a volume attached, odo_tracker_init_rgbd and every odo_tracker_track_rgbd
 * whose Solve succeeded (solve_status == 0; a failed Solve leaves abs_pose NaN) enqueue one integration of that frame's depth with
 * the returned abs_pose on the volume's own stream, without a host wait on the frame's path; a frame whose depth JOB failed (return
 * -1) still has a good pose and a good sensor frame and is integrated. Poses, masks and keyframe decisions are bit-identical to
 * those without a volume. Because the integration reads the caller's depth buffer, a tracker with a volume attached asks for one
 * thing more: a tracked frame's depth buffer must stay unchanged until the next odo_tracker_track_rgbd / init_rgbd / quiesce /
 * destroy has returned — those calls make sure, through an event a whole frame old, that the previous frame's integration has
 * finished before they return (the front end's ring of four slots used two frames ahead satisfies this). */
int odo_tracker_attach_volume(odo_tracker* t, odo_volume* v);

/* ---- Colour in the TSDF volume: the sensor's colour fused beside the geometry, colours for its points and its mesh ------------------
 * Optional. A volume that never calls odo_volume_enable_colour allocates nothing more, behaves and writes exactly as above.
 * Colour grid. A second array beside the voxel grid, one 32-bit word per voxel in the same raster order: uint8 R, G, B (bytes 0, 1,
 * 2) and uint8 wc (byte 3: the colour weight, 0 = never coloured); cleared to 0. +4 B per voxel: 8 B per voxel in all, 49 MB for a
 * 240 x 128 x 200 grid.
 * Colour frame. rows x cols pixels in the grid of the depth frames (the grey camera's), interleaved uint8, dense rows, 3 or 4
 * channels in the order RGB(A) or BGR(A) (the front end's formats); a fourth channel is ignored. Stored as R, G, B whatever the order.
 * Coloured integration of one frame. Steps 1 to 5 of the integration above unchanged: q, w and the counters are bit for bit those
 * of odo_volume_integrate_dev on the same frame. Exactly the voxels that update touches AND that lie in the band, fabsf(sdf) <= mu
 * (the predicate of the in-band counter, so the colour updates of a frame equal that counter), also read the colour pixel (xi, yi)
 * of step 2 — the pixel the depth reading came from, nearest, no interpolation — and update their colour word; no other voxel reads a
 * colour pixel or touches the colour grid. Per channel, with the sample s, in unsigned integer arithmetic with floor division:
 *   c' = (c * wc + s + ((wc + 1) >> 1)) / (wc + 1);   then wc' = min(wc + 1, max_weight).
 * The numerator stays below 2^17, the result is in 0 .. 255, and wc = 0 gives c' = s (odometry_amd/csrc/volume_colour_math.h holds the
 * device's formulation, a multiplication by a reciprocal that gives this value for every (c, wc, s)). A running 8-bit average stalls at
 * weight 255: a sample that differs from c by less than half a level times 256 = 128 levels leaves c where it is. That is known and
 * accepted; a caller who wants an average that tracks sets max_weight small (with 3, a sample moves c by a quarter of the difference).
 * Colour of a point or vertex on the edge (a, b) with the extraction's alpha (in [0, 1] by construction, so no clamp is needed): both
 * voxels have wc > 0: per channel rintf((float)Ca + alpha * ((float)Cb - (float)Ca)), the product rounded, then the sum, and
 * A = 255; exactly one has: that voxel's R, G, B and A = 255; neither: (0, 0, 0, 0). uint8[4] per point, index for index beside
 * xyz0 / nrmw. */
typedef struct {
  int channels;            /* 3 | 4 */
  int bgr;                 /* 0: RGB(A), 1: BGR(A) */
  int max_weight;          /* 1 .. 255 */
} odo_volume_colour_params;
/* Validates first, then allocates the colour grid and clears it on the volume's stream. Refused (-1, nothing changed) on a second
 * call and while the volume is attached to a tracker. */
int odo_volume_enable_colour(odo_volume* v, const odo_volume_colour_params* p);
/* odo_volume_integrate_dev with the colour update: the same stream, ordering, refusal of a non-finite pose and buffer lifetimes (the
 * colour buffer as the depth buffer), one fused launch and the sum. colour_dev: the device colour frame, 4-byte aligned when
 * channels == 4. Refused on a volume without colour. odo_volume_integrate_dev on a volume with colour stays legal and leaves the
 * colour grid alone. */
int odo_volume_integrate_colour_dev(odo_volume* v, const uint16_t* depth_dev, const uint8_t* colour_dev, const float abs_pose_colmajor[16]);
/* The whole colour grid to / from the host, 4 bytes {R, G, B, wc} per voxel in raster order, with the ordering and refusal rules of
 * odo_volume_download / odo_volume_upload (the upload is refused while attached). odo_volume_upload does not touch the colour grid;
 * odo_volume_clear clears it. Refused on a volume without colour. */
int odo_volume_download_colour(odo_volume* v, uint8_t* rgbw);
int odo_volume_upload_colour(odo_volume* v, const uint8_t* rgbw);
/* odo_volume_extract / odo_volume_mesh plus one uint8[4] row per point / vertex (one launch more on the volume's stream, skipped
 * when nothing is written; no atomics). xyz0, nrmw, tri, the counts and the capacity rules are bit for bit those of the uncoloured
 * calls on the same volume. Refused on a volume without colour. Neither grid and no counter is modified. */
int odo_volume_extract_colour(odo_volume* v, long capacity, float* xyz0, float* nrmw, uint8_t* rgba, long* n_points, long* n_dropped);
int odo_volume_mesh_colour(odo_volume* v, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw, uint8_t* rgba,
                           int32_t* tri, long counts[4]);
/* Names the colour frame (device) of the frame that the next odo_tracker_init_rgbd / odo_tracker_track_rgbd gets. That call consumes
 * it whether or not it integrates (a failed Solve integrates nothing, as without colour). With a frame named, the attached volume's
 * integration of that frame is the coloured one; without, the plain one. The buffer follows the depth buffer's rule: unchanged until
 * the next track / init / quiesce / destroy has returned. Refused unless this is an RGB-D tracker with a colour-enabled volume
 * attached. Poses, masks, keyframe flags and motion scores are bit-identical with and without it. */
int odo_tracker_frame_colour(odo_tracker* t, const uint8_t* colour_dev);

/* ---- Ray-cast of the TSDF volume: the model seen from a camera, as depth, normal and colour frames -----------------------------------
 * A pure function of the grid, a camera-to-world pose and the parameters below; the output frame is independent of the volume's own
 * rows / cols / K. All floating point is fp32, one rounding per operation (DESIGN.md section 9.7 holds the same table).
 * Host part (fp64 from the fp32 entries, each result rounded to fp32 once): e_c = (t_c - origin_c) / vs - 0.5 per axis, the camera
 * centre in voxel-index coordinates, in which voxel centres sit at integers; G_rc = R_rc / vs for the nine rotation entries.
 * Per pixel (x, y): dx = ((float)x - cx) / f, dy = ((float)y - cy) / f; g_r = (G_r0 dx + G_r1 dy) + G_r2 for r = x, y, z. The
 * camera-frame direction is (dx, dy, 1), so the ray parameter t is depth along the optical axis: the quantity of the depth frames
 * and of the projective signed distance.
 * Sample n = 0 .. n_steps - 1: t_n = t_min + (float)n * step (not accumulated); p_c = e_c + t_n * g_c; b_c = floorf(p_c). The sample
 * is valid only if b_c >= 0.0f && b_c <= (float)(dim_c - 2) on every axis — compared as floats before any conversion, NaN and inf
 * fail — and all eight corners b + d, d in {0, 1}^3, have w > 0 (the mesh's live cell). fr_c = p_c - b_c.
 * Interpolation, with Q = (float)q of the corners c_xyz:  l_yz = c_0yz + fr_x * (c_1yz - c_0yz);  m_z = l_0z + fr_y * (l_1z - l_0z);
 * F = m_0 + fr_z * (m_1 - m_0).
 * End of a ray. The ray ends at its first valid sample with F <= 0.0f. It is a hit iff sample n - 1 exists, is valid and has
 * F_prev > 0.0f; then z = t_prev + (F_prev / (F_prev - F)) * (t_n - t_prev). Every other ending, and a ray that runs out of samples,
 * gives no hit; an invalid sample between a positive and a non-positive one also gives no hit.
 * Outputs per pixel, row-major:
 *   depth  float32: z, or 0 for no hit.
 *   raw    uint16: (uint16)fminf(65535.0f, rintf(z * depth_scale)) with the volume's depth_scale, or 0 for no hit: a frame that
 *          odo_volume_integrate_dev and the RGB-D tracker accept as it is.
 *   nrmw   float[4]. On a hit the sample arithmetic is evaluated once more at t = z. If that cell is valid, the normal is the gradient
 *          of the interpolant in it: d_yz = c_1yz - c_0yz; gx_z = d_0z + fr_y * (d_1z - d_0z); gx = gx_0 + fr_z * (gx_1 - gx_0);
 *          gy_z = l_1z - l_0z; gy = gy_0 + fr_z * (gy_1 - gy_0); gz = m_1 - m_0; len = sqrtf((gx gx + gy gy) + gz gz); the output is
 *          g / len if len > 0. Otherwise, and without a hit, (0, 0, 0). World axes, as the extraction's normals, pointing into observed
 *          free space. The fourth component is (float) the smallest w of the eight corners where a normal is written, else 0.
 *   rgba   uint8[4], volumes with colour only: the colour word of voxel floorf(p_c + 0.5f) of that same cell evaluation (one of the
 *          cell's corners): (R, G, B, 255) if the cell is valid and that voxel's wc > 0, else four zeros.
 * Validation, all of it before any device work (-1, nothing enqueued, every counter unchanged): rows and cols 1 .. 4096; f finite
 * > 0; cx, cy finite; t_min finite >= 0; step finite > 0; n_steps 1 .. 4096; every pose entry finite; device outputs aligned to
 * their element (4, 2, 16, 4 bytes). */
typedef struct {
  int rows, cols;          /* the output frame, 1 .. 4096 each */
  float f, cx, cy;         /* its pinhole: focal length in pixels (finite > 0) and principal point (finite) */
  float t_min, step;       /* first sample depth (finite >= 0) and sample distance (finite > 0), metres along the optical axis */
  int n_steps;             /* samples per ray, 1 .. 4096 */
} odo_raycast_params;
/* One launch, a thread per pixel, no atomics, asynchronous on the volume's own stream behind everything that changed the volume so
 * far; odo_volume_sync covers it, and a later integration on any stream is ordered behind it. Any output may be NULL (all four: nothing
 * is enqueued); rgba_dev is refused on a volume without colour. Neither grid and no counter is modified. Legal while the volume is
 * attached to a tracker: ordered behind the integrations enqueued so far, as odo_volume_mesh is. */
int odo_volume_raycast_dev(odo_volume* v, const odo_raycast_params* p, const float abs_pose_colmajor[16], float* depth_dev,
                           uint16_t* raw_dev, float* nrmw_dev, uint8_t* rgba_dev);
/* The same with host outputs, through frames on the device that the volume owns (sized on first use, grown on demand, released with
 * the volume); the call waits and copies. */
int odo_volume_raycast(odo_volume* v, const odo_raycast_params* p, const float abs_pose_colmajor[16], float* depth, uint16_t* raw,
                       float* nrmw, uint8_t* rgba);
/* How the ray-cast's colour frame samples the colour grid (DESIGN.md section 9.11 holds the same rule). mode 0, the state at create:
 * the nearest voxel, as the table above states it. mode 1, trilinear: on a hit whose cell evaluation at t = z is valid, with cw_d the
 * colour words of the cell's eight corners d (bit 0 = x, bit 1 = y, bit 2 = z, the corners c_xyz above), m_d = (wc_d > 0) ? 1.0f :
 * 0.0f; M = the interpolation above (l, m, F with fr_x, fr_y, fr_z of that cell evaluation) over m_d in place of the corners; per
 * channel k, P_k = the same over m_d * (float)C_dk. If M > 0.0f the pixel is ((uint8)fminf(255.0f, rintf(P_k / M)), 255) with an IEEE
 * fp32 divide, else four zeros; a cell that is not valid and a pixel without a hit give four zeros, as in mode 0. Eight coloured
 * corners have M == 1.0f exactly. depth, raw and nrmw do not depend on the mode, bit for bit.
 * The mode is read when a ray-cast is enqueued: odo_volume_raycast_dev, odo_volume_raycast and odo_volume_track_photo_dev (whose
 * model frame then carries the interpolated colours) follow it; a ray-cast without rgba and odo_volume_track_dev launch what they
 * launch in mode 0. Refused (-1, nothing enqueued, the mode unchanged) on a volume without a colour grid and for any other mode.
 * Legal while the volume is attached; odo_volume_clear leaves the mode. odo_volume_colour_sampling returns the mode (-1: NULL). */
int odo_volume_set_colour_sampling(odo_volume* v, int mode);
int odo_volume_colour_sampling(odo_volume* v);
/* Diagnostic: one ray-cast to warm and then `reps` (1 .. 10000) of them between two events on the volume's stream, into the frames
 * that the volume owns (depth and nrmw; rgba as well if with_colour), under the colour sampling mode as it is; the call waits.
 * *us: microseconds per ray-cast (the launch and the event that orders a later integration behind it). Validation as
 * odo_volume_raycast. */
int odo_volume_raycast_time(odo_volume* v, const odo_raycast_params* p, const float abs_pose_colmajor[16], int with_colour, int reps,
                            float* us);

/* ---- Frame-to-model tracking: a depth frame aligned to the volume's ray-cast by point-to-plane ICP --------------------------------
 * The model frame is a ray-cast of the volume at the volume's own rows, cols and K (f = K.f0, cx = K.cx0, cy = K.cy0): depth
 * (float32) and nrmw, taken from the camera-to-world pose P_m. The sensor frame is a uint16 raw depth frame as odo_volume_integrate_dev
 * takes it. The unknown is C, the transform from the sensor camera to the model camera (column-major, C_rc at C[4 c + r]); projective
 * association, point-to-plane Gauss-Newton over up to three strides of the sensor frame. All floating point is fp32, one rounding
 * per operation, unless fp64 is named (DESIGN.md section 9.8 holds the same table).
 * Host part (fp64 from the fp32 entries, each result rounded to fp32 once): M = [R^T | -R^T t] of P_m as in the integration;
 * C_0 = M P_init with every entry ((m_r0 p_0c + m_r1 p_1c) + m_r2 p_2c) + m_r3 p_3c; at the end abs_pose = P_m C the same way.
 * Per sensor pixel (x, y) with x % s == 0 && y % s == 0, s the level's stride:
 *   1. r = raw[y cols + x]; skipped if 0. D = (float)r / depth_scale; skipped if D > max_depth (the integration's step 3).
 *   2. dx = ((float)x - cx) / f, dy = ((float)y - cy) / f (the ray-cast's); p = (dx D, dy D, D).
 *   3. pm_r = ((C_r0 p_x + C_r1 p_y) + C_r2 p_z) + C_r3; skipped unless pm_z > 0.
 *   4. u = f (pm_x / pm_z) + cx, v = f (pm_y / pm_z) + cy; xi = floorf(u + 0.5f), yi = floorf(v + 0.5f); skipped unless 0 <= xi < cols
 *      and 0 <= yi < rows, compared as floats before any conversion, so NaN fails (the integration's step 2).
 *   5. zm = depth_m[yi cols + xi]; skipped unless zm > 0. n_w = nrmw_m[yi cols + xi].xyz; skipped if all three are 0.
 *      n_r = (M_r0 n_w.x + M_r1 n_w.y) + M_r2 n_w.z: the normal in the model camera.
 *   6. vm = ((((float)xi - cx) / f) zm, (((float)yi - cy) / f) zm, zm); d = pm - vm; dd = (d_x d_x + d_y d_y) + d_z d_z; skipped
 *      unless dd <= dist_max * dist_max (the product in fp32; equality keeps the pair).
 *   7. res = (n_x d_x + n_y d_y) + n_z d_z;
 *      J = (n_x, n_y, n_z, pm_y n_z - pm_z n_y, pm_z n_x - pm_x n_z, pm_x n_y - pm_y n_x), translation first as in the LM's steps;
 *      w = (|res| <= huber_delta ? 1 : huber_delta / |res|) if huber_delta > 0, else 1.
 *   8. The 29 sums of the pose LM, fp64 over exact products of fp32 values: the upper triangle of sum (J_a w) J_b in row-major order
 *      (21), sum (J_a w) res (6), sum (res w) res, and the number of pairs; J_a w and res w are rounded to fp32 first.
 * The order of the sums is fixed (per block of 16 x 16 lattice points, then over the blocks in raster order: volume_icp.hip.h), no
 * atomics: two calls on the same inputs give the same bits.
 * Step. It fails (status 1) if the number of pairs is below min_pairs or any sum is not finite. Otherwise delta solves the undamped
 * normal equations in fp64 by the pose LM's elimination (a zero pivot leaves its component at 0), rounded to fp32, and
 * C <- matrix(SE3(exp(delta) C)) with the pose LM's exponential, fp32 4 x 4 product and quaternion round trip. The level has
 * converged when sqrtf((d_0 d_0 + d_1 d_1) + d_2 d_2) < eps_t and the same over d_3 .. d_5 is < eps_r; otherwise it ends after
 * iters[level] steps. Levels run in the order given, each from the C the one before left.
 * Conditioning (host, fp64). eig_min and eig_max are the extreme eigenvalues of the 6 x 6 of the last evaluation (cyclic Jacobi).
 * Translation (metres) and rotation (radians) share the matrix unscaled, so the ratio depends on the scene's distance from the
 * camera: it is a test for a direction that the geometry does not constrain at all (a corridor's axis: 1e-6), not a measure of
 * accuracy. If eig_min < min_eig_ratio * eig_max the alignment is refused (status 2). A C with a non-finite entry is status 1.
 * status: 0 aligned; 1 too few pairs or non-finite sums; 2 rank-deficient. On 1 and 2 abs_pose is sixteen NaNs — the trackers'
 * convention for a failed Solve, which odo_volume_integrate_dev refuses. */
typedef struct {
  int levels;                  /* 1 .. 3 */
  int stride[3];               /* per level, 1 .. 16 */
  int iters[3];                /* per level, >= 0; their sum over the levels 1 .. 64 */
  float dist_max;              /* the pair gate in metres, finite > 0 */
  float huber_delta;           /* metres, finite >= 0; 0: no robust weight */
  float eps_t, eps_r;          /* convergence thresholds on the step, metres / radians, finite >= 0 (0: every iteration runs) */
  int min_pairs;               /* >= 6 */
  float min_eig_ratio;         /* 0 .. 1; 0: never refused as rank-deficient */
} odo_icp_params;
typedef struct {
  int status;                  /* 0, 1, 2: above */
  int iterations;              /* steps taken over all levels (a failed one included) */
  double pairs, cost;          /* of the last evaluation: the number of pairs and sum w res^2 */
  double eig_min, eig_max;     /* of its 6 x 6; 0 if nothing was evaluated */
  float C[16];                 /* the last estimate, whatever the status */
} odo_icp_result;
typedef struct {               /* one step of an alignment */
  int level, iteration;        /* iteration counts over all levels from 0 */
  double acc[29];              /* the sums of the evaluation at the C before the step */
  float delta[6];              /* the step (zeros when it failed) */
  float C[16];                 /* the estimate after it */
} odo_icp_trace_row;
/* One evaluation of steps 1 .. 8 at C for one stride: acc receives the 29 sums; rows_dev (device, 16-byte aligned, may be NULL)
 * receives float[8] = {J_0 .. J_5, res, w} for every pixel of the frame, eight zeros for a pixel that is skipped or off the stride.
 * depth_m_dev / nrmw_m_dev: the model frame on the device (4 / 16-byte aligned), model_pose = P_m; raw_dev: the sensor frame.
 * Validation before any device work (-1, nothing enqueued): stride 1 .. 16, dist_max finite > 0, huber_delta finite >= 0, every
 * entry of C and model_pose finite, alignment. The call runs on the volume's own stream behind everything that changed the volume
 * so far and waits. Neither grid and no counter is modified; legal while attached, ordered as odo_volume_raycast_dev is. */
int odo_volume_icp_eval_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const float model_pose_colmajor[16],
                            const uint16_t* raw_dev, const float C_colmajor[16], int stride, float dist_max, float huber_delta,
                            double acc[29], float* rows_dev);
/* Event timing of the two kernels (diagnostic): reps (1 .. 10000) launches of the rows kernel at C for one stride, then reps launches
 * of the step kernel's fold, each batch between two events on the volume's own stream; us[0], us[1] receive the mean time of one
 * launch of either in microseconds. Validated, ordered and legal as odo_volume_icp_eval_dev; nothing of the volume changes. */
int odo_volume_icp_time_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const float model_pose_colmajor[16],
                            const uint16_t* raw_dev, const float C_colmajor[16], int stride, float dist_max, float huber_delta, int reps,
                            float us[2]);
/* The alignment: the sum of iters pairs of ordinary launches (rows, step) on the volume's own stream, each of which returns at once
 * when its level has converged or the alignment has failed; the host waits once, at the end. init_pose = P_init, the first guess of
 * the sensor camera's camera-to-world pose; abs_pose receives P_m C or sixteen NaNs. trace (host, may be NULL) receives the first
 * trace_capacity steps, *trace_n (may be NULL) how many were written. Validation of params, the poses and the alignment before any
 * device work (-1, nothing enqueued). Ordered and legal as odo_volume_icp_eval_dev. */
int odo_volume_icp_align_dev(odo_volume* v, const odo_icp_params* p, const float* depth_m_dev, const float* nrmw_m_dev,
                             const float model_pose_colmajor[16], const uint16_t* raw_dev, const float init_pose_colmajor[16],
                             float abs_pose_colmajor[16], odo_icp_result* result, odo_icp_trace_row* trace, int trace_capacity,
                             int* trace_n);
/* Frame-to-model tracking of one depth frame: a ray-cast of the volume from prev_pose at the volume's own rows, cols and K with
 * t_min = 0, step = mu / 2 and n_steps = min(4096, ceil((max_depth + mu) / step) + 1) (api.TsdfVolume.raycast's defaults) into frames
 * that the volume owns, then odo_volume_icp_align_dev against them with model_pose = init_pose = prev_pose. It does not integrate.
 * Refused when rows or cols exceed the ray-cast's 4096. */
int odo_volume_track_dev(odo_volume* v, const odo_icp_params* p, const uint16_t* raw_dev, const float prev_pose_colmajor[16],
                         float abs_pose_colmajor[16], odo_icp_result* result);

/* ---- Frame-to-model tracking with a photometric term: the model's colour frame observes what its geometry cannot ------------------
 * Beside each geometric row above, a row that compares the sensor's grey value with the grey of the ray-cast's colour frame at the
 * pixel's projection, in the same normal equations (DESIGN.md section 9.10 holds the same table). Inputs beyond those above: grey,
 * rows x cols float32, the sensor's grey frame (what the RGB-D path tracks on); rgba_m, rows x cols uint8[4], the ray-cast's colour
 * frame from P_m; weight (lambda > 0, metres per grey level) and huber_delta (grey levels, >= 0). fp32, one rounding per operation.
 * Per sensor pixel (x, y) on the stride:
 *   1. Steps 1 .. 3 above unchanged (r, D, p, pm, pm_z > 0), then u, v as in step 4. A pixel skipped here has neither row.
 *   2. x0 = floorf(u), y0 = floorf(v); skipped unless x0 >= 0 && x0 < cols - 1 && y0 >= 0 && y0 < rows - 1, compared as floats.
 *   3. xi = floorf(u + 0.5f), yi = floorf(v + 0.5f) (in range by 2); zm = depth_m[yi cols + xi]; skipped unless zm > 0 and
 *      fabsf(pm_z - zm) <= dist_max (equality keeps the pair): the nearest model pixel is the occlusion gate.
 *   4. The four words of rgba_m at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1): g00, g01, g10, g11. Skipped unless all
 *      four have A != 0. g = (float)((R 4899 + G 9617 + B 1868 + 8192) >> 14) in integers, the front end's rule.
 *   5. ax = u - x0, ay = v - y0; dt = g01 - g00, db = g11 - g10; top = g00 + ax dt, bot = g10 + ax db;
 *      val = top + ay (bot - top); gx = dt + ay (db - dt); gy = bot - top.
 *   6. res = lambda (val - grey[y cols + x]); a = (lambda f) / pm_z; jx = a gx, jy = a gy, jz = -((jx pm_x + jy pm_y) / pm_z);
 *      J = (jx, jy, jz, pm_y jz - pm_z jy, pm_z jx - pm_x jz, pm_x jy - pm_y jx);
 *      w = (|res| <= lambda huber_delta ? 1 : lambda huber_delta / |res|) if huber_delta > 0, else 1. A flat patch (gx = gy = 0)
 *      is still a pair: it adds cost and count only.
 * The geometric row of the pixel is the one above, unchanged; a pixel can have both rows, either, or none.
 * Sums: 31 doubles. 0 .. 27 are the 28 sums above over geometric and photometric rows together (exact fp64 products), 28 the
 * geometric pairs, 29 the photometric pairs, 30 the photometric rows' share of sum 27. The step, min_pairs (geometric pairs: texture
 * without a model surface is not an alignment), the eigenvalues and min_eig_ratio are those above on the first 29. The order of the
 * sums is fixed (volume_icp_photo.hip.h), no atomics: two calls on the same inputs give the same bits. */
typedef struct {
  float weight;                /* lambda, metres per grey level: finite > 0 */
  float huber_delta;           /* grey levels, finite >= 0; 0: no robust weight on the photometric rows */
} odo_icp_photo_params;
typedef struct {
  odo_icp_result icp;          /* as above; pairs counts geometric pairs, cost both kinds of row */
  double photo_pairs, photo_cost;   /* of the last evaluation: the photometric pairs and their share of cost */
} odo_icp_photo_result;
typedef struct {               /* one step of an alignment */
  int level, iteration;
  double acc[31];
  float delta[6];
  float C[16];
} odo_icp_photo_trace_row;
/* One evaluation at C for one stride: acc receives the 31 sums; rows_dev (device, 16-byte aligned, may be NULL) receives float[16]
 * per pixel of the frame, {J_0 .. J_5, res, w} of the geometric row and then of the photometric row, zeros for a missing row and for
 * pixels off the stride. grey_dev and rgba_m_dev are 4-byte aligned. Validated, ordered and legal as odo_volume_icp_eval_dev. */
int odo_volume_icp_photo_eval_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const uint8_t* rgba_m_dev,
                                  const float model_pose_colmajor[16], const uint16_t* raw_dev, const float* grey_dev,
                                  const float C_colmajor[16], int stride, float dist_max, float huber_delta,
                                  const odo_icp_photo_params* photo, double acc[31], float* rows_dev);
/* Event timing of the two kernels of this path, as odo_volume_icp_time_dev. */
int odo_volume_icp_photo_time_dev(odo_volume* v, const float* depth_m_dev, const float* nrmw_m_dev, const uint8_t* rgba_m_dev,
                                  const float model_pose_colmajor[16], const uint16_t* raw_dev, const float* grey_dev,
                                  const float C_colmajor[16], int stride, float dist_max, float huber_delta,
                                  const odo_icp_photo_params* photo, int reps, float us[2]);
/* The alignment, as odo_volume_icp_align_dev with the photometric rows: launches, single wait, status, NaNs and validation alike. */
int odo_volume_icp_photo_align_dev(odo_volume* v, const odo_icp_params* p, const odo_icp_photo_params* photo, const float* depth_m_dev,
                                   const float* nrmw_m_dev, const uint8_t* rgba_m_dev, const float model_pose_colmajor[16],
                                   const uint16_t* raw_dev, const float* grey_dev, const float init_pose_colmajor[16],
                                   float abs_pose_colmajor[16], odo_icp_photo_result* result, odo_icp_photo_trace_row* trace,
                                   int trace_capacity, int* trace_n);
/* Frame-to-model tracking of one depth and grey frame: odo_volume_track_dev's ray-cast with the colour frame as well, into frames that
 * the volume owns, then odo_volume_icp_photo_align_dev with model_pose = init_pose = prev_pose. Refused on a volume without a colour
 * grid. It does not integrate. */
int odo_volume_track_photo_dev(odo_volume* v, const odo_icp_params* p, const odo_icp_photo_params* photo, const uint16_t* raw_dev,
                               const float* grey_dev, const float prev_pose_colmajor[16], float abs_pose_colmajor[16],
                               odo_icp_photo_result* result);

/* ---- The moving volume: the grid follows the camera, and what leaves it is kept ------------------------------------------------------
 * Optional. A volume that is never shifted behaves and writes exactly as above, and allocates nothing more.
 * Window. The volume remembers origin0, the origin given to odo_volume_create, and off, the cumulative shift in whole voxels (0 at
 * create). After every shift origin_c = origin0_c + (float)off_c * voxel_size: one fp32 product and one fp32 sum, each rounded once,
 * never accumulated shift by shift, so a shift by d followed by -d restores the origin bit for bit. |off_c| <= 2^24. Every operation
 * above (integration, extraction, mesh, colour, ray-cast, alignment) reads the grid and its origin when it is called and so works in
 * the moved window unchanged. odo_volume_clear empties the grids and the spill store; the window stays where it is.
 * Shift by d = (dx, dy, dz) voxels: the origin moves by +d. New voxel (i, j, k) = old voxel (i + dx, j + dy, k + dz) if that lies in
 * the old grid, else 0 (q = 0, w = 0: never observed); the colour grid likewise. |d_c| >= n_c on any axis leaves an empty grid. One
 * launch writes both grids into a second pair of buffers (+4 B per voxel, +8 B with colour: 25 / 49 MB more for 240 x 128 x 200), and
 * the host swaps the buffers when it enqueues; no atomics. The second buffers are allocated once, with hipMalloc, by whichever comes
 * first of odo_volume_set_follow and the first shift (the colour grid's by the first of either after odo_volume_enable_colour), and
 * kept until destroy: set the follow parameters before attaching and no frame call of the tracker allocates. The frame and update
 * counters do not change.
 * Spill store. Old voxel v leaves under d iff v_c - d_c lies outside [0, n_c) on some axis c. With a store, a shift first appends
 * every point of odo_volume_extract (odo_volume_extract_colour on a volume with colour) on the PRE-shift grid whose edge a -> b has
 * a or b leaving: position, normal from the whole pre-shift neighbourhood, weight and colour bit for bit the extraction's, in (voxel
 * a in raster order, axis) order, behind the points of earlier shifts. An edge with both ends staying survives in the grid, and an
 * entering voxel has w = 0 and carries none: as sets of edges, extraction before = spill + extraction after. (Positions and weights of
 * the surviving points are unchanged; their normals may change where a neighbour left.) Points beyond the store's capacity are
 * counted and dropped. Four launches in front of the shift's (the whole grid is walked, which keeps the order), no host wait. */
/* Spill (if the volume has a store) and shift, enqueued on the volume's own stream behind everything pending; returns at once.
 * d = (0, 0, 0): nothing enqueued, 0. -1 and nothing enqueued when |off_c + d_c| would exceed 2^24. */
int odo_volume_shift(odo_volume* v, const int d[3]);
/* The window now: the cumulative shift and the origin (either may be NULL). No wait. */
int odo_volume_window(odo_volume* v, int off[3], float origin[3]);
/* Allocates the store: capacity (1 .. 2^28) points of float4 xyz0, float4 nrmw and, when the volume has colour (enable it first),
 * uint8[4] rgba: 32 or 36 B per point. Once, and not while attached to a tracker. */
int odo_volume_enable_spill(odo_volume* v, long capacity);
/* The store's points (waits for everything pending): the first min(points in the store, capacity) into xyz0 / nrmw and, unless NULL,
 * rgba (refused on a volume without colour); *n_points = points copied, *n_dropped (may be NULL) = points that qualified since the
 * store was last emptied and did not fit it. clear != 0 empties the store afterwards, whatever was copied. Legal while attached. */
int odo_volume_spill_points(odo_volume* v, long capacity, float* xyz0, float* nrmw, uint8_t* rgba, long* n_points, long* n_dropped,
                            int clear);
/* Event timing (diagnostic, tools/volume_cost.py shift; waits; refused while attached): batches of reps (1 .. 10000) launches between
 * events on the volume's own stream, the mean time of one in microseconds. us[0]: the shift by d into the second buffers, which are
 * not swapped in, so the grids, the window and the store's counted points stay as they are; us[1]: device-to-device hipMemcpyAsync
 * of the same bytes; us[2]: hipMemsetAsync of the same bytes; us[3], us[4], us[5]: the spill's count, scan and scatter for d (0
 * without a store). */
int odo_volume_shift_time(odo_volume* v, const int d[3], int reps, float us[6]);
/* TEST ONLY, for the project's own suite; not part of the interface an integrator uses and free to change. The store's buffers are
 * allocated with a guard of 64 points behind the capacity and filled with 0xAB once; a spill writes the points it appends and nothing
 * else. *n_changed = bytes behind the store's last point, guard included, that no longer hold 0xAB (waits): 0 until the store is
 * first emptied, unless a spill wrote where it must not. */
int odo_debug_volume_spill_guard(odo_volume* v, long* n_changed);
/* Mesh store: the leaving slab as triangles, so that the store and the window's mesh together are a mesh of
 * the whole drive. The staying voxels form a box [lo_c, hi_c] on every axis (empty when |d_c| >= n_c on one). The cell with low
 * corner c, all eight corners inside the grid, is spilled iff at least one corner leaves: on some axis c < lo or c + 1 > hi. An edge
 * (a, e), b = a + d_e, e one of odo_volume_mesh's seven directions, is spilled iff it is an edge of at least one spilled cell of the
 * grid, whatever the data: per axis the candidate low corners are {a} where d_e has a 1, else {a - 1, a} within [0, n - 2], and the
 * edge is spilled iff some axis has a candidate with c < lo or c + 1 > hi. With a mesh store a shift first appends, from the PRE-shift
 * grid, every vertex of odo_volume_mesh whose edge is spilled and every triangle of odo_volume_mesh whose cell is spilled: positions,
 * normals, weights and colours bit for bit the mesh's, vertices in (voxel in raster order, e) order, triangles in (cell, tetrahedron,
 * triangle) order with the mesh's winding and smallest-index-first rotation. A triangle's three indices are the STORE's: vertices
 * already in the store + rank of the vertex among this spill's. As multisets of triangles, mesh before = spill + mesh after; the
 * vertices of the seam between them are in both, and they are not welded: later integrations move the window's copy, so the seam
 * can open by the TSDF's later updates.
 * A spill is appended whole or not at all: if its vertices or its triangles do not fit what is left of either capacity, nothing of it
 * is written and both of its counts go to the dropped totals; later, smaller spills are still appended. The store is therefore a
 * complete mesh of every spill it holds at any time. (odo_volume_mesh differs: it never remaps indices, and with a vertex capacity
 * below the total its triangles name vertices that were not written.)
 * Five launches in front of the shift's (six with colour), no atomics, no host wait; only the slab is walked: a thread whose voxel is
 * more than one voxel from every leaving voxel loads nothing. The mesh's scratch (5 B per voxel) is shared with odo_volume_mesh. */
/* Allocates the mesh store: float4 xyz0 and nrmw (and uint8[4] rgba when the volume has colour: enable it first) per vertex, three
 * int32 per triangle; each capacity 1 .. 2^28. Also allocates the mesh's scratch if no mesh was asked for yet, so that no shift
 * allocates. Once, and not while attached to a tracker. Independent of odo_volume_enable_spill: a volume may have either or both. */
int odo_volume_enable_spill_mesh(odo_volume* v, long vertex_capacity, long triangle_capacity);
/* The store's mesh (waits for everything pending). *n_vertices, *n_triangles and dropped[2] (may be NULL: vertices, triangles that
 * qualified since the store was last emptied and were not written) are set first, in every case below. Both capacities 0: nothing
 * else. Otherwise the whole store is copied, or the call is refused: -1 and nothing copied or cleared when either capacity is below
 * the store's count, because a cut would leave triangles without their vertices. rgba may be NULL (non-NULL is refused on a store
 * without colours). clear != 0 empties the store afterwards. Legal while attached. */
int odo_volume_spill_mesh(odo_volume* v, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw, uint8_t* rgba,
                          int32_t* tri, long* n_vertices, long* n_triangles, long dropped[2], int clear);
/* Event timing (diagnostic, tools/volume_cost.py shift --mesh; waits; refused while attached or without a mesh store): as
 * odo_volume_shift_time, us[0 .. 4] = the mesh spill's count, scan, vertices, triangles and colour (0 without colour) for d. The
 * counters do not move, so the store's contents and counts read the same afterwards. */
int odo_volume_spill_mesh_time(odo_volume* v, const int d[3], int reps, float us[5]);
/* TEST ONLY, as odo_debug_volume_spill_guard: 64 guard items behind each of the mesh store's buffers, 0xAB fill; *n_changed = bytes
 * behind the store's last vertex and last triangle, guards included, that no longer hold 0xAB (waits). */
int odo_debug_volume_spill_mesh_guard(odo_volume* v, long* n_changed);
/* Re-entry store: the leaving VOXELS, put back when the window returns to them. A voxel's global index is
 * g_c = off_c + i_c (off the window's cumulative shift, i its index in the window): the same physical voxel has the same g whenever
 * it is in the window. The store is an ordered list of entries (g[3], voxel word, colour word). With a store, a shift by d != 0 that
 * odo_volume_shift accepts does three things, in this order:
 *   restore  every entry whose g - off_new lies in [0, n) on all three axes is removed from the store and its voxel word (and its colour
 *            word, when the store has colours) written to that voxel of the shifted grid. Entering voxels are 0 there, so this
 *            overwrites zeros only;
 *   keep     the other entries stay, in their order;
 *   save     every voxel of the PRE-shift grid that leaves under d (above) and has a non-zero bit in its voxel word, or in its colour
 *            word on a volume with colour, is appended behind them in raster order (i fastest, then j, then k).
 * Entries beyond the capacity are counted and dropped: the kept entries always fit, so only the tail of the newly saved ones is cut.
 * Between shifts every stored g lies outside the window and no g occurs twice. With enough capacity a shift by d followed by -d, or
 * any closed walk of shifts, restores grid, colour grid and window bit for bit and leaves the store empty. Integers only, no atomics,
 * no host wait; eight launches round the shift's. odo_volume_clear empties the store. The point and mesh stores stay logs of the
 * surfaces that left: geometry that leaves, returns and leaves again appears in them twice. */
/* Allocates the store: capacity (1 .. 2^28) entries in two sets of buffers, 16 B per entry and set (20 B when the volume has colour:
 * enable it first; a store without colours gives its voxels back with colour word 0), and the scratch of its passes, so that no shift
 * allocates. Once, and not while attached to a tracker. */
int odo_volume_enable_reentry(odo_volume* v, long capacity);
/* The store's live entries in store order (waits for everything pending). *n = the live count, in every case below. capacity 0:
 * nothing else. Otherwise -1 and nothing copied or cleared when capacity is below the live count; else g (three int32 per entry), vox
 * and, unless NULL, col (refused on a store without colours) receive them. clear != 0 empties the store and zeroes its counters
 * afterwards. Legal while attached. */
int odo_volume_reentry_voxels(odo_volume* v, long capacity, int32_t (*g)[3], uint32_t* vox, uint32_t* col, long* n, int clear);
/* stats[4] = entries in the store, and since enable / clear: entries appended, entries put back into the grid, leaving voxels that
 * found the store full (waits). live = saved - restored. */
int odo_volume_reentry_stats(odo_volume* v, long stats[4]);
/* Event timing (diagnostic, tools/volume_cost.py shift --reentry; waits; refused while attached or without a store): as
 * odo_volume_shift_time, us[0 .. 4] = save count, save scan, save scatter, the store pass (count, scan and compaction: three launches)
 * and the advance for a shift by d that is not applied. The passes write the grids' and the store's second buffers and a copy of the
 * counters, none of which is swapped in: the volume and the store read the same afterwards. */
int odo_volume_reentry_time(odo_volume* v, const int d[3], int reps, float us[5]);
/* TEST ONLY, as odo_debug_volume_spill_guard: 64 guard entries behind each buffer of both sets, 0xAB fill. *n_changed = bytes of the
 * live set behind its last live entry, guard included, that no longer hold 0xAB (0 while the live count has never gone down);
 * *n_guard = bytes of the guards of both sets that no longer hold it (always 0). Waits. */
int odo_debug_volume_reentry_guard(odo_volume* v, long* n_changed, long* n_guard);
/* Following a camera. The host works in fp64 from the fp32 entries of the camera-to-world pose [R | t]: p = t + focus * R[:, 2] (the
 * point `focus` metres along the optical axis); e_c = (p_c - (origin_c + 0.5 * n_c * vs)) / vs, its distance from the window's centre
 * in voxels; if max |e_c| < threshold then d = 0, else d_c = nearbyint(e_c) (ties to even) clamped to +-n_c. */
typedef struct {
  float focus;             /* metres along the optical axis, finite >= 0 */
  int threshold;           /* voxels, >= 1 */
} odo_volume_follow_params;
/* Sets the parameters; NULL turns following off. Validated before the volume is touched. Non-NULL also allocates the grids' second
 * buffers if they are missing (-1 when that fails), so that the follow steps of an attached tracker do not. */
int odo_volume_set_follow(odo_volume* v, const odo_volume_follow_params* p);
/* The rule above for abs_pose, then odo_volume_shift(d); d_out (may be NULL) receives d. -1 and nothing enqueued for a pose with a
 * non-finite entry or a volume without follow parameters. With parameters set, an attached tracker (odo_tracker_attach_volume) takes
 * this step with every frame's abs_pose in front of that frame's integration, on the volume's own stream, without a host wait; the
 * tracker's poses, masks and keyframe decisions stay bit-identical to those without a volume. */
int odo_volume_follow(odo_volume* v, const float abs_pose_colmajor[16], int d_out[3]);

/* ---- RGB-D front end: raw sensor frames -> the RGB-D tracker's inputs ----------------------------------------------------------
 * A sensor delivers interleaved 8-bit colour and a uint16 depth frame in the DEPTH imager's pixel grid (its own intrinsics, often
 * its own resolution, centimetres beside the colour imager); odo_tracker_*_rgbd take an fp32 grey image and a uint16 depth frame in
 * the GREY camera's grid. The front end makes the second from the first on the device, three launches per frame on a stream of
 * its own, into a ring of output slots, so that frame k + 1 is prepared while the tracker works on frame k.
 * All floating point is fp32, one rounding per operation.
 * Grey. Colour frame rows x cols, 3 or 4 interleaved uint8 channels in the order RGB(A) or BGR(A), dense rows:
 *   grey = (float)((R * 4899 + G * 9617 + B * 1868 + 8192) >> 14) in integer arithmetic (the 8-bit BT.601 fixed-point rule; the
 *   weights sum to 16384, so R = G = B = v gives v). A fourth channel is ignored.
 * Registration. Depth frame depth_rows x depth_cols, 0 = no reading, depth_scale_in raw units per metre, pinhole (depth_fx,
 * depth_fy, depth_cx, depth_cy); target: rows x cols, K, depth_scale_out raw units per metre; colour_from_depth E = [R | t]
 * (metres): P_c = R P_d + t. For every depth pixel (x, y) with r = raw[y][x] != 0:
 *   1. z = (float)r / depth_scale_in;
 *   2. for s in {-0.5, 0, +0.5}: X = (((float)x + s) - depth_cx) / depth_fx * z, Y = (((float)y + s) - depth_cy) / depth_fy * z
 *      (left to right), then row i of the transform as ((R[i][0] X + R[i][1] Y) + R[i][2] z) + t[i]: the two footprint corners
 *      (X0, Y0, Z0) (s = -0.5), (X1, Y1, Z1) (s = +0.5) and the centre depth Zm (s = 0);
 *   3. dropped (dropped_behind) unless Z0 > 0 && Z1 > 0 && Zm > 0;
 *   4. q = rintf(Zm * depth_scale_out); dropped (dropped_range) unless 1 <= q <= 65535;
 *   5. u0 = f0 * (X0 / Z0) + cx0, u1 = f0 * (X1 / Z1) + cx0, likewise v0, v1 with Y and cy0; dropped (dropped_range) if any is
 *      not finite. Columns ceil(min(u0, u1)) .. ceil(max(u0, u1)) - 1 and rows likewise: the target pixels whose centres lie in
 *      the half-open footprint. A range wider or taller than 4 drops the pixel (dropped_splat); an empty range writes nothing and
 *      is not a drop; the part of the range inside the image receives q;
 *   6. a target pixel's value is the minimum q it received, 0 if it received none.
 * With E = identity, equal intrinsics and equal scales the output equals the input bit for bit, and the result does not depend on
 * the order of the writes. Lens distortion of either imager and colour cameras with fx != fy are outside this model. */
typedef struct {
  int depth_rows, depth_cols;
  float depth_fx, depth_fy, depth_cx, depth_cy;
  float depth_scale_in;
  int rows, cols;              /* the tracker's frame */
  odo_intrinsics K;
  float depth_scale_out;
  float colour_from_depth[12]; /* row-major 3 x 4, metres */
  int colour_channels;         /* 3 | 4 */
  int colour_bgr;              /* 0: RGB(A), 1: BGR(A) */
  int slots;                   /* output ring, 2 ... 8 */
} odo_rgbd_frontend_params;
/* Validates everything (sizes > 0, finite positive focal lengths and scales, finite principal points and extrinsic, channels 3 | 4,
 * slots 2 .. 8) before it touches the device. Device memory: 6 B per target pixel and slot + 4 B per target pixel (+ one raw frame per slot once submit_host is used). Uploads of
 * odo_rgbd_frontend_submit_host run on ctx's stream; ctx must outlive the front end. One host thread at a time per front end. */
int odo_rgbd_frontend_create(odo_ctx* ctx, const odo_rgbd_frontend_params* p, odo_rgbd_frontend** out);
/* Enqueues one frame on the front end's stream and returns at once. *gray_out / *depth_out: the ring slot the results go to (rows x
 * cols fp32 / uint16, dense). colour_dev (4-byte aligned) and depth_dev must be complete when the call is made and stay unchanged
 * until the slot is complete. A slot is reused `slots` submits later: the caller must not have a slot's buffers announced to, or
 * in use by, a tracker when the slot comes round again (the "unchanged until consumed" rule of odo_tracker_hint_next_pair).
 * Refuses (-1, nothing enqueued) while `slots` frames are outstanding that the caller never waited for; waiting for a frame
 * accounts for every earlier frame as well. */
int odo_rgbd_frontend_submit_dev(odo_rgbd_frontend* f, const uint8_t* colour_dev, const uint16_t* depth_dev, const float** gray_out,
                                 const uint16_t** depth_out);
/* The same from host memory (row pitches in bytes): uploads through the context's pinned staging path (the caller's buffers may
 * be reused on return unless they are odo_host_alloc blocks: then after the upload's ticket), then the kernels. */
int odo_rgbd_frontend_submit_host(odo_rgbd_frontend* f, const uint8_t* colour, size_t colour_pitch, const uint16_t* depth,
                                  size_t depth_pitch, const float** gray_out, const uint16_t** depth_out);
/* Host wait until the slot with that grey buffer is complete; its two buffers may then be handed to odo_tracker_init_rgbd /
 * _track_rgbd / _hint_next_rgbd. -1 if no frame was ever submitted to that slot. */
int odo_rgbd_frontend_wait(odo_rgbd_frontend* f, const float* gray_out);
/* The device colour frame the slot with that grey buffer was made from: after odo_rgbd_frontend_submit_dev the caller's pointer,
 * after odo_rgbd_frontend_submit_host the slot's own raw copy. Valid (complete and unchanged) from the slot's completion until the
 * slot comes round again; with it a tracker fed by the front end colours its volume (odo_tracker_frame_colour) without a second
 * upload. Does not wait. -1 for a slot that never received a submit. */
int odo_rgbd_frontend_colour(odo_rgbd_frontend* f, const float* gray_out, const uint8_t** colour_dev);
/* out: n_depth (depth pixels with r != 0), n_filled (target pixels with a value), dropped_behind, dropped_range, dropped_splat,
 * frame number (0-based count of submits). Waits for the slot. */
int odo_rgbd_frontend_stats(odo_rgbd_frontend* f, const float* gray_out, long out[6]);
/* Frames in flight are completed first. */
int odo_rgbd_frontend_destroy(odo_rgbd_frontend* f);

/* ---- Bilateral depth filter: an edge-preserving denoiser for uint16 sensor depth, exact to the last bit ------------------------
 * Integers only, no floating point and no exp on the device: the weights are small tables that the caller passes in (Python:
 * api.depth_filter_tables makes Gaussian ones that follow a sensor's noise model), and the sums do not depend on their order.
 * Frame rows x cols uint16, dense rows, 0 = no reading; radius R in 1 .. 4, the window is (2R + 1)^2;
 *   ws[(2R + 1)^2]  spatial weights, row-major, each 0 .. 16, the centre's >= 1 (the rest of ws[81] is ignored);
 *   wr[256]         range weights 0 .. 255, wr[0] >= 1;
 *   shift[256]      0 .. 4, indexed by the centre's high byte.
 * Per pixel with centre c = raw[y][x]: c == 0 gives 0 (nothing is filled in). Otherwise s = shift[c >> 8], and every tap t of the
 * window that lies inside the frame and has t != 0 gives delta = (int)t - (int)c, k = |delta| >> s; the tap counts iff k < 256, with
 * weight w = ws[tap] * wr[k]. S = sum of w * delta and W = sum of w over the counted taps, both int32 (|S| <= 4080 * 4095 * 80 =
 * 1 336 608 000; W >= ws[centre] * wr[0] >= 1). With C's truncating division q = S >= 0 ? (S + W / 2) / W : -((-S + W / 2) / W), and
 * out = c + q. It follows that out == 0 exactly where raw == 0; that out lies between the smallest and the largest counted tap; that
 * a tap further than 256 << s raw units from the centre contributes nothing (a depth edge is never averaged across); and that ws
 * with only its centre non-zero gives out == raw. shift lets the range kernel widen with the sensor's noise, which grows with z^2. */
typedef struct odo_depth_filter odo_depth_filter;
typedef struct {
  int rows, cols, radius;
  uint8_t ws[81], wr[256], shift[256];
} odo_depth_filter_params;
/* Validates every bound above (and rows, cols in 1 .. 8192) before it touches the device: -1 with a message and *out untouched on
 * any violation. Device memory: 512 B + 16 B per tile of 64 x 16 pixels. ctx must outlive the filter. One host thread at a time. */
int odo_depth_filter_create(odo_ctx* ctx, const odo_depth_filter_params* p, odo_depth_filter** out);
/* One launch on ctx's stream, returns at once: out_dev = the filter of in_dev (both rows x cols uint16 on the device, dense; 8-byte
 * alignment and cols % 4 == 0 take the wide loads and stores). -1 and nothing enqueued for a NULL, for in_dev == out_dev and for any
 * other overlap of the two frames. Ordered behind it without a host wait: whatever is enqueued on ctx's stream afterwards
 * (odo_dev_download, odo_ctx_synchronize, and of a volume created on ctx the calls that read a depth frame: odo_volume_integrate_dev /
 * _colour_dev run on ctx's stream, odo_volume_icp_*_dev and odo_volume_track*_dev order the volume's stream behind it). NOT ordered behind it:
 * a tracker, which reads its depth frame on a stream of its own (odo_ctx_synchronize(ctx) before odo_tracker_init_rgbd / _track_rgbd /
 * _hint_next_rgbd receive out_dev), and an RGB-D front end's submit_dev, which runs on the front end's stream. */
int odo_depth_filter_run_dev(odo_depth_filter* f, const uint16_t* in_dev, uint16_t* out_dev);
/* Of the last run, exact: n_valid (pixels with a reading), n_changed (out != raw), sum_abs_change (sum of |out - raw|). Waits for
 * ctx's stream. Zeros before the first run. */
int odo_depth_filter_stats(odo_depth_filter* f, long out[3]);
/* Diagnostic, like odo_volume_raycast_time: one launch to warm, `reps` (1 .. 10000) between two events on ctx's stream; *us = the mean
 * time of one launch in microseconds. Waits. out_dev and the statistics are those of one run afterwards. */
int odo_depth_filter_time_dev(odo_depth_filter* f, const uint16_t* in_dev, uint16_t* out_dev, int reps, float* us);
/* Safe with a run in flight: waits for ctx's stream first. */
int odo_depth_filter_destroy(odo_depth_filter* f);

/* ---- Dense stereo depth: census matching from a rectified pair to a uint16 depth frame, exact to the last bit -------------------
 * L, R: fp32 frames rows x cols, dense, rectified: a point at left column x with disparity d >= 0 lies at right column x - d.
 * Integers dmin >= 1, dmin + 2 <= dmax <= 255, agg_radius A in 0 .. 3, uniqueness in 0 .. 99 (percent), lr_max >= 0 or -1 (no
 * left-right check), max_raw in 1 .. 65535; k = (float)(16.0 * fx * baseline * depth_scale), computed in double, rounded once.
 *   Census   9 wide x 7 high, 62 bits: neighbour < centre as fp32 (a NaN on either side: 0), where 4 <= x < cols - 4, 3 <= y < rows - 3.
 *   Cost     h(x, y, d) = popcount(cL(x, y) ^ cR(x - d, y)); C(x, y, d) = sum of h(x + i, y + j, d) over |i|, |j| <= A (<= 3038).
 *   Interior A + 4 <= x < cols - A - 4 and A + 3 <= y < rows - A - 3; d is admissible iff dmin <= d <= dmax and x - d >= A + 4. A pixel
 *            without an admissible d is not interior: it gets 0 and is counted nowhere.
 *   Winner   dl = the smallest admissible d of minimal cost c0.
 *   Unique   c2 = the minimal cost over admissible d with |d - dl| > 1; rejected if there is none or unless c2 (100 - uniqueness) >
 *            100 c0 (so a flat patch is always rejected).
 *   L-R      CR(x', y, d) = C(x' + d, y, d) over the d for which left pixel x' + d is interior and d admissible there; dr = the
 *            smallest such d of minimal cost; rejected unless |dr(x - dl, y) - dl| <= lr_max.
 *   Sub-pixel, in sixteenths: cm = C(dl - 1), cp = C(dl + 1); f = 0 if dl is dmin or dmax, a neighbour is not admissible, or den =
 *            cm - 2 c0 + cp <= 0; else with num = cm - cp, f = sgn(num) ((16 |num| + den) / (2 den)) (truncating), -8 .. 8.
 *            q = 16 dl + f.
 *   Depth    raw = rintf(k / (float)q), one correctly rounded fp32 division, half to even; raw > max_raw is a range reject (0).
 * Outputs: the depth frame, a uint16 frame of q (0: none), and exact counters; the first reason of a rejection counts only. */
typedef struct odo_stereo_depth odo_stereo_depth;
typedef struct {
  int rows, cols, dmin, dmax, agg_radius, uniqueness, lr_max, max_raw;
  double fx, baseline, depth_scale;
} odo_stereo_depth_params;
/* Validates every bound above (and rows, cols in 1 .. 8192) before it touches the device: -1 with a message and *out untouched on
 * any violation. A frame too small to have an interior pixel is valid and gives all zeros. Device memory, allocated once: 21 B per
 * pixel (two census planes, dr, the q frame, an internal depth frame) + 32 B per tile of 64 x 4 pixels. ctx must outlive the matcher.
 * One host thread at a time. */
int odo_stereo_depth_create(odo_ctx* ctx, const odo_stereo_depth_params* p, odo_stereo_depth** out);
/* Three launches on ctx's stream, returns at once: out_depth_dev = the depth of the pair (rows x cols uint16 on the device, dense;
 * NULL: the matcher's internal frame, odo_stereo_depth_depth_dev; 8-byte alignment and cols % 4 == 0 take the wide stores). -1 and
 * nothing enqueued for a NULL input, a misaligned pointer and an output that overlaps an input. Ordered behind it without a host wait:
 * whatever is enqueued on ctx's stream afterwards (odo_dev_download, odo_ctx_synchronize, and of a volume created on ctx the calls
 * that read a depth frame: odo_volume_integrate_dev / _colour_dev run on ctx's stream, odo_volume_icp_*_dev and odo_volume_track*_dev
 * order the volume's stream behind it). NOT ordered behind it: a tracker, which reads its depth frame on a stream of its own
 * (odo_ctx_synchronize(ctx) before odo_tracker_init_rgbd / _track_rgbd / _hint_next_rgbd receive the frame), and an RGB-D front
 * end's submit_dev, which runs on the front end's stream. */
int odo_stereo_depth_run_dev(odo_stereo_depth* s, const float* left_dev, const float* right_dev, uint16_t* out_depth_dev);
/* The q frame of the last run (rows x cols uint16 on the device, the matcher's own; zeros before the first run). Does not wait. */
int odo_stereo_depth_disparity_dev(odo_stereo_depth* s, const uint16_t** q_dev);
/* The internal depth frame (what a run with out_depth_dev == NULL writes). Does not wait. */
int odo_stereo_depth_depth_dev(odo_stereo_depth* s, const uint16_t** depth_dev);
/* Of the last run, exact: interior, matched, rejected by uniqueness, by left-right, by range, the sum of q over the matched pixels as
 * its low and its high 32-bit word, and a spare 0. Waits for ctx's stream. Zeros before the first run. */
int odo_stereo_depth_stats(odo_stereo_depth* s, long out[8]);
/* Diagnostic, like odo_depth_filter_time_dev: one run to warm, then for each of the three kernels `reps` (1 .. 10000) launches between
 * two events on ctx's stream; us[0 .. 2] = the mean time of one census / right-match / left-match launch in microseconds. Waits. The
 * outputs and the statistics are those of one run afterwards. */
int odo_stereo_depth_time_dev(odo_stereo_depth* s, const float* left_dev, const float* right_dev, uint16_t* out_depth_dev, int reps,
                              float us[3]);
/* Safe with a run in flight: waits for ctx's stream first. */
int odo_stereo_depth_destroy(odo_stereo_depth* s);

/* ---- Speckle filter: small connected components of a uint16 key frame are removed, exact to the last bit ----------------------
 * K: a key frame rows x cols uint16, dense, 0 = no value (the matcher's q frame, or a depth frame). Integers max_diff in 0 .. 65535
 * and min_size in 1 .. 2^30; rows, cols in 1 .. 8192, so a linear pixel index y cols + x fits int32.
 *   Connection  two pixels are connected iff they are 4-neighbours, both keys are non-zero, and |K_a - K_b| <= max_diff.
 *   Component   a class of the transitive closure of that relation. Connection itself is not transitive: a ramp whose neighbours
 *               each differ by exactly max_diff is one component. A non-zero pixel without a connected neighbour is a component of
 *               size 1. A pixel with key 0 belongs to none.
 *   Survival    a non-zero pixel survives iff its component has at least min_size pixels.
 *   Output      every non-surviving pixel is set to 0 in each of up to two uint16 target frames of K's size, in place; K itself may
 *               be one of them. Every other byte of the targets stays as it was. min_size == 1 removes nothing.
 *   Counters    all exact: pixels (non-zero keys), components, removed_components, removed_pixels, largest (the largest component's
 *               size), guard (0; see below).
 * The result does not depend on any order of evaluation and nothing in it is floating point. The kernels are a union-find: integer
 * atomicMin puts the larger root under the smaller, so a component's root is its smallest linear index whatever order the unions
 * happen in, and sizes are integer sums. Every device loop whose trip count depends on data strictly decreases an index and also
 * carries a hard trip bound; a loop that runs into the bound sets a bit of `guard` and leaves. */
typedef struct odo_speckle odo_speckle;
typedef struct {
  int rows, cols, max_diff, min_size;
} odo_speckle_params;
/* Validates every bound above before it touches the device: -1 with the bound named in the message and *out untouched on any
 * violation. Device memory, allocated once: 8 B per pixel (the parent and size planes) + 32 B per tile of 64 x 16 pixels. ctx must
 * outlive the filter. One host thread at a time. */
int odo_speckle_create(odo_ctx* ctx, const odo_speckle_params* p, odo_speckle** out);
/* Four launches on ctx's stream, returns at once, no host wait: the components of key_dev, the non-surviving pixels zeroed in
 * target_a_dev and, unless it is NULL, in target_b_dev (all rows x cols uint16 on the device, dense). A target may be key_dev. -1 and
 * nothing enqueued for a NULL filter, key or target_a, a misaligned pointer and two different targets that overlap. Ordering is
 * odo_depth_filter_run_dev's: what is enqueued on ctx's stream afterwards is ordered behind it; a tracker and an RGB-D front end's
 * submit_dev are not. */
int odo_speckle_run_dev(odo_speckle* s, const uint16_t* key_dev, uint16_t* target_a_dev, uint16_t* target_b_dev);
/* Of the last run, exact: pixels, components, removed_components, removed_pixels, largest, guard, 0, 0. Waits for ctx's stream. Zeros
 * before the first run. */
int odo_speckle_stats(odo_speckle* s, long out[8]);
/* Diagnostic: `reps` (1 .. 10000) launches between two events on ctx's stream for each prefix of the run, on scratch copies of the key
 * and a target; us[0 .. 3] = the mean time of the label / seam / count / apply launch in microseconds (each the difference of two
 * prefixes), us[4] = of the whole run. Waits. The targets and the statistics are those of exactly one run afterwards. */
int odo_speckle_time_dev(odo_speckle* s, const uint16_t* key_dev, uint16_t* target_a_dev, uint16_t* target_b_dev, int reps,
                         float us[5]);
/* Safe with a run in flight: waits for ctx's stream first. */
int odo_speckle_destroy(odo_speckle* s);
/* Every later odo_stereo_depth_run_dev (and _time_dev) enqueues a speckle filter behind the left match, on the same stream: the key is
 * the q frame, the targets are the q frame and the run's depth output, the internal frame or the caller's. The bounds are
 * odo_speckle_create's; min_size == 0 takes the filter off again. odo_stereo_depth_stats keeps returning the match's own counters. A
 * matcher on which this was never called enqueues what it always did. Waits for ctx's stream when it replaces a filter. */
int odo_stereo_depth_enable_speckle(odo_stereo_depth* s, int max_diff, int min_size);
/* odo_speckle_stats of the matcher's filter; -1 while none is enabled. */
int odo_stereo_depth_speckle_stats(odo_stereo_depth* s, long out[8]);

/* ---- Semi-global path aggregation for the dense stereo matcher: an opt-in mode, exact to the last bit ---------------------------
 * Everything of the matcher's rule above stays: census, h, C for the A the matcher was created with, interior, admissibility. In
 * this mode the selection reads an aggregate S in place of C. Integers P1, P2 and paths with
 *   1 <= P1 <= P2;  paths is 4 or 8;  paths (62 (2A + 1)^2 + P2) <= 65534, so that an aggregate fits uint16 and 0xFFFF can mean
 *   "inadmissible";  rows cols D <= 2^30 with D = dmax - dmin + 1.
 *   Active     an interior pixel with at least one admissible candidate: A + 3 <= y < rows - A - 3, A + 4 + dmin <= x < cols - A - 4.
 *              The active pixels form a rectangle; the admissible set of one is dmin .. min(dmax, x - A - 4): contiguous from dmin.
 *   Directions r = (dx, dy): (1, 0), (-1, 0), (0, 1), (0, -1) for 4 paths; these and (1, 1), (-1, -1), (1, -1), (-1, 1) for 8.
 *   Path cost  for an admissible (p, d) let q = p - r. If q is not active, L_r(p, d) = C(p, d): the path starts here. Otherwise with
 *              M = min over q's admissible k of L_r(q, k):  L_r(p, d) = C(p, d) + min(a0, a1, a2, P2),  a0 = L_r(q, d) - M,
 *              a1 = L_r(q, d - 1) - M + P1,  a2 = L_r(q, d + 1) - M + P1,  a term left out if its candidate is not admissible at q.
 *              Hence 0 <= L_r <= C + P2.
 *   Aggregate  S(p, d) = the sum of L_r(p, d) over the directions: integer sums, independent of the order of the paths.
 *   Selection  exactly the rule above with S in place of C: the smallest d of minimal S wins; c2 over |d - dl| > 1; left-right with
 *              SR(x', y, d) = S(x' + d, y, d) and dr the smallest d of minimal cost (255: none); sub-pixel on the S triple, one
 *              division, range reject; the same eight counters.
 * It is not a win everywhere: on an untextured patch the census bits are noise, and no path has a signal to propagate (DESIGN.md
 * section 9.18 has the figures). The default stays the box matcher, bit for bit.
 *
 * odo_stereo_depth_enable_sgm validates before it touches the device: -1 with the bound named in the message, and the matcher as
 * it was, on a bad bound or a failed allocation. Device memory: two uint16 volumes [rows][cols][D], 4 rows cols D bytes, allocated
 * here and freed by paths == 0 (which takes the mode off: a later run gives the box matcher's bytes; waits for ctx's stream) or by
 * destroy. Every later odo_stereo_depth_run_dev enqueues census, cost, one launch per path, right selection and left selection on
 * ctx's stream and returns; an enabled speckle filter follows as before. Its refusals and its ordering are unchanged. Calling it
 * again with other penalties or paths keeps the volumes. */
int odo_stereo_depth_enable_sgm(odo_stereo_depth* s, int p1, int p2, int paths);
/* odo_stereo_depth_time_dev for the semi-global mode: us[0 .. 4] = the mean time in microseconds of the census launch, the cost
 * launch, ALL path launches as one unit (the group is repeated as a whole, because its first launch stores), the right selection
 * and the left selection. reps 1 .. 10000. Waits. The outputs and the statistics are those of one run afterwards. -1 while the mode
 * is off; while it is on, odo_stereo_depth_time_dev returns -1 and names this call. */
int odo_stereo_depth_sgm_time_dev(odo_stereo_depth* s, const float* left_dev, const float* right_dev, uint16_t* out_depth_dev, int reps,
                                  float us[5]);
/* TEST ONLY. Waits for ctx's stream, then copies the last run's S to host_out: rows cols D uint16 in the order [y][x][d - dmin],
 * 0xFFFF where the candidate is not admissible (everywhere before the first run). -1 while the mode is off. */
int odo_debug_sgm_volume(odo_stereo_depth* s, uint16_t* host_out);

/* ---- Mesh welder: coincident vertices merged, degenerate and duplicate triangles removed, exact to the last bit -----------------
 * Input: n_v vertices (xyz0 float4, nrmw float4, optionally rgba uint8[4]) and n_t triangles (int32[3]) on the device, as
 * odo_volume_mesh and odo_volume_spill_mesh give them. A rule: eps > 0 (fp32), origin[3] (fp32, finite), grids in {1, 8},
 * drop_unreferenced in {0, 1}.
 * One pass with grid k (k = 0 .. 7, bit a of k belongs to axis a):
 *   Cell            inv = 1.0f / eps, correctly rounded, once. c_a = floorf((x_a - o_a) * inv + (bit_a ? 0.5f : 0.0f)): three fp32
 *                   operations, each rounded, no contraction. A vertex is keyless if a coordinate or a c_a is not finite or
 *                   |c_a| >= 2^20; a keyless vertex is never merged and is its own representative. Otherwise its key is the three
 *                   cells + 2^20 packed as 21-bit fields into 63 bits.
 *   Representative  rep(i) = the smallest index with the same key.
 *   Triangles       in input order. An index outside [0, n_v): dropped, counted bad_index; no such index is ever dereferenced.
 *                   Otherwise the indices become their representatives; two equal: dropped, counted degenerate. Otherwise the triple
 *                   is rotated so that its smallest index comes first, winding kept; it is dropped and counted duplicate if an
 *                   earlier surviving triangle has the same rotated triple. The opposite winding is a different triangle.
 *   Vertices kept   with drop_unreferenced the representatives a surviving triangle names, without it all representatives; in
 *                   ascending original index, each with its own xyz0, nrmw and rgba bit for bit: nothing is averaged. The
 *                   surviving triangles keep their input order and are written as their rotated triples in the kept vertices' ranks.
 * grids = 1 is pass 0; grids = 8 is passes 0 .. 7 chained, each on the output of the one before. Two vertices closer than eps / 2
 * on every axis share a cell of at least one of the eight grids.
 * Counters (odo_mesh_weld_stats, in this order): vertices_in and triangles_in of the first pass, vertices_out and triangles_out of
 * the last; merged (vertices that took another representative), unreferenced (representatives dropped because no surviving triangle
 * names them; 0 without drop_unreferenced), degenerate, duplicate and bad_index summed over the passes, so that vertices_out =
 * vertices_in - merged - unreferenced and triangles_out = triangles_in - degenerate - duplicate - bad_index; keyless summed over the
 * passes (a vertex keyless in all eight grids counts eight times); guard (0; see below); passes.
 * Nothing depends on timing: keys are integers, the vertex table holds a 64-bit key word claimed with atomicCAS and a smallest-index
 * word lowered with atomicMin, the triangle table holds triangle indices claimed with atomicCAS and lowered with atomicMin, and the
 * compaction is count, scan, scatter. Both tables have 2^ceil(log2(2 capacity)) slots and are probed linearly from a splitmix64
 * hash; every probe loop carries a hard trip bound, the table's size, and a loop that runs into it sets a bit of `guard` and leaves
 * (DESIGN.md section 9.19). No loop waits for another thread. */
typedef struct odo_mesh_weld odo_mesh_weld;
typedef struct {
  int vertex_capacity, triangle_capacity; /* 1 .. 2^28 each */
  int colour;                             /* 0 or 1: room for rgba */
} odo_mesh_weld_params;
typedef struct {
  float eps;
  float origin[3];
  int grids;
  int drop_unreferenced;
} odo_mesh_weld_rule;
/* Validates before it touches the device: -1 with the bound named in the message and *out untouched on any violation. Device memory,
 * allocated once, in one block: per vertex of capacity 73 B (81 B with colour: two sets of output buffers and the scratch), per
 * triangle 40 B, per slot of the vertex table 12 B and of the triangle table 4 B. ctx must outlive the welder. One host thread at a
 * time. */
int odo_mesh_weld_create(odo_ctx* ctx, const odo_mesh_weld_params* p, odo_mesh_weld** out);
/* Enqueues the passes on ctx's stream and returns at once, no host wait; a pass reads the counts of the one before on the device.
 * The inputs are never written. rgba_dev may be NULL (no colours this run); xyz0_dev / nrmw_dev may be NULL iff n_vertices == 0 and
 * tri_dev iff n_triangles == 0, and either count may be 0. -1 and nothing enqueued for: NULL where not allowed; eps not finite or
 * <= 0; a non-finite origin; grids not 1 or 8; drop_unreferenced not 0 or 1; a negative count or one beyond 2^28; a misaligned
 * pointer (16 bytes for xyz0 and nrmw, 4 for rgba and tri) — all decided before the welder is read — and for counts beyond the
 * capacities, rgba_dev on a welder without colour, and an input that overlaps the welder's buffers. Ordering is
 * odo_speckle_run_dev's: what is enqueued on ctx's stream afterwards is ordered behind it; the inputs must stay as they are until
 * then. */
int odo_mesh_weld_run_dev(odo_mesh_weld* w, const odo_mesh_weld_rule* rule, long n_vertices, long n_triangles, const float* xyz0_dev,
                          const float* nrmw_dev, const uint8_t* rgba_dev, const int32_t* tri_dev);
/* The last run's result in the welder's own buffers (valid until the next run or destroy; *rgba_dev NULL when the run carried no
 * colours; any pointer argument may be NULL) and its two counts, for which it waits for ctx's stream. 0, 0 before the first run. */
int odo_mesh_weld_result_dev(odo_mesh_weld* w, const float** xyz0_dev, const float** nrmw_dev, const uint8_t** rgba_dev,
                             const int32_t** tri_dev, long* n_vertices, long* n_triangles);
/* Copies the last run's result into host buffers of the given capacities and waits. Capacities 0, 0: the counts alone. As
 * odo_volume_spill_mesh does, it refuses capacities below the counts (-1, the counts still returned) rather than cutting. rgba may
 * be NULL. */
int odo_mesh_weld_download(odo_mesh_weld* w, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw, uint8_t* rgba,
                           int32_t* tri, long* n_vertices, long* n_triangles);
/* The host-array convenience: upload (a staging block of this call's own), odo_mesh_weld_run_dev, odo_mesh_weld_download. */
int odo_mesh_weld_run(odo_mesh_weld* w, const odo_mesh_weld_rule* rule, long n_vertices, long n_triangles, const float* xyz0,
                      const float* nrmw, const uint8_t* rgba, const int32_t* tri, long vertex_capacity, long triangle_capacity,
                      float* out_xyz0, float* out_nrmw, uint8_t* out_rgba, int32_t* out_tri, long* out_vertices, long* out_triangles);
/* Of the last run, exact, in the order above. Waits for ctx's stream. Zeros before the first run. */
int odo_mesh_weld_stats(odo_mesh_weld* w, long out[12]);
/* Diagnostic: the passes in order, within a pass each of the six groups of launches `reps` (1 .. 10000) times between two events on
 * ctx's stream; us[0 .. 5] = the mean time in microseconds, summed over the passes, of keys + vertex table / representatives /
 * triangle remap + table / survivors / scans / scatters (table clears included), us[6] = their sum. Waits. Then one run: the
 * outputs and the statistics are exactly one run's afterwards. */
int odo_mesh_weld_time_dev(odo_mesh_weld* w, const odo_mesh_weld_rule* rule, long n_vertices, long n_triangles, const float* xyz0_dev,
                           const float* nrmw_dev, const uint8_t* rgba_dev, const int32_t* tri_dev, int reps, float us[7]);
/* Safe with a run in flight: waits for ctx's stream first. */
int odo_mesh_weld_destroy(odo_mesh_weld* w);

/* ---- Mesh component filter: small connected pieces leave an indexed mesh, exact to the last bit ----------------------------------
 * Input: n_v vertices (xyz0 float4, nrmw float4, optionally rgba uint8[4]) and n_t triangles (int32[3]) on the device, as the
 * welder's odo_mesh_weld_result_dev gives them. A rule: min_triangles >= 0, keep_largest in {0, 1}, drop_unreferenced in {0, 1}.
 *   Valid         a triangle is valid iff its three indices lie in [0, n_v). An invalid one is dropped and counted bad_index; its
 *                 indices are never dereferenced and its label is -1. A valid triangle with two equal indices is degenerate: it
 *                 counts towards its component's size, stays or leaves with it like any other, and contributes no edge (a, a).
 *   Component     valid triangles that share a vertex index are connected (vertex connectivity: two tetrahedra that touch in one
 *                 vertex are one component). A component's label is its smallest vertex index, its size its number of valid
 *                 triangles.
 *   Survival      a component survives iff size >= min_triangles (a size equal to the bound stays) and, with keep_largest, it is
 *                 the component of the largest size, of several the one with the smallest label. If the largest is below
 *                 min_triangles nothing survives and the result is an empty mesh.
 *   Output        the surviving triangles in input order, their indices renumbered. The vertices kept are those a surviving
 *                 triangle names and, without drop_unreferenced, also those no valid triangle names; in ascending index, each with
 *                 its own xyz0, nrmw and rgba bit for bit. Per input triangle a label (int32): odo_mesh_components_labels.
 *   Edges         (only on a filter created with edge_stats = 1) the undirected edges a != b of the valid triangles, each with its
 *                 number of uses; an edge lies in exactly one component.
 * Counters (odo_mesh_components_stats, in this order): vertices_in, triangles_in, vertices_out, triangles_out; components,
 * removed_components, removed_triangles, removed_vertices (the vertices of the removed components), largest (the size of the
 * largest component), bad_index, degenerate, unreferenced (vertices no valid triangle names that were dropped; 0 without
 * drop_unreferenced), so that triangles_out = triangles_in - removed_triangles - bad_index and vertices_out = vertices_in -
 * removed_vertices - unreferenced; edges, open_edges (used once), nonmanifold_edges (used more than twice) of the input, and
 * edges_out, open_edges_out, nonmanifold_edges_out of the edges whose component survives (all six 0 without edge_stats); guard (0;
 * see below).
 * Nothing depends on timing: a root is the smallest index of its component whatever the order of the unions (the larger root goes
 * under the smaller with an integer atomicMin, a lost race goes on from the word it read), sizes and use counts are integer sums,
 * the largest is a maximum of size << 32 | ~label, an edge slot is claimed with a 64-bit atomicCAS and never changes its key, and
 * the compaction is count, scan, scatter. The edge table has 2^ceil(log2(6 triangle_capacity)) slots and is probed linearly from a
 * splitmix64 hash. Every data-dependent loop carries a hard trip bound — n_v for a walk to a root and for a union, the table's size
 * for a probe — and a loop that runs into it sets a bit of `guard` and leaves. No loop waits for another
 * thread. */
typedef struct odo_mesh_components odo_mesh_components;
typedef struct {
  int vertex_capacity, triangle_capacity; /* 1 .. 2^28 each */
  int colour;                             /* 0 or 1: room for rgba */
  int edge_stats;                         /* 0 or 1: the edge table and its six counters */
} odo_mesh_components_params;
typedef struct {
  int min_triangles;
  int keep_largest;
  int drop_unreferenced;
} odo_mesh_components_rule;
/* Validates before it touches the device: -1 with the bound named in the message and *out untouched on any violation, and on an
 * allocation the device refuses. Device memory, allocated once, in one block: per vertex of capacity 45 B (49 B with colour), per
 * triangle 16 B, per slot of the edge table 12 B. ctx must outlive the filter. One host thread at a time. */
int odo_mesh_components_create(odo_ctx* ctx, const odo_mesh_components_params* p, odo_mesh_components** out);
/* Enqueues the run on ctx's stream and returns at once, no host wait. The inputs are never written. rgba_dev may be NULL (no
 * colours this run); xyz0_dev / nrmw_dev may be NULL iff n_vertices == 0 and tri_dev iff n_triangles == 0, and either count may be
 * 0. -1 and nothing enqueued for: NULL where not allowed; min_triangles < 0; keep_largest or drop_unreferenced not 0 or 1; a
 * negative count or one beyond 2^28; a misaligned pointer (16 bytes for xyz0 and nrmw, 4 for rgba and tri) — all decided before the
 * filter is read — and for counts beyond the capacities, rgba_dev on a filter without colour, and an input that overlaps the
 * filter's buffers. Ordering is odo_mesh_weld_run_dev's: the inputs may be the welder's result buffers of a weld enqueued on the
 * same stream before, and must stay as they are until the run is done. */
int odo_mesh_components_run_dev(odo_mesh_components* f, const odo_mesh_components_rule* rule, long n_vertices, long n_triangles,
                                const float* xyz0_dev, const float* nrmw_dev, const uint8_t* rgba_dev, const int32_t* tri_dev);
/* The last run's result in the filter's own buffers (valid until the next run or destroy; *rgba_dev NULL when the run carried no
 * colours; any pointer argument may be NULL) and its two counts, for which it waits for ctx's stream. 0, 0 before the first run. */
int odo_mesh_components_result_dev(odo_mesh_components* f, const float** xyz0_dev, const float** nrmw_dev, const uint8_t** rgba_dev,
                                   const int32_t** tri_dev, long* n_vertices, long* n_triangles);
/* Copies the last run's result into host buffers of the given capacities and waits. Capacities 0, 0: the counts alone. Refuses
 * capacities below the counts (-1, the counts still returned) rather than cutting. rgba may be NULL. */
int odo_mesh_components_download(odo_mesh_components* f, long vertex_capacity, long triangle_capacity, float* xyz0, float* nrmw,
                                 uint8_t* rgba, int32_t* tri, long* n_vertices, long* n_triangles);
/* The host-array convenience: upload (a staging block of this call's own), odo_mesh_components_run_dev,
 * odo_mesh_components_download. */
int odo_mesh_components_run(odo_mesh_components* f, const odo_mesh_components_rule* rule, long n_vertices, long n_triangles,
                            const float* xyz0, const float* nrmw, const uint8_t* rgba, const int32_t* tri, long vertex_capacity,
                            long triangle_capacity, float* out_xyz0, float* out_nrmw, uint8_t* out_rgba, int32_t* out_tri,
                            long* out_vertices, long* out_triangles);
/* The last run's labels, one int32 per INPUT triangle (its component's smallest vertex index, -1 for an invalid triangle), in the
 * filter's own buffer, and their number: that run's n_triangles (0 before the first run). Does not wait. */
int odo_mesh_components_labels_dev(odo_mesh_components* f, const int32_t** labels_dev, long* n_triangles);
/* Copies them to the host and waits. capacity 0: the count alone; a capacity below the count is refused. */
int odo_mesh_components_labels(odo_mesh_components* f, long capacity, int32_t* labels, long* n_triangles);
/* Of the last run, exact, in the order above. Waits for ctx's stream. Zeros before the first run. */
int odo_mesh_components_stats(odo_mesh_components* f, long out[19]);
/* Diagnostic: each of the six groups of launches `reps` (1 .. 10000) times between two events on ctx's stream; us[0 .. 5] = the mean
 * time in microseconds of union / flatten + sizes + largest / edge table + census / survivors / scans / scatters (clears
 * included), us[6] = their sum. Waits. Then one run: the outputs, the labels and the statistics are exactly one run's afterwards. */
int odo_mesh_components_time_dev(odo_mesh_components* f, const odo_mesh_components_rule* rule, long n_vertices, long n_triangles,
                                 const float* xyz0_dev, const float* nrmw_dev, const uint8_t* rgba_dev, const int32_t* tri_dev,
                                 int reps, float us[7]);
/* Safe with a run in flight: waits for ctx's stream first. */
int odo_mesh_components_destroy(odo_mesh_components* f);

/* ---- S sequences in lock step on one GPU (the data-parallel axis of SURVEY section 8e inside one device) -----------------
 * One odo_tracker tracks one sequence as a serial chain of ~70 short launches per frame, which leaves most of the chip
 * idle. odo_tracker_batch runs the same frame loop (ref: run_odometry_kitti_offline.cpp:198-271) for n_sequences independent
 * sequences with every launch carrying all of them (blockIdx.y / .z = sequence). Per-sequence arithmetic, reduction order and
 * launch order are those of odo_tracker: poses, depth maps and keyframe decisions are bit-identical to n separate trackers.
 * All sequences share rows / cols / parameters. Arrays are indexed by sequence; poses are n x 16 floats, column-major. */
typedef struct odo_tracker_batch odo_tracker_batch;
int odo_tracker_batch_create(int device, const odo_tracker_params* p, int n_sequences, odo_tracker_batch** out);
int odo_tracker_batch_destroy(odo_tracker_batch* b);
/* The inverse-depth LM of a lock step (ref: src/depth_estimate.cpp:141-168,200-242) in ONE persistent launch for all sequences — each on
 * an XCD of its own, beside the batched pose LM's — instead of a launch per iteration: up to four sequences (more share their XCDs with
 * the pose LM, where the 80 workgroups of a sequence do not fit). *on = 1 while it is in use, *chains_redone = lock steps whose launch
 * gave up and whose depth jobs were run again on the launches per iteration (results unaffected; three switch it off). */
int odo_tracker_batch_depth_persistent_stats(const odo_tracker_batch* b, int* on, int* chains_redone);
int odo_tracker_batch_size(const odo_tracker_batch* b);
/* The pose optimiser of one slot (launch statistics of the batched Solves live with the first slot's: odo_lm_event_timing). */
odo_lm* odo_tracker_batch_lm(odo_tracker_batch* b, int slot);
odo_ctx* odo_tracker_batch_ctx(odo_tracker_batch* b); /* for odo_dev_alloc / upload / download of its frames */
/* Frame 0 (ref: :95-145) of every slot that is given a pair; a slot whose left_dev[i] / right_dev[i] are NULL stays empty.
 * abs_pose0: n x 16, or NULL for identity. Returns -1 if any sequence's ComputeDepth fails ("Init 0-th frame failed!",
 * ref: :103-106; the other slots are initialised all the same). May be called again to start new sequences. */
int odo_tracker_batch_init(odo_tracker_batch* b, const float* const* left_dev, const float* const* right_dev,
                           const float* abs_pose0_colmajor);
/* Starts a new sequence in ONE slot while the other slots keep theirs (sequences of different lengths: when one ends its
 * slot takes the next sequence). Drains both streams first. abs_pose0: 16 floats or NULL for identity. */
int odo_tracker_batch_init_one(odo_tracker_batch* b, int slot, const float* left_dev, const float* right_dev,
                               const float abs_pose0_colmajor[16]);
/* One iteration of the frame loop for every slot that is given a frame. status[i]: 0 tracked; 1 the Solve failed
 * (pseudo-identity, the runner carries on, ref: src/lm_optimizer.cpp:60-65); -1 ComputeDepth failed on this frame (its pose is
 * still written and the sequence stops, ref: :230-232); -2 the slot holds no running sequence (empty, or stopped earlier: its
 * outputs are untouched); -3 no frame was given for the slot (left_dev[i] == NULL): it sits this step out, its state is kept,
 * it costs nothing. Returns -1 only for argument / device errors. pose_to_keyframe, abs_pose, is_new_keyframe, motion_mag may
 * be NULL. */
int odo_tracker_batch_track(odo_tracker_batch* b, const float* const* left_dev, const float* const* right_dev,
                            float* pose_to_keyframe, float* abs_pose, int* is_new_keyframe, float* motion_mag, int* status);
/* Optional pipelining, as odo_tracker_hint_next: the left images of the NEXT step (n pointers, NULL entries allowed), announced
 * before odo_tracker_batch_track of the current one; their pyramids are built behind this step's Solve. Same work, earlier. */
int odo_tracker_batch_hint_next(odo_tracker_batch* b, const float* const* next_left_dev);
/* The same with the right images (odo_tracker_hint_next_pair for every slot): the next step's ComputeDepth, depth pyramids and
 * candidate lists are enqueued a step early, so the depth stream works a step ahead of the pose LM. NULL entries allowed. */
int odo_tracker_batch_hint_next_pair(odo_tracker_batch* b, const float* const* next_left_dev, const float* const* next_right_dev);
/* Counters of the last tracked frame, one entry per sequence (any pointer may be NULL). */
int odo_tracker_batch_stats(const odo_tracker_batch* b, int* lm_evals, int* depth_iters, int* n_valid_depth, int* n_keyframes);
/* The batched twin of odo_tracker_quiesce: posted chains run to completion, the early-started next Solve is dropped,
 * announcements are void, all streams idle; afterwards nothing reads a caller-owned frame buffer. */
int odo_tracker_batch_quiesce(odo_tracker_batch* b);
/* Diagnostics: host-clock averages per lock step since the last call, microseconds: {whole call, table + pyramid launches,
 * batched Solve, wait for the depth chain after the Solve}. */
int odo_tracker_batch_timing(odo_tracker_batch* b, double out[4]);
/* Device pointers to sequence `seq`'s last outputs (rows x cols): validity mask (u8), disparity, inverse depth. */
int odo_tracker_batch_outputs(const odo_tracker_batch* b, int seq, const uint8_t** val_dev, const float** disp_dev,
                              const float** dep_dev);
int odo_tracker_destroy(odo_tracker* t);

/* ---- camera model: rectified intrinsics per level, undistort + rectify ---------------------------------
 * Replaces odometry::CameraPyramid (ref: include/camera.h:16-119).
 * odo_camera_create      = CameraPyramid(levels, fx, fy, f_theta, cx, cy, k1, k2, r1, r2, sensor_w, sensor_h,
 *                          resolution_w, resolution_h) (ref: include/camera.h:34-35; src/camera.cpp:12-38).
 * odo_camera_configure   = ConfigureCamera(rectify_rotation 3x3, new_intrinsic 3x4, new_size, CV_32FC1, false)
 *                          (ref: include/camera.h:56-57; src/camera.cpp:40-69): the intrinsic pyramid
 *                          (f / 2, c <- (c + 0.5) / 2 + 0.5 per level, double) and the cv::initUndistortRectifyMap
 *                          lookup maps, built on the device. R and P are row-major doubles as cv::stereoRectify
 *                          returns them (cv::stereoRectify itself, a one-off host-side calibration step inside
 *                          SetUpStereoCameraSystem, ref: src/camera.cpp:138-141, stays with the caller).
 * odo_camera_undistort_rectify = UndistortRectify(src_raw, dst, INTER_LINEAR, BORDER_CONSTANT, borderValue)
 *                          (ref: include/camera.h:68; src/camera.cpp:71-82): cv::remap through the maps. The
 *                          reference's hard 480x640 check lives in the C++ shim; this entry takes any size.
 *                          dst is map_rows x map_cols. The _dev variant works on device-resident images and
 *                          is asynchronous on the context's stream.
 * odo_camera_intrinsics  = fx/fy/f_theta/cx/cy_double(level) (ref: include/camera.h:80-85), out5 in that order.
 * odo_camera_raw         = the raw-parameter accessors (ref: include/camera.h:91-105). */
int odo_camera_create(odo_ctx* ctx, int levels, double fx, double fy, double f_theta, double cx, double cy, double k1,
                      double k2, double r1, double r2, double sensor_width, double sensor_height, int resolution_width,
                      int resolution_height, odo_camera** out);
int odo_camera_configure(odo_camera* cam, const double R_rowmajor[9], const double P_rowmajor[12], int new_width,
                         int new_height);
int odo_camera_levels(const odo_camera* cam);
int odo_camera_intrinsics(const odo_camera* cam, int level, double out5[5]);
int odo_camera_raw(const odo_camera* cam, double raw5[5], double dist4[4], double sensor2[2], int resolution2[2]);
int odo_camera_map_size(const odo_camera* cam, int* rows, int* cols);
int odo_camera_download_maps(const odo_camera* cam, float* mapx_host, float* mapy_host);
int odo_camera_undistort_rectify(odo_camera* cam, const float* src, int src_rows, int src_cols, float* dst,
                                 float border_value);
int odo_camera_undistort_rectify_dev(odo_camera* cam, const float* src_dev, int src_rows, int src_cols, float* dst_dev,
                                     float border_value);
int odo_camera_destroy(odo_camera* cam);

/* ---- the pose exchange of the multi-GPU path for hosts that are not Python ---------------------------
 * Tracking shards by sequence (rank r owns sequences r, r + N, ...; ref: run_odometry_kitti_offline.cpp:198-271 is sequential
 * inside a sequence and independent across sequences): there is no data-path collective. The one exchange is an all-gather of
 * the results over RCCL: per tracked frame a row of ODO_GATHER_ROW four-byte words (int32 sequence id, int32 frame id — bit
 * patterns in the float row, exact for any id — then the 3x4 absolute pose as floats, row-major), `every` rows per ncclAllGather, on a stream of its own, never waited for while tracking. The schedule is fixed up
 * front: EVERY rank issues ceil(n_max_frames / every) collectives of a fixed block and pads with rows whose sequence id is -1
 * (uneven shards — 11 sequences over 8 GPUs — cannot leave ranks with different numbers of collectives). RCCL is dlopen'ed
 * (librccl.so.1, or ODO_RCCL_SO): no link-time dependency. bench.py uses the same schedule through torch.distributed
 * (odometry_amd/dist.py); on a one-GPU box this entry runs at world size 1 only (RCCL refuses two ranks on one device),
 * tests/test_gpu_gather.py::test_two_ranks_* runs it at world size 2 wherever two devices are visible. */
#define ODO_GATHER_ID_BYTES 128
#define ODO_GATHER_ROW 14
typedef struct odo_gather odo_gather;
/* Rank 0: an ncclUniqueId; hand its bytes to every rank by the host's own means (MPI, a file, a socket). */
int odo_gather_unique_id(unsigned char id[ODO_GATHER_ID_BYTES]);
/* Collective over all ranks (ncclCommInitRank). n_local_frames: rows THIS rank will push; n_max_frames: the largest such number
 * over the ranks (every rank derives both from the same sharding rule). */
int odo_gather_create(int device, int world, int rank, const unsigned char id[ODO_GATHER_ID_BYTES], int every,
                      int n_local_frames, int n_max_frames, odo_gather** out);
/* One tracked frame's result; every `every`-th push issues a collective and returns at once. */
int odo_gather_push(odo_gather* g, int seq_id, int frame_id, const float abs_pose_colmajor[16]);
/* Issues what is left of the schedule (padded) and waits for every collective. */
int odo_gather_flush(odo_gather* g);
/* After flush: the valid rows received from `rank` (ODO_GATHER_ROW words each, in push order; words 0 and 1 are int32 bit
 * patterns: memcpy them into ints). */
int odo_gather_rows(odo_gather* g, int rank, const float** rows, int* n_rows);
int odo_gather_issued(const odo_gather* g);   /* collectives issued so far */
int odo_gather_ranks(const odo_gather* g);    /* ranks in the communicator, from ncclCommCount; -1 on error */
int odo_gather_destroy(odo_gather* g);

#ifdef __cplusplus
}
#endif
#endif /* ODOMETRY_HIP_H */
