"""Python mirror of the reference's public C++ surface over the C ABI (test/bench harness).

Same class names, argument order and error behaviour as the reference
(ref: include/image_pyramid.h:14-69, include/lm_optimizer.h:24-115, include/depth_estimate.h:24-121,
include/keyframe.h:17-60): status ints 0 / -1, messages on stdout, Solve returns the pseudo-identity on
failure. Matrices are numpy 4x4 (row-major view of the reference's column-major Affine4f).
The C++ drop-in is include/odometry_shim.hpp; this module exists so the parity tests read like the
reference's own programs.
"""
import ctypes as C

import numpy as np

from . import _lib as L

_default_ctx = None


class Context:
    """One HIP stream on one device (odo_ctx)."""

    def __init__(self, device=0):
        lib = L.load()
        h = C.c_void_p()
        L.check(lib.odo_ctx_create(device, C.byref(h)), "odo_ctx_create")
        self.h = h
        self.lib = lib

    def synchronize(self):
        L.check(self.lib.odo_ctx_synchronize(self.h), "odo_ctx_synchronize")

    def timer_start(self):
        L.check(self.lib.odo_ctx_timer_start(self.h), "timer_start")

    def timer_stop(self):
        ms = C.c_float(0)
        L.check(self.lib.odo_ctx_timer_stop(self.h, C.byref(ms)), "timer_stop")
        return ms.value

    def alloc(self, nbytes):
        p = C.c_void_p()
        L.check(self.lib.odo_dev_alloc(self.h, nbytes, C.byref(p)), "odo_dev_alloc")
        return p

    def free(self, p):
        L.check(self.lib.odo_dev_free(self.h, p), "odo_dev_free")

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        L.check(self.lib.odo_dev_upload(self.h, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "odo_dev_upload")
        return p

    def download(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        L.check(self.lib.odo_dev_download(self.h, out.ctypes.data_as(C.c_void_p), p, out.nbytes), "odo_dev_download")
        return out

    def close(self):
        if self.h:
            self.lib.odo_ctx_destroy(self.h)
            self.h = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _colmajor(M):
    return _f32(np.asarray(M, np.float32).T).reshape(16)


def _from_colmajor(v):
    return np.asarray(v, np.float32).reshape(4, 4).T.copy()


class _Pyramid:
    _kind = L.PYR_IMAGE

    def __init__(self, num_levels, in_img, smooth, ctx=None, device_ptr=None, shape=None):
        self.ctx = ctx or default_context()
        self.num_levels_ = num_levels
        h = C.c_void_p()
        if device_ptr is not None:
            rows, cols = shape
            st = self.ctx.lib.odo_pyramid_create_dev(self.ctx.h, device_ptr, rows, cols, num_levels, int(bool(smooth)),
                                                     self._kind, C.byref(h))
        else:
            img = _f32(in_img)
            rows, cols = img.shape
            st = self.ctx.lib.odo_pyramid_create(self.ctx.h, _fp(img), rows, cols, 0, num_levels, int(bool(smooth)),
                                                 self._kind, C.byref(h))
        if st != 0:  # ref: src/image_pyramid.cpp:16-18 prints and carries on
            print("Compute Gaussian Image Pyramid failed!" if self._kind == L.PYR_IMAGE
                  else "Compute Gaussian Depth Pyramid failed!")
            raise L.OdoError(L.last_error())
        self.h = h
        self.rows, self.cols = rows, cols

    def rebuild_dev(self, device_ptr, smooth):
        L.check(self.ctx.lib.odo_pyramid_rebuild_dev(self.h, device_ptr, int(bool(smooth))), "odo_pyramid_rebuild_dev")

    def GetNumberLevels(self):
        return self.num_levels_

    def _level(self, level_idx):
        r, c = C.c_int(0), C.c_int(0)
        if self.ctx.lib.odo_pyramid_level_dims(self.h, level_idx, C.byref(r), C.byref(c)) != 0:
            # ref: src/image_pyramid.cpp:22-25 prints and exit(1)s; the mirror raises instead
            raise IndexError(f"Requested image pyramid does not exist! Max pyramid id: {self.num_levels_ - 1}")
        out = np.empty((r.value, c.value), np.float32)
        L.check(self.ctx.lib.odo_pyramid_download(self.h, level_idx, _fp(out)), "odo_pyramid_download")
        return out

    def level_dev(self, level_idx):
        return self.ctx.lib.odo_pyramid_level_dev(self.h, level_idx)

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.odo_pyramid_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ImagePyramid(_Pyramid):
    """ref: include/image_pyramid.h:14-41"""
    _kind = L.PYR_IMAGE

    def GetPyramidImage(self, level_idx):
        return self._level(level_idx)


class DepthPyramid(_Pyramid):
    """ref: include/image_pyramid.h:43-69"""
    _kind = L.PYR_DEPTH

    def GetPyramidDepth(self, level_idx):
        return self._level(level_idx)


class LevenbergMarquardtOptimizer:
    """ref: include/lm_optimizer.h:24-115"""

    def __init__(self, lam, precision, kMaxIterations, kRelativeInit, kCameraPtr=None, robust_est=1,
                 huber_delta=4.0 / 255.0, ctx=None, intrinsics=None):
        self.ctx = ctx or default_context()
        if kCameraPtr is None and intrinsics is None:
            print("LM Optimizer failed! Invalid camera pointer!")  # ref: src/lm_optimizer.cpp:35-36 (warning only)
        mi = (C.c_int * len(kMaxIterations))(*kMaxIterations)
        init = _colmajor(kRelativeInit)
        K = None
        if intrinsics is not None:
            K = C.pointer(L.Intrinsics(*intrinsics))
        h = C.c_void_p()
        L.check(self.ctx.lib.odo_lm_create(self.ctx.h, lam, precision, mi, len(kMaxIterations), _fp(init), robust_est,
                                           huber_delta, K, C.byref(h)), "odo_lm_create")
        self.h = h
        self.n_levels = len(kMaxIterations)

    def Solve(self, kImagePyr1, kDepthPyr1, kImagePyr2):
        out = np.zeros(16, np.float32)
        st = self.ctx.lib.odo_lm_solve(self.h, kImagePyr1.h, kDepthPyr1.h, kImagePyr2.h, _fp(out))
        self.last_status = st
        if st != 0:
            print("Optimize failed! ")  # ref: src/lm_optimizer.cpp:61
        return _from_colmajor(out)

    def SolveBegin(self, kImagePyr1, kDepthPyr1, kImagePyr2):
        """odo_lm_solve_begin: start the Solve a following Solve() with the same pyramids collects. Returns 0 / 1 (not started)."""
        st = self.ctx.lib.odo_lm_solve_begin(self.h, kImagePyr1.h, kDepthPyr1.h, kImagePyr2.h)
        if st < 0:
            raise L.OdoError("odo_lm_solve_begin: " + L.last_error())
        return st

    def CandidateBegin(self, side_ctx, kImagePyr, kDepthPyr, mark=0):
        """Keyframe-candidate point lists of (kImagePyr, kDepthPyr) built ahead on side_ctx's stream (odo_lm_candidate_begin)."""
        return self.ctx.lib.odo_lm_candidate_begin(self.h, side_ctx.h, kImagePyr.h, kDepthPyr.h, mark)

    def Reset(self, kRelativeInit, lam):
        init = _colmajor(kRelativeInit)
        st = self.ctx.lib.odo_lm_reset(self.h, _fp(init), lam)
        if st != 0:
            print("Reset optimizer failed!")
        return st

    def report(self):
        iters = (C.c_int * 4)()
        cost = (C.c_float * 8)()
        L.check(self.ctx.lib.odo_lm_report(self.h, iters, cost), "odo_lm_report")
        return list(iters), [[cost[2 * i], cost[2 * i + 1]] for i in range(4)]

    def ShowReport(self, real=False):
        """ref: src/lm_optimizer.cpp:364-371 — the reference's statistics are never written, so it prints zeros; real=True
        prints what the device counted (report())."""
        iters, cost = self.report() if real else ([0, 0, 0, 0], [[0.0, 0.0]] * 4)
        print("Number of iterations performed per level: " + ", ".join(str(i) for i in iters))
        print("Costs before/after per level: ")
        for c in cost:
            print(f"{c[0]}, {c[1]}")

    # -- diagnostics beyond the reference surface --------------------------------------------------
    def accumulate(self, kImagePyr1, kDepthPyr1, kImagePyr2, level, T):
        acc = np.zeros(L.NACC, np.float64)
        Tc = _colmajor(T)
        st = self.ctx.lib.odo_lm_accumulate(self.h, kImagePyr1.h, kDepthPyr1.h, kImagePyr2.h, level, _fp(Tc),
                                            acc.ctypes.data_as(C.POINTER(C.c_double)))
        return st, acc

    def set_record(self, on):
        """odo_lm_set_record: off = no trace rows / cost statistics, the Solves run the lean LM kernels (what the trackers' own
        optimisers and the drop-in C++ class do)."""
        L.check(self.ctx.lib.odo_lm_set_record(self.h, 1 if on else 0), "odo_lm_set_record")

    def trace(self):
        rows = (L.LmTraceRow * 128)()
        n = C.c_int(0)
        L.check(self.ctx.lib.odo_lm_trace(self.h, rows, 128, C.byref(n)), "odo_lm_trace")
        return [dict(level=r.level, iter=r.iter, n_res=r.n_res, accepted=r.accepted, stop=r.stop, err=r.err,
                     lambda_after=r.lambda_after, delta=np.array(r.delta[:], np.float32)) for r in rows[:n.value]]

    def time_eval(self, kImagePyr1, kDepthPyr1, kImagePyr2, level, T, reps=50):
        mean, mn, b, n = C.c_float(0), C.c_float(0), C.c_double(0), C.c_int(0)
        Tc = _colmajor(T)
        L.check(self.ctx.lib.odo_lm_time_eval(self.h, kImagePyr1.h, kDepthPyr1.h, kImagePyr2.h, level, _fp(Tc), reps,
                                              C.byref(mean), C.byref(mn), C.byref(b), C.byref(n)), "odo_lm_time_eval")
        return dict(mean_us=mean.value, min_us=mn.value, bytes=b.value, n_points=n.value)

    def set_sampling(self, bilinear):
        """False = the reference's floor sampling (parity mode, default); True = bilinear sampling (non-parity option)."""
        L.check(self.ctx.lib.odo_lm_set_sampling(self.h, 1 if bilinear else 0), "odo_lm_set_sampling")

    def set_mode(self, mode):
        L.check(self.ctx.lib.odo_lm_set_mode(self.h, mode), "odo_lm_set_mode")

    def points(self):
        n = (C.c_int * L.MAX_LEVELS)()
        u = (C.c_int * L.MAX_LEVELS)()
        L.check(self.ctx.lib.odo_lm_points(self.h, n, u), "odo_lm_points")
        return list(n)[:self.n_levels], list(u)[:self.n_levels]

    def launch_stats(self):
        a, t, b = C.c_int(0), C.c_int(0), C.c_double(0)
        L.check(self.ctx.lib.odo_lm_launch_stats(self.h, C.byref(a), C.byref(t), C.byref(b)), "odo_lm_launch_stats")
        return a.value, t.value, b.value

    def persistent_stats(self):
        """(workgroups of the persistent fine-level launch — 0: step launches —, Solves redone on the step launches)"""
        k, f = C.c_int(0), C.c_int(0)
        L.check(self.ctx.lib.odo_lm_persistent_stats(self.h, C.byref(k), C.byref(f)), "odo_lm_persistent_stats")
        return k.value, f.value

    def last_plan(self):
        """odo_lm_last_plan: which path the last Solve / solve_batch took, as a dict — n (sequences of the batched Solve, 0: a Solve of
        its own or the sequential fall-back), min_level, fine_lo, workgroups (per sequence of the persistent launch, 0: none issued),
        launches, redone."""
        out = (C.c_int * 6)()
        L.check(self.ctx.lib.odo_lm_last_plan(self.h, out), "odo_lm_last_plan")
        return dict(zip(("n", "min_level", "fine_lo", "workgroups", "launches", "redone"), (int(v) for v in out)))

    def tdist_stats(self):
        """(scale iterations issued on the multi-workgroup kernel, those redone by its single-workgroup fall-back)"""
        a, b = C.c_long(0), C.c_int(0)
        L.check(self.ctx.lib.odo_lm_tdist_stats(self.h, C.byref(a), C.byref(b)), "odo_lm_tdist_stats")
        return a.value, b.value

    def persistent_backoff(self):
        """(give-ups that count — 3: switched off —, Solves a switched-off launch waits before its next try, Solves left until then)"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        L.check(self.ctx.lib.odo_lm_persistent_backoff(self.h, C.byref(a), C.byref(b), C.byref(c)), "odo_lm_persistent_backoff")
        return a.value, b.value, c.value

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.odo_lm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_batch(lms, kf_imgs, kf_deps, cur_imgs):
    """odo_lm_solve_batch: the Solves of several independent sequences in the same launches. Returns (poses [n, 4, 4], status [n])."""
    n = len(lms)
    lib = lms[0].ctx.lib
    arr = lambda objs: (C.c_void_p * n)(*[o.h for o in objs])   # noqa: E731
    out = np.zeros((n, 16), np.float32)
    st = (C.c_int * n)()
    L.check(lib.odo_lm_solve_batch(n, arr(lms), arr(kf_imgs), arr(kf_deps), arr(cur_imgs), _fp(out), st), "odo_lm_solve_batch")
    for m, v in zip(lms, st):
        m.last_status = v
    return np.stack([_from_colmajor(o) for o in out]), list(st)


def time_eval_batch(lms, kf_imgs, kf_deps, cur_imgs, level, T, reps=50):
    """odo_lm_time_eval_batch: `reps` event-timed launches of the batched dense evaluation (blockIdx.y = stream) of `level`."""
    n = len(lms)
    lib = lms[0].ctx.lib
    arr = lambda objs: (C.c_void_p * n)(*[o.h for o in objs])   # noqa: E731
    mean, mn, b, npts = C.c_float(0), C.c_float(0), C.c_double(0), C.c_int(0)
    L.check(lib.odo_lm_time_eval_batch(n, arr(lms), arr(kf_imgs), arr(kf_deps), arr(cur_imgs), level, _fp(_colmajor(T)), reps,
                                       C.byref(mean), C.byref(mn), C.byref(b), C.byref(npts)), "odo_lm_time_eval_batch")
    return dict(mean_us=mean.value, min_us=mn.value, bytes=b.value, n_points=npts.value)


class DepthEstimator:
    """ref: include/depth_estimate.h:24-121"""

    def __init__(self, grad_th, ssd_th, photo_th, min_depth, max_depth, lam, huber_delta, precision, max_iters,
                 boundary, left_cam_ptr=None, right_cam_ptr=None, baseline=0.0, max_residuals=5000, ctx=None,
                 intrinsics=None, max_disparity=0, any_size=False):
        self.ctx = ctx or default_context()
        K = C.pointer(L.Intrinsics(*intrinsics)) if intrinsics is not None else None
        h = C.c_void_p()
        L.check(self.ctx.lib.odo_depth_create(self.ctx.h, grad_th, ssd_th, photo_th, min_depth, max_depth, lam,
                                              huber_delta, precision, max_iters, boundary, K, baseline, max_residuals,
                                              max_disparity, int(any_size), C.byref(h)), "odo_depth_create")
        self.h = h
        self.max_iters_ = max_iters

    def _run(self, fn, left_img, right_img, left_val, left_disp, left_dep):
        if left_img.shape != right_img.shape:
            print("Number of rows/cols do not match for left/right images.")  # ref: src/depth_estimate.cpp:37-40
            return -1
        if left_img.dtype != np.float32 or right_img.dtype != np.float32:
            print("Pixel type of left/right images not 32-bit float.")  # ref: :41-44
            return -1
        left_img = np.ascontiguousarray(left_img)
        right_img = np.ascontiguousarray(right_img)
        rows, cols = left_img.shape
        for a in (left_val, left_disp, left_dep):
            if not a.flags["C_CONTIGUOUS"] or a.shape != (rows, cols):
                print("The cv::Mat matrix is not continuous in disparity search!")  # ref: :259-263
                return -1
        st = fn(self.h, _fp(left_img), _fp(right_img), rows, cols, left_val.ctypes.data_as(C.POINTER(C.c_uint8)),
                _fp(left_disp), _fp(left_dep))
        if st != 0:
            print(L.last_error())
        return st

    def ComputeDepth(self, left_img, right_img, left_val, left_disp, left_dep):
        return self._run(self.ctx.lib.odo_depth_compute, left_img, right_img, left_val, left_disp, left_dep)

    def DisparityDepthEstimate(self, left_img, right_img, left_val, left_disp, left_dep):
        return self._run(self.ctx.lib.odo_depth_disparity, left_img, right_img, left_val, left_disp, left_dep)

    def compute_dev(self, left_dev, right_dev, rows, cols, val_dev, disp_dev, dep_dev):
        return self.ctx.lib.odo_depth_compute_dev(self.h, left_dev, right_dev, rows, cols, val_dev, disp_dev, dep_dev)

    def compute_begin_dev(self, side_ctx, left_dev, right_dev, rows, cols, val_dev, disp_dev, dep_dev, left_stamp, right_stamp, mark=0):
        """ComputeDepth started ahead on side_ctx's stream (returns at once): 0 started, 1 not started, -1 error."""
        return self.ctx.lib.odo_depth_compute_begin_dev(self.h, side_ctx.h, left_dev, right_dev, rows, cols, val_dev, disp_dev,
                                                        dep_dev, left_stamp, right_stamp, mark)

    def compute_end_dev(self, left_dev, right_dev, rows, cols, val_dev, disp_dev, dep_dev, left_stamp, right_stamp):
        return self.ctx.lib.odo_depth_compute_end_dev(self.h, left_dev, right_dev, rows, cols, val_dev, disp_dev, dep_dev,
                                                      left_stamp, right_stamp)

    def early_pending(self):
        return bool(self.ctx.lib.odo_depth_early_pending(self.h))

    def time_stages(self, left_dev, right_dev, rows, cols, reps=20):
        us = (C.c_float * 3)()
        cand, nsel = C.c_double(0), C.c_int(0)
        L.check(self.ctx.lib.odo_depth_time_stages(self.h, left_dev, right_dev, rows, cols, reps, us, C.byref(cand),
                                                   C.byref(nsel)), "odo_depth_time_stages")
        return dict(blur_us=us[0], select_us=us[1], scan_us=us[2], candidates=cand.value, n_selected=nsel.value)

    def report(self):
        it, ns, nm, nv = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        cost = C.c_float(0)
        L.check(self.ctx.lib.odo_depth_report(self.h, C.byref(it), C.byref(cost), C.byref(ns), C.byref(nm),
                                              C.byref(nv)), "odo_depth_report")
        return dict(iters=it.value, cost=cost.value, n_selected=ns.value, n_matched=nm.value, n_valid=nv.value)

    def persistent_stats(self):
        """(1 while DepthOptimization runs as one persistent launch — 0: a launch per iteration —, calls redone on the step launches)"""
        a, b = C.c_int(0), C.c_int(0)
        L.check(self.ctx.lib.odo_depth_persistent_stats(self.h, C.byref(a), C.byref(b)), "odo_depth_persistent_stats")
        return a.value, b.value

    def ReportStatus(self):
        r = self.report()
        print(f"    Number of iters performed: {r['iters']}(max allowed: {self.max_iters_})")
        print(f"    Final cost: {r['cost']}")

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.odo_depth_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


INTER_LINEAR, BORDER_CONSTANT, CV_32FC1 = 1, 0, 5  # the OpenCV constants the reference passes (src/camera.cpp:41,71-72)


class CameraPyramid:
    """ref: include/camera.h:16-119 — raw calibration, rectified intrinsics per pyramid level, undistort + rectify."""

    def __init__(self, levels, fx, fy, f_theta, cx, cy, k1, k2, r1, r2, sensor_width, sensor_height, resolution_width,
                 resolution_height, ctx=None):
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        L.check(self.ctx.lib.odo_camera_create(self.ctx.h, levels, fx, fy, f_theta, cx, cy, k1, k2, r1, r2, sensor_width,
                                               sensor_height, resolution_width, resolution_height, C.byref(h)),
                "odo_camera_create")
        self.h = h
        self.levels_ = levels
        self.sensor_width_, self.sensor_height_ = float(sensor_width), float(sensor_height)
        self.resolution_width_, self.resolution_height_ = int(resolution_width), int(resolution_height)
        self.pixels_per_mm_x_ = resolution_width / sensor_width    # ref: src/camera.cpp:36-37
        self.pixels_per_mm_y_ = resolution_height / sensor_height

    def ConfigureCamera(self, rectify_rotation, new_intrinsic, new_size, map_type=CV_32FC1, use_int_map=False):
        """ref: src/camera.cpp:40-69. new_size = (width, height) like cv::Size; only CV_32FC1 float maps exist."""
        if map_type != CV_32FC1 or use_int_map:
            raise ValueError("only CV_32FC1 floating-point maps are implemented (the reference's defaults)")
        R = np.ascontiguousarray(rectify_rotation, np.float64).reshape(9)
        P = np.ascontiguousarray(new_intrinsic, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        L.check(self.ctx.lib.odo_camera_configure(self.h, R.ctypes.data_as(dp), P.ctypes.data_as(dp), int(new_size[0]),
                                                  int(new_size[1])), "odo_camera_configure")

    def UndistortRectify(self, src_raw, dst, interpolation=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0.0,
                         any_size=False):
        """ref: src/camera.cpp:71-82. dst: float32 array of the configured size, filled in place. Returns 0 / -1.
        any_size=False keeps the reference's hard 480x640 check (:74-77)."""
        src = _f32(src_raw)
        if not any_size and (src.shape[0] != 480 or src.shape[1] != 640):
            print("camera raw image is not 480x640!")
            return -1
        if interpolation != INTER_LINEAR or borderMode != BORDER_CONSTANT:
            raise ValueError("only INTER_LINEAR / BORDER_CONSTANT are implemented (the reference's defaults)")
        st = self.ctx.lib.odo_camera_undistort_rectify(self.h, _fp(src), src.shape[0], src.shape[1], _fp(dst),
                                                       C.c_float(borderValue))
        return 0 if st == 0 else -1

    def maps(self):
        r, c = C.c_int(0), C.c_int(0)
        L.check(self.ctx.lib.odo_camera_map_size(self.h, C.byref(r), C.byref(c)), "odo_camera_map_size")
        mx, my = np.empty((r.value, c.value), np.float32), np.empty((r.value, c.value), np.float32)
        L.check(self.ctx.lib.odo_camera_download_maps(self.h, _fp(mx), _fp(my)), "odo_camera_download_maps")
        return mx, my

    def _intr(self, level):
        out = (C.c_double * 5)()
        L.check(self.ctx.lib.odo_camera_intrinsics(self.h, level, out), "odo_camera_intrinsics")
        return list(out)

    # accessors, ref: include/camera.h:73-85
    def fx_double(self, level): return self._intr(level)[0]
    def fy_double(self, level): return self._intr(level)[1]
    def f_theta_double(self, level): return self._intr(level)[2]
    def cx_double(self, level): return self._intr(level)[3]
    def cy_double(self, level): return self._intr(level)[4]
    def f_meters_double(self, level): return self._intr(level)[0] / self.pixels_per_mm_x_
    def fx_float(self, level): return float(np.float32(self.fx_double(level)))
    def fy_float(self, level): return float(np.float32(self.fy_double(level)))
    def f_theta_float(self, level): return float(np.float32(self.f_theta_double(level)))
    def cx_float(self, level): return float(np.float32(self.cx_double(level)))
    def cy_float(self, level): return float(np.float32(self.cy_double(level)))

    def close(self):
        if self.h:
            self.ctx.lib.odo_camera_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeyFrame:
    """ref: include/keyframe.h:17-60 — holder of four images and an absolute pose."""

    def __init__(self, kLeftImg, kRightImg, kLeftDep, kLeftVal, kAbsoPose):
        self.left_img_ptr_, self.right_img_ptr_ = kLeftImg, kRightImg
        self.left_dep_ptr_, self.left_val_ptr_ = kLeftDep, kLeftVal
        self.abso_pose_ = np.array(kAbsoPose, np.float32)

    def GetLeftImg(self):
        return self.left_img_ptr_

    def GetRightImg(self):
        return self.right_img_ptr_

    def GetLeftDep(self):
        return self.left_dep_ptr_

    def GetLeftVal(self):
        return self.left_val_ptr_

    def GetAbsoPose(self):
        return self.abso_pose_.copy()

    def ModifyLeftDep(self):
        return self.left_dep_ptr_

    def ModifyLeftVal(self):
        return self.left_val_ptr_

    def ModifyAbsoPose(self):
        return self.abso_pose_


class Tracker:
    """The runner's frame loop (ref: run_odometry_kitti_offline.cpp:58-145, 198-271) over odo_tracker_*.
    Frames are device-resident: upload them once with `upload_frame` and pass the handles to init/track."""

    def __init__(self, device=0, **overrides):
        self.lib = L.load()
        self.params = self._params(overrides)
        h = C.c_void_p()
        L.check(self.lib.odo_tracker_create(device, C.byref(self.params), C.byref(h)), "odo_tracker_create")
        self.h = h
        self._ctx = C.c_void_p(self.lib.odo_tracker_ctx(h))
        self._bufs = []

    def _params(self, overrides):
        params = L.TrackerParams()
        L.check(self.lib.odo_tracker_default_params(C.byref(params)), "odo_tracker_default_params")
        for k, v in overrides.items():
            if k == "lm_max_iters":
                for i, m in enumerate(v):
                    params.lm_max_iters[i] = m
            elif k == "K":
                params.K = L.Intrinsics(*v)
            else:
                setattr(params, k, v)
        return params

    def upload_frame(self, img):
        img = _f32(img)
        p = C.c_void_p()
        L.check(self.lib.odo_dev_alloc(self._ctx, img.nbytes, C.byref(p)), "odo_dev_alloc")
        L.check(self.lib.odo_dev_upload(self._ctx, p, img.ctypes.data_as(C.c_void_p), img.nbytes), "odo_dev_upload")
        self._bufs.append(p)
        return p

    def init(self, left_dev, right_dev, abs_pose0=None):
        pose = _colmajor(np.eye(4) if abs_pose0 is None else abs_pose0)
        L.check(self.lib.odo_tracker_init(self.h, left_dev, right_dev, _fp(pose)), "odo_tracker_init")

    def track(self, left_dev, right_dev):
        T = np.zeros(16, np.float32)
        A = np.zeros(16, np.float32)
        nk, ss = C.c_int(0), C.c_int(0)
        mag = C.c_float(0)
        st = self.lib.odo_tracker_track(self.h, left_dev, right_dev, _fp(T), _fp(A), C.byref(nk), C.byref(mag),
                                        C.byref(ss))
        if st != 0:
            raise L.OdoError("odo_tracker_track: " + L.last_error())
        return dict(pose_to_keyframe=_from_colmajor(T), abs_pose=_from_colmajor(A), new_keyframe=bool(nk.value),
                    motion=mag.value, solve_status=ss.value)

    def hint_next(self, next_left_dev, next_right_dev=None):
        """Announce the next frame: left image only (pyramid prefetch + early start of the next Solve) or the pair (the depth
        stream then works a frame ahead as well)."""
        if next_right_dev is None:
            L.check(self.lib.odo_tracker_hint_next(self.h, next_left_dev), "odo_tracker_hint_next")
        else:
            L.check(self.lib.odo_tracker_hint_next_pair(self.h, next_left_dev, next_right_dev), "odo_tracker_hint_next_pair")

    def track_into(self, left_dev, right_dev, pose_to_kf, abs_pose):
        """Lean variant for timing loops: results land in caller-owned float32[16] column-major buffers."""
        if not hasattr(self, "_nk"):
            self._nk, self._ss, self._mag = C.c_int(0), C.c_int(0), C.c_float(0)
        st = self.lib.odo_tracker_track(self.h, left_dev, right_dev, _fp(pose_to_kf), _fp(abs_pose), C.byref(self._nk),
                                        C.byref(self._mag), C.byref(self._ss))
        if st != 0:
            raise L.OdoError("odo_tracker_track: " + L.last_error())
        return self._nk.value

    def stats(self):
        a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        L.check(self.lib.odo_tracker_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "odo_tracker_stats")
        return dict(lm_evals=a.value, depth_iters=b.value, n_valid_depth=c.value, n_keyframes=d.value)

    def outputs(self, rows, cols):
        v, dsp, dep = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(self.lib.odo_tracker_outputs(self.h, C.byref(v), C.byref(dsp), C.byref(dep)), "odo_tracker_outputs")
        out = []
        for ptr, dt in ((v, np.uint8), (dsp, np.float32), (dep, np.float32)):
            a = np.empty((rows, cols), dt)
            L.check(self.lib.odo_dev_download(self._ctx, a.ctypes.data_as(C.c_void_p), ptr, a.nbytes), "download")
            out.append(a)
        return out

    def event_timing(self, on):
        lm = C.c_void_p(self.lib.odo_tracker_lm(self.h))
        L.check(self.lib.odo_lm_event_timing(lm, int(on)), "odo_lm_event_timing")

    def event_stats(self):
        lm = C.c_void_p(self.lib.odo_tracker_lm(self.h))
        us, b = C.c_double(0), C.c_double(0)
        n, a = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_lm_event_stats(lm, C.byref(us), C.byref(n), C.byref(a), C.byref(b)), "odo_lm_event_stats")
        cu, cn = C.c_double(0), C.c_long(0)
        L.check(self.lib.odo_lm_event_stats2(lm, C.byref(cu), C.byref(cn)), "odo_lm_event_stats2")
        return dict(total_us=us.value, launches=n.value, active_launches=a.value, bytes=b.value,
                    coarse_us=cu.value, coarse_launches=cn.value)

    def _sync(self):
        """All three streams of the tracker idle (end of a timed region)."""
        L.check(self.lib.odo_tracker_quiesce(self.h), "odo_tracker_quiesce")

    def event_stats_ex(self):
        """Sampled event timing (event_timing(N)): mean launch durations of the two LM kernels + launch / evaluation counts."""
        lm = C.c_void_p(self.lib.odo_tracker_lm(self.h))
        o = (C.c_double * 12)()
        L.check(self.lib.odo_lm_event_stats_ex(lm, o), "odo_lm_event_stats_ex")
        return dict(step_us=o[0], step_sampled=int(o[1]), coarse_us=o[2], coarse_sampled=int(o[3]), launches=int(o[4]),
                    coarse_launches=int(o[5]), evaluations=int(o[6]), bytes=o[7], step_period_us=o[8], step_periods=int(o[9]),
                    coarse_period_us=o[10], coarse_periods=int(o[11]))

    def persistent_stats(self):
        """(workgroups of the pose LM's persistent fine-level launch — 0: step launches —, Solves redone on the step launches)"""
        lm = C.c_void_p(self.lib.odo_tracker_lm(self.h))
        k, f = C.c_int(0), C.c_int(0)
        L.check(self.lib.odo_lm_persistent_stats(lm, C.byref(k), C.byref(f)), "odo_lm_persistent_stats")
        return k.value, f.value

    def chain_stats(self):
        """(Solves that started on the device behind the Solve before them, chained Solves that ran for nothing)"""
        a, b = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_tracker_chain_stats(self.h, C.byref(a), C.byref(b)), "odo_tracker_chain_stats")
        return a.value, b.value

    def arm_stats(self):
        """(Solves that started armed — coarse launch queued ahead, started by the host's word —, armed launches told to return)"""
        a, b = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_tracker_arm_stats(self.h, C.byref(a), C.byref(b)), "odo_tracker_arm_stats")
        return a.value, b.value

    def depth_persistent_stats(self):
        """(1 while the depth LM runs as one persistent launch, ComputeDepth jobs run again on the step launches)"""
        d = C.c_void_p(self.lib.odo_tracker_depth(self.h))
        a, b = C.c_int(0), C.c_int(0)
        L.check(self.lib.odo_depth_persistent_stats(d, C.byref(a), C.byref(b)), "odo_depth_persistent_stats")
        return a.value, b.value

    def lm_points(self):
        """Points per pyramid level of the current keyframe's lists (level 0 first) and the launches of the last Solve."""
        lm = C.c_void_p(self.lib.odo_tracker_lm(self.h))
        n = (C.c_int * L.MAX_LEVELS)()
        u = (C.c_int * L.MAX_LEVELS)()
        L.check(self.lib.odo_lm_points(lm, n, u), "odo_lm_points")
        a, t, b = C.c_int(0), C.c_int(0), C.c_double(0)
        L.check(self.lib.odo_lm_launch_stats(lm, C.byref(a), C.byref(t), C.byref(b)), "odo_lm_launch_stats")
        return list(n)[:self.params.levels], t.value

    def timing(self):
        out = (C.c_double * 4)()
        L.check(self.lib.odo_tracker_timing(self.h, out), "odo_tracker_timing")
        return dict(frame_us=out[0], solve_us=out[1], depth_job_us=out[2], wait_helper_us=out[3])

    def time_residual(self, level, reps=50):
        mean, mn, b, n = C.c_float(0), C.c_float(0), C.c_double(0), C.c_int(0)
        L.check(self.lib.odo_tracker_time_residual(self.h, level, reps, C.byref(mean), C.byref(mn), C.byref(b),
                                                   C.byref(n)), "odo_tracker_time_residual")
        return dict(mean_us=mean.value, min_us=mn.value, bytes=b.value, n_points=n.value)

    def attach_map(self, m):
        """Every keyframe from now on goes into PointMap `m` (None detaches; pending insertions complete first)."""
        L.check(self.lib.odo_tracker_attach_map(self.h, m.h if m is not None else None), "odo_tracker_attach_map")
        if getattr(self, "_map", None) is not None and self._map is not m:
            self._map._tracker = None
        self._map = m
        if m is not None:
            m._tracker = self

    def close(self):
        if getattr(self, "h", None):
            # frames announced with hint_next may still be read by launches the helper thread has yet to issue (the job posted
            # ahead, the prefetched pyramid, an early Solve): quiesce first, free the frames, then destroy (the buffers come
            # from the tracker's own context, so they cannot outlive it)
            self.lib.odo_tracker_quiesce(self.h)
            for p in self._bufs:
                self.lib.odo_dev_free(self._ctx, p)
            self._bufs = []
            self.lib.odo_tracker_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RgbdTracker(Tracker):
    """The frame loop with sensor depth (odo_tracker_create_rgbd): a grey image and a uint16 depth frame per frame instead of a
    stereo pair. depth_scale: raw units per metre (TUM 5000, RealSense 1000); max_depth_step: the edge guard's relative step
    (float("inf"): off). Everything else — overrides, outputs, stats, timing, attach_map — as Tracker."""

    def __init__(self, device=0, depth_scale=5000.0, max_depth_step=0.05, **overrides):
        self.lib = L.load()
        self.params = self._params(overrides)
        h = C.c_void_p()
        L.check(self.lib.odo_tracker_create_rgbd(device, C.byref(self.params), float(depth_scale), float(max_depth_step), C.byref(h)),
                "odo_tracker_create_rgbd")
        self.h = h
        self._ctx = C.c_void_p(self.lib.odo_tracker_ctx(h))
        self._bufs = []
        self.depth_scale, self.max_depth_step = float(depth_scale), float(max_depth_step)

    def upload_depth(self, raw):
        """A uint16 depth frame (rows x cols) into a device buffer owned by the tracker."""
        raw = np.ascontiguousarray(raw, np.uint16)
        p = C.c_void_p()
        L.check(self.lib.odo_dev_alloc(self._ctx, raw.nbytes, C.byref(p)), "odo_dev_alloc")
        L.check(self.lib.odo_dev_upload(self._ctx, p, raw.ctypes.data_as(C.c_void_p), raw.nbytes), "odo_dev_upload")
        self._bufs.append(p)
        return p

    def upload_colour(self, colour):
        """An interleaved uint8 colour frame (rows x cols x 3 | 4) into a device buffer owned by the tracker: a handle for
        frame_colour."""
        colour = np.ascontiguousarray(colour, np.uint8)
        p = C.c_void_p()
        L.check(self.lib.odo_dev_alloc(self._ctx, colour.nbytes, C.byref(p)), "odo_dev_alloc")
        L.check(self.lib.odo_dev_upload(self._ctx, p, colour.ctypes.data_as(C.c_void_p), colour.nbytes), "odo_dev_upload")
        self._bufs.append(p)
        return p

    def init(self, gray_dev, depth_dev, abs_pose0=None):
        pose = _colmajor(np.eye(4) if abs_pose0 is None else abs_pose0)
        L.check(self.lib.odo_tracker_init_rgbd(self.h, gray_dev, depth_dev, _fp(pose)), "odo_tracker_init_rgbd")

    def track(self, gray_dev, depth_dev):
        T = np.zeros(16, np.float32)
        A = np.zeros(16, np.float32)
        nk, ss = C.c_int(0), C.c_int(0)
        mag = C.c_float(0)
        st = self.lib.odo_tracker_track_rgbd(self.h, gray_dev, depth_dev, _fp(T), _fp(A), C.byref(nk), C.byref(mag), C.byref(ss))
        if st != 0:
            raise L.OdoError("odo_tracker_track_rgbd: " + L.last_error())
        return dict(pose_to_keyframe=_from_colmajor(T), abs_pose=_from_colmajor(A), new_keyframe=bool(nk.value),
                    motion=mag.value, solve_status=ss.value)

    def hint_next(self, gray_dev, depth_dev=None):
        """Announce the next frame: grey image only (pyramid prefetch + early start of the next Solve) or with its depth frame (the
        depth stream then works a frame ahead as well)."""
        if depth_dev is None:
            L.check(self.lib.odo_tracker_hint_next(self.h, gray_dev), "odo_tracker_hint_next")
        else:
            L.check(self.lib.odo_tracker_hint_next_rgbd(self.h, gray_dev, depth_dev), "odo_tracker_hint_next_rgbd")

    def track_into(self, gray_dev, depth_dev, pose_to_kf, abs_pose):
        """Lean variant for timing loops: results land in caller-owned float32[16] column-major buffers."""
        if not hasattr(self, "_nk"):
            self._nk, self._ss, self._mag = C.c_int(0), C.c_int(0), C.c_float(0)
        st = self.lib.odo_tracker_track_rgbd(self.h, gray_dev, depth_dev, _fp(pose_to_kf), _fp(abs_pose), C.byref(self._nk),
                                             C.byref(self._mag), C.byref(self._ss))
        if st != 0:
            raise L.OdoError("odo_tracker_track_rgbd: " + L.last_error())
        return self._nk.value

    def attach_volume(self, v):
        """Every frame with a good pose from now on is integrated into TsdfVolume `v` (None detaches; pending integrations complete
        first). A tracked frame's depth buffer must then stay unchanged until the next track / init / close has returned."""
        L.check(self.lib.odo_tracker_attach_volume(self.h, v.h if v is not None else None), "odo_tracker_attach_volume")
        if getattr(self, "_vol", None) is not None and self._vol is not v:
            self._vol._tracker = None
        self._vol = v
        if v is not None:
            v._tracker = self

    def frame_colour(self, colour_dev):
        """Names the device colour frame of the frame the next init / track gets: with a colour-enabled TsdfVolume attached, that
        frame's integration is the coloured one. The buffer follows the depth buffer's rule (unchanged until the next track / init /
        close has returned)."""
        L.check(self.lib.odo_tracker_frame_colour(self.h, colour_dev), "odo_tracker_frame_colour")

    def depth_report(self):
        """The last frame's depth statistics (odo_depth_report): iters, cost, n_selected, n_matched, n_valid."""
        d = C.c_void_p(self.lib.odo_tracker_depth(self.h))
        it, n1, n2, n3 = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        cost = C.c_float(0)
        L.check(self.lib.odo_depth_report(d, C.byref(it), C.byref(cost), C.byref(n1), C.byref(n2), C.byref(n3)), "odo_depth_report")
        return dict(iters=it.value, cost=cost.value, n_selected=n1.value, n_matched=n2.value, n_valid=n3.value)


class PointMap:
    """Device-resident keyframe point cloud with voxel filtering (odo_map_*; replaces GlobalMap and save_to_vis' export).
    ctx_or_tracker: a Context, or a Tracker whose stream standalone insertions then use (attach with Tracker.attach_map)."""

    def __init__(self, ctx_or_tracker, rows, cols, capacity, voxel_size):
        self.lib = L.load()
        self._owner = ctx_or_tracker   # keeps the stream's owner alive as long as the map
        ctx = ctx_or_tracker._ctx if isinstance(ctx_or_tracker, Tracker) else ctx_or_tracker.h
        self.rows, self.cols = rows, cols
        self._ctx = ctx
        self._tracker = None
        h = C.c_void_p()
        L.check(self.lib.odo_map_create(ctx, rows, cols, capacity, voxel_size, C.byref(h)), "odo_map_create")
        self.h = h

    def _dev(self, a, dtype):
        """A device handle as is; a numpy array uploaded into a temporary buffer (freed once the insertion has read it)."""
        if a is None:
            return None, None
        if isinstance(a, np.ndarray):
            a = np.ascontiguousarray(a, dtype=dtype)
            assert a.shape == (self.rows, self.cols), a.shape
            p = C.c_void_p()
            L.check(self.lib.odo_dev_alloc(self._ctx, a.nbytes, C.byref(p)), "odo_dev_alloc")
            L.check(self.lib.odo_dev_upload(self._ctx, p, a.ctypes.data_as(C.c_void_p), a.nbytes), "odo_dev_upload")
            return p, p
        return a, None

    def insert(self, val, dep, img, K, abs_pose):
        """One keyframe (GlobalMap::InsertKeyFrame): numpy arrays (uploaded) or device handles; val / img may be None.
        K = (f0, cx0, cy0) or None (KITTI-00); abs_pose = 4x4 camera-to-world."""
        tmp = []
        try:
            ptrs = []
            for a, dt in ((val, np.uint8), (dep, np.float32), (img, np.float32)):
                p, t = self._dev(a, dt)
                ptrs.append(p)
                if t is not None:
                    tmp.append(t)
            k = C.byref(L.Intrinsics(*K)) if K is not None else None
            pose = _colmajor(abs_pose)
            L.check(self.lib.odo_map_insert_dev(self.h, ptrs[0], ptrs[1], ptrs[2], k, _fp(pose)), "odo_map_insert_dev")
        finally:
            for p in tmp:   # odo_dev_free waits for the context's stream: the insertion has read them
                self.lib.odo_dev_free(self._ctx, p)

    def __len__(self):
        n = self.lib.odo_map_size(self.h)
        if n < 0:
            raise L.OdoError("odo_map_size: " + L.last_error())
        return n

    def points(self):
        """(N, 4) float32 x, y, z, intensity in world coordinates and (N, 2) int32 keyframe, pixel."""
        n = len(self)
        xyzi = np.zeros((n, 4), np.float32)
        kp = np.zeros((n, 2), np.int32)
        L.check(self.lib.odo_map_download(self.h, 0, n, _fp(xyzi), kp.ctypes.data_as(C.POINTER(C.c_int))), "odo_map_download")
        return xyzi, kp

    def stats(self):
        o = (C.c_long * 6)()
        L.check(self.lib.odo_map_stats(self.h, o), "odo_map_stats")
        return dict(zip(("size", "insertions", "candidates", "dropped_voxel", "dropped_range", "dropped_capacity"), list(o)))

    def keyframe_pose(self, i):
        v = np.zeros(16, np.float32)
        L.check(self.lib.odo_map_keyframe_pose(self.h, i, _fp(v)), "odo_map_keyframe_pose")
        return _from_colmajor(v)

    def clear(self):
        L.check(self.lib.odo_map_clear(self.h), "odo_map_clear")

    def save_ply(self, path):
        """Binary little-endian PLY: float x y z, uchar red green blue (the intensity clamped to 0..255)."""
        xyzi, _ = self.points()
        write_ply(path, xyzi)

    def close(self):
        if getattr(self, "h", None):
            if self._tracker is not None and getattr(self._tracker, "h", None):
                self._tracker.attach_map(None)
            self.lib.odo_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TsdfVolume:
    """Device-resident truncated signed distance volume (odo_volume_*): depth frames with known poses fused into a dense grid, the
    surface read back as oriented points. ctx_or_tracker: a Context, or a Tracker whose stream standalone integrations then use
    (attach with RgbdTracker.attach_volume). dims = (nx, ny, nz), origin = the grid's minimum corner (world, metres), size = (rows,
    cols) of the depth frames, K = (f0, cx0, cy0), depth_scale: raw units per metre."""

    STATS = ("frames", "updated", "in_band", "cumulative")

    def __init__(self, ctx_or_tracker, dims, voxel_size, origin, mu, max_depth, max_weight, size, K, depth_scale):
        self.lib = L.load()
        self._owner = ctx_or_tracker   # keeps the stream's owner alive as long as the volume
        ctx = ctx_or_tracker._ctx if isinstance(ctx_or_tracker, Tracker) else ctx_or_tracker.h
        self._ctx = ctx
        self._tracker = None
        self._follow = None           # (focus, threshold) while set_follow is on
        self._spill_capacity = 0
        self._spill_colour = False
        self._spill_mesh_colour = False
        self._has_spill_mesh = False
        p = L.VolumeParams()
        p.nx, p.ny, p.nz = dims
        p.voxel_size = voxel_size
        for i in range(3):
            p.origin[i] = origin[i]
        p.mu, p.max_depth, p.max_weight = mu, max_depth, max_weight
        p.rows, p.cols = size
        p.K = L.Intrinsics(*K)
        p.depth_scale = depth_scale
        self.params = p
        self.dims = (p.nx, p.ny, p.nz)
        self.rows, self.cols = p.rows, p.cols
        h = C.c_void_p()
        L.check(self.lib.odo_volume_create(ctx, C.byref(p), C.byref(h)), "odo_volume_create")
        self.h = h

    def enable_colour(self, channels=3, bgr=False, max_weight=255):
        """Adds the colour grid (4 B per voxel more): colour frames are rows x cols x channels uint8, RGB(A) or BGR(A); max_weight
        (1 .. 255) caps the colour's running average. Once, and not while attached to a tracker."""
        cp = L.VolumeColourParams(int(channels), int(bool(bgr)), int(max_weight))
        L.check(self.lib.odo_volume_enable_colour(self.h, C.byref(cp)), "odo_volume_enable_colour")
        self.colour_params = cp

    @property
    def has_colour(self):
        return getattr(self, "colour_params", None) is not None

    def _integrate_colour(self, depth, pose, colour):
        if not self.has_colour:
            raise L.OdoError("TsdfVolume.integrate: the volume has no colour grid (enable_colour first)")
        if isinstance(depth, np.ndarray) != isinstance(colour, np.ndarray):
            raise TypeError("depth and colour must both be numpy arrays or both be device handles")
        if not isinstance(depth, np.ndarray):
            L.check(self.lib.odo_volume_integrate_colour_dev(self.h, depth, colour, _fp(pose)), "odo_volume_integrate_colour_dev")
            return
        depth = np.ascontiguousarray(depth, np.uint16)
        assert depth.shape == (self.rows, self.cols), depth.shape
        if colour.dtype != np.uint8 or colour.shape != (self.rows, self.cols, self.colour_params.channels):
            raise ValueError(f"colour frame {colour.dtype} {colour.shape}")
        colour = np.ascontiguousarray(colour)
        bufs = []
        try:
            for a in (depth, colour):
                p = C.c_void_p()
                L.check(self.lib.odo_dev_alloc(self._ctx, a.nbytes, C.byref(p)), "odo_dev_alloc")
                bufs.append(p)
                L.check(self.lib.odo_dev_upload(self._ctx, p, a.ctypes.data_as(C.c_void_p), a.nbytes), "odo_dev_upload")
            L.check(self.lib.odo_volume_integrate_colour_dev(self.h, bufs[0], bufs[1], _fp(pose)), "odo_volume_integrate_colour_dev")
        finally:   # odo_dev_free waits for the context's stream: the integration has read the frames
            for p in bufs:
                self.lib.odo_dev_free(self._ctx, p)

    def integrate(self, depth, abs_pose, colour=None):
        """One depth frame: a uint16 numpy array (uploaded into a temporary buffer) or a device handle; abs_pose = 4x4 camera-to-world.
        colour (a volume with enable_colour): the frame's colour pixels, a numpy array or a device handle like depth; the voxels of
        the band then take their colour from it."""
        pose = _colmajor(abs_pose)
        if colour is not None:
            return self._integrate_colour(depth, pose, colour)
        if isinstance(depth, np.ndarray):
            depth = np.ascontiguousarray(depth, np.uint16)
            assert depth.shape == (self.rows, self.cols), depth.shape
            p = C.c_void_p()
            L.check(self.lib.odo_dev_alloc(self._ctx, depth.nbytes, C.byref(p)), "odo_dev_alloc")
            try:
                L.check(self.lib.odo_dev_upload(self._ctx, p, depth.ctypes.data_as(C.c_void_p), depth.nbytes), "odo_dev_upload")
                L.check(self.lib.odo_volume_integrate_dev(self.h, p, _fp(pose)), "odo_volume_integrate_dev")
            finally:   # odo_dev_free waits for the context's stream: the integration has read the frame
                self.lib.odo_dev_free(self._ctx, p)
        else:
            L.check(self.lib.odo_volume_integrate_dev(self.h, depth, _fp(pose)), "odo_volume_integrate_dev")

    def sync(self):
        L.check(self.lib.odo_volume_sync(self.h), "odo_volume_sync")

    def extract(self, capacity=1 << 20, with_dropped=False, colour=False):
        """The surface: (n, 4) float32 x, y, z, 0 and (n, 4) float32 nx, ny, nz, weight, at most `capacity` points (colour: also
        (n, 4) uint8 R, G, B, A; with_dropped: also the number of points beyond the capacity)."""
        xyz0 = np.zeros((max(capacity, 1), 4), np.float32)
        nrmw = np.zeros((max(capacity, 1), 4), np.float32)
        n, d = C.c_long(0), C.c_long(0)
        if colour:
            rgba = np.zeros((max(capacity, 1), 4), np.uint8)
            L.check(self.lib.odo_volume_extract_colour(self.h, capacity, _fp(xyz0), _fp(nrmw), rgba.ctypes.data_as(L._u8p), C.byref(n),
                                                       C.byref(d)), "odo_volume_extract_colour")
            out = xyz0[:n.value].copy(), nrmw[:n.value].copy(), rgba[:n.value].copy()
        else:
            L.check(self.lib.odo_volume_extract(self.h, capacity, _fp(xyz0), _fp(nrmw), C.byref(n), C.byref(d)), "odo_volume_extract")
            out = xyz0[:n.value].copy(), nrmw[:n.value].copy()
        return out + (d.value,) if with_dropped else out

    def colour_grid(self):
        """(nz, ny, nx, 4) uint8: R, G, B and the colour weight of every voxel."""
        nx, ny, nz = self.dims
        c = np.zeros((nz, ny, nx, 4), np.uint8)
        L.check(self.lib.odo_volume_download_colour(self.h, c.ctypes.data_as(L._u8p)), "odo_volume_download_colour")
        return c

    def upload_colour(self, rgbw):
        """The whole colour grid from the host: (nz, ny, nx, 4) uint8 (what colour_grid() returns). Refused while attached."""
        nx, ny, nz = self.dims
        rgbw = np.ascontiguousarray(rgbw, np.uint8)
        assert rgbw.shape == (nz, ny, nx, 4), rgbw.shape
        L.check(self.lib.odo_volume_upload_colour(self.h, rgbw.ctypes.data_as(L._u8p)), "odo_volume_upload_colour")

    def grid(self):
        """(q int16, w uint16), each of shape (nz, ny, nx)."""
        nx, ny, nz = self.dims
        q = np.zeros((nz, ny, nx), np.int16)
        w = np.zeros((nz, ny, nx), np.uint16)
        L.check(self.lib.odo_volume_download(self.h, q.ctypes.data_as(C.POINTER(C.c_int16)), w.ctypes.data_as(C.POINTER(C.c_uint16))),
                "odo_volume_download")
        return q, w

    def upload(self, q, w):
        """The whole grid from the host: q int16 and w uint16 of shape (nz, ny, nx) (what grid() returns). Refused while attached."""
        nx, ny, nz = self.dims
        q = np.ascontiguousarray(q, np.int16)
        w = np.ascontiguousarray(w, np.uint16)
        assert q.shape == (nz, ny, nx) and w.shape == (nz, ny, nx), (q.shape, w.shape)
        L.check(self.lib.odo_volume_upload(self.h, q.ctypes.data_as(C.POINTER(C.c_int16)), w.ctypes.data_as(C.POINTER(C.c_uint16))),
                "odo_volume_upload")

    def mesh_counts(self):
        """(vertices, triangles) of the mesh, nothing written."""
        o = (C.c_long * 4)()
        L.check(self.lib.odo_volume_mesh(self.h, 0, 0, None, None, None, o), "odo_volume_mesh")
        return o[1], o[3]

    def mesh(self, vertex_capacity=None, triangle_capacity=None, with_counts=False, colour=False):
        """The surface as triangles (marching tetrahedra): (n, 4) float32 x, y, z, e; (n, 4) float32 nx, ny, nz, weight; (m, 3) int32
        vertex indices, counter-clockwise seen from free space. Without capacities it asks for the totals first and then calls with
        exact ones; with them the first `capacity` items are returned, indices unchanged (with_counts: also the four counts).
        colour: (n, 4) uint8 R, G, B, A per vertex as one more array behind the indices."""
        if vertex_capacity is None or triangle_capacity is None:
            nv, nt = self.mesh_counts()
            vertex_capacity = nv if vertex_capacity is None else vertex_capacity
            triangle_capacity = nt if triangle_capacity is None else triangle_capacity
        xyz0 = np.zeros((max(vertex_capacity, 1), 4), np.float32)
        nrmw = np.zeros((max(vertex_capacity, 1), 4), np.float32)
        tri = np.zeros((max(triangle_capacity, 1), 3), np.int32)
        o = (C.c_long * 4)()
        if colour:
            rgba = np.zeros((max(vertex_capacity, 1), 4), np.uint8)
            L.check(self.lib.odo_volume_mesh_colour(self.h, vertex_capacity, triangle_capacity, _fp(xyz0), _fp(nrmw),
                                                    rgba.ctypes.data_as(L._u8p), tri.ctypes.data_as(C.POINTER(C.c_int32)), o),
                    "odo_volume_mesh_colour")
            out = xyz0[:o[0]].copy(), nrmw[:o[0]].copy(), tri[:o[2]].copy(), rgba[:o[0]].copy()
        else:
            L.check(self.lib.odo_volume_mesh(self.h, vertex_capacity, triangle_capacity, _fp(xyz0), _fp(nrmw),
                                             tri.ctypes.data_as(C.POINTER(C.c_int32)), o), "odo_volume_mesh")
            out = xyz0[:o[0]].copy(), nrmw[:o[0]].copy(), tri[:o[2]].copy()
        return out + (tuple(o),) if with_counts else out

    def raycast_params(self, size=None, K=None, t_min=0.0, step=None, n_steps=None):
        """The odo_raycast_params of raycast(): the volume's own size and K, step = mu / 2 and enough samples to reach
        max_depth + mu unless given."""
        p = self.params
        rows, cols = (p.rows, p.cols) if size is None else size
        f, cx, cy = (p.K.f0, p.K.cx0, p.K.cy0) if K is None else K
        step = p.mu / 2 if step is None else step
        if n_steps is None:
            n_steps = min(4096, max(1, int(np.ceil((p.max_depth + p.mu - t_min) / step)) + 1))
        return L.RaycastParams(int(rows), int(cols), f, cx, cy, t_min, step, int(n_steps))

    def raycast(self, abs_pose, size=None, K=None, t_min=0.0, step=None, n_steps=None, raw=False, colour=False):
        """The volume seen from the camera-to-world pose abs_pose (4x4): depth (rows, cols) float32, metres along the optical axis, 0 =
        no surface; normals (rows, cols, 4) float32 nx, ny, nz in world axes and the smallest weight of the cell; with raw=True also
        the depth as a uint16 frame in the volume's depth_scale (what integrate and RgbdTracker take); with colour=True also
        (rows, cols, 4) uint8 R, G, B, A. size = (rows, cols) and K = (f, cx, cy) of the view: the volume's own unless given; rays
        are sampled at t_min + n * step, n < n_steps."""
        rp = self.raycast_params(size, K, t_min, step, n_steps)
        depth = np.zeros((rp.rows, rp.cols), np.float32)
        nrmw = np.zeros((rp.rows, rp.cols, 4), np.float32)
        raw_out = np.zeros((rp.rows, rp.cols), np.uint16) if raw else None
        rgba = np.zeros((rp.rows, rp.cols, 4), np.uint8) if colour else None
        L.check(self.lib.odo_volume_raycast(self.h, C.byref(rp), _fp(_colmajor(abs_pose)), _fp(depth),
                                            raw_out.ctypes.data_as(C.POINTER(C.c_uint16)) if raw else None, _fp(nrmw),
                                            rgba.ctypes.data_as(L._u8p) if colour else None), "odo_volume_raycast")
        out = (depth, nrmw)
        if raw:
            out += (raw_out,)
        if colour:
            out += (rgba,)
        return out

    def raycast_time(self, abs_pose, size=None, K=None, t_min=0.0, step=None, n_steps=None, colour=False, reps=20):
        """Microseconds per ray-cast: `reps` of them between two events on the volume's stream (odo_volume_raycast_time), with the
        colour frame if colour, under the colour sampling mode as it is."""
        rp = self.raycast_params(size, K, t_min, step, n_steps)
        us = C.c_float(0)
        L.check(self.lib.odo_volume_raycast_time(self.h, C.byref(rp), _fp(_colmajor(abs_pose)), int(bool(colour)), int(reps), C.byref(us)),
                "odo_volume_raycast_time")
        return us.value

    COLOUR_SAMPLING = ("nearest", "trilinear")

    def set_colour_sampling(self, mode):
        """How the ray-cast's colour frame samples the colour grid: "nearest" (the voxel nearest to the hit, the state at create) or
        "trilinear" (the average of the hit cell's coloured corners). raycast(colour=True) and track(grey=...) follow it from the next
        call on; depth and normals do not depend on it. Refused on a volume without a colour grid."""
        if mode not in self.COLOUR_SAMPLING:
            raise ValueError(f"colour sampling {mode!r}: one of {self.COLOUR_SAMPLING}")
        L.check(self.lib.odo_volume_set_colour_sampling(self.h, self.COLOUR_SAMPLING.index(mode)), "odo_volume_set_colour_sampling")

    @property
    def colour_sampling(self):
        mode = self.lib.odo_volume_colour_sampling(self.h)
        L.check(min(mode, 0), "odo_volume_colour_sampling")
        return self.COLOUR_SAMPLING[mode]

    # ---- frame-to-model tracking (odo_volume_icp_*, odo_volume_track_dev) ----
    ICP_STATUS = ("aligned", "too few pairs", "rank-deficient")
    # Default of min_eig_ratio: 0, nothing is refused as rank-deficient unless the caller sets a ratio. Measured with the fp32 model
    # at 120 x 160: eig_min / eig_max is at most 6.5e-4 on the plain corridor, which cannot be tracked, and at
    # least 4.95e-3 on a narrow ribbed one, which can; their geometric mean 1.8e-3 separates the two by a factor 2.8 only.
    ICP_MIN_EIG_RATIO = 0.0
    # Defaults of the photometric term (photo_params): of the grid weight {0.001, 0.003, 0.01, 0.03} x huber_delta {0, 4, 12, 36} the
    # pair with the smallest sum of the two pinned cases' worst translation errors, measured with the fp32 model at 120 x 160
    # (DESIGN.md section 9.10 holds the whole grid; tests/test_volume_icp_photo_cpu.py holds these constants to the rule).
    ICP_PHOTO_WEIGHT = 0.01
    ICP_PHOTO_HUBER = 4.0

    def icp_params(self, strides=(4, 2, 1), iters=(4, 5, 10), dist_max=None, huber_delta=0.0, eps_t=1e-5, eps_r=1e-5, min_pairs=None,
                   min_eig_ratio=None):
        """The odo_icp_params of align() and track(): coarse to fine over the strides, dist_max = 2 mu, min_pairs = 1 / 64 of the
        first level's pixels and the measured default of min_eig_ratio unless given."""
        if not 1 <= len(strides) == len(iters) <= 3:
            raise ValueError("one to three levels, a stride and an iteration count for each")
        p = L.IcpParams()
        p.levels = len(strides)
        for i, (s, n) in enumerate(zip(strides, iters)):
            p.stride[i], p.iters[i] = int(s), int(n)
        p.dist_max = 2 * self.params.mu if dist_max is None else dist_max
        p.huber_delta, p.eps_t, p.eps_r = huber_delta, eps_t, eps_r
        s0 = int(strides[0])
        lattice = (-(-self.rows // s0)) * (-(-self.cols // s0)) if s0 >= 1 else 0
        p.min_pairs = max(6, lattice // 64) if min_pairs is None else int(min_pairs)
        p.min_eig_ratio = self.ICP_MIN_EIG_RATIO if min_eig_ratio is None else min_eig_ratio
        return p

    def photo_params(self, weight=None, huber_delta=None):
        """The odo_icp_photo_params of the photometric term: weight in metres per grey level, huber_delta in grey levels (0: no
        robust weight); the measured defaults unless given."""
        return L.IcpPhotoParams(self.ICP_PHOTO_WEIGHT if weight is None else weight,
                                self.ICP_PHOTO_HUBER if huber_delta is None else huber_delta)

    def _frames_dev(self, frames):
        """Device handles of frames given as numpy arrays (uploaded; the second list names the temporaries) or as handles."""
        handles, temps = [], []
        try:
            for a, dtype, shape in frames:
                if isinstance(a, np.ndarray):
                    a = np.ascontiguousarray(a, dtype)
                    if a.shape != shape:
                        raise ValueError(f"frame {a.shape}, expected {shape}")
                    p = C.c_void_p()
                    L.check(self.lib.odo_dev_alloc(self._ctx, a.nbytes, C.byref(p)), "odo_dev_alloc")
                    temps.append(p)
                    L.check(self.lib.odo_dev_upload(self._ctx, p, a.ctypes.data_as(C.c_void_p), a.nbytes), "odo_dev_upload")
                    a = p
                handles.append(a)
        except Exception:
            self._free_dev(temps)
            raise
        return handles, temps

    def _free_dev(self, temps):
        for p in temps:
            self.lib.odo_dev_free(self._ctx, p)

    class _IcpPath:
        """What the two paths of frame-to-model tracking differ in, for icp_eval, the timings, align and track: the geometric path, or
        with photometric=True the one with the photometric term. It knows the frames to upload, the entry point (odo_volume_icp_* /
        odo_volume_icp_photo_*, whose arguments are the geometric ones with the extra frames behind the model's and the sensor's and
        the photometric parameters where `ph` is spliced in) and the shape of the result."""

        def __init__(self, vol, photometric, photo=None):
            self.vol, self.photometric = vol, photometric
            self.nacc, self.row_floats = (L.NACC_PHOTO, 16) if photometric else (L.NACC, 8)
            self.Result, self.TraceRow = (L.IcpPhotoResult, L.IcpPhotoTraceRow) if photometric else (L.IcpResult, L.IcpTraceRow)
            self.ph = [C.byref(vol.photo_params() if photo is None else photo)] if photometric else []

        def frames(self, depth, grey, model=None, colour=None):
            """Device handles of the sensor's frames ([raw] or [raw, grey]) and of the others (the model's [depth, nrmw] or [depth,
            nrmw, rgba] of model = (depth, nrmw, rgba), then a colour frame to fuse), and the temporaries to free."""
            size = (self.vol.rows, self.vol.cols)
            if self.photometric and (grey is None or (model is not None and model[2] is None)):
                raise ValueError("the photometric term needs both grey (the sensor's grey frame) and model_rgba (the ray-cast's colours)")
            frames = [(depth, np.uint16, size)] + ([(grey, np.float32, size)] if self.photometric else [])
            n = len(frames)
            if model is not None:
                frames += [(model[0], np.float32, size), (model[1], np.float32, size + (4,))]
                frames += [(model[2], np.uint8, size + (4,))] if self.photometric else []
            if colour is not None:
                frames.append((colour, np.uint8, size + (self.vol.colour_params.channels,)))
            handles, temps = self.vol._frames_dev(frames)
            return handles[:n], handles[n:], temps

        def call(self, name, *args):
            """The entry point `name`, its {} filled with "_photo" on the photometric path, on the volume."""
            name = name.format("_photo" if self.photometric else "")
            L.check(getattr(self.vol.lib, name)(self.vol.h, *args), name)

        def result(self, r):
            icp = r.icp if self.photometric else r
            out = dict(status=icp.status, iterations=icp.iterations, pairs=icp.pairs, cost=icp.cost, eig_min=icp.eig_min,
                       eig_max=icp.eig_max, C=_from_colmajor(list(icp.C)))
            if self.photometric:
                out.update(photo_pairs=r.photo_pairs, photo_cost=r.photo_cost)
            return out

    def icp_eval(self, depth, model_depth, model_nrmw, model_pose, C_sensor_to_model, stride=1, dist_max=None, huber_delta=0.0,
                 rows=False, grey=None, model_rgba=None, photo=None):
        """One evaluation of the alignment's rows at the 4x4 transform C_sensor_to_model: the 29 sums (float64), with rows=True also
        (rows, cols, 8) float32 {J0 .. J5, res, w} per pixel. depth: the sensor's uint16 frame; model_depth / model_nrmw: a ray-cast
        from model_pose at the volume's size and K; each a numpy array or a device handle. With grey (the sensor's float32 grey
        frame) and model_rgba (the ray-cast's colours) the photometric rows are evaluated as well: 31 sums, and (rows, cols, 16) rows,
        the geometric eight and then the photometric eight; photo: photo_params()."""
        path = self._IcpPath(self, grey is not None or model_rgba is not None, photo)
        sensor, model, temps = path.frames(depth, grey, (model_depth, model_nrmw, model_rgba))
        acc = np.zeros(path.nacc, np.float64)
        out = None
        nbytes = self.rows * self.cols * path.row_floats * 4
        try:
            if rows:
                out = C.c_void_p()
                L.check(self.lib.odo_dev_alloc(self._ctx, nbytes, C.byref(out)), "odo_dev_alloc")
                temps.append(out)
                L.check(self.lib.odo_dev_upload(self._ctx, out, np.full(nbytes, 0xAB, np.uint8).ctypes.data_as(C.c_void_p), nbytes),
                        "odo_dev_upload")
            path.call("odo_volume_icp{}_eval_dev", *model, _fp(_colmajor(model_pose)), *sensor, _fp(_colmajor(C_sensor_to_model)), int(stride),
                      2 * self.params.mu if dist_max is None else dist_max, huber_delta, *path.ph, acc.ctypes.data_as(L._dp), out)
            if rows:
                got = np.empty((self.rows, self.cols, path.row_floats), np.float32)
                L.check(self.lib.odo_dev_download(self._ctx, got.ctypes.data_as(C.c_void_p), out, got.nbytes), "odo_dev_download")
                return acc, got
            return acc
        finally:
            self._free_dev(temps)

    def _icp_time(self, path, depth, grey, model, model_pose, Cm, stride, dist_max, huber_delta, reps):
        sensor, model, temps = path.frames(depth, grey, model)
        us = np.zeros(2, np.float32)
        try:
            path.call("odo_volume_icp{}_time_dev", *model, _fp(_colmajor(model_pose)), *sensor, _fp(_colmajor(Cm)), int(stride),
                      2 * self.params.mu if dist_max is None else dist_max, huber_delta, *path.ph, int(reps), _fp(us))
        finally:
            self._free_dev(temps)
        return float(us[0]), float(us[1])

    def icp_photo_time(self, depth, grey, model_depth, model_nrmw, model_rgba, model_pose, C_sensor_to_model, stride=1, dist_max=None,
                       huber_delta=0.0, photo=None, reps=50):
        """Event timing of the two kernels of the alignment with the photometric term: (rows, step) microseconds per launch."""
        return self._icp_time(self._IcpPath(self, True, photo), depth, grey, (model_depth, model_nrmw, model_rgba), model_pose,
                              C_sensor_to_model, stride, dist_max, huber_delta, reps)

    def icp_time(self, depth, model_depth, model_nrmw, model_pose, C_sensor_to_model, stride=1, dist_max=None, huber_delta=0.0, reps=50):
        """Event timing of the alignment's two kernels: (rows, step) microseconds per launch, means over reps launches each."""
        return self._icp_time(self._IcpPath(self, False), depth, None, (model_depth, model_nrmw, None), model_pose, C_sensor_to_model,
                              stride, dist_max, huber_delta, reps)

    def align(self, depth, model_depth, model_nrmw, model_pose, init_pose, trace=False, params=None, grey=None, model_rgba=None,
              photo=None):
        """Aligns the sensor's depth frame to a model frame (a ray-cast from model_pose at the volume's size and K) from the first
        guess init_pose: (abs_pose 4x4 float32 — NaNs unless status is 0 —, result dict: status, iterations, pairs, cost, eig_min,
        eig_max, C), with trace=True also the steps as a list of dicts (level, iteration, acc, delta, C). With grey and model_rgba
        the photometric rows join the geometric ones (photo: photo_params()); the result gains photo_pairs and photo_cost and a
        trace entry's acc has 31 sums."""
        p = self.icp_params() if params is None else params
        path = self._IcpPath(self, grey is not None or model_rgba is not None, photo)
        sensor, model, temps = path.frames(depth, grey, (model_depth, model_nrmw, model_rgba))
        cap = sum(p.iters[:p.levels]) if trace else 0
        rows = (path.TraceRow * max(cap, 1))()
        n = C.c_int(0)
        res = path.Result()
        pose = np.zeros(16, np.float32)
        try:
            path.call("odo_volume_icp{}_align_dev", C.byref(p), *path.ph, *model, _fp(_colmajor(model_pose)), *sensor,
                      _fp(_colmajor(init_pose)), _fp(pose), C.byref(res), rows if trace else None, cap, C.byref(n))
        finally:
            self._free_dev(temps)
        out = (_from_colmajor(pose), path.result(res))
        if trace:
            out += ([dict(level=r.level, iteration=r.iteration, acc=np.array(r.acc, np.float64), delta=np.array(r.delta, np.float32),
                          C=_from_colmajor(list(r.C))) for r in rows[:n.value]],)
        return out

    def track(self, depth, prev_pose, integrate=False, params=None, grey=None, colour=None, photo=None):
        """Frame-to-model tracking of one depth frame (a uint16 numpy array or a device handle): the volume is ray-cast from prev_pose
        and the frame aligned to that from prev_pose. Returns (abs_pose, result dict) as align(). integrate=True fuses the frame at
        the returned pose when status is 0, behind the follow step for that pose when set_follow is on. With grey (the frame's
        float32 grey image; a volume with colour) the ray-cast includes the colours and the alignment the photometric rows (photo:
        photo_params()); integrate=True with colour (the frame's uint8 colour pixels) then fuses the coloured frame."""
        p = self.icp_params() if params is None else params
        if grey is None and (colour is not None or photo is not None):
            raise ValueError("TsdfVolume.track: colour and photo belong to the photometric path (give grey)")
        if colour is not None and not self.has_colour:
            raise L.OdoError("TsdfVolume.track: the volume has no colour grid (enable_colour first)")
        path = self._IcpPath(self, grey is not None, photo)
        sensor, fuse, temps = path.frames(depth, grey, colour=colour)
        res = path.Result()
        pose = np.zeros(16, np.float32)
        try:
            path.call("odo_volume_track{}_dev", C.byref(p), *path.ph, *sensor, _fp(_colmajor(prev_pose)), _fp(pose), C.byref(res))
            result = path.result(res)
            if integrate and result["status"] == 0:
                if self._follow is not None:   # the window moves for this pose before the frame is fused
                    L.check(self.lib.odo_volume_follow(self.h, _fp(pose), None), "odo_volume_follow")
                if colour is not None:
                    L.check(self.lib.odo_volume_integrate_colour_dev(self.h, sensor[0], fuse[0], _fp(pose)), "odo_volume_integrate_colour_dev")
                else:
                    L.check(self.lib.odo_volume_integrate_dev(self.h, sensor[0], _fp(pose)), "odo_volume_integrate_dev")
        finally:   # odo_dev_free waits for the context's stream: the integration has read the frames
            self._free_dev(temps)
        return _from_colmajor(pose), result

    def stats(self):
        o = (C.c_long * 4)()
        L.check(self.lib.odo_volume_stats(self.h, o), "odo_volume_stats")
        return dict(zip(self.STATS, list(o)))

    def clear(self):
        L.check(self.lib.odo_volume_clear(self.h), "odo_volume_clear")

    # ---- the moving window (odo_volume_shift, odo_volume_follow, the spill store) ----
    def enable_spill(self, capacity):
        """Adds the spill store: room for `capacity` (1 .. 2^28) surface points that shifts would destroy (32 B per point, 36 B with
        colour: enable_colour first). Once, and not while attached to a tracker."""
        L.check(self.lib.odo_volume_enable_spill(self.h, int(capacity)), "odo_volume_enable_spill")
        self._spill_capacity = int(capacity)
        self._spill_colour = self.has_colour   # (a store made before enable_colour has no colours)

    def shift_time(self, d, reps=50):
        """Event timing of a shift by d that is not applied: microseconds per launch or call, means over reps, of (shift, device-to-
        device copy of the same bytes, memset of the same bytes, spill count, spill scan, spill scatter); the last three are 0
        without a spill store. The grids, the window and the store's counted points stay as they are."""
        d = (C.c_int * 3)(*[int(x) for x in d])
        us = np.zeros(6, np.float32)
        L.check(self.lib.odo_volume_shift_time(self.h, d, int(reps), _fp(us)), "odo_volume_shift_time")
        return tuple(float(x) for x in us)

    def shift(self, d):
        """Moves the window by d = (dx, dy, dz) whole voxels: the origin moves by +d, new voxel (i, j, k) is old voxel (i + dx, j + dy,
        k + dz) or empty. With a spill store the points on edges that lose a voxel are appended to it first. Enqueued, no wait."""
        d = (C.c_int * 3)(*[int(x) for x in d])
        L.check(self.lib.odo_volume_shift(self.h, d), "odo_volume_shift")

    def window(self):
        """(off, origin): the cumulative shift in voxels (3 ints) and the grid's origin now (3 float32)."""
        off = (C.c_int * 3)()
        origin = np.zeros(3, np.float32)
        L.check(self.lib.odo_volume_window(self.h, off, _fp(origin)), "odo_volume_window")
        return tuple(off), origin

    def set_follow(self, focus=None, threshold=None):
        """The follow rule's parameters: the window is kept centred on the point `focus` metres in front of the camera and moves once
        that point is `threshold` voxels or more from its centre on some axis. set_follow() with neither turns following off. A
        parameter left out takes its convenience default, focus = max_depth / 2 and threshold = min(dims) // 8 (at least 1)."""
        if focus is None and threshold is None:
            L.check(self.lib.odo_volume_set_follow(self.h, None), "odo_volume_set_follow")
            self._follow = None
            return
        focus = self.params.max_depth / 2 if focus is None else focus
        threshold = max(1, min(self.dims) // 8) if threshold is None else threshold
        fp = L.VolumeFollowParams(focus, int(threshold))
        L.check(self.lib.odo_volume_set_follow(self.h, C.byref(fp)), "odo_volume_set_follow")
        self._follow = (fp.focus, fp.threshold)

    def follow(self, abs_pose):
        """The follow step for the 4x4 camera-to-world abs_pose: decides the shift by the rule of set_follow, applies it and returns
        it as 3 ints ((0, 0, 0): the window stayed)."""
        d = (C.c_int * 3)()
        L.check(self.lib.odo_volume_follow(self.h, _fp(_colmajor(abs_pose)), d), "odo_volume_follow")
        return tuple(d)

    def spilled(self, clear=False, colour=False, with_dropped=False):
        """The spill store's points as extract() returns them: (n, 4) float32 x, y, z, 0 and (n, 4) float32 nx, ny, nz, weight (colour:
        also (n, 4) uint8 R, G, B, A; with_dropped: also the number of points that did not fit the store). clear=True empties the
        store afterwards. Waits for everything pending."""
        cap = self._spill_capacity
        xyz0 = np.zeros((max(cap, 1), 4), np.float32)
        nrmw = np.zeros((max(cap, 1), 4), np.float32)
        rgba = np.zeros((max(cap, 1), 4), np.uint8) if colour else None
        n, d = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_volume_spill_points(self.h, cap, _fp(xyz0), _fp(nrmw), rgba.ctypes.data_as(L._u8p) if colour else None,
                                                 C.byref(n), C.byref(d), int(bool(clear))), "odo_volume_spill_points")
        out = (xyz0[:n.value].copy(), nrmw[:n.value].copy()) + ((rgba[:n.value].copy(),) if colour else ())
        return out + (d.value,) if with_dropped else out

    def save_ply(self, path, capacity=1 << 22, spill=False):
        """Binary little-endian PLY of the extracted surface: float x y z nx ny nz, and uchar red green blue when the volume has
        colour. spill=True: the spill store's points in front of the extraction's (the whole surface of a volume that moved)."""
        colour = self.has_colour
        if spill and colour and not self._spill_colour:
            raise ValueError("save_ply(spill=True): the spill store was enabled before enable_colour and holds no colours, the "
                             "extraction has them; call enable_colour before enable_spill")
        parts = [self.spilled(colour=colour)] if spill else []
        parts.append(self.extract(capacity, colour=colour))
        cols = [np.concatenate([p[i] for p in parts]) for i in range(3 if colour else 2)] if spill else list(parts[0])
        if colour:
            write_ply_normals(path, cols[0], cols[1], rgb=cols[2])
        else:
            write_ply_normals(path, cols[0], cols[1])

    def enable_spill_mesh(self, vertex_capacity, triangle_capacity):
        """Adds the mesh store: room for the vertices and triangles (1 .. 2^28 each) of the mesh of every slab that shifts destroy (32 B
        per vertex, 36 B with colour: enable_colour first; 12 B per triangle). Once, and not while attached to a tracker. It does
        not need enable_spill, and a volume may have both stores."""
        L.check(self.lib.odo_volume_enable_spill_mesh(self.h, int(vertex_capacity), int(triangle_capacity)), "odo_volume_enable_spill_mesh")
        self._spill_mesh_colour = self.has_colour   # (a store made before enable_colour has no colours)
        self._has_spill_mesh = True

    def spilled_mesh(self, clear=False, colour=False, with_dropped=False):
        """The mesh store as mesh() returns a mesh: (n, 4) float32 x, y, z, e; (n, 4) float32 nx, ny, nz, weight; (m, 3) int32 indices
        into these vertices (colour: also (n, 4) uint8 R, G, B, A; with_dropped: also (vertices, triangles) of the spills that did
        not fit and were left out whole). clear=True empties the store afterwards. Waits for everything pending."""
        n, m, d = C.c_long(0), C.c_long(0), (C.c_long * 2)()
        L.check(self.lib.odo_volume_spill_mesh(self.h, 0, 0, None, None, None, None, C.byref(n), C.byref(m), d, 0), "odo_volume_spill_mesh")
        nv, nt = max(n.value, 1), max(m.value, 1)   # (exact buffers: this thread enqueues nothing between the two calls)
        xyz0, nrmw, tri = np.zeros((nv, 4), np.float32), np.zeros((nv, 4), np.float32), np.zeros((nt, 3), np.int32)
        rgba = np.zeros((nv, 4), np.uint8) if colour else None
        L.check(self.lib.odo_volume_spill_mesh(self.h, nv, nt, _fp(xyz0), _fp(nrmw), rgba.ctypes.data_as(L._u8p) if colour else None,
                                               tri.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n), C.byref(m), d, int(bool(clear))),
                "odo_volume_spill_mesh")
        out = (xyz0[:n.value].copy(), nrmw[:n.value].copy(), tri[:m.value].copy()) + ((rgba[:n.value].copy(),) if colour else ())
        return out + ((d[0], d[1]),) if with_dropped else out

    def spill_mesh_time(self, d, reps=50):
        """Event timing of the mesh spill for a shift by d that is not applied: microseconds per launch, means over reps, of (count,
        scan, vertices, triangles, colour); the last is 0 without colour. The store's contents and counts stay as they are."""
        d = (C.c_int * 3)(*[int(x) for x in d])
        us = np.zeros(5, np.float32)
        L.check(self.lib.odo_volume_spill_mesh_time(self.h, d, int(reps), _fp(us)), "odo_volume_spill_mesh_time")
        return tuple(float(x) for x in us)

    # ---- the re-entry store (odo_volume_enable_reentry: the leaving voxels, put back when the window returns) ----
    def enable_reentry(self, capacity):
        """Adds the re-entry store: room for `capacity` (1 .. 2^28) voxels that shifts push out of the window, each kept with its
        integer position in the world and put back by the first shift that brings the window over it again (two sets of buffers: 32 B
        per entry, 40 B with colour: enable_colour first). Once, and not while attached to a tracker. shift, follow, track(...,
        integrate=True) and an attached RgbdTracker use it with no further arguments."""
        L.check(self.lib.odo_volume_enable_reentry(self.h, int(capacity)), "odo_volume_enable_reentry")

    def stored_voxels(self, clear=False, colour=False):
        """The re-entry store's live entries in store order: (n, 3) int32 global voxel index (window offset + index in the window),
        (n,) int16 q and (n,) uint16 w (colour: also (n, 4) uint8 R, G, B, wc). clear=True empties the store and zeroes its counters
        afterwards. Waits for everything pending."""
        n = C.c_long(0)
        L.check(self.lib.odo_volume_reentry_voxels(self.h, 0, None, None, None, C.byref(n), 0), "odo_volume_reentry_voxels")
        m = max(n.value, 1)   # (an exact buffer: this thread enqueues nothing between the two calls)
        g, vox = np.zeros((m, 3), np.int32), np.zeros(m, np.uint32)
        col = np.zeros(m, np.uint32) if colour else None
        u32 = C.POINTER(C.c_uint32)
        L.check(self.lib.odo_volume_reentry_voxels(self.h, m, g.ctypes.data_as(C.POINTER(C.c_int32)), vox.ctypes.data_as(u32),
                                                   col.ctypes.data_as(u32) if colour else None, C.byref(n), int(bool(clear))),
                "odo_volume_reentry_voxels")
        vox = vox[:n.value]
        out = (g[:n.value].copy(), (vox & 0xFFFF).astype(np.uint16).view(np.int16), (vox >> 16).astype(np.uint16))
        return out + (col[:n.value].copy().view(np.uint8).reshape(-1, 4),) if colour else out

    def reentry_stats(self):
        """dict(live, saved, restored, dropped): entries in the re-entry store now, and since enable_reentry / clear the entries
        appended, the entries put back into the grid, and the leaving voxels that found the store full. Waits."""
        s = (C.c_long * 4)()
        L.check(self.lib.odo_volume_reentry_stats(self.h, s), "odo_volume_reentry_stats")
        return dict(live=s[0], saved=s[1], restored=s[2], dropped=s[3])

    def reentry_time(self, d, reps=50):
        """Event timing of the re-entry passes for a shift by d that is not applied: microseconds, means over reps, of (save count, save
        scan, save scatter, store pass, advance). The volume and the store stay as they are."""
        d = (C.c_int * 3)(*[int(x) for x in d])
        us = np.zeros(5, np.float32)
        L.check(self.lib.odo_volume_reentry_time(self.h, d, int(reps), _fp(us)), "odo_volume_reentry_time")
        return tuple(float(x) for x in us)

    def save_mesh_ply(self, path, spill=False):
        """Binary little-endian PLY of the mesh: float x y z nx ny nz per vertex (and uchar red green blue when the volume has
        colour), three int indices per face. spill=True: the mesh store's mesh in front of the window's, whose indices are offset
        by the store's vertices (the whole surface of a volume that moved; the seam's vertices are in both and are not welded)."""
        colour = self.has_colour
        if spill and colour and not self._spill_mesh_colour:
            raise ValueError("save_mesh_ply(spill=True): the mesh store was enabled before enable_colour and holds no colours, the "
                             "mesh has them; call enable_colour before enable_spill_mesh")
        parts = self.mesh(colour=True) if colour else self.mesh()
        if spill:
            store = self.spilled_mesh(colour=colour)
            parts = tuple(np.concatenate([a, b + len(store[0])]) if i == 2 else np.concatenate([a, b])
                          for i, (a, b) in enumerate(zip(store, parts)))
        if colour:
            write_ply_mesh(path, parts[0], parts[1], parts[2], rgb=parts[3])
        else:
            write_ply_mesh(path, parts[0], parts[1], parts[2])

    def welded_mesh(self, eps=None, grids=8, spill=True, colour=False):
        """One mesh of the whole surface, welded (MeshWeld): the mesh store's mesh (where the volume has one and
        spill is set) in front of the window's, whose indices are offset by the store's vertices, as save_mesh_ply(spill=True) writes
        them; then vertices that share a cell of edge eps around the volume's first origin become one, and degenerate and duplicate
        triangles leave. eps=None: voxel_size / 64. dict(xyz0, nrmw, tri, rgba with colour, stats). Waits."""
        spill = bool(spill) and self._has_spill_mesh
        if spill and colour and not self._spill_mesh_colour:
            raise ValueError("welded_mesh(colour=True): the mesh store was enabled before enable_colour and holds no colours, the "
                             "mesh has them; call enable_colour before enable_spill_mesh")
        parts = self.mesh(colour=True) if colour else self.mesh()
        if spill:
            store = self.spilled_mesh(colour=colour)
            parts = tuple(np.concatenate([a, b + len(store[0])]) if i == 2 else np.concatenate([a, b])
                          for i, (a, b) in enumerate(zip(store, parts)))
        eps = np.float32(self.params.voxel_size) / np.float32(64.0) if eps is None else eps
        w = MeshWeld(self._owner, max(len(parts[0]), 1), max(len(parts[2]), 1), colour=colour)
        try:
            return w.run(parts[0], parts[1], parts[2], rgba=parts[3] if colour else None, eps=eps,
                         origin=tuple(self.params.origin), grids=grids, drop_unreferenced=True)
        finally:
            w.close()

    def save_welded_mesh_ply(self, path, eps=None, grids=8, spill=True):
        """welded_mesh() as a binary little-endian PLY, through write_ply_mesh: float x y z nx ny nz per vertex (and uchar red green
        blue when the volume has colour), three int indices per face. Returns the weld's counters."""
        colour = self.has_colour
        m = self.welded_mesh(eps=eps, grids=grids, spill=spill, colour=colour)
        write_ply_mesh(path, m["xyz0"], m["nrmw"], m["tri"], rgb=m["rgba"] if colour else None)
        return m["stats"]

    def cleaned_mesh(self, eps=None, grids=8, spill=True, colour=False, min_triangles=128, keep_largest=False):
        """welded_mesh()'s mesh without its small pieces (MeshComponents): the same inputs go through
        MeshWeld.run_dev, the welder's result stays on the device and MeshComponents.run_dev reads it there; components of fewer
        than min_triangles triangles leave (with keep_largest every component but the largest). dict(xyz0, nrmw, tri, rgba with
        colour, stats, weld_stats). Waits."""
        spill = bool(spill) and self._has_spill_mesh
        if spill and colour and not self._spill_mesh_colour:
            raise ValueError("cleaned_mesh(colour=True): the mesh store was enabled before enable_colour and holds no colours, the "
                             "mesh has them; call enable_colour before enable_spill_mesh")
        parts = self.mesh(colour=True) if colour else self.mesh()
        if spill:
            store = self.spilled_mesh(colour=colour)
            parts = tuple(np.concatenate([a, b + len(store[0])]) if i == 2 else np.concatenate([a, b])
                          for i, (a, b) in enumerate(zip(store, parts)))
        eps = np.float32(self.params.voxel_size) / np.float32(64.0) if eps is None else eps
        nv, nt = len(parts[0]), len(parts[2])
        ctx = self._owner._ctx if isinstance(self._owner, Tracker) else self._owner.h
        w = MeshWeld(self._owner, max(nv, 1), max(nt, 1), colour=colour)
        f = MeshComponents(self._owner, max(nv, 1), max(nt, 1), colour=colour)
        held = []
        try:
            for a in (_f32(parts[0]), _f32(parts[1]), np.ascontiguousarray(parts[2], np.int32)) + \
                    ((np.ascontiguousarray(parts[3], np.uint8),) if colour else ()):
                d = C.c_void_p()
                L.check(self.lib.odo_dev_alloc(ctx, max(a.nbytes, 16), C.byref(d)), "odo_dev_alloc")
                held.append(d)
                if a.nbytes:
                    L.check(self.lib.odo_dev_upload(ctx, d, a.ctypes.data_as(C.c_void_p), a.nbytes), "odo_dev_upload")
            w.run_dev(nv, nt, held[0], held[1], held[2], held[3] if colour else None, eps=eps, origin=tuple(self.params.origin),
                      grids=grids, drop_unreferenced=True)
            x, n, c, t, wv, wt = w.result_dev()
            f.run_dev(wv, wt, x, n, t, c, min_triangles=min_triangles, keep_largest=keep_largest, drop_unreferenced=True)
            out = f.download(colour=colour)
            out["stats"], out["weld_stats"] = f.stats(), w.stats()
            return out
        finally:
            f.close()
            w.close()
            for d in held:
                self.lib.odo_dev_free(ctx, d)

    def save_cleaned_mesh_ply(self, path, eps=None, grids=8, spill=True, min_triangles=128, keep_largest=False):
        """cleaned_mesh() as a binary little-endian PLY, through write_ply_mesh, as save_welded_mesh_ply writes welded_mesh().
        Returns the filter's counters."""
        colour = self.has_colour
        m = self.cleaned_mesh(eps=eps, grids=grids, spill=spill, colour=colour, min_triangles=min_triangles, keep_largest=keep_largest)
        write_ply_mesh(path, m["xyz0"], m["nrmw"], m["tri"], rgb=m["rgba"] if colour else None)
        return m["stats"]

    def close(self):
        if getattr(self, "h", None):
            if self._tracker is not None and getattr(self._tracker, "h", None):
                self._tracker.attach_volume(None)
            self.lib.odo_volume_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RgbdFrontend:
    """Raw sensor frames -> the RGB-D tracker's inputs on the device (odo_rgbd_frontend_*): interleaved 8-bit colour to fp32 grey and
    the depth imager's uint16 frame registered to the grey camera, on a stream of its own, into a ring of `slots` outputs.
    tracker_or_ctx: a Context, or a Tracker (host frames then go up on its stream). depth_K = (fx, fy, cx, cy) of the depth imager,
    K = (f0, cx0, cy0) of the tracker's frame, colour_from_depth: 3x4 or 4x4 [R | t] in metres (None: identity)."""

    STATS = ("n_depth", "n_filled", "dropped_behind", "dropped_range", "dropped_splat", "frame")

    def __init__(self, tracker_or_ctx, depth_size, depth_K, depth_scale_in, size, K, depth_scale_out, colour_from_depth=None,
                 colour_channels=3, colour_bgr=False, slots=3):
        self.lib = L.load()
        self._owner = tracker_or_ctx   # keeps the stream's owner alive as long as the front end
        ctx = tracker_or_ctx._ctx if isinstance(tracker_or_ctx, Tracker) else tracker_or_ctx.h
        self._ctx = ctx
        E = np.eye(4) if colour_from_depth is None else np.asarray(colour_from_depth, np.float64)
        p = L.RgbdFrontendParams()
        p.depth_rows, p.depth_cols = depth_size
        p.depth_fx, p.depth_fy, p.depth_cx, p.depth_cy = depth_K
        p.depth_scale_in = depth_scale_in
        p.rows, p.cols = size
        p.K = L.Intrinsics(*K)
        p.depth_scale_out = depth_scale_out
        for i, v in enumerate(E[:3, :4].reshape(-1)):
            p.colour_from_depth[i] = v
        p.colour_channels, p.colour_bgr, p.slots = colour_channels, int(bool(colour_bgr)), slots
        self.params = p
        self.rows, self.cols, self.channels = p.rows, p.cols, colour_channels
        self.depth_rows, self.depth_cols = p.depth_rows, p.depth_cols
        self._bufs = []
        h = C.c_void_p()
        L.check(self.lib.odo_rgbd_frontend_create(ctx, C.byref(p), C.byref(h)), "odo_rgbd_frontend_create")
        self.h = h

    def upload(self, arr):
        """A raw frame (uint8 colour or uint16 depth) into a device buffer owned by the front end (`close` frees it): a handle for
        `submit`."""
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        L.check(self.lib.odo_dev_alloc(self._ctx, arr.nbytes, C.byref(p)), "odo_dev_alloc")
        L.check(self.lib.odo_dev_upload(self._ctx, p, arr.ctypes.data_as(C.c_void_p), arr.nbytes), "odo_dev_upload")
        self._bufs.append(p)
        return p

    def submit(self, colour, depth):
        """Enqueues one frame and returns (gray_dev, depth_dev) of its slot at once. numpy arrays (rows x cols x channels uint8 and
        depth_rows x depth_cols uint16; any row pitch) take the host path, device handles the device path."""
        g, d = C.c_void_p(), C.c_void_p()
        if isinstance(colour, np.ndarray) != isinstance(depth, np.ndarray):
            raise TypeError("colour and depth must both be numpy arrays or both be device handles")
        if isinstance(colour, np.ndarray):
            if colour.dtype != np.uint8 or colour.shape != (self.rows, self.cols, self.channels):
                raise ValueError(f"colour frame {colour.dtype} {colour.shape}")
            if depth.dtype != np.uint16 or depth.shape != (self.depth_rows, self.depth_cols):
                raise ValueError(f"depth frame {depth.dtype} {depth.shape}")
            if colour.strides[1:] != (self.channels, 1) or colour.strides[0] < self.cols * self.channels:
                colour = np.ascontiguousarray(colour)
            if depth.strides[1] != 2 or depth.strides[0] < 2 * self.depth_cols:
                depth = np.ascontiguousarray(depth)
            L.check(self.lib.odo_rgbd_frontend_submit_host(self.h, colour.ctypes.data_as(C.c_void_p), colour.strides[0],
                                                           depth.ctypes.data_as(C.c_void_p), depth.strides[0], C.byref(g), C.byref(d)),
                    "odo_rgbd_frontend_submit_host")
        else:
            L.check(self.lib.odo_rgbd_frontend_submit_dev(self.h, colour, depth, C.byref(g), C.byref(d)),
                    "odo_rgbd_frontend_submit_dev")
        return g, d

    def wait(self, gray_dev):
        L.check(self.lib.odo_rgbd_frontend_wait(self.h, gray_dev), "odo_rgbd_frontend_wait")

    def colour(self, gray_dev):
        """The device colour frame the slot with that grey buffer was made from (the caller's handle, or the slot's own raw copy of a
        host frame): what RgbdTracker.frame_colour takes. Valid from the slot's completion until the slot comes round again."""
        c = C.c_void_p()
        L.check(self.lib.odo_rgbd_frontend_colour(self.h, gray_dev, C.byref(c)), "odo_rgbd_frontend_colour")
        return c

    def stats(self, gray_dev):
        o = (C.c_long * 6)()
        L.check(self.lib.odo_rgbd_frontend_stats(self.h, gray_dev, o), "odo_rgbd_frontend_stats")
        return dict(zip(self.STATS, list(o)))

    def download(self, gray_dev, depth_dev):
        """A slot's results on the host (waits for the slot): (rows x cols float32, rows x cols uint16)."""
        self.wait(gray_dev)
        gray = np.empty((self.rows, self.cols), np.float32)
        dep = np.empty((self.rows, self.cols), np.uint16)
        L.check(self.lib.odo_dev_download(self._ctx, gray.ctypes.data_as(C.c_void_p), gray_dev, gray.nbytes), "odo_dev_download")
        L.check(self.lib.odo_dev_download(self._ctx, dep.ctypes.data_as(C.c_void_p), depth_dev, dep.nbytes), "odo_dev_download")
        return gray, dep

    def close(self):
        if getattr(self, "h", None):
            self.lib.odo_rgbd_frontend_destroy(self.h)
            self.h = None
            for p in self._bufs:
                self.lib.odo_dev_free(self._ctx, p)
            self._bufs = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KINECT_AXIAL_NOISE = (0.0012, 0.0019, 0.4)   # sigma(z) = a + b (z - z0)^2 metres: the published Kinect axial model (synth.sensor_noise)


def depth_filter_tables(radius=2, sigma_s=1.5, sigma0=8.0, gain=3.0, depth_scale=1000.0, noise=KINECT_AXIAL_NOISE):
    """The three tables of the bilateral depth filter (include/odometry_hip.h, odo_depth_filter_create) as Gaussians that follow a
    sensor's axial noise sigma(z) = a + b (z - z0)^2 metres, noise = (a, b, z0):
      ws[dy][dx] = rint(16 exp(-(dx^2 + dy^2) / (2 sigma_s^2))), (2 radius + 1)^2 uint8;
      wr[k]      = rint(255 exp(-k^2 / (2 sigma0^2))), sigma0 in raw units, 256 uint8;
      shift[j]   = clip(rint(log2(gain sigma(z_j) depth_scale / sigma0)), 0, 4) with z_j = (256 j + 128) / depth_scale: the range
                   kernel's width sigma0 << shift follows gain sigma(z) in raw units.
    Returns (ws, wr, shift)."""
    a, b, z0 = noise
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    ws = np.rint(16.0 * np.exp(-(d[None, :] ** 2 + d[:, None] ** 2) / (2.0 * sigma_s * sigma_s))).astype(np.uint8)
    k = np.arange(256, dtype=np.float64)
    wr = np.rint(255.0 * np.exp(-k * k / (2.0 * sigma0 * sigma0))).astype(np.uint8)
    z = (256.0 * k + 128.0) / depth_scale
    sig = a + b * (z - z0) ** 2
    shift = np.clip(np.rint(np.log2(gain * sig * depth_scale / sigma0)), 0, 4).astype(np.uint8)
    return ws, wr, shift


class DepthFilter:
    """The bilateral depth filter on the device (odo_depth_filter_*): a uint16 sensor depth frame in, the denoised frame out, one
    launch on the context's stream, exact integers (include/odometry_hip.h). ctx_or_tracker: a Context, or a Tracker (its context).
    size = (rows, cols); tables = (ws, wr, shift), default depth_filter_tables(**table_kwargs)."""

    STATS = ("n_valid", "n_changed", "sum_abs_change")

    def __init__(self, ctx_or_tracker, size, tables=None, **table_kwargs):
        self.lib = L.load()
        self._owner = ctx_or_tracker   # keeps the stream's owner alive as long as the filter
        self._ctx = ctx_or_tracker._ctx if isinstance(ctx_or_tracker, Tracker) else ctx_or_tracker.h
        if tables is not None and table_kwargs:
            raise TypeError("tables and table keywords exclude each other")
        ws, wr, shift = depth_filter_tables(**table_kwargs) if tables is None else tables
        ws = np.asarray(ws)
        if ws.ndim != 2 or ws.shape[0] != ws.shape[1] or ws.shape[0] % 2 != 1:
            raise ValueError(f"ws {ws.shape}: a (2R + 1) x (2R + 1) array")
        wr, shift = np.asarray(wr).reshape(-1), np.asarray(shift).reshape(-1)
        if wr.shape != (256,) or shift.shape != (256,):
            raise ValueError("wr and shift have 256 entries each")
        for name, t in (("ws", ws), ("wr", wr), ("shift", shift)):
            if t.min() < 0 or t.max() > 255:
                raise ValueError(f"{name} does not fit uint8")
        p = L.DepthFilterParams()
        p.rows, p.cols = size
        p.radius = (ws.shape[0] - 1) // 2
        flat = ws.reshape(-1)
        if flat.size > 81:
            raise ValueError(f"radius {p.radius} (1 .. 4)")
        for i, v in enumerate(flat):
            p.ws[i] = int(v)
        for i in range(256):
            p.wr[i], p.shift[i] = int(wr[i]), int(shift[i])
        self.params = p
        self.rows, self.cols, self.radius = p.rows, p.cols, p.radius
        self._out = None
        self.h = None
        h = C.c_void_p()
        L.check(self.lib.odo_depth_filter_create(self._ctx, C.byref(p), C.byref(h)), "odo_depth_filter_create")
        self.h = h

    def run(self, depth_dev, out_dev=None):
        """Enqueues the filter of the device frame depth_dev and returns the handle of the output at once: out_dev, or a buffer of
        the filter's own (overwritten by the next such run; `close` frees it)."""
        if out_dev is None:
            if self._out is None:
                p = C.c_void_p()
                L.check(self.lib.odo_dev_alloc(self._ctx, 2 * self.rows * self.cols, C.byref(p)), "odo_dev_alloc")
                self._out = p
            out_dev = self._out
        L.check(self.lib.odo_depth_filter_run_dev(self.h, depth_dev, out_dev), "odo_depth_filter_run_dev")
        return out_dev

    def stats(self):
        """The last run's exact counts (waits for it)."""
        o = (C.c_long * 3)()
        L.check(self.lib.odo_depth_filter_stats(self.h, o), "odo_depth_filter_stats")
        return dict(zip(self.STATS, list(o)))

    def time(self, depth_dev, out_dev=None, reps=50):
        """Mean microseconds of one launch, `reps` between two events (a diagnostic: tools/depth_filter_cost.py)."""
        if out_dev is None:
            out_dev = self.run(depth_dev)
        us = C.c_float(0)
        L.check(self.lib.odo_depth_filter_time_dev(self.h, depth_dev, out_dev, reps, C.byref(us)), "odo_depth_filter_time_dev")
        return us.value

    def download(self, out_dev=None):
        """An output frame on the host (ordered behind the run on the context's stream): rows x cols uint16."""
        out = np.empty((self.rows, self.cols), np.uint16)
        L.check(self.lib.odo_dev_download(self._ctx, out.ctypes.data_as(C.c_void_p), self._out if out_dev is None else out_dev,
                                          out.nbytes), "odo_dev_download")
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.odo_depth_filter_destroy(self.h)
            self.h = None
            if self._out is not None:
                self.lib.odo_dev_free(self._ctx, self._out)
                self._out = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StereoDepth:
    """Dense stereo depth on the device (odo_stereo_depth_*): a rectified pair of fp32 grey frames in, the uint16 depth frame a
    sensor would give out, by census matching in exact integers (include/odometry_hip.h): three launches on the context's stream.
    ctx_or_tracker: a Context, or a Tracker (its context). size = (rows, cols); fx in pixels, baseline in metres; candidates
    min_disp .. max_disp; max_depth in metres (None: whatever fits 16 bits)."""

    STATS = ("interior", "matched", "rej_unique", "rej_lr", "rej_range", "sum_q")

    def __init__(self, ctx_or_tracker, size, fx, baseline, depth_scale=1000.0, min_disp=1, max_disp=127, agg_radius=2, uniqueness=10,
                 lr_max=1, max_depth=None):
        self.lib = L.load()
        self._owner = ctx_or_tracker   # keeps the stream's owner alive as long as the matcher
        self._ctx = ctx_or_tracker._ctx if isinstance(ctx_or_tracker, Tracker) else ctx_or_tracker.h
        p = L.StereoDepthParams()
        p.rows, p.cols = size
        p.dmin, p.dmax, p.agg_radius, p.uniqueness, p.lr_max = int(min_disp), int(max_disp), int(agg_radius), int(uniqueness), int(lr_max)
        p.max_raw = 65535 if max_depth is None else int(min(max(np.floor(float(max_depth) * float(depth_scale)), -1.0), 65535.0))
        p.fx, p.baseline, p.depth_scale = float(fx), float(baseline), float(depth_scale)
        self.params = p
        self.rows, self.cols = p.rows, p.cols
        self._out = None
        self.h = None
        h = C.c_void_p()
        L.check(self.lib.odo_stereo_depth_create(self._ctx, C.byref(p), C.byref(h)), "odo_stereo_depth_create")
        self.h = h

    def run(self, left_dev, right_dev, out_dev=None):
        """Enqueues the depth of the device pair and returns the handle of the output at once: out_dev, or the matcher's internal
        frame (overwritten by the next such run)."""
        L.check(self.lib.odo_stereo_depth_run_dev(self.h, left_dev, right_dev, out_dev), "odo_stereo_depth_run_dev")
        return self._internal() if out_dev is None else out_dev

    def _internal(self):
        if self._out is None:
            p = C.c_void_p()
            L.check(self.lib.odo_stereo_depth_depth_dev(self.h, C.byref(p)), "odo_stereo_depth_depth_dev")
            self._out = p
        return self._out

    def _fetch(self, dev):
        out = np.empty((self.rows, self.cols), np.uint16)
        L.check(self.lib.odo_dev_download(self._ctx, out.ctypes.data_as(C.c_void_p), dev, out.nbytes), "odo_dev_download")
        return out

    def disparity(self):
        """The last run's q frame on the host, sixteenths of a pixel, 0 = none (ordered behind the run): rows x cols uint16."""
        p = C.c_void_p()
        L.check(self.lib.odo_stereo_depth_disparity_dev(self.h, C.byref(p)), "odo_stereo_depth_disparity_dev")
        return self._fetch(p)

    def download(self, out_dev=None):
        """A depth frame on the host (ordered behind the run on the context's stream): rows x cols uint16."""
        return self._fetch(self._internal() if out_dev is None else out_dev)

    def stats(self):
        """The last run's exact counters by name (waits for it)."""
        o = (C.c_long * 8)()
        L.check(self.lib.odo_stereo_depth_stats(self.h, o), "odo_stereo_depth_stats")
        v = list(o)
        return dict(zip(self.STATS, v[:5] + [v[5] + (v[6] << 32)]))

    def time(self, left_dev, right_dev, out_dev=None, reps=20):
        """Mean microseconds of one launch of each kernel, `reps` between two events (a diagnostic: tools/stereo_depth_cost.py):
        dict(census, match_right, match_left)."""
        us = (C.c_float * 3)()
        L.check(self.lib.odo_stereo_depth_time_dev(self.h, left_dev, right_dev, out_dev, reps, us), "odo_stereo_depth_time_dev")
        return dict(zip(("census", "match_right", "match_left"), list(us)))

    def enable_speckle(self, max_diff=8, min_size=200):
        """Every later run enqueues a speckle filter behind the match (SpeckleFilter's rule; max_diff in sixteenths of a pixel): the
        key is the q frame, the targets are the q frame and the run's depth output. min_size=0 takes it off again."""
        L.check(self.lib.odo_stereo_depth_enable_speckle(self.h, int(max_diff), int(min_size)), "odo_stereo_depth_enable_speckle")

    def speckle_stats(self):
        """The last run's speckle counters by name (waits for it); an error while no filter is enabled."""
        o = (C.c_long * 8)()
        L.check(self.lib.odo_stereo_depth_speckle_stats(self.h, o), "odo_stereo_depth_speckle_stats")
        return dict(zip(SpeckleFilter.STATS, list(o)[:len(SpeckleFilter.STATS)]))

    SGM_GROUPS = ("census", "cost", "paths", "select_right", "select_left")

    def enable_sgm(self, p1=None, p2=None, paths=8):
        """Every later run aggregates the box-summed cost along 4 or 8 paths (semi-global matching, include/odometry_hip.h) before
        the selection. p1 / p2: the penalties of a disparity step of one / of more; None: 4 / 24 times the window's area (100 / 600
        at agg_radius 2). Allocates two uint16 volumes rows x cols x (max_disp - min_disp + 1)."""
        n = (2 * self.params.agg_radius + 1) ** 2
        p1 = 4 * n if p1 is None else int(p1)
        p2 = 24 * n if p2 is None else int(p2)
        if int(paths) == 0:
            raise ValueError("paths must be 4 or 8 (disable_sgm takes the mode off)")
        L.check(self.lib.odo_stereo_depth_enable_sgm(self.h, p1, p2, int(paths)), "odo_stereo_depth_enable_sgm")

    def disable_sgm(self):
        """Back to the box matcher; frees the volumes (waits for the runs that use them)."""
        L.check(self.lib.odo_stereo_depth_enable_sgm(self.h, 0, 0, 0), "odo_stereo_depth_enable_sgm")

    def sgm_time(self, left_dev, right_dev, out_dev=None, reps=20):
        """time() for the semi-global mode (tools/stereo_sgm_cost.py): dict(census, cost, paths, select_right, select_left), the
        path launches of one run as one figure."""
        us = (C.c_float * 5)()
        L.check(self.lib.odo_stereo_depth_sgm_time_dev(self.h, left_dev, right_dev, out_dev, reps, us), "odo_stereo_depth_sgm_time_dev")
        return dict(zip(self.SGM_GROUPS, list(us)))

    def sgm_volume(self):
        """The last run's aggregate S on the host (a test's read-out; waits): rows x cols x D uint16, 65535 = not admissible."""
        out = np.empty((self.rows, self.cols, self.params.dmax - self.params.dmin + 1), np.uint16)
        L.check(self.lib.odo_debug_sgm_volume(self.h, out.ctypes.data_as(C.c_void_p)), "odo_debug_sgm_volume")
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.odo_stereo_depth_destroy(self.h)
            self.h = None
            self._out = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpeckleFilter:
    """The speckle filter on the device (odo_speckle_*): the connected components of a uint16 key frame (4-neighbours, both keys
    non-zero, |difference| <= max_diff) with fewer than min_size pixels are zeroed in up to two target frames, in place, in exact
    integers (include/odometry_hip.h): four launches on the context's stream. ctx_or_tracker: a Context, or a Tracker (its
    context). size = (rows, cols)."""

    STATS = ("pixels", "components", "removed_components", "removed_pixels", "largest", "guard")
    KERNELS = ("label", "seams", "count", "apply", "run")

    def __init__(self, ctx_or_tracker, size, max_diff, min_size):
        self.lib = L.load()
        self._owner = ctx_or_tracker   # keeps the stream's owner alive as long as the filter
        self._ctx = ctx_or_tracker._ctx if isinstance(ctx_or_tracker, Tracker) else ctx_or_tracker.h
        p = L.SpeckleParams()
        p.rows, p.cols = size
        p.max_diff, p.min_size = int(max_diff), int(min_size)
        self.params = p
        self.rows, self.cols = p.rows, p.cols
        self.h = None
        h = C.c_void_p()
        L.check(self.lib.odo_speckle_create(self._ctx, C.byref(p), C.byref(h)), "odo_speckle_create")
        self.h = h

    def run(self, key_dev, target_a_dev, target_b_dev=None):
        """Enqueues the filter and returns at once: the components are those of key_dev, the pixels of the small ones are zeroed in
        target_a_dev and target_b_dev (either may be key_dev itself)."""
        L.check(self.lib.odo_speckle_run_dev(self.h, key_dev, target_a_dev, target_b_dev), "odo_speckle_run_dev")
        return target_a_dev

    def stats(self):
        """The last run's exact counters by name (waits for it)."""
        o = (C.c_long * 8)()
        L.check(self.lib.odo_speckle_stats(self.h, o), "odo_speckle_stats")
        return dict(zip(self.STATS, list(o)[:len(self.STATS)]))

    def time(self, key_dev, target_a_dev, target_b_dev=None, reps=20):
        """Mean microseconds of each kernel and of the whole run, `reps` between two events, on scratch copies (a diagnostic:
        tools/speckle_cost.py): dict(label, seams, count, apply, run). The targets hold one run's result afterwards."""
        us = (C.c_float * 5)()
        L.check(self.lib.odo_speckle_time_dev(self.h, key_dev, target_a_dev, target_b_dev, reps, us), "odo_speckle_time_dev")
        return dict(zip(self.KERNELS, list(us)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.odo_speckle_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeshWeld:
    """The mesh welder on the device (odo_mesh_weld_*): vertices that share a cell of edge eps become one (the smallest index stays,
    with its own attributes), triangles that turn degenerate or repeat an earlier one leave, in exact integers behind three fp32
    operations per coordinate (include/odometry_hip.h): every pass's launches go to the context's stream. ctx_or_tracker: a
    Context, or a Tracker (its context)."""

    STATS = ("vertices_in", "vertices_out", "merged", "keyless", "unreferenced", "triangles_in", "triangles_out", "degenerate",
             "duplicate", "bad_index", "guard", "passes")
    GROUPS = ("vertex_table", "representatives", "triangle_table", "survivors", "scans", "scatters", "run")

    def __init__(self, ctx_or_tracker, vertex_capacity, triangle_capacity, colour=False):
        self.lib = L.load()
        self._owner = ctx_or_tracker   # keeps the stream's owner alive as long as the welder
        self._ctx = ctx_or_tracker._ctx if isinstance(ctx_or_tracker, Tracker) else ctx_or_tracker.h
        p = L.MeshWeldParams(int(vertex_capacity), int(triangle_capacity), int(bool(colour)))
        self.params = p
        self.h = None
        h = C.c_void_p()
        L.check(self.lib.odo_mesh_weld_create(self._ctx, C.byref(p), C.byref(h)), "odo_mesh_weld_create")
        self.h = h

    @staticmethod
    def rule(eps, origin=(0.0, 0.0, 0.0), grids=8, drop_unreferenced=True):
        if eps is None:
            raise ValueError("MeshWeld: eps is required (the cell's edge, metres)")
        r = L.MeshWeldRule()
        r.eps = eps
        for i in range(3):
            r.origin[i] = origin[i]
        r.grids, r.drop_unreferenced = int(grids), int(bool(drop_unreferenced))
        return r

    def run_dev(self, n_vertices, n_triangles, xyz0_dev, nrmw_dev, tri_dev, rgba_dev=None, eps=None, origin=(0.0, 0.0, 0.0), grids=8,
                drop_unreferenced=True):
        """Enqueues the weld of a mesh on the device and returns at once; the result stays in the welder's buffers (result_dev,
        download)."""
        L.check(self.lib.odo_mesh_weld_run_dev(self.h, C.byref(self.rule(eps, origin, grids, drop_unreferenced)), int(n_vertices),
                                               int(n_triangles), xyz0_dev, nrmw_dev, rgba_dev, tri_dev), "odo_mesh_weld_run_dev")

    def result_dev(self):
        """(xyz0, nrmw, rgba or None, tri, n_vertices, n_triangles) of the last run: device pointers into the welder's buffers and
        the two counts (waits for them)."""
        p = [C.c_void_p() for _ in range(4)]
        n, m = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_mesh_weld_result_dev(self.h, *[C.byref(x) for x in p], C.byref(n), C.byref(m)), "odo_mesh_weld_result_dev")
        return p[0], p[1], (p[2] if p[2].value else None), p[3], n.value, m.value

    def download(self, colour=False):
        """The last run's result on the host (waits): dict(xyz0 (n, 4) float32, nrmw (n, 4) float32, tri (m, 3) int32, and with colour
        rgba (n, 4) uint8)."""
        n, m = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_mesh_weld_download(self.h, 0, 0, None, None, None, None, C.byref(n), C.byref(m)), "odo_mesh_weld_download")
        nv, nt = n.value, m.value   # (exact buffers: this thread enqueues nothing between the two calls)
        out = dict(xyz0=np.zeros((nv, 4), np.float32), nrmw=np.zeros((nv, 4), np.float32), tri=np.zeros((nt, 3), np.int32))
        if colour:
            out["rgba"] = np.zeros((nv, 4), np.uint8)
        if nv or nt:
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            L.check(self.lib.odo_mesh_weld_download(self.h, nv, nt, vp(out["xyz0"]), vp(out["nrmw"]), vp(out["rgba"]) if colour else None,
                                                    vp(out["tri"]), C.byref(n), C.byref(m)), "odo_mesh_weld_download")
        return out

    def run(self, xyz0, nrmw, tri, rgba=None, eps=None, origin=(0.0, 0.0, 0.0), grids=8, drop_unreferenced=True):
        """Host arrays in, a dict out: xyz0 and nrmw (n, 4) float32, tri (m, 3) int32, rgba (n, 4) uint8 or None -> dict(xyz0, nrmw,
        tri, rgba when given, stats)."""
        xyz0, nrmw = _f32(xyz0).reshape(-1, 4), _f32(nrmw).reshape(-1, 4)
        tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
        if len(nrmw) != len(xyz0):
            raise ValueError("xyz0 and nrmw differ in length")
        if rgba is not None:
            rgba = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)
            if len(rgba) != len(xyz0):
                raise ValueError("xyz0 and rgba differ in length")
        nv, nt = len(xyz0), len(tri)
        out = dict(xyz0=np.zeros((max(nv, 1), 4), np.float32), nrmw=np.zeros((max(nv, 1), 4), np.float32),
                   tri=np.zeros((max(nt, 1), 3), np.int32))
        if rgba is not None:
            out["rgba"] = np.zeros((max(nv, 1), 4), np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        n, m = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_mesh_weld_run(self.h, C.byref(self.rule(eps, origin, grids, drop_unreferenced)), nv, nt, vp(xyz0), vp(nrmw),
                                           vp(rgba), vp(tri), nv, nt, vp(out["xyz0"]), vp(out["nrmw"]), vp(out.get("rgba")) if nv else None,
                                           vp(out["tri"]), C.byref(n), C.byref(m)), "odo_mesh_weld_run")
        out = {k: (v[:m.value] if k == "tri" else v[:n.value]).copy() for k, v in out.items()}
        out["stats"] = self.stats()
        return out

    def stats(self):
        """The last run's exact counters by name (waits for it)."""
        o = (C.c_long * 12)()
        L.check(self.lib.odo_mesh_weld_stats(self.h, o), "odo_mesh_weld_stats")
        return dict(zip(self.STATS, list(o)))

    def time(self, n_vertices, n_triangles, xyz0_dev, nrmw_dev, tri_dev, rgba_dev=None, eps=None, origin=(0.0, 0.0, 0.0), grids=8,
             drop_unreferenced=True, reps=20):
        """Mean microseconds of each group of launches, summed over the passes, and their sum (a diagnostic: tools/mesh_weld_cost.py):
        dict(vertex_table, representatives, triangle_table, survivors, scans, scatters, run). The welder holds one run's result
        afterwards."""
        us = (C.c_float * 7)()
        L.check(self.lib.odo_mesh_weld_time_dev(self.h, C.byref(self.rule(eps, origin, grids, drop_unreferenced)), int(n_vertices),
                                                int(n_triangles), xyz0_dev, nrmw_dev, rgba_dev, tri_dev, int(reps), us),
                "odo_mesh_weld_time_dev")
        return dict(zip(self.GROUPS, list(us)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.odo_mesh_weld_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MeshComponents:
    """The mesh component filter on the device (odo_mesh_components_*): valid triangles that share a vertex index are one component,
    its label its smallest vertex index; components of fewer than min_triangles triangles leave (with keep_largest all but the
    largest), the vertices and triangles that stay are renumbered, in exact integers (include/odometry_hip.h). Every launch goes to
    the context's stream; the input may be a MeshWeld's result_dev() pointers. ctx_or_tracker: a Context, or a Tracker (its
    context). edge_stats: count the edges used once and more than twice, before and after."""

    STATS = ("vertices_in", "triangles_in", "vertices_out", "triangles_out", "components", "removed_components", "removed_triangles",
             "removed_vertices", "largest", "bad_index", "degenerate", "unreferenced", "edges", "open_edges", "nonmanifold_edges",
             "edges_out", "open_edges_out", "nonmanifold_edges_out", "guard")
    GROUPS = ("union", "sizes", "edges", "survivors", "scans", "scatters", "run")

    def __init__(self, ctx_or_tracker, vertex_capacity, triangle_capacity, colour=False, edge_stats=True):
        self.lib = L.load()
        self._owner = ctx_or_tracker   # keeps the stream's owner alive as long as the filter
        self._ctx = ctx_or_tracker._ctx if isinstance(ctx_or_tracker, Tracker) else ctx_or_tracker.h
        p = L.MeshComponentsParams(int(vertex_capacity), int(triangle_capacity), int(bool(colour)), int(bool(edge_stats)))
        self.params = p
        self.h = None
        h = C.c_void_p()
        L.check(self.lib.odo_mesh_components_create(self._ctx, C.byref(p), C.byref(h)), "odo_mesh_components_create")
        self.h = h

    @staticmethod
    def rule(min_triangles, keep_largest=False, drop_unreferenced=True):
        if min_triangles is None:
            raise ValueError("MeshComponents: min_triangles is required (the smallest component that stays)")
        return L.MeshComponentsRule(int(min_triangles), int(bool(keep_largest)), int(bool(drop_unreferenced)))

    def run_dev(self, n_vertices, n_triangles, xyz0_dev, nrmw_dev, tri_dev, rgba_dev=None, min_triangles=None, keep_largest=False,
                drop_unreferenced=True):
        """Enqueues the filter on a mesh on the device and returns at once; the result stays in the filter's buffers (result_dev,
        download, labels)."""
        L.check(self.lib.odo_mesh_components_run_dev(self.h, C.byref(self.rule(min_triangles, keep_largest, drop_unreferenced)),
                                                     int(n_vertices), int(n_triangles), xyz0_dev, nrmw_dev, rgba_dev, tri_dev),
                "odo_mesh_components_run_dev")

    def result_dev(self):
        """(xyz0, nrmw, rgba or None, tri, n_vertices, n_triangles) of the last run: device pointers into the filter's buffers and
        the two counts (waits for them)."""
        p = [C.c_void_p() for _ in range(4)]
        n, m = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_mesh_components_result_dev(self.h, *[C.byref(x) for x in p], C.byref(n), C.byref(m)),
                "odo_mesh_components_result_dev")
        return p[0], p[1], (p[2] if p[2].value else None), p[3], n.value, m.value

    def download(self, colour=False):
        """The last run's result on the host (waits): dict(xyz0 (n, 4) float32, nrmw (n, 4) float32, tri (m, 3) int32, and with colour
        rgba (n, 4) uint8)."""
        n, m = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_mesh_components_download(self.h, 0, 0, None, None, None, None, C.byref(n), C.byref(m)),
                "odo_mesh_components_download")
        nv, nt = n.value, m.value   # (exact buffers: this thread enqueues nothing between the two calls)
        out = dict(xyz0=np.zeros((nv, 4), np.float32), nrmw=np.zeros((nv, 4), np.float32), tri=np.zeros((nt, 3), np.int32))
        if colour:
            out["rgba"] = np.zeros((nv, 4), np.uint8)
        if nv or nt:
            vp = lambda a: a.ctypes.data_as(C.c_void_p)
            L.check(self.lib.odo_mesh_components_download(self.h, nv, nt, vp(out["xyz0"]), vp(out["nrmw"]),
                                                          vp(out["rgba"]) if colour else None, vp(out["tri"]), C.byref(n), C.byref(m)),
                    "odo_mesh_components_download")
        return out

    def run(self, xyz0, nrmw, tri, rgba=None, min_triangles=None, keep_largest=False, drop_unreferenced=True):
        """Host arrays in, a dict out: xyz0 and nrmw (n, 4) float32, tri (m, 3) int32, rgba (n, 4) uint8 or None -> dict(xyz0, nrmw,
        tri, rgba when given, labels (one per input triangle), stats)."""
        xyz0, nrmw = _f32(xyz0).reshape(-1, 4), _f32(nrmw).reshape(-1, 4)
        tri = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
        if len(nrmw) != len(xyz0):
            raise ValueError("xyz0 and nrmw differ in length")
        if rgba is not None:
            rgba = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)
            if len(rgba) != len(xyz0):
                raise ValueError("xyz0 and rgba differ in length")
        nv, nt = len(xyz0), len(tri)
        out = dict(xyz0=np.zeros((max(nv, 1), 4), np.float32), nrmw=np.zeros((max(nv, 1), 4), np.float32),
                   tri=np.zeros((max(nt, 1), 3), np.int32))
        if rgba is not None:
            out["rgba"] = np.zeros((max(nv, 1), 4), np.uint8)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
        n, m = C.c_long(0), C.c_long(0)
        L.check(self.lib.odo_mesh_components_run(self.h, C.byref(self.rule(min_triangles, keep_largest, drop_unreferenced)), nv, nt,
                                                 vp(xyz0), vp(nrmw), vp(rgba), vp(tri), nv, nt, vp(out["xyz0"]), vp(out["nrmw"]),
                                                 vp(out.get("rgba")) if nv else None, vp(out["tri"]), C.byref(n), C.byref(m)),
                "odo_mesh_components_run")
        out = {k: (v[:m.value] if k == "tri" else v[:n.value]).copy() for k, v in out.items()}
        out["labels"] = self.labels()
        out["stats"] = self.stats()
        return out

    def labels_dev(self):
        """(device pointer to the last run's labels, their number): one int32 per input triangle. Does not wait."""
        p, n = C.c_void_p(), C.c_long(0)
        L.check(self.lib.odo_mesh_components_labels_dev(self.h, C.byref(p), C.byref(n)), "odo_mesh_components_labels_dev")
        return p, n.value

    def labels(self):
        """The last run's label per input triangle (waits): its component's smallest vertex index, -1 for an invalid triangle."""
        n = C.c_long(0)
        L.check(self.lib.odo_mesh_components_labels(self.h, 0, None, C.byref(n)), "odo_mesh_components_labels")
        out = np.zeros(n.value, np.int32)
        if n.value:
            L.check(self.lib.odo_mesh_components_labels(self.h, n.value, out.ctypes.data_as(C.c_void_p), C.byref(n)),
                    "odo_mesh_components_labels")
        return out

    def stats(self):
        """The last run's exact counters by name (waits for it)."""
        o = (C.c_long * 19)()
        L.check(self.lib.odo_mesh_components_stats(self.h, o), "odo_mesh_components_stats")
        return dict(zip(self.STATS, list(o)))

    def time(self, n_vertices, n_triangles, xyz0_dev, nrmw_dev, tri_dev, rgba_dev=None, min_triangles=None, keep_largest=False,
             drop_unreferenced=True, reps=20):
        """Mean microseconds of each group of launches and their sum (a diagnostic: tools/mesh_components_cost.py): dict(union,
        sizes, edges, survivors, scans, scatters, run). The filter holds one run's result afterwards."""
        us = (C.c_float * 7)()
        L.check(self.lib.odo_mesh_components_time_dev(self.h, C.byref(self.rule(min_triangles, keep_largest, drop_unreferenced)),
                                                      int(n_vertices), int(n_triangles), xyz0_dev, nrmw_dev, rgba_dev, tri_dev, int(reps),
                                                      us), "odo_mesh_components_time_dev")
        return dict(zip(self.GROUPS, list(us)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.odo_mesh_components_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_ply(path, xyzi):
    """(N, 4) float32 x, y, z, intensity -> binary little-endian PLY with float x y z and uchar red green blue (grey)."""
    xyzi = np.asarray(xyzi, np.float32).reshape(-1, 4)
    rec = np.zeros(len(xyzi), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")]))
    rec["x"], rec["y"], rec["z"] = xyzi[:, 0], xyzi[:, 1], xyzi[:, 2]
    grey = np.clip(np.nan_to_num(xyzi[:, 3]), 0, 255).astype(np.uint8)
    rec["r"] = rec["g"] = rec["b"] = grey
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n") % len(xyzi)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def _ply_vertices(xyz, normals, rgb):
    """The vertex records and their property lines: float x y z nx ny nz, then uchar red green blue when rgb (N, >= 3) is given."""
    xyz = np.asarray(xyz, np.float32)
    normals = np.asarray(normals, np.float32)
    assert xyz.ndim == 2 and normals.shape[0] == xyz.shape[0] and xyz.shape[1] >= 3 and normals.shape[1] >= 3
    fields = [(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")]
    props = "".join("property float %s\n" % k for k in ("x", "y", "z", "nx", "ny", "nz"))
    if rgb is not None:
        rgb = np.asarray(rgb, np.uint8)
        assert rgb.ndim == 2 and rgb.shape[0] == xyz.shape[0] and rgb.shape[1] >= 3
        fields += [(k, "u1") for k in ("red", "green", "blue")]
        props += "".join("property uchar %s\n" % k for k in ("red", "green", "blue"))
    rec = np.zeros(len(xyz), np.dtype(fields))
    for c, k in enumerate(("x", "y", "z")):
        rec[k] = xyz[:, c]
        rec["n" + k] = normals[:, c]
    if rgb is not None:
        for c, k in enumerate(("red", "green", "blue")):
            rec[k] = rgb[:, c]
    return rec, props


def write_ply_normals(path, xyz, normals, rgb=None):
    """(N, >= 3) positions and (N, >= 3) normals -> binary little-endian PLY with float x y z nx ny nz; rgb (N, >= 3) uint8: also
    uchar red green blue."""
    rec, props = _ply_vertices(xyz, normals, rgb)
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(rec)) + props + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def write_ply_mesh(path, xyz, normals, tri, rgb=None):
    """(N, >= 3) positions, (N, >= 3) normals and (M, 3) vertex indices -> binary little-endian PLY: vertex float x y z nx ny nz (rgb
    (N, >= 3) uint8: also uchar red green blue), face list uchar int vertex_indices."""
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    rec, props = _ply_vertices(xyz, normals, rgb)
    faces = np.zeros(len(tri), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    faces["n"] = 3
    faces["v"] = tri
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(rec)) + props + (
        "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(tri))
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())
        f.write(faces.tobytes())


class TrackerBatch:
    """n_sequences independent sequences tracked in lock step on one GPU (odo_tracker_batch_*): the frame loop of
    ref: run_odometry_kitti_offline.cpp:198-271 once per sequence, every launch carrying all of them. Bit-identical to
    n_sequences separate `Tracker` objects; frames are device-resident handles from `upload_frame`."""

    def __init__(self, n_sequences, device=0, **overrides):
        self.lib = L.load()
        self.n = int(n_sequences)
        self.params = L.TrackerParams()
        L.check(self.lib.odo_tracker_default_params(C.byref(self.params)), "odo_tracker_default_params")
        for k, v in overrides.items():
            if k == "lm_max_iters":
                for i, m in enumerate(v):
                    self.params.lm_max_iters[i] = m
            elif k == "K":
                self.params.K = L.Intrinsics(*v)
            else:
                setattr(self.params, k, v)
        h = C.c_void_p()
        L.check(self.lib.odo_tracker_batch_create(device, C.byref(self.params), self.n, C.byref(h)), "odo_tracker_batch_create")
        self.h = h
        self._ctx = C.c_void_p(self.lib.odo_tracker_batch_ctx(h))
        self._bufs = []
        self._T = np.zeros(16 * self.n, np.float32)
        self._A = np.zeros(16 * self.n, np.float32)
        self._nk = (C.c_int * self.n)()
        self._st = (C.c_int * self.n)()
        self._mag = (C.c_float * self.n)()

    def upload_frame(self, img):
        img = _f32(img)
        p = C.c_void_p()
        L.check(self.lib.odo_dev_alloc(self._ctx, img.nbytes, C.byref(p)), "odo_dev_alloc")
        L.check(self.lib.odo_dev_upload(self._ctx, p, img.ctypes.data_as(C.c_void_p), img.nbytes), "odo_dev_upload")
        self._bufs.append(p)
        return p

    def _ptrs(self, handles):
        if len(handles) != self.n:
            raise ValueError(f"expected {self.n} frames, got {len(handles)}")
        return (C.c_void_p * self.n)(*[h.value if isinstance(h, C.c_void_p) else h for h in handles])

    def init(self, lefts, rights, abs_pose0=None):
        pose = None
        if abs_pose0 is not None:
            pose = _fp(np.concatenate([_colmajor(P) for P in abs_pose0]).astype(np.float32))
        L.check(self.lib.odo_tracker_batch_init(self.h, self._ptrs(lefts), self._ptrs(rights), pose), "odo_tracker_batch_init")

    def init_one(self, slot, left, right, abs_pose0=None):
        pose = None if abs_pose0 is None else _fp(_colmajor(abs_pose0))
        L.check(self.lib.odo_tracker_batch_init_one(self.h, slot, left, right, pose), "odo_tracker_batch_init_one")

    def hint_next(self, next_lefts, next_rights=None):
        """next_lefts / next_rights: n handles (None allowed) or prepared (c_void_p * n) arrays. With the right images the depth
        stream works a step ahead as well (odo_tracker_batch_hint_next_pair)."""
        arr = next_lefts if isinstance(next_lefts, C.Array) else self._ptrs(next_lefts)
        if next_rights is None:
            L.check(self.lib.odo_tracker_batch_hint_next(self.h, arr), "odo_tracker_batch_hint_next")
        else:
            arr_r = next_rights if isinstance(next_rights, C.Array) else self._ptrs(next_rights)
            L.check(self.lib.odo_tracker_batch_hint_next_pair(self.h, arr, arr_r), "odo_tracker_batch_hint_next_pair")

    def track_raw(self, left_ptrs, right_ptrs):
        """Lean variant for timing loops: takes prepared (c_void_p * n) arrays, returns the status array; poses stay in
        self._T / self._A (n x 16, column-major)."""
        st = self.lib.odo_tracker_batch_track(self.h, left_ptrs, right_ptrs, _fp(self._T), _fp(self._A), self._nk, self._mag,
                                              self._st)
        if st != 0:
            raise L.OdoError("odo_tracker_batch_track: " + L.last_error())
        return self._st

    def track(self, lefts, rights):
        self.track_raw(self._ptrs(lefts), self._ptrs(rights))
        out = []
        for i in range(self.n):
            out.append(dict(pose_to_keyframe=_from_colmajor(self._T[16 * i:16 * i + 16].copy()),
                            abs_pose=_from_colmajor(self._A[16 * i:16 * i + 16].copy()), new_keyframe=bool(self._nk[i]),
                            motion=float(self._mag[i]), status=int(self._st[i])))
        return out

    def stats(self):
        arr = [(C.c_int * self.n)() for _ in range(4)]
        L.check(self.lib.odo_tracker_batch_stats(self.h, *arr), "odo_tracker_batch_stats")
        return [dict(lm_evals=arr[0][i], depth_iters=arr[1][i], n_valid_depth=arr[2][i], n_keyframes=arr[3][i])
                for i in range(self.n)]

    def timing(self):
        out = (C.c_double * 4)()
        L.check(self.lib.odo_tracker_batch_timing(self.h, out), "odo_tracker_batch_timing")
        return dict(step_us=out[0], head_us=out[1], solve_us=out[2], depth_wait_us=out[3])

    def event_timing(self, on):
        """Execution-span sampling of the batched LM launches (every `on`-th; 0 = off); statistics live with slot 0's optimiser."""
        L.check(self.lib.odo_lm_event_timing(C.c_void_p(self.lib.odo_tracker_batch_lm(self.h, 0)), int(on)), "odo_lm_event_timing")

    def event_stats_ex(self):
        o = (C.c_double * 12)()
        L.check(self.lib.odo_lm_event_stats_ex(C.c_void_p(self.lib.odo_tracker_batch_lm(self.h, 0)), o), "odo_lm_event_stats_ex")
        return dict(step_us=o[0], step_sampled=int(o[1]), coarse_us=o[2], coarse_sampled=int(o[3]), launches=int(o[4]),
                    coarse_launches=int(o[5]), evaluations=int(o[6]), bytes=o[7], step_period_us=o[8], step_periods=int(o[9]),
                    coarse_period_us=o[10], coarse_periods=int(o[11]))

    def outputs(self, seq, rows, cols):
        v, dsp, dep = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(self.lib.odo_tracker_batch_outputs(self.h, seq, C.byref(v), C.byref(dsp), C.byref(dep)), "odo_tracker_batch_outputs")
        out = []
        for ptr, dt in ((v, np.uint8), (dsp, np.float32), (dep, np.float32)):
            a = np.empty((rows, cols), dt)
            L.check(self.lib.odo_dev_download(self._ctx, a.ctypes.data_as(C.c_void_p), ptr, a.nbytes), "download")
            out.append(a)
        return out

    def depth_persistent_stats(self):
        """(1 while the lock step's inverse-depth LMs run in one persistent launch, lock steps whose launch gave up and were redone)"""
        a, b = C.c_int(0), C.c_int(0)
        L.check(self.lib.odo_tracker_batch_depth_persistent_stats(self.h, C.byref(a), C.byref(b)), "odo_tracker_batch_depth_persistent_stats")
        return a.value, b.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.odo_tracker_batch_quiesce(self.h)   # see Tracker.close
            for p in self._bufs:
                self.lib.odo_dev_free(self._ctx, p)
            self._bufs = []
            self.lib.odo_tracker_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
