"""Loader of the device-math harness (tests/devmath_harness.hip) and of its host twin (tests/hostemu.cpp), behind one interface.

The harness is the arithmetic that decides the pose as hipcc compiles it for gfx950, call by call; it is built with exactly
odometry_amd.build.FLAGS, once under the main unit's machine scheduler and once under the LM chain unit's (build._flags_for), into
tests/_build_devmath_<scheduler>.so. The host twin runs the same cases (tests/devmath_ops.h) through g++. `Ops` gives both the same
methods, numpy in, numpy out, so a test reads `dev.se3_exp(a)` against `host.se3_exp(a)`.

Also here: ctypes mirrors of the structures that cross the boundary (LmState, DenseLevel, LmScript, PixLevel). The harness exports
sizeof / offsetof of the C++ side (dm_layout); tests/test_devmath_cpu.py asserts the mirrors match."""
import ctypes as C
import os
import subprocess

import numpy as np

from odometry_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
SRC = os.path.join(HERE, "devmath_harness.hip")
DEPS = [SRC, os.path.join(HERE, "devmath_ops.h"), os.path.join(B._HERE, "csrc", "kernels.hip.h"), os.path.join(B._HERE, "csrc", "dense.hip.h"),
        os.path.join(B._HERE, "csrc", "odo_math.h"), os.path.abspath(B.__file__)]
UNITS = ("main", "chain")     # whose machine scheduler the harness is compiled under


def flags(unit):
    return B._flags_for(B.SRC_CHAIN if unit == "chain" else B.SRC, B.FLAGS)


def scheduler(unit):
    for f in flags(unit):
        if f.startswith("-amdgpu-sched-strategy="):
            return f.split("=", 1)[1]
    return "default"


def so_path(unit):
    """ODO_DEVMATH_DIR: a directory of prebuilt harness libraries to load instead (A/B builds, as ODOMETRY_HIP_LIB is for the library)."""
    return os.path.join(os.environ.get("ODO_DEVMATH_DIR") or HERE, "_build_devmath_%s.so" % scheduler(unit))


def build(unit, force=False, verbose=False):
    so = so_path(unit)
    if force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS):
        cmd = [B.HIPCC] + flags(unit) + ["-shared", "-o", so, SRC]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return so


def build_all(force=False, verbose=False):
    """Both builds side by side (what __graft_entry__.build() calls)."""
    todo = {}
    for u in UNITS:
        so = so_path(u)
        if so not in todo and (force or not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in DEPS)):
            todo[so] = [B.HIPCC] + flags(u) + ["-shared", "-o", so, SRC]
    procs = []
    for so, cmd in todo.items():
        if verbose:
            print(" ".join(cmd))
        procs.append((subprocess.Popen(cmd), cmd))
    for pr, cmd in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    return [so_path(u) for u in UNITS]


# ---- structure mirrors ------------------------------------------------------------------------------------------------------------
class Se3(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("qx", "qy", "qz", "qw", "tx", "ty", "tz")]


class LmState(C.Structure):
    _fields_ = [("cur", Se3), ("inc", Se3), ("last", Se3), ("T", C.c_float * 16), ("lambda_", C.c_float), ("err_last", C.c_float),
                ("err_now", C.c_float), ("level", C.c_int), ("iter", C.c_int), ("active", C.c_int), ("status", C.c_int),
                ("n_evals", C.c_int), ("stop_reason", C.c_int), ("iters_level", C.c_int * 8), ("delta", C.c_float * 6),
                ("pending", C.c_int), ("pending_nblk", C.c_int), ("max_iters", C.c_int), ("finished", C.c_int)]


class LevelK(C.Structure):
    _fields_ = [("fl", C.c_double), ("cx", C.c_float), ("cy", C.c_float), ("bilinear", C.c_int)]


class DenseLevel(C.Structure):
    _fields_ = [("I1", C.c_void_p), ("I2", C.c_void_p), ("D1", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("k", LevelK),
                ("nblk", C.c_int), ("n_strips", C.c_int), ("n_rg", C.c_int), ("fast_ok", C.c_int), ("max_iters", C.c_int)]


class LmScript(C.Structure):
    _fields_ = [("n_levels", C.c_int), ("stop_level", C.c_int), ("n_evals", C.c_int), ("acc_first", C.c_int), ("lambda0", C.c_float),
                ("precision", C.c_float), ("max_iters", C.c_int * 8), ("init", C.c_float * 16)]


class PixLevel(C.Structure):
    _fields_ = [("I1", C.c_void_p), ("I2", C.c_void_p), ("D1", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("k", LevelK),
                ("T", C.c_float * 16), ("robust", C.c_int), ("huber_delta", C.c_float), ("scale_sqr", C.c_float)]


LM_STATE = np.dtype(LmState)     # an array of states: np.zeros(n, LM_STATE); .view(np.uint32).reshape(n, 64) for the bit patterns
LM_SCRIPT = np.dtype(LmScript)
LM_STATE_FIELDS = ("cur", "inc", "last", "T", "lambda_", "err_last", "err_now", "level", "iter", "active", "status", "n_evals", "stop_reason",
                   "iters_level", "delta", "pending", "pending_nblk", "max_iters", "finished")
DENSE_LEVEL_FIELDS = ("I1", "I2", "D1", "rows", "cols", ("k", "fl"), ("k", "cx"), ("k", "cy"), ("k", "bilinear"), "nblk", "n_strips", "n_rg",
                      "fast_ok", "max_iters")


def mirror_layout():
    """The mirrors' own sizeof / offsetof, in dm_layout's order (without its last two entries: kCoarseBlock, kFirstCap)."""
    out = [C.sizeof(LmState)] + [getattr(LmState, f).offset for f in LM_STATE_FIELDS] + [C.sizeof(DenseLevel)]
    for f in DENSE_LEVEL_FIELDS:
        out.append(getattr(DenseLevel, f).offset if isinstance(f, str) else getattr(DenseLevel, f[0]).offset + getattr(LevelK, f[1]).offset)
    return out + [C.sizeof(LmScript), C.sizeof(PixLevel), C.sizeof(LevelK)]


ENTRIES = ("dm_layout_count", "dm_layout", "dm_dense_fast_ok", "dm_level_k", "dm_sincos", "dm_se3_exp", "dm_se3_roundtrip", "dm_se3_left_update",
           "dm_solve_damped", "dm_robust_weight", "dm_apply_step", "dm_depth_schedule", "dm_lm_script", "dm_sincos_pair_wave",
           "dm_se3_exp_wave", "dm_solve_damped_wave", "dm_apply_step_wave", "dm_pixels", "dm_dense_pixels", "dm_div32", "dm_div64",
           "dm_callsites", "dm_dense_runs", "dm_dense_eval", "dm_dense_eval_batch", "dm_tdist_scale", "dm_make_points", "dm_kf_lists",
           "dm_list_eval")
MAX_LEVELS = 8                # ODO_MAX_LEVELS_K


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


class Ops:
    """The cases of tests/devmath_ops.h on the host (device=False: tests/_build_hostemu.so) or on the GPU (device=True: one build of
    the harness). Same methods, same array shapes. Device only: the wave-wide and block-level forms, the dense scan, the scale
    kernels, the keyframe point lists (kf_lists) and the kernels that read them (list_eval)."""

    def __init__(self, lib, device):
        self.lib, self.device = lib, device
        if device:
            n = lib.dm_layout_count()
            lay = np.zeros(n, np.int32)
            lib.dm_layout(_p(lay))
            self.layout = [int(v) for v in lay]
            self.coarse_block, self.first_cap = self.layout[-2], self.layout[-1]
            lib.dm_dense_fast_ok.argtypes = [C.c_double, C.c_float, C.c_float, C.c_int, C.c_int]

    def _call(self, name, *args):
        if self.device:
            rc = getattr(self.lib, "dm_" + name)(*args)
            assert rc == 0, "dm_%s: HIP error %d" % (name, rc)
        else:
            getattr(self.lib, "emu_" + name + "_n")(*args)

    # -- one case per thread --
    def level_k(self, f0, cx0, cy0, level):
        f0, cx0, cy0, level = _f32(f0), _f32(cx0), _f32(cy0), _i32(level)
        n = len(f0)
        fl, cxy = np.zeros(n, np.float64), np.zeros((n, 3), np.float32)
        self._call("level_k", n, _p(f0), _p(cx0), _p(cy0), _p(level), _p(fl), _p(cxy))
        return fl, cxy

    def sincos(self, x):
        x = _f32(x)
        s, c = np.zeros_like(x), np.zeros_like(x)
        self._call("sincos", len(x), _p(x), _p(s), _p(c))
        return s, c

    def _qm(self, n):
        return np.zeros((n, 7), np.float32), np.zeros((n, 16), np.float32)

    def se3_exp(self, a):
        a = _f32(a).reshape(-1, 6)
        q, M = self._qm(len(a))
        self._call("se3_exp", len(a), _p(a), _p(q), _p(M))
        return q, M

    def se3_roundtrip(self, Min):
        Min = _f32(Min).reshape(-1, 16)
        q, M = self._qm(len(Min))
        self._call("se3_roundtrip", len(Min), _p(Min), _p(q), _p(M))
        return q, M

    def se3_left_update(self, d6, cur, variant=0):
        d6, cur = _f32(d6).reshape(-1, 6), _f32(cur).reshape(-1, 16)
        q, M = self._qm(len(d6))
        self._call("se3_left_update", len(d6), _p(d6), _p(cur), int(variant), _p(q), _p(M))
        return q, M

    def solve_damped(self, acc, lam):
        acc, lam = _f64(acc).reshape(-1, 29), _f32(lam)
        d = np.zeros((len(acc), 6), np.float32)
        self._call("solve_damped", len(acc), _p(acc), _p(lam), _p(d))
        return d

    def robust_weight(self, r, robust, huber, scale):
        r, robust, huber, scale = _f32(r), _i32(robust), _f32(huber), _f32(scale)
        w = np.zeros_like(r)
        self._call("robust_weight", len(r), _p(r), _p(robust), _p(huber), _p(scale), _p(w))
        return w

    def apply_step(self, states):
        states = np.ascontiguousarray(states, LM_STATE)
        out = np.zeros(len(states), LM_STATE)
        self._call("apply_step", len(states), _p(states), _p(out))
        return out

    def depth_schedule(self, errs, n_errs, lambda0, precision, max_iters):
        errs = _f32(errs)
        n, cap = errs.shape
        rec, fin = np.zeros((n, cap, 5), np.int32), np.zeros((n, 3), np.int32)
        self._call("depth_schedule", n, cap, _p(errs), _p(_i32(n_errs)), _p(_f32(lambda0)), _p(_f32(precision)), _p(_i32(max_iters)),
                   _p(rec), _p(fin))
        return rec, fin

    def lm_script(self, scripts, acc, form=0, block=64):
        """form 0: lm_consume (per thread); device only: 1 = lm_state_machine, 2 = lm_state_machine_hot, one block of `block` threads
        per script. Returns (states after every evaluation [n_acc], evaluations consumed per script [n])."""
        scripts, acc = np.ascontiguousarray(scripts, LM_SCRIPT), _f64(acc).reshape(-1, 29)
        out, count = np.zeros(len(acc), LM_STATE), np.zeros(len(scripts), np.int32)
        if self.device:
            self._call("lm_script", len(scripts), _p(scripts), len(acc), _p(acc), int(form), int(block), _p(out), _p(count))
        else:
            assert form == 0
            self._call("lm_script", len(scripts), _p(scripts), _p(acc), _p(out), _p(count))
        return out, count

    def pixels(self, I1, I2, D1, k, T, mode, robust=1, huber_delta=28.0, scale_sqr=1.0):
        """k = (fl, cx, cy, bilinear); T: 4x4 row-major numpy. Returns hit [rows, cols], r, w, J [rows, cols, 6]."""
        I1, I2, D1 = _f32(I1), _f32(I2), _f32(D1)
        rows, cols = I1.shape
        L = PixLevel(I1.ctypes.data, I2.ctypes.data, D1.ctypes.data, rows, cols, LevelK(*k))
        L.T[:] = [float(v) for v in _f32(np.asarray(T, np.float32).T).reshape(16)]
        L.robust, L.huber_delta, L.scale_sqr = int(robust), float(huber_delta), float(scale_sqr)
        hit = np.zeros((rows, cols), np.int32)
        r, w, J = np.zeros((rows, cols), np.float32), np.zeros((rows, cols), np.float32), np.zeros((rows, cols, 6), np.float32)
        if self.device:
            rc = self.lib.dm_pixels(C.byref(L), int(mode), _p(hit), _p(r), _p(w), _p(J))
            assert rc == 0, "dm_pixels: HIP error %d" % rc
        else:
            assert mode != 2, "point_residual_g exists on the device only"
            self.lib.emu_pixels(C.byref(L), int(mode), _p(hit), _p(r), _p(w), _p(J))
        return hit, r, w, J

    def make_points(self, I1, D1, K, level):
        """make_point of every pixel of a level, its intrinsics make_level_k(*K, level) with K = (f0, cx0, cy0): [rows, cols, 13] in the
        order of a list entry (a: X Y Z i1, b: fx_z jw02 jw03 jw04, c: jw05 jw12 jw13 jw14, d: jw15)."""
        I1, D1 = _f32(I1), _f32(D1)
        rows, cols = I1.shape
        out = np.zeros((rows, cols, 13), np.float32)
        self._call("make_points", rows * cols, _p(I1), _p(D1), cols, C.c_float(K[0]), C.c_float(K[1]), C.c_float(K[2]), int(level), _p(out))
        return out

    # -- device only --
    def kf_lists(self, sets, K, dense_above=0, spare=3, by_ref=False):
        """The keyframe point lists of `sets` = [[(I1, D1) of level 0, of level 1, ...], ...]: level shapes shared by the sets, contents
        their own. by_ref False: kf_count_kernel + kf_fill_kernel as the product launches them, one pair per set; True: the by-reference
        bodies over a table, one entry per set, in one pair of launches. Everything starts as 0xAB bytes and is built twice into the same
        buffers. Per set: dict(rowcnt [2, rows_total + 1] int32, npts [2, 8] int32, lists = for each of the 8 levels [2, interior +
        spare, 13] float32)."""
        shapes = [np.shape(im) for im, _ in sets[0]]
        assert all([np.shape(im) for im, _ in s] == shapes and all(np.shape(d) == np.shape(im) for im, d in s) for s in sets)
        n_sets, n_levels = len(sets), len(shapes)
        rows, cols = _i32([s[0] for s in shapes]), _i32([s[1] for s in shapes])
        I1 = _f32(np.stack([np.concatenate([_f32(im).ravel() for im, _ in s]) for s in sets]))
        D1 = _f32(np.stack([np.concatenate([_f32(d).ravel() for _, d in s]) for s in sets]))
        inner = [(r - 8, c - 8) if r > 8 and c > 8 else (0, 0) for r, c in shapes] + [(0, 0)] * (MAX_LEVELS - n_levels)
        cap = [ih * iw + spare for ih, iw in inner]
        rt, ct = sum(ih for ih, _ in inner), sum(cap)
        rowcnt, npts = np.zeros((2, n_sets, rt + 1), np.int32), np.zeros((2, n_sets, MAX_LEVELS), np.int32)
        a, b, c = (np.zeros((2, n_sets, ct, 4), np.float32) for _ in range(3))
        d = np.zeros((2, n_sets, ct, 1), np.float32)
        rc = self.lib.dm_kf_lists(n_sets, int(bool(by_ref)), n_levels, _p(rows), _p(cols), _p(I1), _p(D1), C.c_float(K[0]), C.c_float(K[1]),
                                  C.c_float(K[2]), int(dense_above), int(spare), _p(rowcnt), _p(npts), _p(a), _p(b), _p(c), _p(d))
        assert rc == 0, "dm_kf_lists: HIP error %d" % rc
        out = []
        for i in range(n_sets):
            lists, at = [], 0
            for n in cap:
                lists.append(np.concatenate([v[:, i, at:at + n] for v in (a, b, c, d)], axis=2))
                at += n
            out.append(dict(rowcnt=rowcnt[:, i], npts=npts[:, i], lists=lists))
        return out

    def list_eval(self, I1, I2, D1, k, T, nblk, n_cap, robust=1, huber_delta=28.0, scale_sqr=1.0, active=1, level_ok=1):
        """The level's list built by kf_count_kernel / kf_fill_kernel, then lm_residual_only_list_kernel and lm_residual_list_kernel on
        nblk blocks, twice, every launch into 0xAB bytes. Returns (n = the level's point count, partial rows [2, nblk + 1, 29], residuals
        [2, n_cap]); n_cap >= n."""
        I1, I2, D1 = _f32(I1), _f32(I2), _f32(D1)
        rows, cols = I1.shape
        L = PixLevel(I1.ctypes.data, I2.ctypes.data, D1.ctypes.data, rows, cols, LevelK(*k))
        L.T[:] = [float(v) for v in _f32(np.asarray(T, np.float32).T).reshape(16)]
        L.robust, L.huber_delta, L.scale_sqr = int(robust), float(huber_delta), float(scale_sqr)
        found = np.full(1, -1, np.int32)
        partials, res = np.zeros((2, nblk + 1, 29), np.float64), np.zeros((2, n_cap), np.float32)
        rc = self.lib.dm_list_eval(C.byref(L), int(nblk), int(active), int(level_ok), int(n_cap), _p(found), _p(partials), _p(res))
        assert rc == 0, "dm_list_eval: HIP error %d (the level's list holds %d points, room for %d)" % (rc, found[0], n_cap)
        return int(found[0]), partials, res

    def _wave(self, name, n, *args):
        off = np.zeros(n, np.int32)
        self._call(name, n, *args, _p(off))
        return off

    def sincos_pair_wave(self, xa, xb):
        xa, xb = _f32(xa), _f32(xb)
        out = np.zeros((len(xa), 4), np.float32)
        off = self._wave("sincos_pair_wave", len(xa), _p(xa), _p(xb), _p(out))
        return out, off

    def se3_exp_wave(self, a):
        a = _f32(a).reshape(-1, 6)
        q, M = self._qm(len(a))
        off = self._wave("se3_exp_wave", len(a), _p(a), _p(q), _p(M))
        return q, M, off

    def solve_damped_wave(self, acc, lam):
        acc, lam = _f64(acc).reshape(-1, 29), _f32(lam)
        d = np.zeros((len(acc), 6), np.float32)
        off = self._wave("solve_damped_wave", len(acc), _p(acc), _p(lam), _p(d))
        return d, off

    def apply_step_wave(self, states):
        states = np.ascontiguousarray(states, LM_STATE)
        out = np.zeros(len(states), LM_STATE)
        off = self._wave("apply_step_wave", len(states), _p(states), _p(out))
        return out, off

    def dense_pixels(self, I1, I2, D1, k, T, fast, robust=1, huber_delta=28.0, scale_sqr=1.0):
        """dense_stage_a + dense_stage_b per pixel: hit [rows, cols], the pixel's 29 products [rows, cols, 29]."""
        I1, I2, D1 = _f32(I1), _f32(I2), _f32(D1)
        rows, cols = I1.shape
        L = DenseLevel(I1.ctypes.data, I2.ctypes.data, D1.ctypes.data, rows, cols, LevelK(*k))
        Tc = _f32(np.asarray(T, np.float32).T).reshape(16)
        hit, acc = np.zeros((rows, cols), np.int32), np.zeros((rows, cols, 29), np.float64)
        rc = self.lib.dm_dense_pixels(C.byref(L), _p(Tc), int(robust), C.c_float(huber_delta), C.c_float(scale_sqr), int(fast), _p(hit), _p(acc))
        assert rc == 0, "dm_dense_pixels: HIP error %d" % rc
        return hit, acc

    # -- the dense scan block by block, the scale kernels (device only) --
    @staticmethod
    def _dense_level(I1, I2, D1, k):
        rows, cols = I1.shape
        return DenseLevel(I1.ctypes.data, I2.ctypes.data, D1.ctypes.data, rows, cols, LevelK(*k))

    def dense_runs(self, rows, cols, cap, n_rows):
        """((n_strips, n_rg, nblk), dense_block_run of every block [nblk, 5]) as the device computes them for grid cap `cap`."""
        L = DenseLevel(None, None, None, rows, cols, LevelK(1.0, 0.0, 0.0, 0))
        geom, out = np.zeros(3, np.int32), np.full((n_rows, 5), -1, np.int32)
        rc = self.lib.dm_dense_runs(C.byref(L), int(cap), int(n_rows), _p(geom), _p(out))
        assert rc == 0, "dm_dense_runs: HIP error %d" % rc
        return tuple(int(v) for v in geom), out[:geom[2]]

    def dense_eval(self, I1, I2, D1, k, T, cap, n_rows, robust=1, huber_delta=28.0, scale_sqr=1.0, plain_div=0):
        """lm_dense_eval_kernel as launch_dense_eval launches it: the partial rows [n_rows, 29] (rows past the level's nblk keep their
        0xAB fill)."""
        I1, I2, D1 = _f32(I1), _f32(I2), _f32(D1)
        L = self._dense_level(I1, I2, D1, k)
        Tc = _f32(np.asarray(T, np.float32).T).reshape(16)
        out = np.zeros((n_rows, 29), np.float64)
        rc = self.lib.dm_dense_eval(C.byref(L), int(cap), _p(Tc), int(robust), C.c_float(huber_delta), C.c_float(scale_sqr), int(plain_div),
                                    int(n_rows), _p(out))
        assert rc == 0, "dm_dense_eval: HIP error %d" % rc
        return out

    def dense_eval_batch(self, items, plain_div=0):
        """lm_dense_eval_batch_kernel over items = [dict(I1, I2, D1, k, T, cap, n_rows, robust, huber_delta, scale_sqr, active)]: one
        array of partial rows per item."""
        n = len(items)
        keep = [[_f32(it[a]) for a in ("I1", "I2", "D1")] for it in items]
        Ls = (DenseLevel * n)(*[self._dense_level(*imgs, it["k"]) for imgs, it in zip(keep, items)])
        T = _f32(np.stack([np.asarray(it["T"], np.float32).T.reshape(16) for it in items]))
        off = _i32(np.concatenate([[0], np.cumsum([it["n_rows"] for it in items])]))
        out = np.zeros((int(off[-1]), 29), np.float64)
        rc = self.lib.dm_dense_eval_batch(n, Ls, _p(_i32([it["cap"] for it in items])), _p(T), _p(_i32([it["robust"] for it in items])),
                                          _p(_f32([it["huber_delta"] for it in items])), _p(_f32([it["scale_sqr"] for it in items])),
                                          _p(_i32([it["active"] for it in items])), int(plain_div), _p(off), _p(out))
        assert rc == 0, "dm_dense_eval_batch: HIP error %d" % rc
        return [out[off[i]:off[i + 1]] for i in range(n)]

    def tdist_scale(self, res, order, reps=1):
        """The t-distribution scale of a residual vector (NaN: no residual). order 0: list order, 1: strided, 2: the product's launch
        sequence. Returns (sigma^2 [reps] float32, info [reps, 4] = (G, gave up, writer: 0 list / 1 strided / 2 multi, 0))."""
        res = _f32(res)
        s2, info = np.zeros(reps, np.float32), np.zeros((reps, 4), np.int32)
        rc = self.lib.dm_tdist_scale(_p(res), len(res), int(order), int(reps), _p(s2), _p(info))
        assert rc == 0, "dm_tdist_scale: HIP error %d" % rc
        return s2, info

    def dense_fast_ok(self, fl, cx, cy, rows, cols):
        return int(self.lib.dm_dense_fast_ok(float(fl), float(cx), float(cy), int(rows), int(cols)))

    def _div(self, name, n, n_out, dtype, *args):
        n_bad, first, q = np.zeros(1, np.uint64), np.zeros(self.first_cap, np.int32), np.zeros((2, n_out), dtype)
        self._call(name, n, *args, _p(n_bad), _p(first), int(n_out), _p(q))
        return int(n_bad[0]), first[first >= 0], q[0], q[1]

    def div32(self, a, b, form, n_out=0):
        """form 0: div_shared against a / b; 1: recip_shared against 1 / b; 2: div_shared_z against a / b. Returns (mismatches, indices of the first few, the first
        n_out shared-form results, the first n_out plain-division results)."""
        a, b = _f32(a), _f32(b)
        return self._div("div32", len(b), n_out, np.float32, int(form), _p(a), _p(b))

    def div64(self, a, b, n_out=0):
        a, b = _f64(a), _f64(b)
        return self._div("div64", len(b), n_out, np.float64, _p(a), _p(b))

    def callsites(self, x, y, d, fl, cx, cy, T):
        """point_xyz / point_jacobian / warp, shared form against plain: (mismatch counts [3], first indices [3][<= cap])."""
        x, y, d, fl, cx, cy = _i32(x), _i32(y), _f32(d), _f64(fl), _f32(cx), _f32(cy)
        T = _f32(T).reshape(-1, 16)
        n_bad, first = np.zeros(3, np.uint64), np.zeros((3, self.first_cap), np.int32)
        self._call("callsites", len(x), _p(x), _p(y), _p(d), _p(fl), _p(cx), _p(cy), len(T), _p(T), _p(n_bad), _p(first))
        return [int(v) for v in n_bad], [f[f >= 0] for f in first]


def load_host():
    from test_hostemu_parity import load_emu
    return Ops(load_emu(), device=False)


def load_device(unit):
    return Ops(C.CDLL(build(unit)), device=True)


def same_bits(a, b):
    """Elementwise: equal bit patterns, or both NaN (the host and the device may choose different NaN payloads / signs)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))
    return a == b


def state_words(states):
    return np.ascontiguousarray(states, LM_STATE).view(np.uint32).reshape(-1, 64)


FLOAT_WORDS = np.r_[0:40, 54:60]     # the dwords of an LmState that hold floats (cur, inc, last, T, lambda, err_last, err_now; delta)


def same_states(a, b):
    """[n, 64] bool: dword for dword, NaNs as NaNs in the float fields."""
    wa, wb = state_words(a), state_words(b)
    eq = wa == wb
    fa, fb = wa[:, FLOAT_WORDS].view(np.float32), wb[:, FLOAT_WORDS].view(np.float32)
    eq[:, FLOAT_WORDS] |= np.isnan(fa) & np.isnan(fb)
    return eq
