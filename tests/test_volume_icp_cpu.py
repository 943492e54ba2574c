"""Frame-to-model tracking on the TSDF volume (odo_volume_icp_eval_dev, odo_volume_icp_align_dev, odo_volume_track_dev,
api.TsdfVolume.icp_eval / align / track) without a GPU: the ABI and the argument checks, the numpy model of the specification
(include/odometry_hip.h) pinned to the prose by a plain-loop implementation that does one fp32 operation at a
time, every branch of the specification reached by a row made for it, the host + device header
odometry_amd/csrc/volume_icp_math.h compiled by g++ as a library and, with sanitizers, as a program, a Python restatement of the
step, the model against the ground truth of a narrow ribbed corridor, its refusal of the pinned corridor, and the kernels'
code-object metadata.

The model is the yardstick of tests/test_gpu_volume_icp.py, which asks the GPU for the same bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from test_volume_cpu import _pose, bits, empty_grid, integrate_model, params, world_to_camera
from test_volume_raycast_cpu import default_view, raycast_model, tiny_volumes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NACC = 29

NEW_SYMBOLS = ["odo_volume_icp_eval_dev", "odo_volume_icp_align_dev", "odo_volume_track_dev", "odo_volume_icp_time_dev"]
# The instantiations for 29 sums of the kernel templates of volume_icp_kernels.hip, as the code object names them.
ICP_KERNELS = ["volume_icp_rows_kernelILi29E", "volume_icp_step_kernelILi29E", "volume_icp_init_kernelILi29E"]
TALLIES = ("raw0", "far", "behind", "off_left", "off_right", "off_top", "off_bottom", "nan_proj", "model_hole", "normal_zero", "gated",
           "on_gate", "huber_below", "huber_on", "huber_above", "pairs", "lattice")

# The ground truth's scene, grid and procedure: a narrow corridor with ribs across it constrains all six
# degrees of freedom; the project's own corridor (four planes parallel to the drive) does not, and is the test of the refusal.
RIBBED_SCENE = dict(spectrum=1.55, sigma=80.0, half_width=(1.5, 1.5), ceil_height=1.0, cam_height=1.2, ribs=(2.0, 1.0, 1.8))
RIBBED_GRID = dict(dims=(136, 104, 208), vs=0.025, origin=(-1.7, -1.2, 0.3), mu=0.075, max_depth=5.0, max_weight=65535)
SMALL = (120, 160)
# Measured with this model (test_ground_truth_on_the_ribbed_corridor prints them): the largest error of the six frames. The
# assertions there and in tests/test_gpu_volume_icp.py are twice these.
MEASURED_T_M = 0.004357      # frame 3
MEASURED_R_DEG = 0.2253     # frame 1, against a volume of one frame
# The geometric mean of the two cases' eig_min / eig_max as measured with this model (largest of the pinned corridor 6.5e-4, smallest
# of the ribbed corridor 4.95e-3): it separates them, by a factor 2.8 either way. Too little for a default; the refusal tests set it.
REFUSAL_RATIO = 1.8e-3


def icp(strides=(4, 2, 1), iters=(4, 5, 10), dist_max=None, huber_delta=0.0, eps_t=1e-5, eps_r=1e-5, min_pairs=None, min_eig_ratio=None,
        p=None):
    """The model's odo_icp_params; the defaults of api.TsdfVolume.icp_params for the volume parameters p."""
    from odometry_amd import api
    rows, cols = p["size"]
    s0 = strides[0]
    return dict(strides=tuple(strides), iters=tuple(iters), dist_max=2 * float(f32(p["mu"])) if dist_max is None else dist_max,
                huber_delta=huber_delta, eps_t=eps_t, eps_r=eps_r,
                min_pairs=max(6, (-(-rows // s0)) * (-(-cols // s0)) // 64) if min_pairs is None else min_pairs,
                min_eig_ratio=api.TsdfVolume.ICP_MIN_EIG_RATIO if min_eig_ratio is None else min_eig_ratio)


# ---- the model: host part ------------------------------------------------------------------------------------------------------
def mul4(A, B):
    """A B of two 4x4 fp32 matrices: fp64 from the fp32 entries, ((a_r0 b_0c + a_r1 b_1c) + a_r2 b_2c) + a_r3 b_3c, rounded once."""
    A, B = np.asarray(A, f32).astype(np.float64), np.asarray(B, f32).astype(np.float64)
    out = np.zeros((4, 4), np.float64)
    with np.errstate(all="ignore"):
        for r in range(4):
            for c in range(4):
                out[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
        return out.astype(f32)


def icp_frame(P_m, P_init):
    """M (world to model camera) and C0 = M P_init."""
    M = world_to_camera(P_m)
    return M, mul4(M, P_init)


# ---- the model: rows -------------------------------------------------------------------------------------------------------------
def icp_rows_model(raw, depth_m, nrmw_m, M, Cm, p, stride, dist_max, huber_delta):
    """(rows, cols, 8) float32 {J0 .. J5, res, w} — zeros where there is no pair — and the mask of the pairs."""
    rows, cols = p["size"]
    f, cx, cy = (f32(v) for v in p["K"])
    scale, maxd = f32(p["depth_scale"]), f32(p["max_depth"])
    dist_max, huber_delta = f32(dist_max), f32(huber_delta)
    Cm, M = np.asarray(Cm, f32), np.asarray(M, f32)
    ys, xs = np.arange(0, rows, stride), np.arange(0, cols, stride)
    X, Y = [a.reshape(-1) for a in np.meshgrid(xs, ys)]
    with np.errstate(all="ignore"):
        r = np.asarray(raw, np.uint16)[Y, X]
        ok = r != 0
        D = r.astype(f32) / scale
        ok &= ~(D > maxd)
        dx, dy = (X.astype(f32) - cx) / f, (Y.astype(f32) - cy) / f
        pt = [dx * D, dy * D, D]
        pm = [((Cm[k, 0] * pt[0] + Cm[k, 1] * pt[1]) + Cm[k, 2] * pt[2]) + Cm[k, 3] for k in range(3)]
        ok &= pm[2] > f32(0.0)
        u, v = f * (pm[0] / pm[2]) + cx, f * (pm[1] / pm[2]) + cy
        xi, yi = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        ok &= (xi >= f32(0.0)) & (xi < f32(cols)) & (yi >= f32(0.0)) & (yi < f32(rows))      # as floats; NaN fails
        xj, yj = np.where(ok, xi, f32(0.0)).astype(np.int64), np.where(ok, yi, f32(0.0)).astype(np.int64)
        zm = np.asarray(depth_m, f32)[yj, xj]
        ok &= zm > f32(0.0)
        nw = np.asarray(nrmw_m, f32)[yj, xj, :3]
        ok &= ~((nw[:, 0] == 0) & (nw[:, 1] == 0) & (nw[:, 2] == 0))
        n = [(M[k, 0] * nw[:, 0] + M[k, 1] * nw[:, 1]) + M[k, 2] * nw[:, 2] for k in range(3)]
        vm = [((xi - cx) / f) * zm, ((yi - cy) / f) * zm, zm]
        d = [pm[k] - vm[k] for k in range(3)]
        dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        ok &= dd <= dist_max * dist_max
        res = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]
        J = [n[0], n[1], n[2], pm[1] * n[2] - pm[2] * n[1], pm[2] * n[0] - pm[0] * n[2], pm[0] * n[1] - pm[1] * n[0]]
        if huber_delta > 0:
            w = np.where(np.abs(res) <= huber_delta, f32(1.0), huber_delta / np.abs(res))
        else:
            w = np.ones(len(res), f32)
        row = np.stack(J + [res, w], 1).astype(f32)
    out = np.zeros((rows, cols, 8), f32)
    out[Y, X] = np.where(ok[:, None], row, f32(0.0))
    mask = np.zeros((rows, cols), bool)
    mask[Y, X] = ok
    return out, mask


def icp_terms(rows8, mask):
    """The exact fp64 terms of the 29 sums, one row of 29 per pair, in raster order."""
    r = rows8[mask]
    with np.errstate(all="ignore"):
        jw = (r[:, :6] * r[:, 7:8]).astype(f32).astype(np.float64)
        rw = (r[:, 6] * r[:, 7]).astype(f32).astype(np.float64)
        Jd, rd = r[:, :6].astype(np.float64), r[:, 6].astype(np.float64)
        cols = [jw[:, a] * Jd[:, b] for a in range(6) for b in range(a, 6)] + [jw[:, a] * rd for a in range(6)] + [rw * rd, np.ones(len(r))]
    return np.stack(cols, 1) if len(r) else np.zeros((0, NACC))


def icp_acc(rows8, mask):
    """The 29 sums in fp64 (numpy's pairwise order) and, per sum, the sum of the terms' magnitudes."""
    t = icp_terms(rows8, mask)
    return t.sum(0), np.abs(t).sum(0)


ICP_TILE, ICP_LANES = 16, 8      # kIcpTile and kIcpFoldLanes of odometry_amd/csrc/volume_icp.hip.h


def icp_lane_sums(terms):
    """(n, k) fp64 terms, summed as eight lanes do: lane s starts at +0.0 and adds rows s, s + 8, s + 16, ... in that order, then the
    lanes are folded as ((0 + 4) + (2 + 6)) + ((1 + 5) + (3 + 7))."""
    terms = np.asarray(terms, np.float64)
    v = np.zeros((ICP_LANES,) + terms.shape[1:])
    with np.errstate(all="ignore"):
        for i in range(0, len(terms), ICP_LANES):
            chunk = terms[i:i + ICP_LANES]
            v[:len(chunk)] += chunk
        return ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]))


def icp_tiles(stride, *frames):
    """The frames on the stride's lattice, cut into the rows kernel's blocks in the order block = blockIdx.y * gridDim.x + blockIdx.x:
    per block and frame an array whose first axis is the thread, t = (t % tile, t / tile); zeros outside the frame."""
    lat = [np.asarray(a)[::stride, ::stride] for a in frames]
    ly, lx = lat[0].shape[:2]
    T = ICP_TILE
    for by in range(-(-ly // T)):
        for bx in range(-(-lx // T)):
            out = []
            for a in lat:
                tile = np.zeros((T, T) + a.shape[2:], a.dtype)
                part = a[by * T:(by + 1) * T, bx * T:(bx + 1) * T]
                tile[:part.shape[0], :part.shape[1]] = part
                out.append(tile.reshape((T * T,) + a.shape[2:]))
            yield out


def icp_acc_kernel_order(rows8, mask, stride):
    """The 29 sums in the kernels' order: per block of the rows kernel the 256 rows of its threads (all-zero where there is no pair)
    through icp_lane_sums, then the blocks' partials through icp_lane_sums again. The device's bits."""
    partials = []
    for r, m in icp_tiles(stride, rows8, mask):
        t = icp_terms(r, np.ones(len(r), bool))
        t[:, NACC - 1] = m
        partials.append(icp_lane_sums(t))
    return icp_lane_sums(np.array(partials))


# ---- the same, one fp32 operation at a time --------------------------------------------------------------------------------------
def icp_rows_loop(raw, depth_m, nrmw_m, M, Cm, p, stride, dist_max, huber_delta):
    """icp_rows_model as plain loops over scalars; also the sums in raster order (accumulate_row) and how often each branch was taken."""
    rows, cols = p["size"]
    f, cx, cy = (f32(v) for v in p["K"])
    scale, maxd = f32(p["depth_scale"]), f32(p["max_depth"])
    dist_max, huber_delta = f32(dist_max), f32(huber_delta)
    Cm, M = np.asarray(Cm, f32), np.asarray(M, f32)
    half, zero = f32(0.5), f32(0.0)
    out = np.zeros((rows, cols, 8), f32)
    acc = [0.0] * NACC
    met = {k: 0 for k in TALLIES}
    with np.errstate(all="ignore"):
        gate = f32(dist_max * dist_max)
        for y in range(0, rows, stride):
            for x in range(0, cols, stride):
                met["lattice"] += 1
                r = int(raw[y, x])
                if r == 0:
                    met["raw0"] += 1
                    continue
                D = f32(f32(r) / scale)
                if D > maxd:
                    met["far"] += 1
                    continue
                dx, dy = f32(f32(f32(x) - cx) / f), f32(f32(f32(y) - cy) / f)
                pt = [f32(dx * D), f32(dy * D), D]
                pm = [f32(f32(f32(f32(Cm[k, 0] * pt[0]) + f32(Cm[k, 1] * pt[1])) + f32(Cm[k, 2] * pt[2])) + Cm[k, 3]) for k in range(3)]
                if not pm[2] > zero:
                    met["behind"] += 1
                    continue
                u = f32(f32(f * f32(pm[0] / pm[2])) + cx)
                v = f32(f32(f * f32(pm[1] / pm[2])) + cy)
                xi, yi = np.floor(f32(u + half)), np.floor(f32(v + half))
                if np.isnan(xi) or np.isnan(yi):
                    met["nan_proj"] += 1
                    continue
                if not xi >= zero:
                    met["off_left"] += 1
                    continue
                if not xi < f32(cols):
                    met["off_right"] += 1
                    continue
                if not yi >= zero:
                    met["off_top"] += 1
                    continue
                if not yi < f32(rows):
                    met["off_bottom"] += 1
                    continue
                zm = f32(depth_m[int(yi), int(xi)])
                if not zm > zero:
                    met["model_hole"] += 1
                    continue
                nw = [f32(c) for c in nrmw_m[int(yi), int(xi), :3]]
                if nw[0] == 0 and nw[1] == 0 and nw[2] == 0:
                    met["normal_zero"] += 1
                    continue
                n = [f32(f32(f32(M[k, 0] * nw[0]) + f32(M[k, 1] * nw[1])) + f32(M[k, 2] * nw[2])) for k in range(3)]
                vm = [f32(f32(f32(xi - cx) / f) * zm), f32(f32(f32(yi - cy) / f) * zm), zm]
                d = [f32(pm[k] - vm[k]) for k in range(3)]
                dd = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
                if not dd <= gate:
                    met["gated"] += 1
                    continue
                met["on_gate"] += int(dd == gate)
                res = f32(f32(f32(n[0] * d[0]) + f32(n[1] * d[1])) + f32(n[2] * d[2]))
                J = [n[0], n[1], n[2], f32(f32(pm[1] * n[2]) - f32(pm[2] * n[1])), f32(f32(pm[2] * n[0]) - f32(pm[0] * n[2])),
                     f32(f32(pm[0] * n[1]) - f32(pm[1] * n[0]))]
                w = f32(1.0)
                if huber_delta > 0:
                    a = np.abs(res)
                    met["huber_below" if a < huber_delta else "huber_on" if a == huber_delta else "huber_above"] += 1
                    if not a <= huber_delta:
                        w = f32(huber_delta / a)
                out[y, x] = J + [res, w]
                met["pairs"] += 1
                jw = [float(f32(J[a] * w)) for a in range(6)]
                k = 0
                for a in range(6):
                    for b in range(a, 6):
                        acc[k] += jw[a] * float(J[b])          # exact products of fp32 values: what fma adds
                        k += 1
                for a in range(6):
                    acc[21 + a] += jw[a] * float(res)
                acc[27] += float(f32(res * w)) * float(res)
                acc[28] += 1.0
    return out, np.array(acc), met


# ---- a Python restatement of the step (odo_math.h's solve, exponential and compose, icp_step's rule) -----------------------------
def _sincos(xf):
    x = float(xf)
    kf = float(np.floor(x * 6.36619772367581382433e-01 + 0.5))
    r = (x - kf * 1.57079632673412561417e+00) - kf * 6.07710050650619224932e-11
    r2 = r * r
    ps = 1.0 / 355687428096000.0
    for c in (-1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0):
        ps = ps * r2 + c
    sr = ps * r
    pc = 1.0 / 6402373705728000.0
    for c in (-1.0 / 20922789888000.0, 1.0 / 87178291200.0, -1.0 / 479001600.0, 1.0 / 3628800.0, -1.0 / 40320.0, 1.0 / 720.0, -1.0 / 24.0,
              1.0 / 2.0):
        pc = pc * r2 + c
    pc = pc * r2
    cr = 1.0 - pc
    q = int(kf) & 3
    s, c = ((sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr))[q]
    return f32(s), f32(c)


def _quat_to_rot(q):
    qx, qy, qz, qw = q[:4]
    two, one = f32(2), f32(1)
    tx, ty, tz = two * qx, two * qy, two * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)]


def _rot_to_quat(R):
    half, one = f32(0.5), f32(1)
    t = (R[0] + R[4]) + R[8]
    if t > 0:
        t = np.sqrt(t + one)
        qw = half * t
        t = half / t
        return ((R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t, qw)
    i = 1 if R[4] > R[0] else 0
    if R[8] > (R[4] if i == 1 else R[0]):
        i = 2
    if i == 0:
        t = np.sqrt(((R[0] - R[4]) - R[8]) + one)
        qx = half * t
        t = half / t
        return (qx, (R[3] + R[1]) * t, (R[6] + R[2]) * t, (R[7] - R[5]) * t)
    if i == 1:
        t = np.sqrt(((R[4] - R[8]) - R[0]) + one)
        qy = half * t
        t = half / t
        return ((R[1] + R[3]) * t, qy, (R[7] + R[5]) * t, (R[2] - R[6]) * t)
    t = np.sqrt(((R[8] - R[0]) - R[4]) + one)
    qz = half * t
    t = half / t
    return ((R[2] + R[6]) * t, (R[5] + R[7]) * t, qz, (R[3] - R[1]) * t)


def _se3_to_colmajor(s):
    R = _quat_to_rot(s)
    Mx = [f32(0)] * 16
    for i in range(3):
        for j in range(3):
            Mx[j * 4 + i] = R[i * 3 + j]
    Mx[12], Mx[13], Mx[14], Mx[15] = s[4], s[5], s[6], f32(1)
    return Mx


def _se3_exp(a):
    a = [f32(v) for v in a]
    ox, oy, oz = a[3], a[4], a[5]
    theta_sq = (ox * ox + oy * oy) + oz * oz
    theta = np.sqrt(theta_sq)
    half_theta = f32(0.5) * theta
    small = theta < f32(1e-5)
    if small:
        po4 = theta_sq * theta_sq
        imag = (f32(0.5) - f32(1.0 / 48.0) * theta_sq) + f32(1.0 / 3840.0) * po4
        real = (f32(1.0) - f32(1.0 / 8.0) * theta_sq) + f32(1.0 / 384.0) * po4
    else:
        sh, ch = _sincos(half_theta)
        imag, real = sh / theta, ch
    q = (imag * ox, imag * oy, imag * oz, real)
    z = f32(0)
    Om = [z, -oz, oy, oz, z, -ox, -oy, ox, z]
    Om2 = [(Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j]) + Om[i * 3 + 2] * Om[6 + j] for i in range(3) for j in range(3)]
    if small:
        V = _quat_to_rot(q)
    else:
        st, ct = _sincos(theta)
        tsq = theta * theta
        ca = (f32(1.0) - ct) / tsq
        cb = (theta - st) / (tsq * theta)
        V = [((f32(1.0) if i in (0, 4, 8) else z) + ca * Om[i]) + cb * Om2[i] for i in range(9)]
    t = [(V[3 * i] * a[0] + V[3 * i + 1] * a[1]) + V[3 * i + 2] * a[2] for i in range(3)]
    return q + tuple(t)


def _solve(acc):
    """odo::solve_damped(acc, 0.0f) in Python floats (fp64)."""
    A = [[0.0] * 7 for _ in range(6)]
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = float(acc[k])
            k += 1
    for a in range(6):
        A[a][a] = A[a][a] + 0.0 * A[a][a]
        A[a][6] = -float(acc[21 + a])
    ok = [False] * 6
    for c in range(6):
        ok[c] = abs(A[c][c]) > 0.0
        if ok[c]:
            for i in range(c + 1, 6):
                fct = A[i][c] / A[c][c]
                for j in range(c, 7):
                    A[i][j] = A[i][j] - fct * A[c][j]
    rinv = [1.0 / A[c][c] if ok[c] else 0.0 for c in range(6)]
    xs = [0.0] * 6
    for c in range(5, -1, -1):
        s = A[c][6]
        for j in range(c + 1, 6):
            s = s - A[c][j] * xs[j]
        xs[c] = s * rinv[c] if ok[c] else 0.0
    return np.array(xs).astype(f32)


def icp_step_py(acc, Cm, min_pairs, eps_t, eps_r):
    """icp_step: (failed, converged, delta (6,), C' 4x4). Cm: 4x4 float32."""
    acc = np.asarray(acc, np.float64)
    Cm = np.asarray(Cm, f32)
    if not (acc[28] >= min_pairs and np.isfinite(acc).all()):
        return 1, 0, np.zeros(6, f32), Cm.copy()
    with np.errstate(all="ignore"):
        delta = _solve(acc)
        Dm = _se3_to_colmajor(_se3_exp(delta))
        Cc = [f32(v) for v in Cm.T.reshape(16)]
        Mx = [f32(0)] * 16
        for i in range(4):
            for j in range(4):
                Mx[j * 4 + i] = ((Dm[i] * Cc[j * 4] + Dm[4 + i] * Cc[j * 4 + 1]) + Dm[8 + i] * Cc[j * 4 + 2]) + Dm[12 + i] * Cc[j * 4 + 3]
        R = [Mx[j * 4 + i] for i in range(3) for j in range(3)]
        moved = tuple(_rot_to_quat(R)) + (Mx[12], Mx[13], Mx[14])
        out = np.array(_se3_to_colmajor(moved), f32).reshape(4, 4).T.copy()
        nt = np.sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2])
        nr = np.sqrt((delta[3] * delta[3] + delta[4] * delta[4]) + delta[5] * delta[5])
    return 0, int(nt < f32(eps_t) and nr < f32(eps_r)), delta, out


def acc_matrix(acc):
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[a, b] = A[b, a] = acc[k]
            k += 1
    return A


def icp_align_model(raw, depth_m, nrmw_m, P_m, P_init, p, ic, step=icp_step_py, sums=None, strided_sums=None):
    """The whole loop: dict(status, iterations, pairs, cost, eig_min, eig_max, C, abs_pose, trace [(level, acc, delta, C)]). step: the
    step function (the Python restatement, or the host library's); sums(rows8, mask) -> acc: the order of the sums (default: fp64
    pairwise); strided_sums(rows8, mask, stride) -> acc: the same for an order that depends on the level's stride, as the kernels'
    does (icp_acc_kernel_order)."""
    if strided_sums:
        assert sums is None
    M, Cm = icp_frame(P_m, P_init)
    status, n, trace, acc = 0, 0, [], None
    for level, (stride, iters) in enumerate(zip(ic["strides"], ic["iters"])):
        for _ in range(iters):
            if status:
                break
            rows8, mask = icp_rows_model(raw, depth_m, nrmw_m, M, Cm, p, stride, ic["dist_max"], ic["huber_delta"])
            acc = strided_sums(rows8, mask, stride) if strided_sums else sums(rows8, mask) if sums else icp_acc(rows8, mask)[0]
            failed, converged, delta, Cm = step(acc, Cm, ic["min_pairs"], ic["eps_t"], ic["eps_r"])
            trace.append((level, acc, delta, Cm))
            n += 1
            status = 1 if failed else 0
            if converged:
                break
    out = dict(status=status, iterations=n, pairs=0.0, cost=0.0, eig_min=0.0, eig_max=0.0, C=Cm, trace=trace)
    if acc is not None:
        ev = np.linalg.eigvalsh(acc_matrix(acc)) if np.isfinite(acc).all() else np.full(6, np.nan)
        out.update(pairs=acc[28], cost=acc[27], eig_min=ev[0], eig_max=ev[-1])
    if out["status"] == 0 and not np.isfinite(Cm).all():
        out["status"] = 1
    if out["status"] == 0 and (acc is None or out["eig_min"] < float(f32(ic["min_eig_ratio"])) * out["eig_max"]):
        out["status"] = 2 if acc is not None else 1
    out["abs_pose"] = mul4(P_m, Cm) if out["status"] == 0 else np.full((4, 4), np.nan, f32)
    return out


def pose_error(A, B):
    """Translation distance (metres) and rotation angle (degrees) between two camera-to-world poses."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    R = A[:3, :3].T @ B[:3, :3]
    return float(np.linalg.norm(A[:3, 3] - B[:3, 3])), float(np.degrees(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))))


# ---- frames --------------------------------------------------------------------------------------------------------------------
def random_frames(seed, size=(24, 32), K=(30.0, 15.5, 11.5), motion=((0.01, -0.015, 0.02), (0.02, -0.01, 0.015))):
    """A random sensor frame and a random model frame with holes, zero normals and far readings, and a small motion (rotation angles,
    translation) between them."""
    rng = np.random.default_rng(100 + seed)
    p = params(K, 1000.0, size, dims=(4, 4, 4), vs=0.5, origin=(0.0, 0.0, 0.0), mu=0.1, max_depth=4.0, max_weight=5)
    base = 1.5 + 0.4 * np.sin(np.arange(size[1]) / 5.0)[None, :] + 0.3 * np.cos(np.arange(size[0]) / 4.0)[:, None]
    raw = np.rint((base + rng.normal(0, 0.01, size)) * 1000).astype(np.uint16)
    raw[rng.uniform(size=size) < 0.1] = 0
    raw[rng.uniform(size=size) < 0.05] = 65535
    depth = (base + rng.normal(0, 0.01, size)).astype(f32)
    depth[rng.uniform(size=size) < 0.1] = 0
    n = rng.normal(size=size + (3,)) * 0.3 + np.array([0.0, 0.0, -1.0])
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    nrmw = np.concatenate([n, rng.integers(1, 9, size + (1,))], 2).astype(f32)
    nrmw[rng.uniform(size=size) < 0.1] = 0
    P_m = _pose((0.1 * seed, -0.2, 0.05), (0.3, -0.1, 0.2 * seed))
    P_init = P_m @ _pose(*motion)
    return p, raw, depth, nrmw, P_m, P_init


def tiny_views():
    """The tiny volumes' ray-casts from their own poses as model frames, their frames' raw depth as sensor frames: (p, raw, depth,
    nrmw, P_m, P_init), the 3e38 poses among them."""
    out = []
    from test_volume_cpu import tiny_cases
    for (p, q, w, col, poses), (_, frames) in zip(tiny_volumes(), tiny_cases()):
        rp = default_view(p, n_steps=30)
        for k, pose in enumerate(poses):
            depth, _, nrmw, _ = raycast_model(q, w, None, pose, p, rp)
            raw, other = frames[(k + 1) % len(frames)]
            out.append((p, raw, depth, nrmw, pose, other))
    return out


EXACT_K = (4.0, 0.0, 0.0)      # dx = x / 4: with D = 2 and a translation of 2 along z every quantity below is a dyadic rational


def exact_frame(size=(4, 6), zm=3.5):
    """raw = 2000 at 1000 per metre (D = 2 exactly), the model a plane at depth zm facing the camera, identity poses."""
    p = params(EXACT_K, 1000.0, size, dims=(4, 4, 4), vs=0.5, origin=(0.0, 0.0, 0.0), mu=0.25, max_depth=8.0, max_weight=5)
    raw = np.full(size, 2000, np.uint16)
    depth = np.full(size, zm, f32)
    nrmw = np.zeros(size + (4,), f32)
    nrmw[..., 2], nrmw[..., 3] = -1.0, 1.0
    return p, raw, depth, nrmw


def branch_rows():
    """(name, p, raw, depth, nrmw, M, C, stride, dist_max, huber_delta, predicate on the loop's tallies): each row is there for the
    branch its predicate names."""
    out = []
    eye = np.eye(4, dtype=f32)
    fwd = _pose(t=(0.0, 0.0, 2.0)).astype(f32)            # pm_z = 4

    def add(name, fr, Cm, pred, stride=1, dist_max=1.0, huber=0.0, M=eye):
        p, raw, depth, nrmw = fr
        out.append((name, p, raw, depth, nrmw, M, Cm, stride, dist_max, huber, pred))

    p, raw, depth, nrmw = exact_frame()
    holes = raw.copy()
    holes[::2, ::3] = 0
    add("raw 0", (p, holes, depth, nrmw), fwd, lambda m: m["raw0"] == 4 and m["pairs"] == m["lattice"] - 4)
    far = raw.copy()
    far[1, :] = 65535
    add("D > max_depth", (p, far, depth, nrmw), fwd, lambda m: m["far"] == 6 and m["pairs"] > 0)
    add("pm_z <= 0", exact_frame(), _pose(t=(0.0, 0.0, -2.0)), lambda m: m["behind"] == m["lattice"] and m["pairs"] == 0)
    add("pm_z negative", exact_frame(), _pose(t=(0.0, 0.0, -3.0)), lambda m: m["behind"] == m["lattice"])
    add("off the left edge", exact_frame(), _pose(t=(-8.0, 0.0, 2.0)), lambda m: m["off_left"] == m["lattice"])
    add("off the right edge", exact_frame(), _pose(t=(8.0, 0.0, 2.0)), lambda m: m["off_right"] == m["lattice"])
    add("off the top edge", exact_frame(), _pose(t=(0.0, -8.0, 2.0)), lambda m: m["off_top"] == m["lattice"])
    add("off the bottom edge", exact_frame(), _pose(t=(0.0, 8.0, 2.0)), lambda m: m["off_bottom"] == m["lattice"])
    nanC = fwd.copy()
    nanC[0, 0], nanC[0, 2] = 3e38, -3e38                  # pm_x = (+inf) + (-inf) where p_x >= 1.5 (x >= 3), -inf left of that
    add("a NaN projection", exact_frame(), nanC, lambda m: m["nan_proj"] == 4 * 3 and m["off_left"] == 4 * 3)
    hole = depth.copy()
    hole[0, :2] = 0
    add("model depth 0", (p, raw, hole, nrmw), fwd, lambda m: m["model_hole"] > 0 and m["pairs"] > 0, dist_max=4.0)
    flat = nrmw.copy()
    flat[0, :2, :3] = 0
    add("a zero normal", (p, raw, depth, flat), fwd, lambda m: m["normal_zero"] > 0 and m["model_hole"] == 0 and m["pairs"] > 0, dist_max=4.0)
    # pixel (0, 0): pm = (0, 0, 4) lands on model pixel (0, 0) at zm = 3.5: d = (0, 0, 0.5), dd = 0.25 = dist_max^2 exactly; its
    # neighbours have a d_x of their own and are gated
    add("dd exactly on the gate", exact_frame(), fwd, lambda m: m["on_gate"] >= 1 and m["gated"] > 0 and m["pairs"] == m["on_gate"],
        dist_max=0.5)
    step = depth.copy()                                    # res = -(4 - zm) by column: 0.125, 0.25, 0.5
    step[:, 0], step[:, 1], step[:, 2:] = 3.875, 3.75, 3.5
    add("Huber below, on and above delta", (p, raw, step, nrmw), fwd,
        lambda m: m["huber_below"] > 0 and m["huber_on"] > 0 and m["huber_above"] > 0, dist_max=4.0, huber=0.25)
    for s in (1, 2, 4, 16):
        fr = exact_frame((17, 23))
        add(f"stride {s} on 17 x 23", fr, fwd, lambda m, s=s: m["lattice"] == (-(-17 // s)) * (-(-23 // s)) and m["pairs"] > 0, stride=s, dist_max=4.0)
    add("no pair at all", (p, np.zeros_like(raw), depth, nrmw), fwd, lambda m: m["pairs"] == 0 and m["raw0"] == m["lattice"])
    return out


def rows_equal(got, want, tag=""):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (tag, int((bits(got) != bits(want)).sum()))


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    assert C.sizeof(_lib.IcpParams) == 52 and C.sizeof(_lib.IcpResult) == 104 and C.sizeof(_lib.IcpTraceRow) == 328
    for t in ("odo_icp_params", "odo_icp_result", "odo_icp_trace_row"):
        assert t in hdr
    for name in ("icp_params", "icp_eval", "icp_time", "align", "track"):
        assert callable(getattr(api.TsdfVolume, name))


def good_params():
    from odometry_amd import _lib as L
    p = L.IcpParams()
    p.levels = 3
    p.stride[:], p.iters[:] = (4, 2, 1), (4, 5, 10)
    p.dist_max, p.huber_delta, p.eps_t, p.eps_r, p.min_pairs, p.min_eig_ratio = 0.15, 0.0, 1e-5, 1e-5, 100, 1e-4
    return p


BAD_PARAMS = [dict(levels=0), dict(levels=4), dict(stride=(0, 2, 1)), dict(stride=(4, 17, 1)), dict(stride=(4, 2, -1)), dict(iters=(4, -1, 10)),
              dict(iters=(0, 0, 0)), dict(iters=(30, 30, 5)), dict(iters=(65, 0, 0)), dict(dist_max=0.0), dict(dist_max=-1.0),
              dict(dist_max=float("nan")), dict(dist_max=float("inf")), dict(huber_delta=-0.1), dict(huber_delta=float("nan")),
              dict(huber_delta=float("inf")), dict(eps_t=-1.0), dict(eps_t=float("nan")), dict(eps_r=-1.0), dict(eps_r=float("inf")),
              dict(min_pairs=5), dict(min_pairs=-1), dict(min_eig_ratio=-0.1), dict(min_eig_ratio=1.5), dict(min_eig_ratio=float("nan"))]


def bad_params():
    for kw in BAD_PARAMS:
        p = good_params()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        yield kw, p


def test_bad_arguments_are_refused_before_touching_a_device():
    from odometry_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(64)   # never dereferenced: every case below is refused by the argument checks
    nan, inf = float("nan"), float("inf")
    eye = (C.c_float * 16)(*np.eye(4, dtype=f32).ravel())
    out = (C.c_float * 16)()
    acc = (C.c_double * NACC)()
    res = L.IcpResult()
    for kw, p in bad_params():
        assert lib.odo_volume_icp_align_dev(fake, C.byref(p), fake, fake, eye, fake, eye, out, C.byref(res), None, 0, None) == -1, kw
        assert "odo_volume_icp_align_dev:" in L.last_error(), (kw, L.last_error())
        assert lib.odo_volume_track_dev(fake, C.byref(p), fake, eye, out, C.byref(res)) == -1, kw
        assert "odo_volume_track_dev:" in L.last_error(), (kw, L.last_error())
    good = good_params()
    for i in (0, 5, 12, 15):
        for v in (nan, inf, -inf):
            A = (C.c_float * 16)(*np.eye(4, dtype=f32).ravel())
            A[i] = v
            assert lib.odo_volume_icp_align_dev(fake, C.byref(good), fake, fake, A, fake, eye, out, C.byref(res), None, 0, None) == -1
            assert lib.odo_volume_icp_align_dev(fake, C.byref(good), fake, fake, eye, fake, A, out, C.byref(res), None, 0, None) == -1
            assert "pose" in L.last_error()
            assert lib.odo_volume_icp_eval_dev(fake, fake, fake, A, fake, eye, 1, 0.1, 0.0, acc, None) == -1
            assert lib.odo_volume_icp_eval_dev(fake, fake, fake, eye, fake, A, 1, 0.1, 0.0, acc, None) == -1 and "pose" in L.last_error()
    for args in ((0, 0.1, 0.0), (17, 0.1, 0.0), (1, 0.0, 0.0), (1, nan, 0.0), (1, inf, 0.0), (1, 0.1, -1.0), (1, 0.1, nan)):
        assert lib.odo_volume_icp_eval_dev(fake, fake, fake, eye, fake, eye, *args, acc, None) == -1, args
        assert "odo_volume_icp_eval_dev:" in L.last_error()
    for args in ((C.c_void_p(2), fake, fake, None), (fake, C.c_void_p(8), fake, None), (fake, fake, C.c_void_p(1), None),
                 (fake, fake, fake, C.c_void_p(8))):
        assert lib.odo_volume_icp_eval_dev(fake, args[0], args[1], eye, args[2], eye, 1, 0.1, 0.0, acc, args[3]) == -1
        assert "misaligned" in L.last_error(), args
    assert lib.odo_volume_icp_align_dev(fake, C.byref(good), C.c_void_p(2), fake, eye, fake, eye, out, C.byref(res), None, 0, None) == -1
    assert "misaligned" in L.last_error()
    trace = (L.IcpTraceRow * 1)()
    assert lib.odo_volume_icp_align_dev(fake, C.byref(good), fake, fake, eye, fake, eye, out, C.byref(res), trace, 0, None) == -1
    assert lib.odo_volume_icp_align_dev(None, C.byref(good), fake, fake, eye, fake, eye, out, C.byref(res), None, 0, None) == -1
    assert lib.odo_volume_icp_align_dev(fake, None, fake, fake, eye, fake, eye, out, C.byref(res), None, 0, None) == -1
    assert lib.odo_volume_icp_align_dev(fake, C.byref(good), fake, fake, eye, fake, eye, out, None, None, 0, None) == -1
    assert lib.odo_volume_track_dev(None, C.byref(good), fake, eye, out, C.byref(res)) == -1
    assert lib.odo_volume_track_dev(fake, C.byref(good), None, eye, out, C.byref(res)) == -1
    assert lib.odo_volume_icp_eval_dev(fake, fake, fake, eye, fake, eye, 1, 0.1, 0.0, None, None) == -1


# ---- the model against the prose -------------------------------------------------------------------------------------------------
def test_vectorised_rows_equal_the_loop_bit_for_bit():
    total = {k: 0 for k in TALLIES}
    cases = [(fr, s, 0.3, h) for seed in range(3) for fr in [random_frames(seed)] for s, h in ((1, 0.0), (2, 0.02), (4, 0.005))]
    cases += [(fr, s, 2 * float(f32(fr[0]["mu"])), 0.01) for fr in tiny_views() for s in (1, 3)]
    for (p, raw, depth, nrmw, P_m, P_init), stride, dist_max, huber in cases:
        M, Cm = icp_frame(P_m, P_init)
        got, mask = icp_rows_model(raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
        want, acc, met = icp_rows_loop(raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
        rows_equal(got, want, (stride, dist_max))
        assert mask.sum() == met["pairs"] and (got[~mask] == 0).all()
        s, mag = icp_acc(got, mask)
        assert (np.abs(s - acc) <= max(1, met["pairs"]) * 2.0 ** -52 * mag)[np.isfinite(mag)].all()
        for k, v in met.items():
            total[k] += v
    print(len(cases), "evaluations:", total)
    for k in ("raw0", "far", "model_hole", "normal_zero", "gated", "huber_below", "huber_above", "pairs", "off_left", "off_right"):
        assert total[k] > 0, (k, total)


def test_the_kernels_order_of_the_sums_is_one_of_the_orders():
    """icp_acc_kernel_order, which tests/test_gpu_volume_icp.py holds the GPU to bit for bit: inside the bound of any order round the
    pairwise sums and the count exact, on one block, on several, with two partials per lane and with more than 64 blocks; a single
    row comes out as its own terms."""
    for size, stride, blocks in (((1, 1), 1, 1), ((17, 23), 1, 4), ((65, 33), 1, 15), ((65, 33), 4, 2), (SMALL, 1, 80)):
        K = (1.3 * max(*size, 8), (size[1] - 1) / 2, (size[0] - 1) / 2)
        p, raw, depth, nrmw, P_m, P_init = random_frames(0, size, K)
        rows8, mask = icp_rows_model(raw, depth, nrmw, *icp_frame(P_m, P_init), p, stride, 0.3, 0.01)
        assert len(list(icp_tiles(stride, mask))) == blocks
        s, mag = icp_acc(rows8, mask)
        order = icp_acc_kernel_order(rows8, mask, stride)
        n = int(mask.sum())
        assert n > 0 and order[28] == n and (np.abs(order - s) <= n * 2.0 ** -52 * mag).all(), (size, stride)
        if n == 1:
            assert np.array_equal(order, icp_terms(rows8, mask)[0])


@pytest.mark.parametrize("row", branch_rows(), ids=lambda r: r[0])
def test_every_branch_is_reached_by_the_row_made_for_it(row):
    name, p, raw, depth, nrmw, M, Cm, stride, dist_max, huber, predicate = row
    got, mask = icp_rows_model(raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
    want, acc, met = icp_rows_loop(raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
    rows_equal(got, want, name)
    assert predicate(met), (name, met)
    assert mask.sum() == met["pairs"]
    if name == "dd exactly on the gate":
        assert mask[0, 0] and got[0, 0].tolist() == [0.0, 0.0, -1.0, 0.0, 0.0, 0.0, -0.5, 1.0]
    if name.startswith("Huber"):
        assert got[0, 0, 7] == 1.0 and got[0, 2, 7] == 1.0 and got[0, 5, 7] == 0.5, got[0, :, 6:]
    if name == "no pair at all":
        assert not acc.any() and icp_step_py(acc, np.eye(4), 6, 1e-5, 1e-5)[0] == 1


# ---- the shared header on the host -------------------------------------------------------------------------------------------------
HARNESS = os.path.join(ROOT, "tests", "volume_icp_math_harness.cpp")
HEAD = np.dtype([("rows", "<i4"), ("cols", "<i4"), ("stride", "<i4"), ("f", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("depth_scale", "<f4"),
                 ("max_depth", "<f4"), ("dist_max", "<f4"), ("huber_delta", "<f4"), ("M", "<f4", 16), ("C", "<f4", 16)])
STEP_REC = np.dtype([("acc", "<f8", NACC), ("C", "<f4", 16), ("min_pairs", "<i4"), ("eps_t", "<f4"), ("eps_r", "<f4"), ("pad", "<i4")])
STEP_OUT = np.dtype([("failed", "<i4"), ("converged", "<i4"), ("delta", "<f4", 6), ("C", "<f4", 16)])


def build_host_library(directory):
    """volume_icp_math.h + host_fp.h as a shared library for ctypes (the flags of the other host builds)."""
    so = os.path.join(str(directory), "volume_icp_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-DICP_HARNESS_LIBRARY", "-shared", "-fPIC",
                           HARNESS, "-o", so])
    return C.CDLL(so)


def build_sanitized_program(directory):
    exe = os.path.join(str(directory), "volume_icp_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", HARNESS, "-o", exe])
    return exe


def head_of(p, M, Cm, stride, dist_max, huber):
    h = np.zeros(1, HEAD)
    h["rows"], h["cols"], h["stride"] = p["size"][0], p["size"][1], stride
    h["f"], h["cx"], h["cy"] = p["K"]
    h["depth_scale"], h["max_depth"], h["dist_max"], h["huber_delta"] = p["depth_scale"], p["max_depth"], dist_max, huber
    with np.errstate(all="ignore"):
        h["M"], h["C"] = np.asarray(M, f32).T.reshape(16), np.asarray(Cm, f32).T.reshape(16)
    return h


def host_step(lib):
    """The host library's icp_step with icp_step_py's signature."""
    def step(acc, Cm, min_pairs, eps_t, eps_r):
        rec, out = np.zeros(1, STEP_REC), np.zeros(1, STEP_OUT)
        rec["acc"], rec["C"], rec["min_pairs"], rec["eps_t"], rec["eps_r"] = acc, np.asarray(Cm, f32).T.reshape(16), min_pairs, eps_t, eps_r
        lib.icp_host_step(rec.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return int(out["failed"][0]), int(out["converged"][0]), out["delta"][0].copy(), out["C"][0].reshape(4, 4).T.copy()
    return step


def host_rows(lib, raw, depth, nrmw, M, Cm, p, stride, dist_max, huber):
    h = head_of(p, M, Cm, stride, dist_max, huber)
    raw, depth, nrmw = np.ascontiguousarray(raw, np.uint16), np.ascontiguousarray(depth, f32), np.ascontiguousarray(nrmw, f32)
    out = np.zeros(p["size"] + (8,), f32)
    acc = np.zeros(NACC)
    lib.icp_host_rows(h.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(C.c_void_p), depth.ctypes.data_as(C.c_void_p),
                      nrmw.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), acc.ctypes.data_as(C.c_void_p))
    return out, acc


def step_cases():
    """(acc, C, min_pairs, eps_t, eps_r): sums of random rows at small and large residuals, a Jacobian column that is identically zero
    (a zero pivot), fewer pairs than min_pairs, NaN and inf sums, thresholds on both sides of the step."""
    rng = np.random.default_rng(9)
    cases = []
    for i in range(60):
        n = int(rng.integers(8, 200))
        rows8 = np.zeros((1, n, 8), f32)
        rows8[0, :, :3] = rng.normal(size=(n, 3))
        rows8[0, :, 3:6] = rng.normal(size=(n, 3)) * rng.choice([0.5, 3.0])
        rows8[0, :, 6] = rng.normal(size=n) * rng.choice([1e-4, 1e-2, 0.3])
        rows8[0, :, 7] = rng.choice([1.0, 0.5], n)
        if i % 10 == 3:
            rows8[0, :, int(rng.integers(0, 6))] = 0                # a zero pivot: that component of the step stays 0
        acc = icp_acc(rows8, np.ones((1, n), bool))[0]
        Cm = _pose(rng.uniform(-0.3, 0.3, 3), rng.uniform(-1, 1, 3)).astype(f32)
        if i % 10 == 7:
            Cm = _pose((3.0, 0.2, -0.1), (0.1, 0.2, 0.3)).astype(f32)   # a rotation past 90 degrees: the quaternion's other branches
        mp = n + 1 if i % 10 == 5 else 6
        if i % 10 == 6:
            acc[int(rng.integers(0, NACC))] = rng.choice([np.nan, np.inf, -np.inf])
        eps_t, eps_r = float(rng.choice([0.0, 1e-5, 1e-1, 10.0])), float(rng.choice([0.0, 1e-5, 10.0]))
        if i % 10 in (1, 2):
            eps_t = eps_r = 10.0                                     # converged whatever the step
        cases.append((acc, Cm, mp, eps_t, eps_r))
    return cases


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_library(tmp_path_factory.mktemp("icp_host"))


def test_host_library_rows_and_step_equal_the_loop_and_the_restatement(host):
    for fr, stride, dist_max, huber in [(random_frames(0), 1, 0.3, 0.02), (random_frames(1), 2, 0.3, 0.0)] + \
            [(fr, 1, 0.15, 0.01) for fr in tiny_views()[:4]]:
        p, raw, depth, nrmw, P_m, P_init = fr
        M, Cm = icp_frame(P_m, P_init)
        got, acc = host_rows(host, raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
        want, acc_loop, _ = icp_rows_loop(raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
        rows_equal(got, want)
        assert np.array_equal(acc.view(np.uint64), acc_loop.view(np.uint64)) or not np.isfinite(acc_loop).all()
    for row in branch_rows():
        name, p, raw, depth, nrmw, M, Cm, stride, dist_max, huber, _ = row
        got, acc = host_rows(host, raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
        want, acc_loop, _ = icp_rows_loop(raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
        rows_equal(got, want, name)
        assert np.array_equal(acc.view(np.uint64), acc_loop.view(np.uint64)), name
    step = host_step(host)
    seen = dict(failed=0, converged=0, zero=0, moved=0)
    for acc, Cm, mp, et, er in step_cases():
        a, b = step(acc, Cm, mp, et, er), icp_step_py(acc, Cm, mp, et, er)
        assert a[:2] == b[:2] and np.array_equal(bits(a[2]), bits(b[2])) and np.array_equal(bits(a[3]), bits(b[3])), (a, b)
        seen["failed"] += a[0]
        seen["converged"] += a[1]
        seen["zero"] += int(not a[0] and (a[2] == 0).any())
        seen["moved"] += int(not a[0])
    print(seen)
    assert seen["failed"] >= 10 and seen["converged"] >= 5 and seen["zero"] >= 5 and seen["moved"] >= 40


def test_host_part_equals_the_model(host):
    """hostfp::icp_frame and hostfp::mul4 on the poses of tests/test_volume_raycast_cpu.py (the 3e38 poses among them) and random ones."""
    rng = np.random.default_rng(5)
    poses = [pose for _, _, _, _, ps in tiny_volumes() for pose in ps]
    pairs = [(a, b) for a in poses for b in poses[:4]]
    pairs += [(_pose(rng.uniform(-3, 3, 3), rng.uniform(-50, 50, 3)), _pose(rng.uniform(-3, 3, 3), rng.uniform(-50, 50, 3))) for _ in range(100)]
    nonfinite = 0
    for P_m, P_init in pairs:
        out = np.zeros(48, f32)
        with np.errstate(all="ignore"):
            a, b = np.asarray(P_m, f32).T.reshape(16).copy(), np.asarray(P_init, f32).T.reshape(16).copy()
        host.icp_host_frame(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        M, C0 = icp_frame(P_m, P_init)
        back = mul4(P_m, C0)
        for got, want in zip(out.reshape(3, 4, 4), (M, C0, back)):
            g, w = bits(got.T), bits(want)
            assert ((g == w) | (np.isnan(got.T) & np.isnan(want))).all()
        nonfinite += int(not np.isfinite(out).all())
    assert nonfinite > 0


def test_shared_header_under_sanitizers(tmp_path, host):
    """The stand-alone program (AddressSanitizer, UBSan) gives the library's bytes on rows, steps, eigenvalues and frames."""
    exe = build_sanitized_program(tmp_path)

    def run(mode, blob):
        src, dst = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
        open(src, "wb").write(blob)
        out = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
        return open(dst, "rb").read()

    frames = [(random_frames(2), 1, 0.3, 0.02)] + [(fr, 2, 0.15, 0.0) for fr in tiny_views()]
    for row in branch_rows():
        frames.append(((row[1], row[2], row[3], row[4], None, None), row[7], row[8], row[9], row[5], row[6]))
    for item in frames:
        (p, raw, depth, nrmw, P_m, P_init), stride, dist_max, huber = item[:4]
        M, Cm = item[4:] if len(item) == 6 else icp_frame(P_m, P_init)
        blob = head_of(p, M, Cm, stride, dist_max, huber).tobytes() + np.ascontiguousarray(raw, np.uint16).tobytes() + \
            np.ascontiguousarray(depth, f32).tobytes() + np.ascontiguousarray(nrmw, f32).tobytes()
        got = run("rows", blob)
        want_rows, want_acc = host_rows(host, raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
        assert got == want_rows.tobytes() + want_acc.tobytes()
    cases = step_cases()
    rec = np.zeros(len(cases), STEP_REC)
    for i, (acc, Cm, mp, et, er) in enumerate(cases):
        rec["acc"][i], rec["C"][i], rec["min_pairs"][i], rec["eps_t"][i], rec["eps_r"][i] = acc, Cm.T.reshape(16), mp, et, er
    got = np.frombuffer(run("step", rec.tobytes()), STEP_OUT)
    step = host_step(host)
    for i, (acc, Cm, mp, et, er) in enumerate(cases):
        a = step(acc, Cm, mp, et, er)
        assert (int(got["failed"][i]), int(got["converged"][i])) == a[:2]
        assert np.array_equal(bits(got["delta"][i]), bits(a[2])) and np.array_equal(bits(got["C"][i].reshape(4, 4).T), bits(a[3]))
    finite = np.array([c[0] for c in cases if np.isfinite(c[0]).all()])
    ev = np.frombuffer(run("eig", finite.tobytes()), "<f8").reshape(-1, 6)
    for a, e in zip(finite, ev):
        want = np.zeros(6)
        host.icp_host_eigenvalues(np.ascontiguousarray(a).ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p))
        assert np.array_equal(e, want)


def eigen_close(acc, ev):
    """Jacobi against LAPACK: numpy.linalg.eigvalsh is itself only accurate to a few ulp of the LARGEST eigenvalue (backward stable:
    an absolute error of about 6 * 2^-53 * ||A||), so that is the scale of the comparison; 1e-12 leaves three decimal digits."""
    want = np.linalg.eigvalsh(acc_matrix(acc))
    scale = np.abs(want).max()
    return np.abs(np.asarray(ev) - want).max() <= 1e-12 * scale, np.abs(np.asarray(ev) - want).max() / scale if scale else 0.0


def host_eigenvalues(lib, acc):
    ev = np.zeros(6)
    lib.icp_host_eigenvalues(np.ascontiguousarray(acc, np.float64).ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p))
    return ev


def test_jacobi_eigenvalues_on_random_sums(host):
    worst = 0.0
    for acc, *_ in step_cases():
        if np.isfinite(acc).all():
            ok, err = eigen_close(acc, host_eigenvalues(host, acc))
            worst = max(worst, err)
            assert ok, err
    diag = np.zeros(NACC)
    diag[[0, 6, 11, 15, 18, 20]] = [5.0, 1.0, 3.0, 0.0, 2.0, 4.0]
    assert host_eigenvalues(host, diag).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    print("largest |Jacobi - eigvalsh| / eig_max:", worst)


# ---- the model against the ground truth -----------------------------------------------------------------------------------------
def small_K():
    from odometry_amd import synth
    return (synth.TUM_F / 4, synth.TUM_CX / 4, synth.TUM_CY / 4)


def ribbed_sequence(n=7):
    """The narrow ribbed corridor at 120 x 160 along the RGB-D drive's trajectory: sensor frames of Scene.render, true poses."""
    from odometry_amd import synth
    scene = synth.Scene(0, **RIBBED_SCENE)
    poses = synth.trajectory(n, 0, fwd_range=(0.1, 0.2), max_offset=1.0)
    f, cx, cy = small_K()
    depth = [synth.sensor_depth(scene.render(T, SMALL[0], SMALL[1], f, cx, cy)[1], 1000.0, 30.0) for T in poses]
    return dict(depth=depth, poses=poses, p=params((f, cx, cy), 1000.0, SMALL, **RIBBED_GRID))


def corridor_sequence(n=7):
    """The pinned `natural` case at 120 x 160, the intrinsics divided by four, in the pinned grid."""
    from odometry_amd import synth
    f, cx, cy = small_K()
    seq = synth.make_rgbd_sequence(n, seed=0, rows=SMALL[0], cols=SMALL[1], f=f, cx=cx, cy=cy)
    return dict(depth=seq["depth"], poses=seq["poses"], p=params(seq, size=SMALL))


def frame_to_model(seq, ic_of, frames=range(1, 7), step=icp_step_py):
    """Frames 0 .. k - 1 fused at their true poses, the ray-cast taken from pose k - 1, frame k aligned from that pose: per k the
    model's result and the model frame."""
    p = seq["p"]
    q, w = empty_grid(p)
    out = {}
    rp = default_view(p)
    for k in range(0, max(frames)):
        q, w, _, _ = integrate_model(q, w, seq["depth"][k], seq["poses"][k], p)
        if k + 1 in frames:
            depth, _, nrmw, _ = raycast_model(q, w, None, seq["poses"][k], p, rp)
            r = icp_align_model(seq["depth"][k + 1], depth, nrmw, seq["poses"][k], seq["poses"][k], p, ic_of(p), step=step)
            r["model"] = (depth, nrmw)
            out[k + 1] = r
    return out


@pytest.fixture(scope="module")
def ribbed(host):
    seq = ribbed_sequence()
    return seq, frame_to_model(seq, lambda p: icp(p=p, min_eig_ratio=0.0), step=host_step(host))


@pytest.fixture(scope="module")
def corridor(host):
    seq = corridor_sequence()
    return seq, frame_to_model(seq, lambda p: icp(p=p, min_eig_ratio=0.0), step=host_step(host))


def test_ground_truth_on_the_ribbed_corridor(ribbed, host):
    """Six frames, each against the volume of the frames before it. Measured with this model (translation mm, rotation degrees,
    pairs, eig_min / eig_max, steps): see MEASURED_* and DESIGN.md section 9.8."""
    seq, results = ribbed
    errs = []
    for k, r in results.items():
        assert r["status"] == 0, (k, r["status"])
        et, er = pose_error(r["abs_pose"], seq["poses"][k])
        e0 = pose_error(seq["poses"][k - 1], seq["poses"][k])
        print(f"frame {k}: {et * 1e3:.2f} mm {er:.3f} deg (from {e0[0] * 1e3:.0f} mm {e0[1]:.2f} deg), pairs {r['pairs']:.0f}, "
              f"ratio {r['eig_min'] / r['eig_max']:.2e}, steps {r['iterations']}")
        ok, err = eigen_close(r["trace"][-1][1], host_eigenvalues(host, r["trace"][-1][1]))
        assert ok, err
        errs.append((et, er))
    worst_t, worst_r = max(e[0] for e in errs), max(e[1] for e in errs)
    print(f"largest: {worst_t * 1e3:.3f} mm {worst_r:.4f} deg")
    assert worst_t <= 2 * MEASURED_T_M and worst_r <= 2 * MEASURED_R_DEG
    assert all(r["eig_min"] >= REFUSAL_RATIO * r["eig_max"] for r in results.values())   # none would be refused under it


def test_the_pinned_corridor_is_refused(corridor, host):
    """The project's own corridor cannot be tracked geometrically: nothing but the noise of the volume's normals constrains the
    translation along its axis, and an alignment that is not refused slides (printed below). Every frame is refused under
    REFUSAL_RATIO — which is not the default, see test_default_min_eig_ratio_follows_the_rule_of_the_two_measurements."""
    seq, results = corridor
    for k, r in results.items():
        ratio = r["eig_min"] / r["eig_max"]
        et, er = pose_error(r["abs_pose"], seq["poses"][k])
        print(f"frame {k}: ratio {ratio:.2e}, pairs {r['pairs']:.0f}, steps {r['iterations']}; unrefused it ends {et * 1e3:.1f} mm {er:.3f} deg "
              f"from the truth")
        assert r["status"] == 0                                # (run with min_eig_ratio = 0: nothing else is wrong with it)
        ok, err = eigen_close(r["trace"][-1][1], host_eigenvalues(host, r["trace"][-1][1]))
        assert ok, err
        depth, nrmw = r["model"]                                # the same alignment with the ratio set
        d = icp_align_model(seq["depth"][k], depth, nrmw, seq["poses"][k - 1], seq["poses"][k - 1], seq["p"],
                            icp(p=seq["p"], min_eig_ratio=REFUSAL_RATIO), step=host_step(host))
        assert d["status"] == 2 and np.isnan(d["abs_pose"]).all(), (k, d["status"], ratio)


def test_default_min_eig_ratio_follows_the_rule_of_the_two_measurements(ribbed, corridor):
    """The default is the geometric mean of the largest ratio of the pinned corridor and the smallest of the ribbed one if that mean
    lies a factor ten from both, else 0 (nothing is refused unless the caller sets a ratio). Measured with this model: 6.5e-4 and
    4.95e-3, mean 1.8e-3, a factor 2.8 from either: the default is 0. (The corridor's ratio is not the 1e-6 of exact normals: the
    normals of the volume's interpolant scatter by a degree or so, and that scatter alone 'observes' the axis.)"""
    from odometry_amd import api
    lo = max(r["eig_min"] / r["eig_max"] for r in corridor[1].values())
    hi = min(r["eig_min"] / r["eig_max"] for r in ribbed[1].values())
    mean = float(np.sqrt(lo * hi))
    print(f"largest ratio of the corridor {lo:.3e}, smallest of the ribbed corridor {hi:.3e}, geometric mean {mean:.3e}, "
          f"a factor {hi / mean:.2f} from both")
    assert lo < REFUSAL_RATIO < hi and 0.9 * mean <= REFUSAL_RATIO <= 1.1 * mean
    if hi / mean >= 10:
        assert 0.9 * mean <= api.TsdfVolume.ICP_MIN_EIG_RATIO <= 1.1 * mean
    else:
        assert api.TsdfVolume.ICP_MIN_EIG_RATIO == 0.0


# ---- code object ------------------------------------------------------------------------------------------------------------------
def test_icp_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
    from odometry_amd import _lib
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools here")
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "lib.so")
        shutil.copy(_lib.LIB_PATH, so)
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], cwd=td, check=True, capture_output=True)
        notes = ""
        for f in sorted(os.listdir(td)):
            if "gfx950" in f:
                notes += subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(td, f)], check=True,
                                        capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        for k in ICP_KERNELS:
            if k in name:
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
                print(k, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
    assert sorted(found) == sorted(ICP_KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found
