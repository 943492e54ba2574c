"""The ray-cast of the TSDF volume (odo_volume_raycast_dev, odo_volume_raycast, api.TsdfVolume.raycast) without a GPU: the ABI and the
argument checks, the numpy model of the specification (include/odometry_hip.h) pinned to the prose by a
plain-loop implementation that does one fp32 operation at a time, every branch of the specification reached by a row made for it, a
closed form, the host + device header odometry_amd/csrc/volume_raycast_math.h compiled by g++ with sanitizers, the model against the
ground truth of the synthetic corridor, and the kernel's code-object metadata.

The model is the yardstick of tests/test_gpu_volume_raycast.py, which asks the GPU for the same bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from test_volume_cpu import _pose, bits, empty_grid, integrate_model, params, pinned, plane_errors, report, tiny_cases  # noqa: F401
from test_volume_colour_cpu import empty_colour, integrate_colour_model, random_colour, random_frame
from test_volume_mesh_cpu import grid_params, random_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

NEW_SYMBOLS = ["odo_volume_raycast_dev", "odo_volume_raycast"]
RAYCAST_KERNELS = ["volume_raycast_kernel"]
TALLIES = ("outside", "nonfinite", "unobserved", "end0", "end_after_invalid", "hit", "hit_f0", "ran_out", "missed", "dir_zero",
           "normal_invalid", "normal_zero", "normal", "raw_saturated", "coloured", "colour_hole")


def view(size, K, t_min, step, n_steps):
    """The model's odo_raycast_params."""
    return dict(size=tuple(size), K=tuple(K), t_min=t_min, step=step, n_steps=n_steps)


def default_view(p, n_steps=None, size=None, K=None):
    """The volume's own size and K, step = mu / 2."""
    step = float(f32(p["mu"])) / 2
    return view(size or p["size"], K or p["K"], 0.0, step,
                n_steps or int(np.ceil((float(f32(p["max_depth"])) + float(f32(p["mu"]))) / step)) + 1)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def raycast_frame(pose, p):
    """e_c = (t_c - origin_c) / vs - 0.5 and G = R / vs: fp64 from the fp32 entries, each result rounded to fp32 once."""
    A = np.asarray(pose, f32).astype(np.float64)
    vs = np.float64(f32(p["vs"]))
    o = np.asarray(p["origin"], f32).astype(np.float64)
    with np.errstate(all="ignore"):
        return ((A[:3, 3] - o) / vs - 0.5).astype(f32), (A[:3, :3] / vs).astype(f32)


def _lerp(a, b, fr):
    return a + fr * (b - a)


def _cells(q, w, e, g, t):
    """The sample arithmetic for N rays at depths t (N,), directions g (3, N): valid, corners (8, N) as fp32, fractions, points, the
    cell's voxel and the smallest weight."""
    nz, ny, nx = q.shape
    with np.errstate(all="ignore"):
        pt = [e[c] + t * g[c] for c in range(3)]
        b = [np.floor(x) for x in pt]
        ok = np.ones(len(t), bool)
        for c, dim in enumerate((nx, ny, nz)):
            ok &= (b[c] >= f32(0.0)) & (b[c] <= f32(dim - 2))         # as floats; NaN and inf fail
        bi = [np.where(ok, x, f32(0.0)).astype(np.int64) for x in b]
        fr = [pt[c] - b[c] for c in range(3)]
    base = (bi[2] * ny + bi[1]) * nx + bi[0]
    qf, wf = q.reshape(-1), w.reshape(-1)
    cs, wmin = [], None
    for d in range(8):
        idx = base + ((d >> 2) * ny + ((d >> 1) & 1)) * nx + (d & 1)
        cs.append(qf.take(idx).astype(f32))
        wd = wf.take(idx)
        wmin = wd if wmin is None else np.minimum(wmin, wd)
    ok &= wmin > 0
    return ok, cs, fr, pt, bi, wmin


def _interp(cs, fr):
    l = [_lerp(cs[2 * i], cs[2 * i + 1], fr[0]) for i in range(4)]   # l_00, l_10, l_01, l_11 (y, then z)
    m = [_lerp(l[0], l[1], fr[1]), _lerp(l[2], l[3], fr[1])]
    return _lerp(m[0], m[1], fr[2]), l, m


def raycast_model(q, w, col, pose, p, rp):
    """depth (rows, cols) fp32, raw uint16, nrmw (rows, cols, 4) fp32, rgba (rows, cols, 4) uint8 (zeros without a colour grid)."""
    rows, cols = rp["size"]
    f, cx, cy = (f32(v) for v in rp["K"])
    t_min, step, scale = f32(rp["t_min"]), f32(rp["step"]), f32(p["depth_scale"])
    e, G = raycast_frame(pose, p)
    N = rows * cols
    with np.errstate(all="ignore"):
        dx = np.tile((np.arange(cols, dtype=f32) - cx) / f, rows)
        dy = np.repeat((np.arange(rows, dtype=f32) - cy) / f, cols)
        g = np.stack([(G[r, 0] * dx + G[r, 1] * dy) + G[r, 2] for r in range(3)])
    active = np.ones(N, bool)
    have = np.zeros(N, bool)
    t_prev, F_prev, z = np.zeros(N, f32), np.zeros(N, f32), np.zeros(N, f32)
    hit = np.zeros(N, bool)
    for n in range(rp["n_steps"]):
        ia = np.nonzero(active)[0]
        if not len(ia):
            break
        with np.errstate(all="ignore"):
            t = t_min + f32(n) * step
            ok, cs, fr, _, _, _ = _cells(q, w, e, g[:, ia], np.full(len(ia), t, f32))
            F, _, _ = _interp(cs, fr)
            end = ok & (F <= f32(0.0))
            h = end & have[ia]
            zz = t_prev[ia] + (F_prev[ia] / (F_prev[ia] - F)) * (t - t_prev[ia])
        z[ia[h]] = zz[h]
        hit[ia[h]] = True
        active[ia[end]] = False
        have[ia] = ok
        t_prev[ia] = t
        F_prev[ia] = np.where(ok, F, f32(0.0))
    depth = np.where(hit, z, f32(0.0))
    with np.errstate(all="ignore"):
        raw = np.where(hit, np.minimum(f32(65535.0), np.rint(depth * scale)), f32(0.0)).astype(np.uint16)
    nrmw = np.zeros((N, 4), f32)
    rgba = np.zeros((N, 4), np.uint8)
    ih = np.nonzero(hit)[0]
    if len(ih):
        with np.errstate(all="ignore"):
            ok, cs, fr, pt, _, wmin = _cells(q, w, e, g[:, ih], depth[ih])
            _, l, m = _interp(cs, fr)
            d = [cs[2 * i + 1] - cs[2 * i] for i in range(4)]
            gx = _lerp(_lerp(d[0], d[1], fr[1]), _lerp(d[2], d[3], fr[1]), fr[2])
            gy = _lerp(l[1] - l[0], l[3] - l[2], fr[2])
            gz = m[1] - m[0]
            ln = np.sqrt((gx * gx + gy * gy) + gz * gz)
            good = ok & (ln > 0)
            nrm = np.stack([gx / ln, gy / ln, gz / ln, wmin.astype(f32)], 1)
            nrmw[ih] = np.where(good[:, None], nrm, f32(0.0))
            if col is not None:
                near = [np.where(ok, np.floor(x + f32(0.5)), f32(0.0)).astype(np.int64) for x in pt]
                cw = col[near[2], near[1], near[0]]
                has = ok & (cw[:, 3] > 0)
                rgba[ih] = np.where(has[:, None], np.concatenate([cw[:, :3], np.full((len(ih), 1), 255, np.uint8)], 1), 0)
    return depth.reshape(rows, cols), raw.reshape(rows, cols), nrmw.reshape(rows, cols, 4), rgba.reshape(rows, cols, 4)


# ---- the same, one fp32 operation at a time --------------------------------------------------------------------------------------
def _cell_loop(q, w, e, g, t, met=None):
    """None for an invalid sample, else (corners, fractions, point, cell, smallest weight)."""
    nz, ny, nx = q.shape
    with np.errstate(all="ignore"):
        pt = [f32(e[c] + f32(t * g[c])) for c in range(3)]
        b = [np.floor(x) for x in pt]
    for c, dim in enumerate((nx, ny, nz)):
        if not (b[c] >= f32(0.0) and b[c] <= f32(dim - 2)):
            if met is not None:
                met["outside"] += 1
                met["nonfinite"] += int(not all(np.isfinite(x) for x in pt))
            return None
    bi = [int(x) for x in b]
    cs, wmin = [], 1 << 20
    for d in range(8):
        k, j, i = bi[2] + (d >> 2), bi[1] + ((d >> 1) & 1), bi[0] + (d & 1)
        cs.append(f32(int(q[k, j, i])))
        wmin = min(wmin, int(w[k, j, i]))
    if wmin == 0:
        if met is not None:
            met["unobserved"] += 1
        return None
    return cs, [f32(pt[c] - b[c]) for c in range(3)], pt, bi, wmin


def _lerp1(a, b, fr):
    return f32(a + f32(fr * f32(b - a)))


def _interp_loop(cs, fr):
    l = [_lerp1(cs[2 * i], cs[2 * i + 1], fr[0]) for i in range(4)]
    m = [_lerp1(l[0], l[1], fr[1]), _lerp1(l[2], l[3], fr[1])]
    return _lerp1(m[0], m[1], fr[2]), l, m


def ray_loop(q, w, col, e, g, t_min, step, n_steps, scale, met):
    """One ray: (z, raw, (nx, ny, nz, w), (R, G, B, A)); met counts the branches taken."""
    zero4 = [f32(0.0)] * 4
    met["dir_zero"] += int(any(x == 0 for x in g))
    have, t_prev, F_prev = False, f32(0.0), f32(0.0)
    z, in_grid_before = None, met["outside"]
    seen = 0
    for n in range(n_steps):
        with np.errstate(all="ignore"):
            t = f32(t_min + f32(f32(n) * step))
        cell = _cell_loop(q, w, e, g, t, met)
        if cell is None:
            have = False
            continue
        seen += 1
        F, _, _ = _interp_loop(cell[0], cell[1])
        if F <= f32(0.0):
            if not have:
                met["end0" if n == 0 else "end_after_invalid"] += 1
                return f32(0.0), 0, zero4, [0] * 4
            with np.errstate(all="ignore"):
                z = f32(t_prev + f32(f32(F_prev / f32(F_prev - F)) * f32(t - t_prev)))
            met["hit"] += 1
            met["hit_f0"] += int(F == 0 and z == t)
            break
        have, t_prev, F_prev = True, t, F
    if z is None:
        met["missed" if met["outside"] - in_grid_before == n_steps else "ran_out"] += 1
        return f32(0.0), 0, zero4, [0] * 4
    with np.errstate(all="ignore"):
        raw = int(min(f32(65535.0), np.rint(f32(z * scale))))
    met["raw_saturated"] += int(raw == 65535)
    cell = _cell_loop(q, w, e, g, z)
    if cell is None:
        met["normal_invalid"] += 1
        return z, raw, zero4, [0] * 4
    cs, fr, pt, _, wmin = cell
    _, l, m = _interp_loop(cs, fr)
    d = [f32(cs[2 * i + 1] - cs[2 * i]) for i in range(4)]
    gx = _lerp1(_lerp1(d[0], d[1], fr[1]), _lerp1(d[2], d[3], fr[1]), fr[2])
    gy = _lerp1(f32(l[1] - l[0]), f32(l[3] - l[2]), fr[2])
    gz = f32(m[1] - m[0])
    ln = np.sqrt(f32(f32(f32(gx * gx) + f32(gy * gy)) + f32(gz * gz)))
    if ln > 0:
        nrm = [f32(gx / ln), f32(gy / ln), f32(gz / ln), f32(wmin)]
        met["normal"] += 1
    else:
        nrm = zero4
        met["normal_zero"] += 1
    rgba = [0] * 4
    if col is not None:
        i, j, k = (int(np.floor(f32(x + f32(0.5)))) for x in pt)
        cw = col[k, j, i]
        if cw[3] > 0:
            rgba = [int(cw[0]), int(cw[1]), int(cw[2]), 255]
            met["coloured"] += 1
        else:
            met["colour_hole"] += 1
    return z, raw, nrm, rgba


def raycast_loop(q, w, col, pose, p, rp):
    """raycast_model as plain loops over scalars; also returns how often each branch was taken."""
    rows, cols = rp["size"]
    f, cx, cy = (f32(v) for v in rp["K"])
    e, G = raycast_frame(pose, p)
    met = {k: 0 for k in TALLIES}
    nx, ny, nz = p["dims"]
    met["camera_inside"] = int(all(0 <= e[c] < dim - 1 for c, dim in enumerate((nx, ny, nz))))
    depth, raw = np.zeros((rows, cols), f32), np.zeros((rows, cols), np.uint16)
    nrmw, rgba = np.zeros((rows, cols, 4), f32), np.zeros((rows, cols, 4), np.uint8)
    for y in range(rows):
        for x in range(cols):
            with np.errstate(all="ignore"):
                dx, dy = f32(f32(f32(x) - cx) / f), f32(f32(f32(y) - cy) / f)
                g = [f32(f32(f32(G[r, 0] * dx) + f32(G[r, 1] * dy)) + G[r, 2]) for r in range(3)]
            depth[y, x], raw[y, x], nrmw[y, x], rgba[y, x] = ray_loop(q, w, col, e, g, f32(rp["t_min"]), f32(rp["step"]), rp["n_steps"],
                                                                      f32(p["depth_scale"]), met)
    return depth, raw, nrmw, rgba, met


def frames_equal(got, want, tag=""):
    for name, a, b in zip(("depth", "raw", "nrmw", "rgba"), got, want):
        if a.dtype == f32:
            a, b = bits(a), bits(b)
        assert a.shape == b.shape and np.array_equal(a, b), (tag, name, int((a != b).sum()))


# ---- grids -----------------------------------------------------------------------------------------------------------------------
def tiny_volumes():
    """tiny_cases() integrated (with colour: weight cap 2): [(p, q, w, col, poses)], the 3e38 poses among them."""
    out = []
    for n, (p, frames) in enumerate(tiny_cases()):
        q, w = empty_grid(p)
        col = empty_colour(p)
        for k, (raw, pose) in enumerate(frames):
            q, w, col, _, _, _ = integrate_colour_model(q, w, col, raw, random_frame(p, 3, 10 * n + k), pose, p, 3, False, 2)
        out.append((p, q, w, col, [pose for _, pose in frames]))
    return out


def plane_grid(dims, vs, origin, mu, h, depth_scale=1000.0):
    """A grid filled by formula from the plane z = h seen from smaller z: q = rint(32767 * clip((h - Z) / mu, -1, 1)), every w = 1."""
    p = params((40.0, 16.0, 12.0), depth_scale, (24, 32), dims=dims, vs=vs, origin=origin, mu=mu, max_depth=8.0, max_weight=65535)
    nx, ny, nz = dims
    Z = float(f32(origin[2])) + (np.arange(nz) + 0.5) * float(f32(vs))
    qz = np.rint(32767.0 * np.clip((h - Z) / float(f32(mu)), -1.0, 1.0)).astype(np.int16)
    q = np.broadcast_to(qz[:, None, None], (nz, ny, nx)).copy()
    return p, q, np.ones((nz, ny, nx), np.uint16)


def random_volume(dims, seed, holes=0.1, zeros=0.1):
    """A random grid with holes and q == 0 entries, a random colour grid with holes of its own, in a small world."""
    p = grid_params(dims, vs=0.05, origin=(-0.2, -0.2, 0.3))
    p.update(mu=0.15, max_depth=4.0, max_weight=65535, depth_scale=5000.0, K=(30.0, 7.5, 5.5), size=(12, 16))
    q, w = random_grid(dims, seed, holes=holes, zeros=zeros)
    return p, q, w, random_colour(q.shape, 70 + seed, holes=0.3)


# vs = 0.25 and an origin that puts the voxel centres at multiples of 0.25: with the camera at the world's origin and samples 0.125
# apart every quantity of the principal ray is exact
EXACT = dict(dims=(5, 5, 9), vs=0.25, origin=(-0.625, -0.625, -0.125), mu=0.5, h=1.0)


def branch_rows():
    """(name, p, q, w, col, pose, view, predicate on the loop model's tallies): each row is there for the branch its predicate names."""
    rows = []
    p, q, w = plane_grid(**EXACT)
    K, size = (40.0, 2.0, 1.0), (3, 5)      # the principal point is pixel (2, 1)
    rows.append(("ends at sample 0", p, q, w, None, _pose(), view(size, K, 1.25, 0.125, 4), lambda m: m["end0"] > 0 and m["hit"] == 0))
    holed = w.copy()
    holed[3] = 0                             # the cells below the surface's are unobserved: positive, invalid, non-positive
    rows.append(("no hit behind an invalid sample", p, q, holed, None, _pose(), view(size, K, 0.0, 0.125, 16),
                 lambda m: m["end_after_invalid"] > 0 and m["unobserved"] > 0 and m["hit"] == 0))
    rows.append(("a hit with F == 0 exactly", p, q, w, None, _pose(), view(size, K, 0.0, 0.125, 16),
                 lambda m: m["hit_f0"] > 0 and m["dir_zero"] > 0))
    rows.append(("runs out of samples", p, q, w, None, _pose(), view(size, K, 0.0, 0.125, 5),
                 lambda m: m["ran_out"] == 15 and m["hit"] == 0))
    rows.append(("misses the grid", p, q, w, None, _pose((0.0, np.pi, 0.0), (0.0, 0.0, -1.0)), view(size, K, 0.0, 0.125, 16),
                 lambda m: m["missed"] == 15 and m["camera_inside"] == 0))
    rows.append(("a direction component exactly 0, the camera inside", p, q, w, None, _pose(), view(size, K, 0.0, 0.125, 16),
                 lambda m: m["dir_zero"] > 0 and m["camera_inside"] == 1 and m["hit"] > 0))
    rows.append(("the camera outside", p, q, w, None, _pose(t=(0.05, -0.02, -0.7)), view(size, K, 0.0, 0.11, 24),
                 lambda m: m["camera_inside"] == 0 and m["hit"] > 0 and m["outside"] > 0))
    gap = w.copy()
    gap[5] = 0                               # samples 0.75 apart: p_z = 3 and 6 are valid, the crossing at p_z = 4 is in a cell that is not
    rows.append(("a hit whose normal cell is invalid", p, q, gap, None, _pose(), view(size, K, 0.0, 0.75, 4),
                 lambda m: m["normal_invalid"] > 0 and m["hit"] == m["normal_invalid"] + m["normal"] + m["normal_zero"]))
    rows.append(("n_steps == 1", p, q, w, None, _pose(), view(size, K, 1.25, 0.125, 1), lambda m: m["end0"] == 15))
    rows.append(("n_steps == 1 in front of the surface", p, q, w, None, _pose(), view(size, K, 0.5, 0.125, 1), lambda m: m["ran_out"] == 15))
    ps, qs, ws = plane_grid(depth_scale=100000.0, **EXACT)
    rows.append(("raw saturates", ps, qs, ws, None, _pose(), view(size, K, 0.0, 0.125, 16), lambda m: m["raw_saturated"] == m["hit"] > 0))
    pr, qr, wr, cr = random_volume((9, 8, 7), 1)
    rows.append(("a coloured volume with wc == 0 holes", pr, qr, wr, cr, _pose((0.1, -0.2, 0.05), (0.02, -0.03, 0.1)),
                 view(pr["size"], pr["K"], 0.0, 0.02, 40), lambda m: m["coloured"] > 0 and m["colour_hole"] > 0))
    flat = np.zeros_like(q)                  # an interpolant without a gradient cannot be crossed from a positive sample; a zero field
    rows.append(("a field that is zero ends every ray where it enters", p, flat, w, None, _pose(), view(size, K, 0.0, 0.125, 16),
                 lambda m: m["end0"] == 15))
    return rows


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    assert C.sizeof(_lib.RaycastParams) == 32 and "odo_raycast_params" in hdr
    assert callable(api.TsdfVolume.raycast) and callable(api.TsdfVolume.raycast_params)


def test_bad_arguments_are_refused_before_touching_a_device():
    from odometry_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(8)   # never dereferenced: every case below is refused by the argument checks
    nan, inf = float("nan"), float("inf")

    def rp(**kw):
        r = L.RaycastParams(48, 64, 50.0, 32.0, 24.0, 0.0, 0.05, 100)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    pose = (C.c_float * 16)(*np.eye(4, dtype=f32).ravel())
    out = (C.c_float * 4)()
    bad = [dict(rows=0), dict(rows=4097), dict(cols=0), dict(cols=4097), dict(rows=-1), dict(f=0.0), dict(f=-1.0), dict(f=nan), dict(f=inf),
           dict(cx=nan), dict(cx=inf), dict(cy=nan), dict(cy=-inf), dict(t_min=-0.001), dict(t_min=nan), dict(t_min=inf), dict(step=0.0),
           dict(step=-0.1), dict(step=nan), dict(step=inf), dict(n_steps=0), dict(n_steps=4097), dict(n_steps=-5)]
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        for kw in bad:
            assert fn(fake, C.byref(rp(**kw)), pose, out, None, None, None) == -1, (name, kw)
            assert name + ":" in L.last_error(), (name, kw, L.last_error())
        for i in (0, 5, 12, 15):
            for v in (nan, inf, -inf):
                A = (C.c_float * 16)(*np.eye(4, dtype=f32).ravel())
                A[i] = v
                assert fn(fake, C.byref(rp()), A, out, None, None, None) == -1 and "pose" in L.last_error(), (name, i, v)
        assert fn(None, C.byref(rp()), pose, out, None, None, None) == -1
        assert fn(fake, None, pose, out, None, None, None) == -1
        assert fn(fake, C.byref(rp()), None, out, None, None, None) == -1
    for args in ((C.c_void_p(2), None, None, None), (None, C.c_void_p(1), None, None), (None, None, C.c_void_p(8), None),
                 (None, None, None, C.c_void_p(2))):
        assert lib.odo_volume_raycast_dev(fake, C.byref(rp()), pose, *args) == -1 and "misaligned" in L.last_error(), args


# ---- the model against the prose -------------------------------------------------------------------------------------------------
def test_vectorised_model_equals_the_loop_model_bit_for_bit():
    total = {}
    views = 0
    for p, q, w, col, poses in tiny_volumes():
        for pose in poses:
            rp = default_view(p, n_steps=30)
            got = raycast_model(q, w, col, pose, p, rp)
            *want, met = raycast_loop(q, w, col, pose, p, rp)
            frames_equal(got, want, "tiny")
            for k, v in met.items():
                total[k] = total.get(k, 0) + v
            views += 1
    for seed in range(3):
        p, q, w, col = random_volume((9, 8, 7), seed)
        assert (w == 0).any() and (q == 0).any()
        for pose, step in ((_pose((0.05 * seed, -0.1, 0.02), (0.0, 0.01, 0.0)), 0.02), (_pose((0.4, 0.3, -0.2), (-0.3, -0.25, 0.2)), 0.07)):
            rp = view(p["size"], p["K"], 0.0, step, 40)
            got = raycast_model(q, w, col, pose, p, rp)
            *want, met = raycast_loop(q, w, col, pose, p, rp)
            frames_equal(got, want, f"random {seed}")
            for k, v in met.items():
                total[k] = total.get(k, 0) + v
            views += 1
    print(views, "views:", total)
    assert total["nonfinite"] > 0                                          # the 3e38 poses: inf / NaN positions come out invalid
    for k in ("outside", "unobserved", "hit", "ran_out", "missed", "normal", "coloured", "colour_hole", "end_after_invalid"):
        assert total[k] > 0, (k, total)


@pytest.mark.parametrize("row", branch_rows(), ids=lambda r: r[0])
def test_every_branch_is_reached_by_the_row_made_for_it(row):
    name, p, q, w, col, pose, rp, predicate = row
    got = raycast_model(q, w, col, pose, p, rp)
    *want, met = raycast_loop(q, w, col, pose, p, rp)
    frames_equal(got, want, name)
    assert predicate(met), (name, met)
    if name == "a hit with F == 0 exactly":
        assert got[0][1, 2] == f32(1.0) and got[1][1, 2] == 1000


# ---- closed form -----------------------------------------------------------------------------------------------------------------
def test_principal_ray_against_a_plane_in_closed_form():
    """The plane z = h by formula in a grid of 0.1 m voxels with mu = 0.3, an axis-aligned camera at (0.03, -0.02, Z0), samples
    mu / 2 = 0.15 apart: the two samples that bracket the crossing and all their corners (at most step + vs = 0.25 < mu from the
    plane) lie where the field is linear, f = 32767 (h - z) / mu, so the interpolant is exact up to the roundings of the chain:
      stored q: |rint| <= 0.5;
      fr: two roundings of p < 16, 2 * 2^-24 * 16 voxels, times the slope 32767 vs / mu = 10 922 per voxel: 0.021;
      seven lerps of three operations on values below 65 536: 21 * 2^-24 * 65 536 = 0.082;
    together E <= 0.61 units at either sample. The secant through two values that are each within E of a line of slope 32767 / mu
    per metre, 16 383 units apart, crosses zero within 1.001 * E * mu / 32767 of the line's zero; the hit formula adds four roundings
    of quantities no larger than z and the depth z is h - Z0 up to the rounding of Z0 into e: 6 * 2^-24 * (h - Z0).
    The field does not depend on x and y: c_0yz == c_1yz, gx and gy are exactly zero and the normal is exactly (0, 0, -1)."""
    vs, mu = 0.1, 0.3
    for h, Z0 in ((1.234, 0.0), (0.987, -0.31), (1.4, 0.4111)):
        p, q, w = plane_grid((8, 7, 16), vs, (-0.4, -0.35, 0.05), mu, h)
        rp = view((3, 3), (50.0, 1.0, 1.0), 0.0, 0.15, 20)
        depth, raw, nrmw, _ = raycast_model(q, w, None, _pose(t=(0.03, -0.02, Z0)), p, rp)
        z = float(depth[1, 1])
        bound = 1.001 * 0.61 * float(f32(mu)) / 32767.0 + 6 * 2.0 ** -24 * (h - Z0)
        print(f"h {h} Z0 {Z0}: z {z!r} error {abs(z - (h - Z0)):.3e} bound {bound:.3e}")
        assert abs(z - (h - Z0)) <= bound
        assert raw[1, 1] == int(np.rint(f32(z) * f32(1000.0)))
        assert nrmw[1, 1].tolist() == [0.0, 0.0, -1.0, 1.0]
        assert (depth > 0).all() and (np.abs(depth - (h - Z0)) <= 4 * bound).all()   # every ray's t is depth along the axis: the same z


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------
REC = np.dtype([("vox", "<u4", 8), ("e", "<f4", 3), ("g", "<f4", 3), ("t_min", "<f4"), ("step", "<f4"), ("n_steps", "<i4"), ("scale", "<f4")])
OUT = np.dtype([("hit", "<i4"), ("z", "<f4"), ("raw", "<u4"), ("nrmw", "<f4", 4)])


def _harness(tmp_path):
    exe = str(tmp_path / "volume_raycast_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "volume_raycast_math_harness.cpp"), "-o", exe])
    return exe


def test_host_part_equals_the_models(tmp_path):
    """hostfp::raycast_frame (the library's host code) against raycast_frame: e and G bit for bit, the 3e38 poses among the records."""
    exe = _harness(tmp_path)
    rng = np.random.default_rng(5)
    poses, grids = [], []
    for p, _, _, _, ps in tiny_volumes():
        poses += ps
        grids += [p] * len(ps)
    for i in range(200):
        poses.append(_pose(rng.uniform(-3, 3, 3), rng.uniform(-50, 50, 3)))
        grids.append(dict(vs=float(rng.choice([0.04, 0.07, 0.25, 1e-3, 3.0])), origin=rng.uniform(-20, 20, 3)))
    rec = np.zeros(len(poses), np.dtype([("A", "<f4", 16), ("origin", "<f4", 3), ("vs", "<f4")]))
    for i, (A, p) in enumerate(zip(poses, grids)):
        with np.errstate(all="ignore"):
            rec["A"][i] = np.asarray(A, f32).T.reshape(16)
        rec["origin"][i], rec["vs"][i] = p["origin"], p["vs"]
    src, dst = str(tmp_path / "frames.bin"), str(tmp_path / "frames_out.bin")
    rec.tofile(src)
    out = subprocess.run([exe, "frame", src, dst], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
    got = np.fromfile(dst, "<f4").reshape(len(poses), 12)
    for i, (A, p) in enumerate(zip(poses, grids)):
        e, G = raycast_frame(A, p)
        assert np.array_equal(bits(got[i, :3]), bits(e)) and np.array_equal(bits(got[i, 3:]), bits(G.reshape(9))), i
    assert np.isinf(got).any()                                             # 3e38 / vs: the overflow arrives as inf on both sides


def test_shared_header_equals_the_loop_model_under_sanitizers(tmp_path):
    """odometry_amd/csrc/volume_raycast_math.h — the lines the device compiles — as a stand-alone g++ program with AddressSanitizer and
    UBSan, on 20 000 random rays through random 2 x 2 x 2 grids (holes, zeros, directions with zero components, rays that miss)."""
    exe = _harness(tmp_path)
    rng = np.random.default_rng(12)
    n = 20000
    rec = np.zeros(n, REC)
    qv = rng.integers(-32767, 32768, (n, 8))
    smooth = rng.uniform(size=n) < 0.5                                      # half the grids hold a plane: rays that cross it
    nrm = rng.normal(size=(n, 3))
    off = rng.uniform(-0.5, 1.5, n)
    corner = np.array([[d & 1, (d >> 1) & 1, d >> 2] for d in range(8)], float)
    plane = np.clip(((corner[None] * nrm[:, None, :]).sum(2) - off[:, None]) * 20000, -32767, 32767)
    qv = np.where(smooth[:, None], np.rint(plane).astype(np.int64), qv)
    qv[rng.uniform(size=(n, 8)) < 0.05] = 0
    wv = rng.integers(1, 65536, (n, 8))
    holed = np.nonzero(rng.uniform(size=n) < 0.1)[0]                        # one corner never observed: the whole grid is invalid
    wv[holed, rng.integers(0, 8, len(holed))] = 0
    rec["vox"] = (wv.astype(np.uint32) << 16) | (qv.astype(np.int16).view(np.uint16).astype(np.uint32))
    rec["step"] = rng.uniform(0.01, 0.3, n)
    rec["n_steps"] = rng.integers(1, 60, n)
    # from a point in or near the cell towards a point inside it, reaching it after 0.3 .. 1.2 of the ray's length
    e = rng.uniform(-0.3, 1.3, (n, 3))
    g = (rng.uniform(0.0, 1.0, (n, 3)) - e) / (rec["step"] * rec["n_steps"] * rng.uniform(0.3, 1.2, n))[:, None]
    g[rng.uniform(size=(n, 3)) < 0.1] = 0.0
    rec["e"], rec["g"] = e, g
    rec["t_min"] = np.where(rng.uniform(size=n) < 0.5, 0.0, rng.uniform(0, 0.5, n))
    rec["step"] = rng.uniform(0.01, 0.3, n)
    rec["n_steps"] = rng.integers(1, 60, n)
    rec["scale"] = rng.choice([1000.0, 5000.0, 1e6], n)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rec.tofile(src)
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
    got = np.fromfile(dst, OUT)
    assert len(got) == n
    met = {k: 0 for k in TALLIES}
    for i in range(n):
        q = (rec["vox"][i] & 0xffff).astype(np.uint16).view(np.int16).reshape(2, 2, 2)
        w = (rec["vox"][i] >> 16).astype(np.uint16).reshape(2, 2, 2)
        before = met["hit"]
        z, raw, nrmw, _ = ray_loop(q, w, None, rec["e"][i], list(rec["g"][i]), rec["t_min"][i], rec["step"][i], int(rec["n_steps"][i]),
                                   rec["scale"][i], met)
        want = np.zeros(1, OUT)
        want["hit"], want["z"], want["raw"], want["nrmw"] = met["hit"] - before, z, raw, nrmw
        assert got[i].tobytes() == want[0].tobytes(), (i, got[i], want[0])
    print(met)
    # (a grid of one cell is convex and observed or not as a whole: no ray re-enters it, no crossing lies in an invalid cell. Those
    # two branches are the branch rows' and the random grids'.)
    assert met["hit"] > 1000 and met["normal"] > 500 and met["end0"] > 100 and met["missed"] > 100 and met["ran_out"] > 100
    assert met["raw_saturated"] > 0 and met["unobserved"] > 100 and met["dir_zero"] > 100


# ---- the model against the ground truth -----------------------------------------------------------------------------------------
PINNED_STEPS = 140


@pytest.fixture(scope="module")
def pinned_views(pinned):   # noqa: F811
    """The pinned case (10 frames, true poses) seen at 480 x 640 with the volume's K from poses 0, 5 and 9: t_min = 0, step = mu / 2,
    140 samples."""
    from odometry_amd import synth
    seq = synth.make_rgbd_sequence(10, seed=0)
    p, q, w, _ = pinned
    rp = default_view(p, n_steps=PINNED_STEPS)
    return seq, p, rp, {k: raycast_model(q, w, None, seq["poses"][k], p, rp) for k in (0, 5, 9)}


def world_points(depth, pose, rp):
    """The hits' pixels and their world points (fp64)."""
    f, cx, cy = rp["K"]
    y, x = np.nonzero(depth > 0)
    z = depth[y, x].astype(np.float64)
    A = np.asarray(pose, f32).astype(np.float64)
    cam = np.stack([(x - cx) / f * z, (y - cy) / f * z, z], 1)
    return y, x, cam @ A[:3, :3].T + A[:3, 3]


def test_pinned_case_against_the_corridors_planes(pinned_views):
    """Measured with this model (hits of 307 200; distance to the nearest plane in voxels: median, 99th percentile, maximum; hits
    without a normal; first percentile and minimum of the normals' dot product; against the sensor frame: median, maximum):
      pose 0: 133 060; 0.013 0.076 0.286; 2 670; 0.990 0.429; 0.036 0.641
      pose 5: 118 687; 0.012 0.058 0.313;     2; 0.994 0.420; 0.031 0.662
      pose 9:  89 815; 0.013 0.058 0.287;     3; 0.996 0.445; 0.034 0.598
    The half voxel is the extraction's own bound (tests/test_volume_cpu.py)."""
    seq, p, rp, frames = pinned_views
    for k, (depth, raw, nrmw, _) in frames.items():
        y, x, P = world_points(depth, seq["poses"][k], rp)
        N = nrmw[y, x]
        dist, dots, ln, zero = plane_errors(np.concatenate([P, np.zeros((len(P), 1))], 1), N, p["vs"])
        report(f"pose {k}", dist, dots, ln, zero)
        print(f"pose {k}: pixels without a hit {int((depth == 0).sum())}")
        assert len(P) > 80_000
        assert dist.max() <= 0.5, dist.max()                               # EVERY hit within half a voxel of a plane
        assert np.abs(ln[~zero] - 1.0).max() <= 1e-6
        assert (dots[~zero] > 0).all(), dots[~zero].min()
        assert np.percentile(dots[~zero], 1) >= 0.9
        assert ((N[:, 3] > 0) == ~zero).all() and (nrmw[depth == 0] == 0).all()
        sensor = seq["depth"][k].astype(np.float64) / p["depth_scale"]
        both = (depth > 0) & (seq["depth"][k] > 0)
        diff = np.abs(depth[both] - sensor[both]) / p["vs"]
        print(f"pose {k}: against the sensor frame at {int(both.sum())} pixels: median {np.median(diff):.3f} max {diff.max():.3f} voxels")
        assert both.sum() > 80_000 and np.median(diff) < 0.25
        want_raw = np.minimum(65535, np.rint(depth * f32(p["depth_scale"]))).astype(np.uint16)
        assert np.array_equal(raw, want_raw)


# ---- code object ------------------------------------------------------------------------------------------------------------------
def test_raycast_kernel_is_in_the_gfx950_code_object_without_spills_or_scratch():
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
        for k in RAYCAST_KERNELS:
            if k in name:
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
                print(k, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
    assert sorted(found) == sorted(RAYCAST_KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found
