"""The TSDF volume (odo_volume_*, api.TsdfVolume) without a GPU: the ABI, the numpy model of the specification (include/odometry_hip.h,
DESIGN.md section 9.4) pinned to the prose by a plain-loop implementation that does one fp32 operation at a time, the model against
the ground truth of the synthetic corridor, the kernels' code-object metadata and the PLY writer.

The model is the yardstick of tests/test_gpu_volume.py, which asks the GPU for the same bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

NEW_SYMBOLS = ["odo_volume_create", "odo_volume_integrate_dev", "odo_volume_sync", "odo_volume_extract", "odo_volume_download",
               "odo_volume_stats", "odo_volume_clear", "odo_volume_destroy", "odo_tracker_attach_volume"]
VOLUME_KERNELS = ["volume_integrate_kernel", "volume_sum_kernel", "volume_count_kernel", "volume_scan_kernel", "volume_scatter_kernel"]

# The pinned case: the first frames of the RGB-D drive of tests/test_rgbd_cpu.py in a grid round the corridor's first eight metres.
PINNED = dict(dims=(240, 128, 200), vs=0.04, origin=(-4.8, -3.3, 0.4), mu=0.12, max_depth=8.0, max_weight=65535)


def params(seq_or_K, depth_scale=None, size=(480, 640), **kw):
    """Model parameters: PINNED overridden by kw, K / depth_scale from a sequence (or given)."""
    p = dict(PINNED)
    p.update(kw)
    if isinstance(seq_or_K, dict) and "K" in seq_or_K:
        k = seq_or_K["K"]
        p.update(K=(k["f0"], k["cx0"], k["cy0"]), depth_scale=seq_or_K["depth_scale"])
    else:
        p.update(K=tuple(seq_or_K), depth_scale=depth_scale)
    p["size"] = size
    return p


# ---- the model -----------------------------------------------------------------------------------------------------------------
def world_to_camera(pose):
    """M = [R^T | -R^T t] of a 4x4 camera-to-world pose: fp64 from the fp32 entries, the translation as -((r0 t0 + r1 t1) + r2 t2),
    each entry rounded to fp32 once."""
    A = np.asarray(pose, f32).astype(np.float64)
    M = np.zeros((4, 4), np.float64)
    for r in range(3):
        for c in range(3):
            M[r, c] = A[c, r]
        M[r, 3] = -((A[0, r] * A[0, 3] + A[1, r] * A[1, 3]) + A[2, r] * A[2, 3])
    M[3, 3] = 1.0
    return M.astype(f32)


def centres(p):
    nx, ny, nz = p["dims"]
    vs = f32(p["vs"])
    o = np.asarray(p["origin"], f32)
    return [o[c] + (np.arange(n, dtype=f32) + f32(0.5)) * vs for c, n in enumerate((nx, ny, nz))]


def empty_grid(p):
    nx, ny, nz = p["dims"]
    return np.zeros((nz, ny, nx), np.int16), np.zeros((nz, ny, nx), np.uint16)


def integrate_model(q, w, raw, pose, p):
    """One frame into (q, w) (arrays of shape (nz, ny, nx)); returns q', w', voxels updated, of those in the band."""
    rows, cols = p["size"]
    f0, cx0, cy0 = (f32(v) for v in p["K"])
    mu, maxd, scale = f32(p["mu"]), f32(p["max_depth"]), f32(p["depth_scale"])
    cx_, cy_, cz_ = centres(p)
    X, Y, Z = cx_[None, None, :], cy_[None, :, None], cz_[:, None, None]
    M = world_to_camera(pose)
    with np.errstate(all="ignore"):
        xc, yc, zc = [((M[r, 0] * X + M[r, 1] * Y) + M[r, 2] * Z) + M[r, 3] for r in range(3)]
        ok = zc > f32(0.0)
        u = f0 * (xc / zc) + cx0
        v = f0 * (yc / zc) + cy0
        xi = np.floor(u + f32(0.5))
        yi = np.floor(v + f32(0.5))
        ok = ok & (xi >= f32(0.0)) & (xi < f32(cols)) & (yi >= f32(0.0)) & (yi < f32(rows))   # as floats; NaN fails
        xi = np.where(ok, xi, f32(0.0)).astype(np.int64)
        yi = np.where(ok, yi, f32(0.0)).astype(np.int64)
        r = np.asarray(raw, np.uint16)[yi, xi]
        ok &= r != 0
        D = r.astype(f32) / scale
        ok &= ~(D > maxd)
        sdf = D - zc
        ok &= ~(sdf < -mu)
        s = np.minimum(f32(1.0), sdf / mu) * f32(32767.0)
        W = w.astype(f32)
        F = (q.astype(f32) * W + s) / (W + f32(1.0))
        qn = np.rint(np.where(ok, F, f32(0.0))).astype(np.int16)
        band = ok & (np.abs(sdf) <= mu)
    wn = np.minimum(w.astype(np.int64) + 1, p["max_weight"]).astype(np.uint16)
    return np.where(ok, qn, q), np.where(ok, wn, w), int(ok.sum()), int(band.sum())


def _gradient(Q, obs):
    """Per voxel the gradient of the specification (shape + (3,), component c along x, y, z) and whether it exists."""
    g = np.zeros(Q.shape + (3,), f32)
    has = np.ones(Q.shape, bool)
    two = f32(2.0)
    for c, ax in ((0, 2), (1, 1), (2, 0)):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        qp = np.zeros(Q.shape, f32)
        qm = np.zeros(Q.shape, f32)
        op = np.zeros(Q.shape, bool)
        om = np.zeros(Q.shape, bool)
        qp[lo], op[lo] = Q[hi], obs[hi]
        qm[hi], om[hi] = Q[lo], obs[lo]
        g[..., c] = np.where(op & om, qp - qm, np.where(op, two * (qp - Q), np.where(om, two * (Q - qm), f32(0.0))))
        has &= op | om
    return g, has


def extract_model(q, w, p):
    """The oriented points of the volume in (voxel, axis) order: (n, 4) x y z 0 and (n, 4) nx ny nz weight."""
    nz, ny, nx = q.shape
    vs = f32(p["vs"])
    cen = centres(p)
    Q = q.astype(f32)
    obs = w > 0
    g, has = _gradient(Q, obs)
    keys, pts, nrm = [], [], []
    for c, ax in ((0, 2), (1, 1), (2, 0)):
        sa = [slice(None)] * 3
        sb = [slice(None)] * 3
        sa[ax], sb[ax] = slice(0, -1), slice(1, None)
        sa, sb = tuple(sa), tuple(sb)
        m = obs[sa] & obs[sb] & ((q[sa] > 0) != (q[sb] > 0))
        k, j, i = np.nonzero(m)
        qa, qb = Q[sa][m], Q[sb][m]
        alpha = qa / (qa - qb)
        P = np.zeros((len(alpha), 4), f32)
        P[:, 0], P[:, 1], P[:, 2] = cen[0][i], cen[1][j], cen[2][k]
        P[:, c] = P[:, c] + alpha * vs
        ga, gb = g[sa][m], g[sb][m]
        both = has[sa][m] & has[sb][m]
        n = ga + alpha[:, None] * (gb - ga)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        good = both & (ln > 0)
        N = np.zeros((len(alpha), 4), f32)
        with np.errstate(all="ignore"):
            N[:, :3] = np.where(good[:, None], n / ln[:, None], f32(0.0))
        N[:, 3] = np.minimum(w[sa][m], w[sb][m]).astype(f32)
        keys.append(((k.astype(np.int64) * ny + j) * nx + i) * 3 + c)
        pts.append(P)
        nrm.append(N)
    order = np.argsort(np.concatenate(keys), kind="stable")
    return np.concatenate(pts)[order], np.concatenate(nrm)[order]


# ---- the same, one fp32 operation at a time --------------------------------------------------------------------------------------
def integrate_loop(q, w, raw, pose, p):
    """integrate_model as plain loops over scalars; also returns how often each skip class / special case was met."""
    rows, cols = p["size"]
    nx, ny, nz = p["dims"]
    f0, cx0, cy0 = (f32(v) for v in p["K"])
    mu, maxd, scale, vs = f32(p["mu"]), f32(p["max_depth"]), f32(p["depth_scale"]), f32(p["vs"])
    o = [f32(v) for v in p["origin"]]
    M = world_to_camera(pose)
    q, w = q.copy(), w.copy()
    met = dict(behind=0, outside=0, nan=0, hole=0, far=0, beyond=0, clamped=0, saturated=0, ties=0, updated=0, band=0)
    half = f32(0.5)
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    X = o[0] + (f32(i) + half) * vs
                    Y = o[1] + (f32(j) + half) * vs
                    Z = o[2] + (f32(k) + half) * vs
                    xc = f32(f32(f32(M[0, 0] * X) + f32(M[0, 1] * Y)) + f32(M[0, 2] * Z)) + M[0, 3]
                    yc = f32(f32(f32(M[1, 0] * X) + f32(M[1, 1] * Y)) + f32(M[1, 2] * Z)) + M[1, 3]
                    zc = f32(f32(f32(M[2, 0] * X) + f32(M[2, 1] * Y)) + f32(M[2, 2] * Z)) + M[2, 3]
                    if not zc > f32(0.0):
                        met["behind"] += 1
                        continue
                    u = f32(f0 * f32(xc / zc)) + cx0
                    v = f32(f0 * f32(yc / zc)) + cy0
                    xi = np.floor(f32(u + half))
                    yi = np.floor(f32(v + half))
                    if np.isnan(xi) or np.isnan(yi):
                        met["nan"] += 1
                        continue
                    if not (xi >= f32(0.0) and xi < f32(cols) and yi >= f32(0.0) and yi < f32(rows)):
                        met["outside"] += 1
                        continue
                    r = int(raw[int(yi), int(xi)])
                    if r == 0:
                        met["hole"] += 1
                        continue
                    D = f32(r) / scale
                    if D > maxd:
                        met["far"] += 1
                        continue
                    sdf = f32(D - zc)
                    if sdf < -mu:
                        met["beyond"] += 1
                        continue
                    t = f32(sdf / mu)
                    if t > f32(1.0):
                        met["clamped"] += 1
                        t = f32(1.0)
                    s = f32(t * f32(32767.0))
                    W = f32(int(w[k, j, i]))
                    F = f32(f32(f32(f32(int(q[k, j, i])) * W) + s) / f32(W + f32(1.0)))
                    if F - np.floor(F) == half:
                        met["ties"] += 1
                    q[k, j, i] = int(np.rint(F))
                    if int(w[k, j, i]) + 1 > p["max_weight"]:
                        met["saturated"] += 1
                    w[k, j, i] = min(int(w[k, j, i]) + 1, p["max_weight"])
                    met["updated"] += 1
                    met["band"] += int(abs(sdf) <= mu)
    return q, w, met


def extract_loop(q, w, p):
    nz, ny, nx = q.shape
    vs = f32(p["vs"])
    o = [f32(v) for v in p["origin"]]
    dims = (nx, ny, nz)
    half, two = f32(0.5), f32(2.0)

    def Q(v):
        return f32(int(q[v[2], v[1], v[0]]))

    def usable(v):
        return all(0 <= v[c] < dims[c] for c in range(3)) and w[v[2], v[1], v[0]] > 0

    def grad(v):
        out = []
        for c in range(3):
            vp, vm = list(v), list(v)
            vp[c] += 1
            vm[c] -= 1
            if usable(vp) and usable(vm):
                out.append(f32(Q(vp) - Q(vm)))
            elif usable(vp):
                out.append(f32(two * f32(Q(vp) - Q(v))))
            elif usable(vm):
                out.append(f32(two * f32(Q(v) - Q(vm))))
            else:
                return None
        return out

    pts, nrm = [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                a = (i, j, k)
                for c in range(3):
                    b = list(a)
                    b[c] += 1
                    if b[c] >= dims[c] or not (w[k, j, i] > 0 and w[b[2], b[1], b[0]] > 0):
                        continue
                    if (q[k, j, i] > 0) == (q[b[2], b[1], b[0]] > 0):
                        continue
                    alpha = f32(Q(a) / f32(Q(a) - Q(b)))
                    P = [f32(o[d] + f32(f32(f32(a[d]) + half) * vs)) for d in range(3)]
                    P[c] = f32(P[c] + f32(alpha * vs))
                    ga, gb = grad(a), grad(b)
                    n = [f32(0.0)] * 3
                    if ga is not None and gb is not None:
                        m = [f32(ga[d] + f32(alpha * f32(gb[d] - ga[d]))) for d in range(3)]
                        ln = np.sqrt(f32(f32(f32(m[0] * m[0]) + f32(m[1] * m[1])) + f32(m[2] * m[2])))
                        if ln > 0:
                            n = [f32(m[d] / ln) for d in range(3)]
                    pts.append(P + [f32(0.0)])
                    nrm.append(n + [f32(min(int(w[k, j, i]), int(w[b[2], b[1], b[0]])))])
    return np.array(pts, f32).reshape(-1, 4), np.array(nrm, f32).reshape(-1, 4)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- ground truth ---------------------------------------------------------------------------------------------------------------
def plane_errors(xyz0, nrmw, vs):
    """Against the corridor's five planes: each point's distance to the nearest plane in voxels, the dot product of its normal with
    that plane's normal towards the corridor's inside, the normals' lengths, and which normals are zero."""
    from odometry_amd import synth
    sc = synth.drive_scene("natural", 0)
    P = xyz0[:, :3].astype(np.float64)
    best = np.full(len(P), np.inf)
    inward = np.zeros((len(P), 3))
    for n, h, _ in sc.planes:
        d = np.abs(P @ n - h)
        better = d < best
        best[better] = d[better]
        inward[better] = -np.sign(h) * n   # the camera drives along the axis: the inside is the origin's side
    N = nrmw[:, :3].astype(np.float64)
    ln = np.sqrt((N * N).sum(1))
    return best / vs, (N * inward).sum(1), ln, ln == 0


def report(tag, dist, dots, ln, zero):
    print(f"{tag}: {len(dist)} points; distance / voxel median {np.median(dist):.3f} p99 {np.percentile(dist, 99):.3f} max {dist.max():.3f}; "
          f"zero normals {int(zero.sum())}; |len - 1| max {np.abs(ln[~zero] - 1).max():.2e}; dot min {dots[~zero].min():.3f} "
          f"p1 {np.percentile(dots[~zero], 1):.3f}")


@pytest.fixture(scope="module")
def pinned():
    from odometry_amd import synth
    seq = synth.make_rgbd_sequence(10, seed=0)
    p = params(seq)
    q, w = empty_grid(p)
    counts = []
    for k in range(10):
        q, w, upd, band = integrate_model(q, w, seq["depth"][k], seq["poses"][k], p)
        counts.append((upd, band))
    return p, q, w, counts


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    for name in ("integrate", "extract", "grid", "stats", "clear", "save_ply", "close"):
        assert callable(getattr(api.TsdfVolume, name))
    assert callable(api.RgbdTracker.attach_volume) and callable(api.write_ply_normals)


def test_create_validates_before_touching_a_device():
    from odometry_amd import _lib as L
    lib = L.load()

    def make(**kw):
        p = L.VolumeParams()
        p.nx, p.ny, p.nz, p.voxel_size, p.mu, p.max_depth, p.max_weight = 8, 8, 8, 0.1, 0.3, 5.0, 100
        p.rows, p.cols, p.K, p.depth_scale = 48, 64, L.Intrinsics(50.0, 32.0, 24.0), 1000.0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    h = C.c_void_p()
    fake_ctx = C.c_void_p(8)   # never dereferenced: every case below is refused by the validation
    bad = [dict(nx=1), dict(nz=0), dict(nx=1024, ny=1024, nz=1025), dict(voxel_size=0.0), dict(voxel_size=float("nan")),
           dict(voxel_size=float("inf")), dict(mu=0.0), dict(mu=float("nan")), dict(max_depth=-1.0), dict(max_weight=0),
           dict(max_weight=65536), dict(rows=0), dict(depth_scale=0.0), dict(depth_scale=float("inf"))]
    for kw in bad:
        assert lib.odo_volume_create(fake_ctx, C.byref(make(**kw)), C.byref(h)) == -1 and not h.value, kw
        assert "odo_volume_create" in L.last_error(), kw
    assert lib.odo_volume_create(None, C.byref(make()), C.byref(h)) == -1
    assert lib.odo_volume_create(fake_ctx, None, C.byref(h)) == -1
    assert lib.odo_volume_destroy(None) == 0
    assert lib.odo_volume_integrate_dev(None, None, None) == -1


# ---- the model against the prose -------------------------------------------------------------------------------------------------
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _pose(rot=(0, 0, 0), t=(0, 0, 0)):
    A = np.eye(4)
    A[:3, :3] = _rot(*rot)
    A[:3, 3] = t
    return A


def tiny_cases():
    """(parameters, [(raw, pose) ...]) of tiny volumes that between them reach every skip class and special case."""
    rng = np.random.default_rng(3)
    K, size = (40.0, 15.5, 11.5), (24, 32)
    near = np.full(size, 1000, np.uint16)
    near[::5, ::3] = 0                                    # holes
    near[1::6, 1::4] = 65535                              # 65.5 m: beyond max_depth
    wavy = (1000 + 60 * np.sin(np.arange(32) / 3.0)[None, :] + 40 * np.cos(np.arange(24) / 2.0)[:, None]).astype(np.uint16)
    far = np.full(size, 3000, np.uint16)
    cases = []
    # the camera inside the grid (voxels behind it and beside the image), a surface through the grid, then one far behind it (every
    # voxel in front of the first clamps at 1: (even q + 32767) / 2 is a tie), max_weight 2 over four frames
    p = params(K, 1000.0, size, dims=(7, 6, 9), vs=0.2, origin=(-0.7, -0.6, -0.5), mu=0.3, max_depth=8.0, max_weight=2)
    cases.append((p, [(wavy, _pose()), (far, _pose()), (near, _pose((0.02, -0.03, 0.01), (0.01, 0.02, -0.03))), (wavy, _pose())]))
    # rotation about all three axes, a start away from the origin, TUM's 5000 units per metre, dimensions 5 x 4 x 6
    p = params(K, 5000.0, size, dims=(5, 4, 6), vs=0.15, origin=(0.6, -0.2, 1.4), mu=0.25, max_depth=3.0, max_weight=65535)
    fr = []
    for n in range(3):
        raw = (rng.uniform(0.8, 2.6, size) * 5000).astype(np.uint16)
        raw[rng.uniform(size=size) < 0.1] = 0
        raw[rng.uniform(size=size) < 0.05] = 65535
        fr.append((raw, _pose((0.3 + 0.05 * n, -0.4, 0.2), (1.2, 0.1 * n, -0.2))))
    cases.append((p, fr))
    # a pose that is no rotation at all: +inf and -inf meet in the projection (NaN), or the projection overflows every integer
    p = params(K, 1000.0, size, dims=(4, 4, 4), vs=0.5, origin=(0.25, 0.25, 0.5), mu=0.3, max_depth=8.0, max_weight=5)
    A = np.eye(4)
    A[0, 0], A[1, 0] = 3e38, -3e38     # M row 0 = (3e38, -3e38, 0): (+inf) + (-inf)
    B = np.eye(4)
    B[0, 0] = 3e38                     # xc = +inf, u = +inf: outside, as a float
    cases.append((p, [(near, A), (near, B), (near, _pose())]))
    # a surface that stays inside the grid, seen twice through holes: edges on all three axes, central and one-sided gradients and
    # voxels without one
    p = params(K, 1000.0, size, dims=(9, 8, 10), vs=0.12, origin=(-0.5, -0.45, 0.5), mu=0.3, max_depth=8.0, max_weight=65535)
    holed = wavy.copy()
    holed[::4, ::5] = 0
    holed[10:14, 12:20] = 0
    cases.append((p, [(holed, _pose()), (holed, _pose((0.03, -0.05, 0.02), (0.02, -0.01, 0.01)))]))
    return cases


def test_vectorised_model_equals_the_loop_model_bit_for_bit():
    total = {}
    n_points = n_zero = 0
    for p, frames in tiny_cases():
        q, w = empty_grid(p)
        ql, wl = empty_grid(p)
        for raw, pose in frames:
            q, w, upd, band = integrate_model(q, w, raw, pose, p)
            ql, wl, met = integrate_loop(ql, wl, raw, pose, p)
            assert np.array_equal(q, ql) and np.array_equal(w, wl)
            assert (upd, band) == (met["updated"], met["band"])
            for k, v in met.items():
                total[k] = total.get(k, 0) + v
        P, N = extract_model(q, w, p)
        Pl, Nl = extract_loop(q, w, p)
        assert P.shape == Pl.shape and np.array_equal(bits(P), bits(Pl)) and np.array_equal(bits(N), bits(Nl))
        n_points += len(P)
        zero = (N[:, :3] == 0).all(1)
        n_zero += int(zero.sum())
    assert all(v > 0 for v in total.values()), total   # every class was reached
    assert n_points > 50 and 0 < n_zero < n_points, (n_points, n_zero)   # with and without a normal


def test_update_rule_on_hand_made_values():
    """One voxel, one pixel: the running average, ties to even, the clamp and the saturation, by hand."""
    K, size = (10.0, 0.0, 0.0), (1, 1)
    p = params(K, 1000.0, size, dims=(2, 2, 2), vs=1.0, origin=(-0.5, -0.5, 0.5), mu=0.5, max_depth=10.0, max_weight=3)
    # voxel (0, 0, 0) has centre (0, 0, 1): pixel (0, 0); voxel (0, 0, 1) centre (0, 0, 2)
    q, w = empty_grid(p)
    q, w, upd, band = integrate_model(q, w, np.array([[1250]], np.uint16), np.eye(4), p)   # sdf = +0.25 / -0.75 (skipped)
    assert (q[0, 0, 0], w[0, 0, 0], w[1, 0, 0], upd, band) == (16384, 1, 0, 1, 1)          # rint(0.5 * 32767 = 16383.5) = 16384
    q, w, upd, band = integrate_model(q, w, np.array([[5000]], np.uint16), np.eye(4), p)   # both in front: clamp at 1
    assert (q[0, 0, 0], w[0, 0, 0], q[1, 0, 0], w[1, 0, 0], upd, band) == (24576, 2, 32767, 1, 2, 0)   # (16384 + 32767) / 2 = 24575.5
    for _ in range(3):
        q, w, _, _ = integrate_model(q, w, np.array([[5000]], np.uint16), np.eye(4), p)
    assert w[0, 0, 0] == 3 and w[1, 0, 0] == 3 and q[1, 0, 0] == 32767
    assert (q[:, :, 1] == 0).all() and (w[:, 1, :] == 0).all()                             # beside the 1 x 1 image: never touched
    M = world_to_camera(_pose((0.1, 0.2, 0.3), (1, 2, 3)))
    assert np.allclose(M @ _pose((0.1, 0.2, 0.3), (1, 2, 3)), np.eye(4), atol=1e-6)


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------
def words(q, w):
    """The grid as the device holds it: one 32-bit word per voxel in raster order, q in the low half."""
    return ((w.astype(np.uint32) << 16) | q.view(np.uint16).astype(np.uint32)).reshape(-1)


def _run_harness(exe, tmp_path, mode, head, p, *arrays):
    nx, ny, nz = p["dims"]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([nx, ny, nz], "<i4").tobytes() + np.array([p["vs"], *p["origin"]], "<f4").tobytes() + head)
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
    return dst, {ln.split()[0]: int(ln.split()[1]) for ln in out.stdout.splitlines()[:-1]}


def test_shared_header_equals_the_loop_models_under_sanitizers(tmp_path):
    """odometry_amd/csrc/volume_math.h — the lines the device compiles — as a stand-alone g++ program with AddressSanitizer and UBSan:
    every frame of tiny_cases() integrated into the whole grid against integrate_loop, the points of those grids against
    extract_loop, and the vertices of the mesh's random grids against its loop model, all bit for bit. The header's early-out
    (zc > zc_far) is not a step of the model: it may only take voxels that the model skips for another reason, and one more case
    puts voxels behind it."""
    from test_volume_mesh_cpu import mesh_loop, small_grids
    exe = str(tmp_path / "volume_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "volume_math_harness.cpp"), "-o", exe])
    cases = tiny_cases()
    K, size = (40.0, 15.5, 11.5), (24, 32)
    flat = np.full(size, 1500, np.uint16)
    flat[::5, ::3] = 0
    cases.append((params(K, 1000.0, size, dims=(4, 4, 12), vs=0.3, origin=(-0.6, -0.6, 0.5), mu=0.3, max_depth=2.0, max_weight=2),
                  [(flat, _pose())] * 3))
    total, grids = {}, []
    for p, frames in cases:
        q, w = empty_grid(p)
        for raw, pose in frames:
            M = world_to_camera(pose)
            head = np.array([*p["size"], p["max_weight"]], "<i4").tobytes() + np.array(
                [*p["K"], p["depth_scale"], p["max_depth"], p["mu"], *M[:3, :].T.reshape(12),
                 f32(f32(p["max_depth"]) + f32(p["mu"])) * f32(1.001)], "<f4").tobytes()
            dst, got = _run_harness(exe, tmp_path, "integrate", head, p, words(q, w), np.asarray(raw, np.uint16))
            q, w, met = integrate_loop(q, w, raw, pose, p)
            assert np.array_equal(np.fromfile(dst, "<u4"), words(q, w))
            assert (got["updated"], got["band"], got["behind"], got["saturated"]) == (met["updated"], met["band"], met["behind"], met["saturated"])
            assert got["past"] + got["outside"] + got["hole"] + got["far"] + got["beyond"] == \
                met["outside"] + met["nan"] + met["hole"] + met["far"] + met["beyond"]
            assert got["outside"] <= met["outside"] + met["nan"] and got["hole"] <= met["hole"] and got["far"] <= met["far"] and \
                got["beyond"] <= met["beyond"]
            for k, v in got.items():
                total[k] = total.get(k, 0) + v
        grids.append((p, q, w))
    print(total)
    assert all(v > 0 for v in total.values()), total   # every rejection, the early-out, the weight's clamp
    met = {}
    n_points = 0
    for mode, loop, todo in (("extract", extract_loop, grids), ("mesh", lambda q, w, p: mesh_loop(q, w, p)[:2],
                                                               [g for n, g in small_grids().items() if n.startswith("random")])):
        for p, q, w in todo:
            dst, got = _run_harness(exe, tmp_path, mode, b"", p, words(q, w))
            P, N = loop(q, w, p)
            rec = np.fromfile(dst, "<f4").reshape(-1, 8)
            assert len(rec) == len(P) and np.array_equal(bits(rec[:, :4]), bits(P)) and np.array_equal(bits(rec[:, 4:]), bits(N)), mode
            n_points += len(P)
            for k, v in got.items():
                met[mode + " " + k] = met.get(mode + " " + k, 0) + v
    print(met, n_points)
    assert len(met) == 8 and all(v > 0 for v in met.values()), met   # two-sided, either one-sided, none: in both modes
    assert n_points > 500


# ---- the model against the ground truth -----------------------------------------------------------------------------------------
def test_pinned_case_against_the_corridors_planes(pinned):
    """True poses, ten frames. Measured with this model: 570-650 k voxels updated per frame, 41 011 points, distance to the nearest
    plane median 0.018, 99th percentile 0.098, maximum 0.170 voxels; 62 points without a normal."""
    p, q, w, counts = pinned
    print("updated / in band per frame:", counts)
    assert all(500_000 < u < 700_000 and 0 < b <= u for u, b in counts), counts
    P, N = extract_model(q, w, p)
    dist, dots, ln, zero = plane_errors(P, N, p["vs"])
    report("true poses, model", dist, dots, ln, zero)
    assert 40_000 < len(P) < 42_000
    assert dist.max() <= 0.5, dist.max()                       # EVERY point within half a voxel of a plane
    assert np.abs(ln[~zero] - 1.0).max() <= 1e-6
    assert (dots[~zero] > 0).all(), dots[~zero].min()          # every normal points into the corridor
    assert zero.mean() <= 0.01, zero.mean()
    assert (N[:, 3] >= 1).all() and (N[:, 3] <= 10).all() and (P[:, 3] == 0).all()


# ---- code object, PLY -----------------------------------------------------------------------------------------------------------
def test_volume_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        for k in VOLUME_KERNELS:
            if k in name:
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
                print(k, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
    assert sorted(found) == sorted(VOLUME_KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found


def test_ply_writer_with_normals_round_trips(tmp_path):
    from odometry_amd import api
    rng = np.random.default_rng(1)
    xyz0 = rng.normal(size=(37, 4)).astype(f32)
    nrmw = rng.normal(size=(37, 4)).astype(f32)
    path = tmp_path / "surface.ply"
    api.write_ply_normals(str(path), xyz0, nrmw)
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and "element vertex 37" in lines
    assert [ln.split()[-1] for ln in lines if ln.startswith("property float")] == ["x", "y", "z", "nx", "ny", "nz"]
    rec = np.frombuffer(body, "<f4").reshape(37, 6)
    assert np.array_equal(rec[:, :3], xyz0[:, :3]) and np.array_equal(rec[:, 3:], nrmw[:, :3])
    api.write_ply_normals(str(path), np.zeros((0, 4), f32), np.zeros((0, 4), f32))
    assert b"element vertex 0" in open(path, "rb").read()
