"""Colour in the TSDF volume (odo_volume_enable_colour, odo_volume_integrate_colour_dev, odo_volume_extract_colour / _mesh_colour,
odo_tracker_frame_colour, odo_rgbd_frontend_colour) without a GPU: the numpy model of the specification (include/odometry_hip.h,
DESIGN.md section 9.6) pinned to the prose by plain loops, the update rule by hand and, through the host + device header
odometry_amd/csrc/volume_colour_math.h compiled by g++, for every (c, wc, s); the pinned case's counts, the colours against the
rendered frames, the mesh's colours against the extraction's, the kernels' code-object metadata, the PLY writers and the argument
checks.

The model is the yardstick of tests/test_gpu_volume_colour.py, which asks the GPU for the same bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from test_volume_cpu import bits, centres, empty_grid, extract_model, integrate_model, params, tiny_cases, world_to_camera
from test_volume_mesh_cpu import DIRS, grid_params, mesh_model, random_grid, read_ply_mesh  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

NEW_SYMBOLS = ["odo_volume_enable_colour", "odo_volume_integrate_colour_dev", "odo_volume_download_colour", "odo_volume_upload_colour",
               "odo_volume_extract_colour", "odo_volume_mesh_colour", "odo_tracker_frame_colour", "odo_rgbd_frontend_colour"]
COLOUR_KERNELS = ["volume_integrate_colour_kernel", "volume_extract_colour_kernel", "volume_mesh_colour_kernel"]
LAYOUTS = [(3, False), (3, True), (4, False), (4, True)]   # (channels, bgr): RGB, BGR, RGBA, BGRA


# ---- the model -----------------------------------------------------------------------------------------------------------------
def empty_colour(p):
    nx, ny, nz = p["dims"]
    return np.zeros((nz, ny, nx, 4), np.uint8)


def update_rule(c, wc, s, max_weight):
    """The table's rule on integer arrays: c' and wc'."""
    c, wc, s = (np.asarray(a, np.int64) for a in (c, wc, s))
    return (c * wc + s + ((wc + 1) >> 1)) // (wc + 1), np.minimum(wc + 1, max_weight)


def rgb_of(colour, bgr):
    """(rows, cols, 3) R, G, B of an interleaved frame with 3 or 4 channels."""
    c = np.asarray(colour)[..., :3]
    return c[..., ::-1] if bgr else c


def integrate_colour_model(q, w, col, raw, colour, pose, p, channels=3, bgr=False, max_weight=255):
    """One frame into (q, w, col): the steps of integrate_model written out again (the sample's pixel and the band are needed per
    voxel), then the colour update in the band. Returns q', w', col', voxels updated, in the band, colour updates."""
    rows, cols = p["size"]
    assert np.asarray(colour).shape == (rows, cols, channels)
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
        ok = ok & (xi >= f32(0.0)) & (xi < f32(cols)) & (yi >= f32(0.0)) & (yi < f32(rows))
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
    sample = rgb_of(colour, bgr)[yi[band], xi[band]]                       # (n, 3) R, G, B
    old = col[band]
    c_new, w_new = update_rule(old[:, :3], old[:, 3:4], sample, max_weight)
    assert c_new.min(initial=0) >= 0 and c_new.max(initial=0) <= 255
    out = col.copy()
    out[band] = np.concatenate([c_new, w_new], 1).astype(np.uint8)
    return np.where(ok, qn, q), np.where(ok, wn, w), out, int(ok.sum()), int(band.sum()), int(band.sum())


def edge_colours_model(q, w, col, dirs, detail=False):
    """(n, 4) uint8 R, G, B, A of the points on the edges (voxel, e), e indexing `dirs`, in (voxel in raster order, e) order. detail:
    also the class of every point (2: both voxels coloured, 1: exactly one, 0: neither) and e."""
    nz, ny, nx = q.shape
    Q = q.astype(f32)
    obs = w > 0
    keys, out, cls, es = [], [], [], []
    for e, (dx, dy, dz) in enumerate(dirs):
        sa = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        sb = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        m = obs[sa] & obs[sb] & ((q[sa] > 0) != (q[sb] > 0))
        k, j, i = np.nonzero(m)
        qa, qb = Q[sa][m], Q[sb][m]
        alpha = qa / (qa - qb)
        assert ((alpha >= 0) & (alpha <= 1)).all()                         # in [0, 1] by construction: no clamp
        ca, cb = col[sa][m], col[sb][m]
        has_a, has_b = ca[:, 3] > 0, cb[:, 3] > 0
        fa, fb = ca[:, :3].astype(f32), cb[:, :3].astype(f32)
        both = np.rint(fa + alpha[:, None] * (fb - fa))
        assert both.min(initial=0) >= 0 and both.max(initial=0) <= 255
        rgb = np.where((has_a & has_b)[:, None], both.astype(np.int64),
                       np.where(has_a[:, None], ca[:, :3], np.where(has_b[:, None], cb[:, :3], 0)))
        a = np.where(has_a | has_b, 255, 0)
        out.append(np.concatenate([rgb, a[:, None]], 1).astype(np.uint8))
        keys.append(((k.astype(np.int64) * ny + j) * nx + i) * len(dirs) + e)
        cls.append(has_a.astype(int) + has_b.astype(int))
        es.append(np.full(len(k), e))
    order = np.argsort(np.concatenate(keys), kind="stable")
    rgba = np.concatenate(out)[order]
    return (rgba, np.concatenate(cls)[order], np.concatenate(es)[order]) if detail else rgba


def point_colours_model(q, w, col, detail=False):
    """The colours of extract_model's points, index for index."""
    return edge_colours_model(q, w, col, DIRS[:3], detail)


def mesh_colours_model(q, w, col, detail=False):
    """The colours of mesh_model's vertices, index for index."""
    return edge_colours_model(q, w, col, DIRS, detail)


def random_colour(shape, seed, holes=0.2):
    """(nz, ny, nx, 4) uint8: random colours, weights 1 .. 255 with 1, 254 and 255 frequent, a share `holes` never coloured."""
    rng = np.random.default_rng(seed)
    col = rng.integers(0, 256, shape + (4,)).astype(np.uint8)
    wc = rng.integers(1, 256, shape)
    pick = rng.uniform(size=shape)
    wc = np.where(pick < 0.15, 1, np.where(pick < 0.3, 254, np.where(pick < 0.45, 255, wc)))
    wc[rng.uniform(size=shape) < holes] = 0
    col[..., 3] = wc
    col[wc == 0, :3] = 0
    return col


def random_frame(p, channels, seed):
    return np.random.default_rng(seed).integers(0, 256, tuple(p["size"]) + (channels,)).astype(np.uint8)


# ---- the same, one operation at a time -------------------------------------------------------------------------------------------
def integrate_colour_loop(q, w, col, raw, colour, pose, p, channels, bgr, max_weight):
    rows, cols = p["size"]
    nx, ny, nz = p["dims"]
    f0, cx0, cy0 = (f32(v) for v in p["K"])
    mu, maxd, scale, vs = f32(p["mu"]), f32(p["max_depth"]), f32(p["depth_scale"]), f32(p["vs"])
    o = [f32(v) for v in p["origin"]]
    M = world_to_camera(pose)
    q, w, col = q.copy(), w.copy(), col.copy()
    half = f32(0.5)
    n_col = 0
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
                        continue
                    xi = np.floor(f32(f32(f32(f0 * f32(xc / zc)) + cx0) + half))
                    yi = np.floor(f32(f32(f32(f0 * f32(yc / zc)) + cy0) + half))
                    if not (xi >= f32(0.0) and xi < f32(cols) and yi >= f32(0.0) and yi < f32(rows)):
                        continue
                    r = int(raw[int(yi), int(xi)])
                    if r == 0:
                        continue
                    D = f32(r) / scale
                    if D > maxd:
                        continue
                    sdf = f32(D - zc)
                    if sdf < -mu:
                        continue
                    s = f32(min(f32(1.0), f32(sdf / mu)) * f32(32767.0))
                    W = f32(int(w[k, j, i]))
                    q[k, j, i] = int(np.rint(f32(f32(f32(f32(int(q[k, j, i])) * W) + s) / f32(W + f32(1.0)))))
                    w[k, j, i] = min(int(w[k, j, i]) + 1, p["max_weight"])
                    if abs(sdf) <= mu:
                        px = [int(x) for x in colour[int(yi), int(xi)]]
                        sample = [px[2], px[1], px[0]] if bgr else px[:3]
                        wc = int(col[k, j, i, 3])
                        for ch in range(3):
                            col[k, j, i, ch] = (int(col[k, j, i, ch]) * wc + sample[ch] + ((wc + 1) >> 1)) // (wc + 1)
                        col[k, j, i, 3] = min(wc + 1, max_weight)
                        n_col += 1
    return q, w, col, n_col


def edge_colours_loop(q, w, col, dirs):
    nz, ny, nx = q.shape
    dims = (nx, ny, nz)
    out = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for d in dirs:
                    b = (i + d[0], j + d[1], k + d[2])
                    if any(b[c] >= dims[c] for c in range(3)) or not (w[k, j, i] > 0 and w[b[2], b[1], b[0]] > 0):
                        continue
                    if (q[k, j, i] > 0) == (q[b[2], b[1], b[0]] > 0):
                        continue
                    qa, qb = f32(int(q[k, j, i])), f32(int(q[b[2], b[1], b[0]]))
                    alpha = f32(qa / f32(qa - qb))
                    ca, cb = col[k, j, i], col[b[2], b[1], b[0]]
                    if ca[3] > 0 and cb[3] > 0:
                        rgb = [int(np.rint(f32(f32(int(ca[ch])) + f32(alpha * f32(f32(int(cb[ch])) - f32(int(ca[ch]))))))) for ch in range(3)]
                        out.append(rgb + [255])
                    elif ca[3] > 0:
                        out.append([int(x) for x in ca[:3]] + [255])
                    elif cb[3] > 0:
                        out.append([int(x) for x in cb[:3]] + [255])
                    else:
                        out.append([0, 0, 0, 0])
    return np.array(out, np.uint8).reshape(-1, 4)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    assert C.sizeof(_lib.VolumeColourParams) == 12
    for name in ("enable_colour", "colour_grid", "upload_colour"):
        assert callable(getattr(api.TsdfVolume, name))
    assert callable(api.RgbdTracker.frame_colour) and callable(api.RgbdFrontend.colour)


def test_bad_arguments_are_refused_before_touching_a_device():
    from odometry_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(8)   # never dereferenced: every case below is refused by the argument checks
    good = L.VolumeColourParams(3, 0, 255)
    assert lib.odo_volume_enable_colour(None, C.byref(good)) == -1 and lib.odo_volume_enable_colour(fake, None) == -1
    for cp in [(2, 0, 255), (5, 0, 255), (0, 0, 255), (3, 2, 255), (3, -1, 255), (4, 0, 0), (3, 0, 256), (3, 0, -1)]:
        assert lib.odo_volume_enable_colour(fake, C.byref(L.VolumeColourParams(*cp))) == -1, cp
        assert "odo_volume_enable_colour" in L.last_error(), cp
    pose = (C.c_float * 16)()
    for args in ((None, fake, fake, pose), (fake, None, fake, pose), (fake, fake, None, pose), (fake, fake, fake, None)):
        assert lib.odo_volume_integrate_colour_dev(*args) == -1 and "odo_volume_integrate_colour_dev" in L.last_error()
    b = (C.c_uint8 * 4)()
    for fn in (lib.odo_volume_download_colour, lib.odo_volume_upload_colour):
        assert fn(None, b) == -1 and fn(fake, None) == -1
    n, d = C.c_long(0), C.c_long(0)
    buf = (C.c_float * 4)()
    idx = (C.c_int32 * 3)()
    counts = (C.c_long * 4)()
    for args in ((None, 0, None, None, None, C.byref(n), C.byref(d)), (fake, 0, None, None, None, None, None),
                 (fake, -1, None, None, None, C.byref(n), None), (fake, (1 << 28) + 1, buf, buf, b, C.byref(n), None),
                 (fake, 1, None, buf, b, C.byref(n), None), (fake, 1, buf, None, b, C.byref(n), None), (fake, 1, buf, buf, None, C.byref(n), None)):
        assert lib.odo_volume_extract_colour(*args) == -1 and "odo_volume_extract_colour" in L.last_error(), args[1]
    for args in ((None, 0, 0, None, None, None, None, counts), (fake, 0, 0, None, None, None, None, None),
                 (fake, -1, 0, None, None, None, None, counts), (fake, 0, -1, None, None, None, None, counts),
                 (fake, (1 << 28) + 1, 0, buf, buf, b, None, counts), (fake, 0, (1 << 28) + 1, None, None, None, idx, counts),
                 (fake, 1, 0, None, buf, b, None, counts), (fake, 1, 0, buf, None, b, None, counts), (fake, 1, 0, buf, buf, None, None, counts),
                 (fake, 0, 1, None, None, None, None, counts)):
        assert lib.odo_volume_mesh_colour(*args) == -1 and "odo_volume_mesh_colour" in L.last_error(), args[1:3]
    assert lib.odo_tracker_frame_colour(None, fake) == -1 and lib.odo_tracker_frame_colour(fake, None) == -1
    out = C.c_void_p()
    for args in ((None, fake, C.byref(out)), (fake, None, C.byref(out)), (fake, fake, None)):
        assert lib.odo_rgbd_frontend_colour(*args) == -1 and "odo_rgbd_frontend_colour" in L.last_error()


# ---- the model against the prose -------------------------------------------------------------------------------------------------
def _coloured_tiny_grids():
    """tiny_cases() integrated with random colour frames in the four layouts: [(p, q, w, col)]."""
    out = []
    for n, (p, frames) in enumerate(tiny_cases()):
        channels, bgr = LAYOUTS[n]
        q, w = empty_grid(p)
        col = empty_colour(p)
        for f, (raw, pose) in enumerate(frames):
            q, w, col, _, _, _ = integrate_colour_model(q, w, col, raw, random_frame(p, channels, 10 * n + f), pose, p, channels, bgr, 2)
        out.append((p, q, w, col))
    return out


def test_vectorised_model_equals_the_loop_model_bit_for_bit():
    n_updates = 0
    for n, (p, frames) in enumerate(tiny_cases()):
        channels, bgr = LAYOUTS[n]
        mw = (2, 255, 1, 3)[n]
        q, w = empty_grid(p)
        col = empty_colour(p)
        ql, wl, cl = q, w, col
        for f, (raw, pose) in enumerate(frames):
            frame = random_frame(p, channels, 10 * n + f)
            q, w, col, upd, band, n_col = integrate_colour_model(q, w, col, raw, frame, pose, p, channels, bgr, mw)
            ql, wl, cl, nl = integrate_colour_loop(ql, wl, cl, raw, frame, pose, p, channels, bgr, mw)
            assert np.array_equal(q, ql) and np.array_equal(w, wl) and np.array_equal(col, cl), (n, f)
            assert n_col == nl == band
            n_updates += n_col
        assert col[..., 3].max() <= mw
    assert n_updates > 100
    classes = np.zeros(3, int)
    grids = [(q, w, col) for _, q, w, col in _coloured_tiny_grids()]
    for seed, dims in enumerate([(6, 5, 4), (5, 7, 3), (4, 4, 6)]):
        q, w = random_grid(dims, seed, holes=0.15, zeros=0.1)
        grids.append((q, w, random_colour(q.shape, 40 + seed, holes=0.3)))
    for q, w, col in grids:
        for dirs, name in ((DIRS[:3], "points"), (DIRS, "vertices")):
            got, cls, _ = edge_colours_model(q, w, col, dirs, detail=True)
            assert np.array_equal(got, edge_colours_loop(q, w, col, dirs)), name
            classes += np.bincount(cls, minlength=3)
    print("points / vertices with neither, one, both voxels coloured:", classes.tolist())
    assert (classes > 0).all(), classes                                   # the one-sided class and the uncoloured one both occur
    wcs = np.concatenate([g[2][..., 3].ravel() for g in grids])
    assert all((wcs == v).any() for v in (0, 1, 254, 255))
    assert any((g[0] == 0).any() for g in grids)


def test_point_and_vertex_colours_sit_beside_the_models_points():
    for p, q, w, col in _coloured_tiny_grids():
        assert len(point_colours_model(q, w, col)) == len(extract_model(q, w, p)[0])
        X = mesh_model(q, w, p)[0]
        rgba, _, e = mesh_colours_model(q, w, col, detail=True)
        assert len(rgba) == len(X) and np.array_equal(e.astype(f32), X[:, 3])


def test_geometry_is_unchanged_and_colour_updates_equal_in_band():
    for n, (p, frames) in enumerate(tiny_cases()):
        channels, bgr = LAYOUTS[n]
        q, w = empty_grid(p)
        qc, wc_ = empty_grid(p)
        col = empty_colour(p)
        for f, (raw, pose) in enumerate(frames):
            q, w, upd, band = integrate_model(q, w, raw, pose, p)
            before = col
            qc, wc_, col, upd_c, band_c, n_col = integrate_colour_model(qc, wc_, col, raw, random_frame(p, channels, f), pose, p, channels, bgr)
            assert np.array_equal(q, qc) and np.array_equal(w, wc_) and (upd, band) == (upd_c, band_c)
            assert n_col == band
            # every colour update raises a weight below the cap by one: the words that changed weight are the band
            assert int((col[..., 3].astype(int) - before[..., 3].astype(int)).sum()) == band


# ---- the update rule -------------------------------------------------------------------------------------------------------------
def test_update_rule_on_hand_made_values():
    one = lambda c, wc, s, mw=255: tuple(int(x) for x in update_rule(c, wc, s, mw))   # noqa: E731
    assert one(0, 0, 200) == (200, 1) and one(77, 0, 0) == (0, 1)          # the first sample replaces whatever was there
    assert one(10, 1, 11) == (11, 2)                                        # 10.5: the tie rounds up
    assert one(10, 3, 12) == (11, 4)                                        # 10.5 again: (30 + 12 + 2) // 4
    assert one(10, 2, 11) == (10, 3)                                        # 10.33
    assert one(0, 255, 0) == (0, 255) and one(255, 255, 255) == (255, 255) and one(255, 1, 255) == (255, 2) and one(0, 7, 0) == (0, 8)
    assert one(255, 255, 0) == (254, 255) and one(0, 255, 255) == (1, 255)  # (255 * 255 + 128) // 256, (255 + 128) // 256
    for mw in (1, 3, 255):                                                  # saturation
        c, wc = 0, 0
        for n in range(300):
            c, wc = one(c, wc, 100, mw)
            assert wc == min(n + 1, mw) and c == 100
    assert one(50, 1, 90, 1) == (70, 1)                                     # max_weight 1: the mean of the last two samples ...
    assert one(50, 3, 90, 3) == (60, 3)                                     # ... 3: a quarter of the difference
    # the stall at weight 255: a sample less than 128 levels away leaves c where it is, one 128 away moves it by one
    assert one(100, 255, 227) == (100, 255) and one(100, 255, 228) == (101, 255)
    assert one(100, 255, 0) == (100, 255) and one(200, 255, 71) == (199, 255) and one(200, 255, 72) == (200, 255)


def _harness(tmp_path):
    exe = str(tmp_path / "volume_colour_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "volume_colour_math_harness.cpp"), "-o", exe])
    return exe


def test_shared_header_gives_the_rule_for_every_c_wc_s(tmp_path):
    exe = _harness(tmp_path)
    table = str(tmp_path / "table.bin")
    out = subprocess.run([exe, "update", table], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
    got = np.fromfile(table, np.uint8).reshape(256, 256, 256)              # [c, wc, s]
    c, wc, s = np.meshgrid(np.arange(256), np.arange(256), np.arange(256), indexing="ij")
    want, _ = update_rule(c, wc, s, 255)
    assert want.max() <= 255 and (c * wc + s + ((wc + 1) >> 1)).max() < 1 << 17
    assert np.array_equal(got, want.astype(np.uint8)), int((got != want).sum())
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("weight")]
    assert len(rows) == 3 * 256
    for _, mw, w0, w1 in rows:
        assert int(w1) == min(int(w0) + 1, int(mw))


def test_shared_header_interpolates_as_the_model(tmp_path):
    exe = _harness(tmp_path)
    rng = np.random.default_rng(8)
    n = 20000
    rec = np.zeros(n, np.dtype([("ca", "<u4"), ("cb", "<u4"), ("alpha", "<f4")]))
    rec["ca"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    rec["cb"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    rec["ca"][rng.uniform(size=n) < 0.3] &= 0xffffff                       # never coloured
    rec["cb"][rng.uniform(size=n) < 0.3] &= 0xffffff
    qa = rng.integers(-32767, 32768, n)
    qb = np.where(qa > 0, -rng.integers(0, 32768, n), rng.integers(1, 32768, n))
    rec["alpha"] = qa.astype(f32) / (qa.astype(f32) - qb.astype(f32))
    rec["alpha"][:4] = [0.0, -0.0, 1.0, 0.5]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rec.tofile(src)
    out = subprocess.run([exe, "interp", src, dst], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
    got = np.fromfile(dst, "<u4").view(np.uint8).reshape(n, 4)
    ca, cb = rec["ca"].copy().view(np.uint8).reshape(n, 4), rec["cb"].copy().view(np.uint8).reshape(n, 4)
    has_a, has_b = ca[:, 3] > 0, cb[:, 3] > 0
    fa, fb = ca[:, :3].astype(f32), cb[:, :3].astype(f32)
    both = np.rint(fa + rec["alpha"][:, None] * (fb - fa)).astype(np.int64)
    rgb = np.where((has_a & has_b)[:, None], both, np.where(has_a[:, None], ca[:, :3], np.where(has_b[:, None], cb[:, :3], 0)))
    want = np.concatenate([rgb, np.where(has_a | has_b, 255, 0)[:, None]], 1).astype(np.uint8)
    assert np.array_equal(got, want), int((got != want).any(1).sum())
    assert (has_a & has_b).sum() > 1000 and (has_a != has_b).sum() > 1000 and (~has_a & ~has_b).sum() > 100


# ---- channel order ---------------------------------------------------------------------------------------------------------------
def test_the_four_channel_layouts_give_the_same_colour_grid():
    from odometry_amd import synth
    p, frames = tiny_cases()[3]
    gray = np.random.default_rng(4).uniform(0, 255, p["size"])
    grids = []
    for channels, bgr in LAYOUTS:
        q, w = empty_grid(p)
        col = empty_colour(p)
        for raw, pose in frames:
            q, w, col, _, _, _ = integrate_colour_model(q, w, col, raw, synth.colour_from_gray(gray, channels, bgr, tint_seed=1), pose, p,
                                                        channels, bgr)
        grids.append(col)
    assert all(np.array_equal(grids[0], g) for g in grids[1:])
    seen = grids[0][grids[0][..., 3] > 0]
    assert len(seen) > 50 and (seen[:, 0] != seen[:, 2]).any()             # the tint makes R and B differ: a swap would show
    rgb = synth.colour_from_gray(gray, 3, False, tint_seed=1)
    wrong = empty_colour(p)
    q, w = empty_grid(p)
    for raw, pose in frames:
        q, w, wrong, _, _, _ = integrate_colour_model(q, w, wrong, raw, rgb, pose, p, 3, True)   # RGB data read as BGR
    assert not np.array_equal(wrong, grids[0])


# ---- the pinned case -------------------------------------------------------------------------------------------------------------
PINNED_UPDATES = [70_818, 72_332, 72_905, 70_656, 67_353, 63_428, 57_442, 52_819, 46_027, 40_781]


@pytest.fixture(scope="module")
def pinned_colour():
    """make_rgbd_sequence(10, seed=0), colour_from_gray(gray, 3, False, tint_seed=1), true poses, colour weight 255."""
    from odometry_amd import synth
    seq = synth.make_rgbd_sequence(10, seed=0)
    p = params(seq)
    frames = [synth.colour_from_gray(g, 3, False, tint_seed=1) for g in seq["gray"]]
    q, w = empty_grid(p)
    col = empty_colour(p)
    counts = []
    for k in range(10):
        q, w, col, upd, band, n_col = integrate_colour_model(q, w, col, seq["depth"][k], frames[k], seq["poses"][k], p)
        counts.append((upd, band, n_col))
    return seq, p, frames, q, w, col, counts


def test_pinned_case_reproduces_the_counts(pinned_colour):
    seq, p, frames, q, w, col, counts = pinned_colour
    print("updated / in band / colour updates per frame:", counts)
    assert [c[2] for c in counts] == PINNED_UPDATES and [c[1] for c in counts] == PINNED_UPDATES
    assert (int((col[..., 3] > 0).sum()), int((w > 0).sum())) == (98_198, 1_200_587)
    assert (col[..., 3] <= np.minimum(w, 255)).all()                       # a voxel is coloured at most as often as it is observed
    rgba, cls, _ = point_colours_model(q, w, col, detail=True)
    print("extracted points with neither / one / both voxels coloured:", np.bincount(cls, minlength=3).tolist())
    assert len(rgba) == 41_011 and (cls == 2).all() and (rgba[:, 3] == 255).all()


def _against_frame(P, rgba, seq, p, frame, k):
    """Largest-channel difference between the points' colours and frame k's pixels, for the points whose depth reading in frame k
    agrees with them within one voxel; and the same with the colours permuted among those points."""
    K = seq["K"]
    M = world_to_camera(seq["poses"][k]).astype(np.float64)
    cam = P[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    z = cam[:, 2]
    front = z > 0.1
    u = np.where(front, K["f0"] * cam[:, 0] / np.where(front, z, 1.0) + K["cx0"], -1.0)
    v = np.where(front, K["f0"] * cam[:, 1] / np.where(front, z, 1.0) + K["cy0"], -1.0)
    xi, yi = np.floor(u + 0.5).astype(np.int64), np.floor(v + 0.5).astype(np.int64)
    rows, cols = p["size"]
    ok = front & (xi >= 0) & (xi < cols) & (yi >= 0) & (yi < rows)
    xi, yi = np.where(ok, xi, 0), np.where(ok, yi, 0)
    D = seq["depth"][k][yi, xi].astype(np.float64) / seq["depth_scale"]
    ok &= (D > 0) & (np.abs(D - z) <= p["vs"])
    pix = frame[yi[ok], xi[ok]].astype(np.int64)
    mine = rgba[ok, :3].astype(np.int64)
    diff = np.abs(mine - pix).max(1)
    perm = np.random.default_rng(k).permutation(len(mine))
    control = np.abs(mine[perm] - pix).max(1)
    return int(ok.sum()), diff, control


def test_pinned_case_colours_against_the_rendered_frames(pinned_colour):
    """Measured with this model: median largest-channel difference 2 / 3 / 3 levels against frames 0 / 5 / 9
    (99th percentile 18 / 19 / 19), the permuted control 75."""
    seq, p, frames, q, w, col, _ = pinned_colour
    P, _ = extract_model(q, w, p)
    rgba = point_colours_model(q, w, col)
    for k in (0, 5, 9):
        n, diff, control = _against_frame(P, rgba, seq, p, frames[k], k)
        print(f"frame {k}: {n} of {len(P)} points seen; largest-channel difference median {np.median(diff):.0f} p99 "
              f"{np.percentile(diff, 99):.0f} max {diff.max()}; permuted control median {np.median(control):.0f}")
        assert n > 5000
        assert np.median(diff) < np.median(control) / 4, (k, np.median(diff), np.median(control))


def test_pinned_mesh_colours_contain_the_extractions(pinned_colour):
    seq, p, frames, q, w, col, _ = pinned_colour
    rgba, cls, e = mesh_colours_model(q, w, col, detail=True)
    assert np.array_equal(rgba[e < 3], point_colours_model(q, w, col))
    diag = e >= 3
    print(f"mesh: {len(rgba)} vertices; on the four diagonal directions {int(diag.sum())}, of them one-sided {int((cls[diag] == 1).sum())}, "
          f"uncoloured {int((cls[diag] == 0).sum())}; on the three axes one-sided {int((cls[~diag] == 1).sum())}, uncoloured "
          f"{int((cls[~diag] == 0).sum())}")
    assert len(rgba) == 151_864
    assert ((cls == 0) == (rgba[:, 3] == 0)).all()


# ---- code object, PLY -----------------------------------------------------------------------------------------------------------
def test_colour_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        for k in COLOUR_KERNELS:
            if re.fullmatch(r"_ZN3odo%d%sE\w+" % (len(k), k), name):      # the mangled odo::<k>(...): the name matched exactly
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
                print(k, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
    assert sorted(found) == sorted(COLOUR_KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found


def _old_write_ply_normals(path, xyz, normals):
    """The writer as it was before colour: what `rgb=None` must still produce byte for byte."""
    rec = np.zeros(len(xyz), np.dtype([(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")]))
    for c, k in enumerate(("x", "y", "z")):
        rec[k] = xyz[:, c]
        rec["n" + k] = normals[:, c]
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(xyz)) + "".join(
        "property float %s\n" % k for k in ("x", "y", "z", "nx", "ny", "nz")) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def read_ply_colour(path, faces):
    """(vertices (n, 6) float32, rgb (n, 3) uint8, faces (m, 3) or None) of a coloured PLY."""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    props = [ln for ln in lines if ln.startswith("property ")]
    want = ["property float %s" % k for k in ("x", "y", "z", "nx", "ny", "nz")] + ["property uchar %s" % k for k in ("red", "green", "blue")]
    assert props[:9] == want
    dt = np.dtype([("f", "<f4", (6,)), ("c", "u1", (3,))])
    assert dt.itemsize == 27
    vert = np.frombuffer(body[:27 * nv], dt)
    if not faces:
        assert len(props) == 9 and len(body) == 27 * nv
        return vert["f"], vert["c"], None
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    assert props[9:] == ["property list uchar int vertex_indices"] and len(body) == 27 * nv + 13 * nf
    face = np.frombuffer(body[27 * nv:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert (face["n"] == 3).all()
    return vert["f"], vert["c"], face["v"]


def test_ply_writers_round_trip_colour_and_keep_the_uncoloured_bytes(tmp_path):
    from odometry_amd import api
    rng = np.random.default_rng(6)
    xyz0 = rng.normal(size=(53, 4)).astype(f32)
    nrmw = rng.normal(size=(53, 4)).astype(f32)
    rgba = rng.integers(0, 256, (53, 4)).astype(np.uint8)
    tri = rng.integers(0, 53, (91, 3)).astype(np.int32)
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    api.write_ply_normals(a, xyz0, nrmw, rgb=rgba)
    vert, rgb, _ = read_ply_colour(a, False)
    assert np.array_equal(vert[:, :3], xyz0[:, :3]) and np.array_equal(vert[:, 3:], nrmw[:, :3]) and np.array_equal(rgb, rgba[:, :3])
    api.write_ply_mesh(a, xyz0, nrmw, tri, rgb=rgba)
    vert, rgb, face = read_ply_colour(a, True)
    assert np.array_equal(vert[:, :3], xyz0[:, :3]) and np.array_equal(rgb, rgba[:, :3]) and np.array_equal(face, tri)
    api.write_ply_mesh(a, xyz0[:0], nrmw[:0], tri[:0], rgb=rgba[:0])
    assert [len(x) for x in read_ply_colour(a, True)] == [0, 0, 0]
    # without colour: today's bytes
    api.write_ply_normals(a, xyz0, nrmw)
    _old_write_ply_normals(b, xyz0, nrmw)
    assert open(a, "rb").read() == open(b, "rb").read()
    api.write_ply_normals(a, xyz0, nrmw, rgb=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    api.write_ply_mesh(a, xyz0, nrmw, tri)
    vert, face = read_ply_mesh(a)                                          # the existing reader: 24 B per vertex, 13 B per face
    assert np.array_equal(vert[:, :3], xyz0[:, :3]) and np.array_equal(vert[:, 3:], nrmw[:, :3]) and np.array_equal(face, tri)
    plain = open(b, "rb").read()                                           # the same vertex records behind a header with the face element
    faces = np.zeros(len(tri), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    faces["n"], faces["v"] = 3, tri
    want = plain.replace(b"end_header\n", b"element face 91\nproperty list uchar int vertex_indices\nend_header\n", 1) + faces.tobytes()
    assert open(a, "rb").read() == want
