"""The RGB-D front end without a GPU: a numpy model of the spec (include/odometry_hip.h, odo_rgbd_frontend_create) — pinned to the
prose by a second, naive implementation —, its properties (identity, ground truth on three sensor rigs), the grey rule, the C ABI's
six new entries and the 8-bit colour PNG reader. The GPU tests (test_gpu_rgbd_frontend.py) hold the kernels to this model bit for
bit."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["odo_rgbd_frontend_create", "odo_rgbd_frontend_submit_dev", "odo_rgbd_frontend_submit_host", "odo_rgbd_frontend_wait",
               "odo_rgbd_frontend_stats", "odo_rgbd_frontend_destroy"]
FRONTEND_KERNELS = ["rgbd_fe_grey_kernel", "rgbd_fe_register_kernel", "rgbd_fe_resolve_kernel"]
f32 = np.float32
MAX_SPLAT = 4
STAT_KEYS = ("n_depth", "n_filled", "dropped_behind", "dropped_range", "dropped_splat")


# ---- the rigs ------------------------------------------------------------------------------------------------------------------
def rig(depth_size, depth_f, size, f, t_mm, rot_mrad):
    """A sensor rig: depth imager depth_size = (rows, cols) with focal length depth_f, colour camera size with f, principal points at
    the image centres, colour_from_depth from t (millimetres) and the rotation about x, y, z (milliradians)."""
    from odometry_amd import synth
    (dr, dc), (r, c) = depth_size, size
    return dict(depth_size=depth_size, depth_K=(depth_f, depth_f, (dc - 1) / 2.0, (dr - 1) / 2.0), size=size,
                K=(f, (c - 1) / 2.0, (r - 1) / 2.0),
                E=synth.rig_extrinsic([v * 1e-3 for v in t_mm], [v * 1e-3 for v in rot_mrad]))


def RIGS():
    return dict(A=rig((480, 640), 385.0, (480, 640), 525.0, (15.0, 0.5, -0.3), (2.0, -3.0, 1.0)),
                B=rig((480, 640), 570.0, (480, 640), 525.0, (-25.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
                C=rig((480, 848), 425.0, (720, 1280), 920.0, (15.0, 0.0, 0.0), (2.0, -3.0, 1.0)),
                identity=rig((480, 640), 525.0, (480, 640), 525.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))


DRIVE = dict(seed=0, drive="natural", fwd_range=(0.1, 0.2), depth_scale=1000.0, max_range=30.0)


def raw_sequence(r, n, frames=None, **kw):
    """make_raw_rgbd_sequence of the natural drive (seed 0, 0.1-0.2 m per frame, scale 1000, 30 m range) seen by rig r."""
    from odometry_amd import synth
    (rows, cols), (f, cx, cy) = r["size"], r["K"]
    args = dict(DRIVE)
    args.update(kw)
    return synth.make_raw_rgbd_sequence(n, rows=rows, cols=cols, f=f, cx=cx, cy=cy, depth_size=r["depth_size"], depth_f=r["depth_K"][0],
                                        depth_c=r["depth_K"][2:], colour_from_depth=r["E"], frames=frames, **args)


# ---- numpy model of the spec ---------------------------------------------------------------------------------------------------
def grey_model(colour, bgr=False):
    """rows x cols x (3 | 4) uint8 -> fp32 grey: (R 4899 + G 9617 + B 1868 + 8192) >> 14; a fourth channel is ignored."""
    c = np.asarray(colour).astype(np.uint32)
    r, g, b = (c[..., 2], c[..., 1], c[..., 0]) if bgr else (c[..., 0], c[..., 1], c[..., 2])
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.float32)


def register_model(raw, depth_K, K, E, scale_in, scale_out, rows, cols):
    """Steps 1-6 of the registration spec, vectorised: (rows x cols uint16, statistics)."""
    raw = np.asarray(raw, np.uint16)
    fxd, fyd, cxd, cyd = map(f32, depth_K)
    fc, cxc, cyc = map(f32, K)
    E = np.asarray(E, np.float64)
    R, t = E[:3, :3].astype(f32), E[:3, 3].astype(f32)
    s_in, s_out = f32(scale_in), f32(scale_out)
    ys, xs = np.nonzero(raw)
    z = raw[ys, xs].astype(f32) / s_in

    def corner(s):
        X = ((xs.astype(f32) + f32(s)) - cxd) / fxd * z
        Y = ((ys.astype(f32) + f32(s)) - cyd) / fyd * z
        return tuple(((R[i, 0] * X + R[i, 1] * Y) + R[i, 2] * z) + t[i] for i in range(3))

    with np.errstate(all="ignore"):
        X0, Y0, Z0 = corner(-0.5)
        X1, Y1, Z1 = corner(0.5)
        Zm = corner(0.0)[2]
        front = (Z0 > 0) & (Z1 > 0) & (Zm > 0)
        q = np.rint(Zm * s_out)
        u0, u1 = fc * (X0 / Z0) + cxc, fc * (X1 / Z1) + cxc
        v0, v1 = fc * (Y0 / Z0) + cyc, fc * (Y1 / Z1) + cyc
        in_range = (q >= 1) & (q <= 65535) & np.isfinite(u0) & np.isfinite(u1) & np.isfinite(v0) & np.isfinite(v1)
        ua, ub = np.ceil(np.minimum(u0, u1)), np.ceil(np.maximum(u0, u1)) - f32(1)
        va, vb = np.ceil(np.minimum(v0, v1)), np.ceil(np.maximum(v0, v1)) - f32(1)
        big = ((ub - ua) + f32(1) > MAX_SPLAT) | ((vb - va) + f32(1) > MAX_SPLAT)
    behind = ~front
    rng = front & ~in_range
    splat = front & in_range & big
    ok = front & in_range & ~big
    zb = np.full(rows * cols, 0xFFFFFFFF, np.uint32)
    for dy in range(MAX_SPLAT):
        for dx in range(MAX_SPLAT):
            with np.errstate(all="ignore"):
                uu, vv = ua + f32(dx), va + f32(dy)
                m = ok & (uu <= ub) & (vv <= vb) & (uu >= 0) & (uu <= cols - 1) & (vv >= 0) & (vv <= rows - 1)
            idx = vv[m].astype(np.int64) * cols + uu[m].astype(np.int64)
            np.minimum.at(zb, idx, q[m].astype(np.uint32))
    filled = zb != 0xFFFFFFFF
    out = np.where(filled, zb, 0).astype(np.uint16).reshape(rows, cols)
    st = dict(n_depth=int(len(z)), n_filled=int(filled.sum()), dropped_behind=int(behind.sum()), dropped_range=int(rng.sum()),
              dropped_splat=int(splat.sum()))
    return out, st


def register_naive(raw, depth_K, K, E, scale_in, scale_out, rows, cols):
    """The same spec, read off the prose one pixel and one fp32 operation at a time."""
    fxd, fyd, cxd, cyd = (f32(v) for v in depth_K)
    fc, cxc, cyc = (f32(v) for v in K)
    R = [[f32(E[i][j]) for j in range(3)] for i in range(3)]
    t = [f32(E[i][3]) for i in range(3)]
    out = [[None] * cols for _ in range(rows)]
    st = dict(n_depth=0, n_filled=0, dropped_behind=0, dropped_range=0, dropped_splat=0)
    with np.errstate(all="ignore"):
        for y in range(raw.shape[0]):
            for x in range(raw.shape[1]):
                r = int(raw[y][x])
                if r == 0:
                    continue
                st["n_depth"] += 1
                z = f32(r) / f32(scale_in)                                                     # step 1
                pts = []
                for s in (f32(-0.5), f32(0.0), f32(0.5)):                                      # step 2
                    X = f32(f32(f32(f32(f32(x) + s) - cxd) / fxd) * z)
                    Y = f32(f32(f32(f32(f32(y) + s) - cyd) / fyd) * z)
                    pts.append([f32(f32(f32(f32(R[i][0] * X) + f32(R[i][1] * Y)) + f32(R[i][2] * z)) + t[i]) for i in range(3)])
                (X0, Y0, Z0), (_, _, Zm), (X1, Y1, Z1) = pts
                if not (Z0 > 0 and Z1 > 0 and Zm > 0):                                         # step 3
                    st["dropped_behind"] += 1
                    continue
                q = np.rint(f32(Zm * f32(scale_out)))                                          # step 4
                if not (1 <= q <= 65535):
                    st["dropped_range"] += 1
                    continue
                u0, u1 = f32(f32(fc * f32(X0 / Z0)) + cxc), f32(f32(fc * f32(X1 / Z1)) + cxc)   # step 5
                v0, v1 = f32(f32(fc * f32(Y0 / Z0)) + cyc), f32(f32(fc * f32(Y1 / Z1)) + cyc)
                if not all(np.isfinite(w) for w in (u0, u1, v0, v1)):
                    st["dropped_range"] += 1
                    continue
                ua, ub = np.ceil(min(u0, u1)), f32(np.ceil(max(u0, u1)) - f32(1))
                va, vb = np.ceil(min(v0, v1)), f32(np.ceil(max(v0, v1)) - f32(1))
                if f32(f32(ub - ua) + f32(1)) > MAX_SPLAT or f32(f32(vb - va) + f32(1)) > MAX_SPLAT:
                    st["dropped_splat"] += 1
                    continue
                if ua > ub or va > vb or ub < 0 or vb < 0 or ua > cols - 1 or va > rows - 1:
                    continue                                                                   # empty, or wholly outside the image
                for v in range(max(int(va), 0), min(int(vb), rows - 1) + 1):
                    for u in range(max(int(ua), 0), min(int(ub), cols - 1) + 1):
                        out[v][u] = int(q) if out[v][u] is None else min(out[v][u], int(q))    # step 6
    st["n_filled"] = sum(1 for row in out for w in row if w is not None)
    return np.array([[0 if w is None else w for w in row] for row in out], np.uint16), st


def frontend_model(colour, raw, r, scale_in, scale_out, bgr=False):
    """One frame through the model for rig r: (grey, registered depth, statistics)."""
    rows, cols = r["size"]
    dep, st = register_model(raw, r["depth_K"], r["K"], r["E"], scale_in, scale_out, rows, cols)
    return grey_model(colour, bgr), dep, st


# ---- the model against its naive twin --------------------------------------------------------------------------------------------
def _small_raw(seed, rows, cols, lo=300, hi=6000):
    rng = np.random.default_rng(seed)
    raw = rng.integers(lo, hi, (rows, cols)).astype(np.uint16)
    raw[rng.random((rows, cols)) < 0.15] = 0
    raw[0, 0], raw[-1, -1] = 65535, 1
    return raw


@pytest.mark.parametrize("case", ["rig", "identity", "magnify", "flipped", "scale_out", "near_plane", "downsample"])
def test_vectorised_model_equals_the_naive_one_bit_for_bit(case):
    from odometry_amd import synth
    dsize, size = (20, 28), (20, 28)
    dK, K = (30.0, 31.0, 13.5, 9.5), (40.0, 13.5, 9.5)
    E = synth.rig_extrinsic((0.015, 0.0005, -0.0003), (0.002, -0.003, 0.001))
    s_in = s_out = 1000.0
    raw = _small_raw(3, *dsize)
    if case == "identity":
        dK, E = (40.0, 40.0, 13.5, 9.5), np.eye(4)
    elif case == "magnify":           # footprints of 4 to 5 pixels: both sides of the splat bound
        K = (122.0, 13.5, 9.5)
        size = (30, 40)
    elif case == "flipped":           # 180 degrees about y: everything behind the colour camera
        E = synth.rig_extrinsic((0.0, 0.0, 0.0), (0.0, np.pi, 0.0))
    elif case == "scale_out":         # q past 65535 for most readings
        s_out = 30000.0
    elif case == "near_plane":        # the colour camera 1 m in front of the depth imager: corners on both sides of Z = 0
        E = synth.rig_extrinsic((0.0, 0.0, -1.0), (0.3, 0.2, 0.0))
        raw = _small_raw(4, *dsize, lo=900, hi=1200)
    elif case == "downsample":        # a depth grid finer than the target: empty footprints
        K = (12.0, 6.0, 4.0)
        size = (10, 14)
    a, sa = register_model(raw, dK, K, E, s_in, s_out, *size)
    b, sb = register_naive(raw, dK, K, E, s_in, s_out, *size)
    assert sa == sb, (sa, sb)
    assert np.array_equal(a, b), f"{int((a != b).sum())} pixels differ"
    n = sa["n_depth"]
    assert n == int((raw != 0).sum())
    if case == "identity":
        assert np.array_equal(a, raw) and sa["n_filled"] == n
    if case == "magnify":
        assert 0 < sa["dropped_splat"] < n and sa["n_filled"] > 0
    if case == "flipped":
        assert sa["dropped_behind"] == n and not a.any()
    if case == "scale_out":
        assert sa["dropped_range"] > n // 2 and sa["n_filled"] > 0
    if case == "near_plane":
        assert sa["dropped_behind"] > 0
    if case == "downsample":
        assert sa["dropped_splat"] == 0 and sa["n_filled"] < n


# ---- identity --------------------------------------------------------------------------------------------------------------------
def test_identity_rig_reproduces_its_input_exactly():
    r = RIGS()["identity"]
    seq = raw_sequence(r, 6, frames=[0, 5])
    for raw in seq["raw_depth"] + [np.full((480, 640), 65535, np.uint16), np.zeros((480, 640), np.uint16),
                                   _small_raw(9, 480, 640, 1, 65536)]:
        out, st = register_model(raw, r["depth_K"], r["K"], r["E"], 1000.0, 1000.0, 480, 640)
        assert np.array_equal(out, raw)
        n = int((raw != 0).sum())
        assert st == dict(n_depth=n, n_filled=n, dropped_behind=0, dropped_range=0, dropped_splat=0)


# ---- ground truth ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,min_fill", [("A", 0.99), ("B", 0.80), ("C", 0.99)])
def test_registered_depth_against_ground_truth(name, min_fill):
    r = RIGS()[name]
    seq = raw_sequence(r, 6, frames=[0, 5])
    for k, raw, gt in zip(seq["frames"], seq["raw_depth"], seq["depth_gt"]):
        out, st = register_model(raw, r["depth_K"], r["K"], r["E"], 1000.0, 1000.0, *r["size"])
        have, filled = gt > 0, out > 0
        both = have & filled
        rel = np.abs(out.astype(np.int64) - gt.astype(np.int64))[both] / gt[both]
        fill = both.sum() / have.sum()
        w1, w2 = np.mean(rel <= 0.01), np.mean(rel <= 0.02)
        stray = (filled & ~have).sum() / out.size
        print(f"rig {name} frame {k}: filled {fill:.4f} of ground truth, within 1 % {w1:.4f}, within 2 % {w2:.4f}, "
              f"filled without ground truth {stray:.5f} of the frame, {st}")
        assert fill >= min_fill
        assert w1 >= 0.98 and w2 >= 0.999
        assert stray <= 0.002
        assert st["dropped_splat"] == 0


# ---- grey ------------------------------------------------------------------------------------------------------------------------
def test_grey_rule():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(grey_model(np.stack([v, v, v], -1)[None]), v.astype(np.float32)[None])
    rng = np.random.default_rng(11)
    px = rng.integers(0, 256, (256, 256, 4)).astype(np.uint8)
    want = np.array([[(int(r) * 4899 + int(g) * 9617 + int(b) * 1868 + 8192) >> 14 for r, g, b, _ in row] for row in px], np.float32)
    assert np.array_equal(grey_model(px), want)
    assert np.array_equal(grey_model(px[..., :3]), want)                       # alpha ignored
    assert np.array_equal(grey_model(px[..., [2, 1, 0, 3]], bgr=True), want)   # BGR(A) = RGB(A) with the channels swapped
    assert not np.array_equal(grey_model(px, bgr=True), want)
    assert want.min() >= 0 and want.max() <= 255


def test_raw_sequence_is_the_rgbd_drive_seen_by_a_rig():
    from odometry_amd import synth
    ident = raw_sequence(RIGS()["identity"], 3)
    ref = synth.make_rgbd_sequence(3, **DRIVE)
    for k in range(3):
        assert np.array_equal(grey_model(ident["colour"][k]), ref["gray"][k])
        assert np.array_equal(ident["raw_depth"][k], ref["depth"][k]) and np.array_equal(ident["depth_gt"][k], ref["depth"][k])
    a = raw_sequence(RIGS()["A"], 3, frames=[2], channels=4, bgr=True, tint_seed=1)
    c = a["colour"][0]
    assert c.shape == (480, 640, 4) and c.dtype == np.uint8 and a["raw_depth"][0].shape == (480, 640)
    assert not np.array_equal(c[..., 0], c[..., 1]) and not np.array_equal(c[..., 1], c[..., 2])
    assert not np.array_equal(a["raw_depth"][0], a["depth_gt"][0])
    rgb = raw_sequence(RIGS()["A"], 3, frames=[2], channels=3, bgr=False, tint_seed=1)["colour"][0]
    assert np.array_equal(rgb, c[..., [2, 1, 0]])


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def _params(**kw):
    from odometry_amd import _lib as L
    p = L.RgbdFrontendParams()
    p.depth_rows, p.depth_cols, p.rows, p.cols = 480, 640, 480, 640
    p.depth_fx = p.depth_fy = 385.0
    p.depth_cx, p.depth_cy = 319.5, 239.5
    p.depth_scale_in = p.depth_scale_out = 1000.0
    p.K = L.Intrinsics(525.0, 319.5, 239.5)
    for i, v in enumerate(np.eye(4)[:3].reshape(-1)):
        p.colour_from_depth[i] = v
    p.colour_channels, p.colour_bgr, p.slots = 3, 0, 3
    for k, v in kw.items():
        if k == "K":
            p.K = L.Intrinsics(*v)
        elif k == "e0":
            p.colour_from_depth[0] = v
        else:
            setattr(p, k, v)
    return p


def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    assert C.sizeof(_lib.RgbdFrontendParams) == 4 * (2 + 5 + 2 + 3 + 1 + 12 + 3)
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in FRONTEND_KERNELS:
        assert k.encode() in blob, f"{k} is not in the library"


def test_create_validates_before_touching_a_device_and_fails_cleanly_without_one():
    from odometry_amd import _lib as L
    from odometry_amd import api
    lib = L.load()
    h = C.c_void_p()
    inf, nan = float("inf"), float("nan")
    bad = [dict(depth_rows=0), dict(depth_cols=-1), dict(rows=0), dict(cols=0), dict(depth_fx=0.0), dict(depth_fy=-1.0),
           dict(depth_fx=inf), dict(depth_fy=nan), dict(K=(0.0, 1.0, 1.0)), dict(K=(nan, 1.0, 1.0)), dict(K=(525.0, inf, 1.0)),
           dict(depth_cx=nan), dict(depth_scale_in=0.0), dict(depth_scale_in=inf), dict(depth_scale_out=-1.0),
           dict(depth_scale_out=nan), dict(e0=nan), dict(e0=inf), dict(colour_channels=1), dict(colour_channels=5),
           dict(colour_bgr=2), dict(slots=1), dict(slots=9)]
    for kw in bad:
        assert lib.odo_rgbd_frontend_create(None, C.byref(_params(**kw)), C.byref(h)) == -1 and not h.value, kw
        assert "odo_rgbd_frontend_create" in L.last_error() and "NULL" not in L.last_error(), (kw, L.last_error())
    assert lib.odo_rgbd_frontend_create(None, None, C.byref(h)) == -1
    assert lib.odo_rgbd_frontend_create(None, C.byref(_params()), C.byref(h)) == -1 and "NULL ctx" in L.last_error()
    assert lib.odo_rgbd_frontend_destroy(None) == 0
    assert lib.odo_rgbd_frontend_wait(None, None) == -1 and lib.odo_rgbd_frontend_stats(None, None, None) == -1
    ctx = C.c_void_p()
    if lib.odo_ctx_create(0, C.byref(ctx)) != 0:      # no device: the front end fails as the context does, no fallback
        with pytest.raises(L.OdoError):
            api.RgbdFrontend(api.Context(0), (480, 640), (385.0, 385.0, 319.5, 239.5), 1000.0, (480, 640), (525.0, 319.5, 239.5), 1000.0)
    else:
        assert lib.odo_rgbd_frontend_create(ctx, C.byref(_params()), C.byref(h)) == 0 and h.value
        assert lib.odo_rgbd_frontend_destroy(h) == 0 and lib.odo_ctx_destroy(ctx) == 0


# ---- 8-bit colour PNG reader ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def io_rgb8(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("io_rgb8") / "io_rgb8_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "io_rgb8_harness.cpp")])
    return C.CDLL(so)


def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)


def _filter_row(ft, cur, up, bpp):
    out = bytearray(len(cur))
    for x in range(len(cur)):
        a = cur[x - bpp] if x >= bpp else 0
        b = up[x] if up is not None else 0
        c = up[x - bpp] if (up is not None and x >= bpp) else 0
        if ft == 0:
            p = 0
        elif ft == 1:
            p = a
        elif ft == 2:
            p = b
        elif ft == 3:
            p = (a + b) // 2
        else:
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
        out[x] = (cur[x] - p) & 0xff
    return bytes(out)


def write_png(path, rows, width, bpp, filters, depth, colour, interlace=0, split=0, extra=b""):
    """rows: the unfiltered bytes of each row; bpp: the filters' distance."""
    raw = b"".join(bytes([filters[y % len(filters)]]) + _filter_row(filters[y % len(filters)], rows[y], rows[y - 1] if y else None, bpp)
                   for y in range(len(rows)))
    comp = zlib.compress(raw, 6)
    parts = [comp] if not split else [comp[i:i + split] for i in range(0, len(comp), split)]
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", width, len(rows), depth, colour, 0, 0, interlace)) + extra
    data += b"".join(_chunk(b"IDAT", p) for p in parts) + _chunk(b"IEND", b"")
    open(path, "wb").write(data)
    return data


def _read_rgb8(io, path, cap):
    out = np.zeros(cap, np.uint8)
    w, h, ch = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = io.io_read_png_rgb8(str(path).encode(), out.ctypes.data_as(C.c_void_p), cap, C.byref(w), C.byref(h), C.byref(ch))
    return rc, out[:w.value * h.value * ch.value].reshape(h.value, w.value, ch.value) if rc == 0 else None


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("filters,split", [([0], 0), ([1], 0), ([2], 0), ([3], 0), ([4], 0), ([0, 1, 2, 3, 4], 0), ([4, 3, 2, 1, 0], 97)])
def test_png_rgb8_reader_round_trips(io_rgb8, tmp_path, filters, split, channels):
    rng = np.random.default_rng(len(filters) * 7 + split + channels)
    img = rng.integers(0, 256, (23, 37, channels)).astype(np.uint8)
    img[3:9, 5:20] = (100 + np.arange(15, dtype=np.uint8))[None, :, None] + np.arange(channels, dtype=np.uint8)   # smooth: predictors matter
    img[0, 0], img[-1, -1] = 0, 255
    p = tmp_path / "c.png"
    write_png(p, [img[y].tobytes() for y in range(23)], 37, channels, filters, 8, 2 if channels == 3 else 6, split=split)
    rc, got = _read_rgb8(io_rgb8, p, img.size)
    assert rc == 0 and got.shape == img.shape and np.array_equal(got, img)


def test_png_rgb8_reader_rejects_other_formats_and_truncation(io_rgb8, tmp_path):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (12, 10, 3)).astype(np.uint8)
    rows = [img[y].tobytes() for y in range(12)]
    p = tmp_path / "x.png"
    cap = 4 * img.size
    write_png(p, [r + r for r in rows], 10, 6, [0], 16, 2)                                  # 16-bit colour
    assert _read_rgb8(io_rgb8, p, cap)[0] == -1
    write_png(p, [r[:10] for r in rows], 10, 1, [0], 8, 3, extra=_chunk(b"PLTE", bytes(range(48))))   # palette
    assert _read_rgb8(io_rgb8, p, cap)[0] == -1
    write_png(p, [r[:10] for r in rows], 10, 1, [0], 8, 0)                                  # 8-bit grey
    assert _read_rgb8(io_rgb8, p, cap)[0] == -1
    write_png(p, rows, 10, 3, [0], 8, 2, interlace=1)                                       # Adam7 flag
    assert _read_rgb8(io_rgb8, p, cap)[0] == -1
    data = write_png(p, rows, 10, 3, [4], 8, 2)
    assert _read_rgb8(io_rgb8, p, cap)[0] == 0
    for cut in (len(data) - 20, len(data) // 2, 40):                                        # truncated inside IDAT / IHDR
        open(p, "wb").write(data[:cut])
        assert _read_rgb8(io_rgb8, p, cap)[0] == -1
    assert _read_rgb8(io_rgb8, tmp_path / "missing.png", cap)[0] == -1
