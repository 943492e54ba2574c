"""RGB-D tracking without a GPU: the C ABI's four new entries, a numpy model of the sensor-depth spec (include/odometry_hip.h,
odo_tracker_create_rgbd) — the point selection pinned to the oracle's ComputeDepth, bit for bit —, a model runner of the frame
loop that the GPU tests compare against, the 16-bit PNG reader, and the new kernels' code object."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["odo_tracker_create_rgbd", "odo_tracker_init_rgbd", "odo_tracker_track_rgbd", "odo_tracker_hint_next_rgbd"]
RGBD_KERNELS = ["rgbd_depth_kernel", "rgbd_stats_kernel"]

# The drive the tracking tests use (pinned with RgbdModelRunner below): the natural drive's scene seen by a RealSense-like sensor.
DRIVE = dict(seed=0, drive="natural", fwd_range=(0.1, 0.2), depth_scale=1000.0, max_range=30.0)
N_FRAMES = 52
MAX_DEPTH_STEP = 0.05


# ---- numpy model of the spec -----------------------------------------------------------------------------------------------
def select_model(gray, boundary=4, grad_th=8.0):
    """The point selection (ref: src/depth_estimate.cpp:300-342) on the 3x3-blurred image: uint8 mask."""
    from oracle import oracle as O
    L = O.blur3x3(np.asarray(gray, np.float32))
    rows, cols = L.shape
    bw, bh = (cols - 2 * boundary) // 32, (rows - 2 * boundary) // 16
    val = np.zeros((rows, cols), np.uint8)
    half, th_add = np.float32(0.5), np.float32(grad_th)
    for b in range(16 * 32):
        sy, sx = boundary + (b // 32) * bh, boundary + (b % 32) * bw
        gx = half * (L[sy:sy + bh, sx + 1:sx + bw + 1] - L[sy:sy + bh, sx - 1:sx + bw - 1])
        gy = half * (L[sy + 1:sy + bh + 1, sx:sx + bw] - L[sy - 1:sy + bh - 1, sx:sx + bw])
        m = np.sqrt(gx * gx + gy * gy).reshape(-1)
        th = np.float32(np.sort(m)[m.size // 2] + th_add)
        for e in np.flatnonzero(m > th)[:80]:
            val[sy + e // bw, sx + e % bw] = 1
    return val


def convert_model(sel, raw, depth_scale, max_depth_step, min_depth=0.1, max_depth=30.0):
    """Step 2 and 3 of the spec on a selection mask: (val, dep, stats)."""
    sel = np.asarray(sel) != 0
    raw = np.asarray(raw, np.uint16)
    r = raw.astype(np.int64)
    rf = raw.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = np.float32(depth_scale) / rf
        z = np.float32(1) / d
        lim = np.float32(max_depth_step) * rf
    good = sel & (raw != 0) & ~((z > np.float32(max_depth)) | (z < np.float32(min_depth)))
    pad = np.pad(r, 1)   # outside the image: 0, which the guard skips
    rows, cols = raw.shape
    for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
        q = pad[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols]
        with np.errstate(invalid="ignore"):
            good &= ~((q != 0) & (np.abs(q - r).astype(np.float32) > lim))
    val = good.astype(np.uint8)
    dep = np.where(good, d, np.float32(0)).astype(np.float32)
    n_valid = int(good.sum())
    st = dict(n_selected=int(sel.sum()), n_matched=int((sel & (raw != 0)).sum()), n_valid=n_valid, iters=0, cost=0.0,
              status=-1 if n_valid < 500 else 0)
    return val, dep, st


def rgbd_depth_model(gray, raw, depth_scale, max_depth_step, boundary=4, grad_th=8.0, min_depth=0.1, max_depth=30.0):
    return convert_model(select_model(gray, boundary, grad_th), raw, depth_scale, max_depth_step, min_depth, max_depth)


def invert4_f32(T):
    """The tracker's 4x4 inverse (tracker.hip.h invert4): Gauss-Jordan with partial pivoting in fp64, rounded to fp32."""
    a = np.zeros((4, 8))
    a[:, :4] = np.asarray(T, np.float32).astype(np.float64)
    a[:, 4:] = np.eye(4)
    for c in range(4):
        piv = c
        for i in range(c + 1, 4):
            if abs(a[i, c]) > abs(a[piv, c]):
                piv = i
        if a[piv, c] == 0.0:
            return np.full((4, 4), np.nan, np.float32)
        if piv != c:
            a[[c, piv]] = a[[piv, c]]
        a[c] = a[c] / a[c, c]
        for i in range(4):
            if i != c:
                a[i] = a[i] - a[i, c] * a[c]
    return a[:, 4:].astype(np.float32)


class RgbdModelRunner:
    """The reference's frame loop (oracle/runner.py) with the depth of every frame from the model above: oracle pyramids and LM,
    the runner's chaining and keyframe test."""

    def __init__(self, K, depth_scale, max_depth_step=MAX_DEPTH_STEP, boundary=4, levels=4, motion_th=1.1):
        from oracle import oracle as O
        self.O = O
        self.lp = O.lm_params(K=K, max_iters=(10, 20, 30, 30)[:levels])
        self.depth_args = dict(depth_scale=depth_scale, max_depth_step=max_depth_step, boundary=boundary)
        self.levels, self.motion_th = levels, np.float32(motion_th)

    def depth(self, gray, raw):
        return rgbd_depth_model(gray, raw, **self.depth_args)

    def init(self, gray, raw, abs_pose0=None):
        val, dep, st = self.depth(gray, raw)
        if st["status"] != 0:
            raise RuntimeError("Init 0-th frame failed!")
        self.kf_img = self.O.image_pyramid(gray, self.levels, True, flat=True)
        self.kf_dep = self.O.depth_pyramid(dep, self.levels, flat=True)
        self.kf_abs = np.eye(4, dtype=np.float32) if abs_pose0 is None else np.asarray(abs_pose0, np.float32)
        self.init_pose = np.eye(4, dtype=np.float32)
        self.n_keyframes = 1
        return dict(val=val, dep=dep, **st)

    def track(self, gray, raw):
        from oracle.runner import KEYFRAME_WEIGHT, matmul4_f32, motion_angles
        rows, cols = np.asarray(gray).shape
        img = self.O.image_pyramid(gray, self.levels, True, flat=True)
        r = self.O.lm_solve(self.kf_img, self.kf_dep, img, rows, cols, self.lp, init=self.init_pose)
        T = r["pose"]
        val, dep, st = self.depth(gray, raw)
        cur = matmul4_f32(self.kf_abs, invert4_f32(T))
        out = dict(pose_to_keyframe=T, abs_pose=cur, solve_status=r["status"], val=val, dep=dep, **st)
        if st["status"] != 0:
            out.update(new_keyframe=False, motion=0.0)
            return out
        mot = np.concatenate([np.abs(motion_angles(T)), np.abs(T[:3, 3])]).astype(np.float32)
        mag = np.float32(0)
        for m, w in zip(mot, KEYFRAME_WEIGHT):
            mag = np.float32(mag + np.float32(m * w))
        new_kf = bool(mag > self.motion_th)
        if new_kf:
            self.kf_img, self.kf_dep, self.kf_abs = img, self.O.depth_pyramid(dep, self.levels, flat=True), cur
            self.n_keyframes += 1
        self.init_pose = T
        out.update(new_keyframe=new_kf, motion=float(mag))
        return out


def drive(n=N_FRAMES):
    from odometry_amd import synth
    return synth.make_rgbd_sequence(n, **DRIVE)


def run_model(seq, n=None):
    """Rows of the model runner over the drive (frame 0 = init)."""
    n = n or len(seq["gray"])
    K = seq["K"]
    m = RgbdModelRunner(K, seq["depth_scale"])
    rows = [m.init(seq["gray"][0], seq["depth"][0])]
    for k in range(1, n):
        rows.append(m.track(seq["gray"][k], seq["depth"][k]))
    return rows, m.n_keyframes


def translation_errors(rows, poses):
    return np.array([np.linalg.norm(r["abs_pose"][:3, 3].astype(np.float64) - np.asarray(P)[:3, 3]) for r, P in zip(rows[1:], poses[1:])])


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"


def test_rgbd_tracker_rejects_bad_arguments_before_touching_a_device():
    from odometry_amd import _lib as L
    lib = L.load()
    p = L.TrackerParams()
    assert lib.odo_tracker_default_params(C.byref(p)) == 0
    h = C.c_void_p()
    for scale, step in ((0.0, 0.05), (-1.0, 0.05), (float("inf"), 0.05), (float("nan"), 0.05), (1000.0, -0.01), (1000.0, float("nan"))):
        assert lib.odo_tracker_create_rgbd(0, C.byref(p), scale, step, C.byref(h)) != 0 and not h.value
        assert "odo_tracker_create_rgbd" in L.last_error()
    p.boundary = 0
    assert lib.odo_tracker_create_rgbd(0, C.byref(p), 1000.0, 0.05, C.byref(h)) != 0 and "boundary" in L.last_error()
    assert lib.odo_tracker_create_rgbd(0, None, 1000.0, 0.05, C.byref(h)) != 0


# ---- the model against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(480, 640), (376, 1241)])
def test_selection_model_equals_the_oracles_compute_depth_selection(O, shape):
    from odometry_amd import synth
    rows, cols = shape
    scene = synth.drive_scene("natural", 1)
    for k, T in enumerate(synth.trajectory(3, 1, fwd_range=(0.2, 0.4))):
        img, _ = scene.render(T, rows, cols, 1.2 * cols / 2, (cols - 1) / 2, (rows - 1) / 2, 0.0)
        for boundary in (4, 2):
            ref = O.compute_depth(img, img, O.depth_params(any_size=1, boundary=boundary), stage=1)["val"]
            got = select_model(img, boundary)
            assert np.array_equal(got, ref), f"frame {k}, boundary {boundary}: {int((got != ref).sum())} pixels differ"
            assert got.sum() > 1000


def test_conversion_model_on_hand_made_cases():
    sel = np.zeros((6, 8), np.uint8)
    raw = np.full((6, 8), 1000, np.uint16)
    sel[1, 1] = sel[1, 3] = sel[1, 5] = sel[3, 1] = sel[3, 3] = sel[3, 5] = sel[0, 7] = sel[5, 0] = 1
    raw[1, 1] = 0                     # hole
    raw[1, 3] = 50                    # 0.05 m at scale 1000: below min_depth 0.1
    raw[1, 5] = 65535                 # 65.5 m: beyond max_depth 30
    raw[2, 1] = 1050                  # a step of exactly 5 %: kept (the guard is strict)
    raw[3, 4] = 1051                  # 5.1 %: dropped
    raw[0, 6] = 0                     # a hole next to a selected pixel: skipped
    raw[5, 0] = 1000                  # corner: the neighbours outside are skipped
    val, dep, st = convert_model(sel, raw, 1000.0, 0.05)
    assert val[1, 1] == 0 and val[1, 3] == 0 and val[1, 5] == 0
    assert val[3, 1] == 1 and dep[3, 1] == np.float32(1000.0) / np.float32(1000.0)
    assert val[3, 3] == 0 and val[3, 5] == 0         # raw[3, 4] = 1051 next to both
    assert val[0, 7] == 1 and val[5, 0] == 1
    assert st["n_selected"] == 8 and st["n_matched"] == 7 and st["n_valid"] == int(val.sum()) and st["status"] == -1
    val2, _, st2 = convert_model(sel, raw, 1000.0, np.inf)
    assert val2[3, 3] == 1 and val2[3, 5] == 1 and st2["n_valid"] == st["n_valid"] + 2
    assert np.all(dep[val == 0] == 0)


# ---- the drive -----------------------------------------------------------------------------------------------------------------
def test_model_runner_tracks_the_pinned_drive():
    """The drive the GPU tests use: the reference's keyframe policy switches at least twice, and the model stays within 5 cm of the
    ground truth on at least 90 % of the frames."""
    seq = drive()
    rows, n_kf = run_model(seq)
    err = translation_errors(rows, seq["poses"])
    assert rows[0]["n_valid"] > 10000
    assert n_kf >= 3, n_kf
    assert np.mean(err < 0.05) >= 0.9, np.round(err, 3)


# ---- 16-bit PNG reader ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def io16(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("io16") / "io16_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "io16_harness.cpp")])
    return C.CDLL(so)


def _chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)


def _filter_row(ft, cur, up, bpp=2):
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


def write_png16(path, img, filters, split=0, depth=16, colour=0):
    h, w = img.shape
    rows = [img[y].astype(">u2").tobytes() for y in range(h)]
    raw = b"".join(bytes([filters[y % len(filters)]]) + _filter_row(filters[y % len(filters)], rows[y], rows[y - 1] if y else None)
                   for y in range(h))
    comp = zlib.compress(raw, 6)
    parts = [comp] if not split else [comp[i:i + split] for i in range(0, len(comp), split)]
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, 0))
    data += b"".join(_chunk(b"IDAT", p) for p in parts) + _chunk(b"IEND", b"")
    open(path, "wb").write(data)
    return data


def _read16(io16, path, cap):
    out = np.zeros(cap, np.uint16)
    w, h = C.c_int(0), C.c_int(0)
    rc = io16.io_read_png16(str(path).encode(), out.ctypes.data_as(C.c_void_p), cap, C.byref(w), C.byref(h))
    return rc, out[:w.value * h.value].reshape(h.value, w.value) if rc == 0 else None


@pytest.mark.parametrize("filters,split", [([0], 0), ([1], 0), ([2], 0), ([3], 0), ([4], 0), ([0, 1, 2, 3, 4], 0), ([4, 3, 2, 1, 0], 97)])
def test_png16_reader_round_trips(io16, tmp_path, filters, split):
    rng = np.random.default_rng(len(filters) * 7 + split)
    img = rng.integers(0, 65536, (23, 37)).astype(np.uint16)
    img[3:9, 5:20] = 5000 + np.arange(15, dtype=np.uint16)   # smooth patches where the predictors matter
    img[0, 0], img[-1, -1] = 0, 65535
    p = tmp_path / "d.png"
    write_png16(p, img, filters, split)
    rc, got = _read16(io16, p, img.size)
    assert rc == 0 and np.array_equal(got, img)


def test_png16_reader_rejects_other_formats_and_truncation(io16, tmp_path):
    img = np.arange(12 * 10, dtype=np.uint16).reshape(12, 10) * 500
    p = tmp_path / "x.png"
    write_png16(p, img.astype(np.uint8), [0], depth=8)                    # 8-bit grey
    assert _read16(io16, p, img.size)[0] == -1
    rgb = np.repeat(img, 3, axis=1)
    write_png16(p, rgb, [0], colour=2)                                     # 16-bit colour
    assert _read16(io16, p, rgb.size)[0] == -1
    data = write_png16(p, img, [4])
    for cut in (len(data) - 20, len(data) // 2, 40):                       # truncated inside IDAT / IHDR
        open(p, "wb").write(data[:cut])
        assert _read16(io16, p, img.size)[0] == -1
    assert _read16(io16, tmp_path / "missing.png", img.size)[0] == -1


# ---- code object ---------------------------------------------------------------------------------------------------------------
def test_rgbd_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        for k in RGBD_KERNELS:
            if k in name:
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert sorted(found) == sorted(RGBD_KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found
