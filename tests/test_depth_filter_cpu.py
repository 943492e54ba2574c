"""The bilateral depth filter (odo_depth_filter_*, api.DepthFilter, api.depth_filter_tables, synth.sensor_noise) without a GPU: the
numpy model of the specification (include/odometry_hip.h) pinned to the prose by a plain loop on every row
of tests/depth_filter_cases.py, every row held to the situation it is in the table for, the rule's four properties on random frames
and tables, the host + device header odometry_amd/csrc/depth_filter_math.h as a stand-alone g++ program under sanitizers, the default
tables, three mutants of the rule each caught by its row, the sequences' bytes without noise, what the filter does to the Kinect
noise model on the ribbed corridor, the ABI and the kernels' code-object metadata.

The model is the yardstick of tests/test_gpu_depth_filter.py, which asks the GPU for the same bits."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import depth_filter_cases as dfc

ROOT = dfc.ROOT
HARNESS = os.path.join(ROOT, "tests", "depth_filter_harness.cpp")
NEW_SYMBOLS = ["odo_depth_filter_create", "odo_depth_filter_run_dev", "odo_depth_filter_stats", "odo_depth_filter_time_dev",
               "odo_depth_filter_destroy"]
LOOP_PIXELS = 2500   # rows up to this size go through the loop at every radius, larger ones at the radius their predicate names

# Measured with this model on frame 1 of the ribbed corridor, noise seed 7, depth_filter_tables(radius=2, sigma0=8, gain=3)
# (test_filter_lowers_the_noise_of_the_ribbed_corridor prints them): RMS error against the clean frame over Z <= 5 m, raw units,
# before -> after the filter, and the RMS by which the filter moves the CLEAN frame.
MEASURED = {(120, 160): dict(before=17.39, after=12.13, clean=3.59), (240, 320): dict(before=17.17, after=7.98, clean=2.49)}


def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api, synth
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", header) and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert C.sizeof(_lib.DepthFilterParams) == 12 + 81 + 256 + 256 + 3      # (padded to the ints' alignment)
    assert hasattr(api, "DepthFilter") and hasattr(api, "depth_filter_tables") and hasattr(synth, "sensor_noise")
    assert api.KINECT_AXIAL_NOISE == synth.KINECT_AXIAL_NOISE == (0.0012, 0.0019, 0.4)


def _params(rows=8, cols=8, tables=None):
    from odometry_amd import _lib
    ws, wr, shift = tables or dfc.default_tables(2)
    p = _lib.DepthFilterParams()
    p.rows, p.cols, p.radius = rows, cols, (len(ws) - 1) // 2
    for i, v in enumerate(np.asarray(ws).reshape(-1)):
        p.ws[i] = int(v)
    for i in range(256):
        p.wr[i], p.shift[i] = int(wr[i]), int(shift[i])
    return p


def bad_params():
    """(what, params) for every bound of odo_depth_filter_create."""
    out = []

    def bad(what, **kw):
        p = _params()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        out.append((what, p))

    for what, kw in (("rows 0", dict(rows=0)), ("cols 0", dict(cols=0)), ("rows -1", dict(rows=-1)), ("rows 8193", dict(rows=8193)),
                     ("cols 8193", dict(cols=8193)), ("radius 0", dict(radius=0)), ("radius 5", dict(radius=5)),
                     ("radius -1", dict(radius=-1)), ("ws[0] 17", dict(ws=(0, 17))), ("ws[24] 255", dict(ws=(24, 255))),
                     ("centre 0", dict(ws=(12, 0))), ("wr[0] 0", dict(wr=(0, 0))), ("shift[0] 5", dict(shift=(0, 5))),
                     ("shift[255] 255", dict(shift=(255, 255)))):
        bad(what, **kw)
    return out


def test_bad_arguments_are_refused_before_touching_a_device():
    """Every bound of create on a context handle that is never dereferenced; *out stays as it was. NULLs everywhere."""
    from odometry_amd import _lib
    lib = _lib.load()
    fake_ctx = C.c_void_p(0x1000)
    for what, p in bad_params():
        h = C.c_void_p(0x5A5A)
        assert lib.odo_depth_filter_create(fake_ctx, C.byref(p), C.byref(h)) == -1, what
        assert h.value == 0x5A5A and "odo_depth_filter_create" in _lib.last_error(), what
    h = C.c_void_p(0x5A5A)
    good = _params()
    assert lib.odo_depth_filter_create(None, C.byref(good), C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_depth_filter_create(fake_ctx, None, C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_depth_filter_create(fake_ctx, C.byref(good), None) == -1
    # ws beyond the (2R + 1)^2 entries in use is ignored: not a violation (the refusal of such a table would need a device to show)
    out3, us = (C.c_long * 3)(7, 7, 7), C.c_float(7.0)
    assert lib.odo_depth_filter_run_dev(None, C.c_void_p(8), C.c_void_p(16)) == -1
    assert lib.odo_depth_filter_stats(None, out3) == -1 and list(out3) == [7, 7, 7]
    assert lib.odo_depth_filter_time_dev(None, C.c_void_p(8), C.c_void_p(16), 1, C.byref(us)) == -1 and us.value == 7.0
    assert lib.odo_depth_filter_destroy(None) == 0


# ---- model, loop, rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(dfc.rows())), ids=dfc.row_ids())
def test_model_equals_the_loop_and_the_row_reaches_its_situation(index):
    name, raw, tables_of, R, pred = dfc.rows()[index]
    radii = dfc.RADII if raw.size <= LOOP_PIXELS else (R,)
    for r in radii:
        out, stats = dfc.model_of(index, r)
        lout, lstats, T = dfc.loop_of(index, r)
        assert np.array_equal(out, lout), (name, r, np.argwhere(out != lout)[:4])
        assert stats == lstats, (name, r, stats, lstats)
        ws, wr, shift = tables_of(r)
        assert np.asarray(ws).shape == (2 * r + 1, 2 * r + 1) and max(np.max(ws), 0) <= 16 and ws[r][r] >= 1 and wr[0] >= 1 and max(shift) <= 4
    T = dfc.loop_of(index, R)[2]
    assert pred(T), (name, {k: v for k, v in T.items() if k != "hole_positions"})


def test_rows_cover_the_launch_geometry():
    """Both load paths, one and several workgroups in either direction, every cols % 4, and frames smaller than every radius."""
    k = dfc.constants()
    assert k["kDfBlock"] == 256 and k["kDfTileW"] * k["kDfTileH"] == k["kDfBlock"] * k["kDfPerThread"] and k["kDfPad"] >= k["kDfMaxRadius"] == 4
    g = [dfc.geometry(r[1].shape, k) for r in dfc.rows()]
    assert {x["vec"] for x in g} == {True, False}
    assert {r[1].shape[1] % 4 for r in dfc.rows()} == {0, 1, 2, 3}
    assert any(x["blocks_x"] > 1 and x["blocks_y"] > 1 for x in g) and any(x["blocks_x"] == 1 == x["blocks_y"] for x in g)
    shapes = {r[1].shape for r in dfc.rows()}
    for dr, dc in ((0, -1), (0, 0), (0, 1), (-1, 0), (1, 0)):
        assert (k["kDfTileH"] + dr, k["kDfTileW"] + dc) in shapes
    assert {r[3] for r in dfc.rows()} == set(dfc.RADII)


# ---- the four properties ------------------------------------------------------------------------------------------------------------------
def test_properties_on_random_frames_and_tables():
    """out == 0 exactly where raw == 0; out between the smallest and the largest counted tap; a tap further than 256 << s away
    contributes nothing (replacing it by a hole changes no output); ws with only its centre gives out == raw."""
    rng = np.random.default_rng(0x9707)
    moved = lonely_seen = 0
    for i in range(200):
        R = int(rng.integers(1, 5))
        size = (int(rng.integers(1, 24)), int(rng.integers(1, 24)))
        raw = dfc.surface_frame(i, size, holes=0.2, base=int(rng.integers(300, 60000))) if i % 2 else dfc.random_frame(1000 + i, size, 0.2)
        ws, wr, shift = dfc.random_tables(i, R)
        out, stats = dfc.filter_model(raw, ws, wr, shift)
        assert np.array_equal(out == 0, raw == 0)
        c = raw.astype(np.int64)
        pad = np.zeros((size[0] + 2 * R, size[1] + 2 * R), np.int64)
        pad[R:R + size[0], R:R + size[1]] = c
        s = shift.astype(np.int64)[c >> 8]
        lo, hi = c.copy(), c.copy()
        far = np.zeros_like(pad, bool)
        for dy in range(2 * R + 1):
            for dx in range(2 * R + 1):
                t = pad[dy:dy + size[0], dx:dx + size[1]]
                counts = (c != 0) & (t != 0) & ((np.abs(t - c) >> s) < 256)
                lo, hi = np.where(counts, np.minimum(lo, t), lo), np.where(counts, np.maximum(hi, t), hi)
        assert ((out >= lo) & (out <= hi))[raw != 0].all() and (out[raw != 0] >= 1).all()
        # a pixel that no window counts (further than 256 << s from every centre that sees it) may as well be a hole
        seen = np.zeros(size, bool)
        for dy in range(2 * R + 1):
            for dx in range(2 * R + 1):
                t = pad[dy:dy + size[0], dx:dx + size[1]]
                counts = (c != 0) & (t != 0) & ((np.abs(t - c) >> s) < 256) & ~((dy == R) & (dx == R))
                ys, xs = np.nonzero(counts)
                seen[ys + dy - R, xs + dx - R] = True
        lonely = ~seen & (raw != 0)
        if lonely.any():
            holed = raw.copy()
            holed[lonely] = 0
            out2, _ = dfc.filter_model(holed, ws, wr, shift)
            assert np.array_equal(out2[~lonely], out[~lonely])
            lonely_seen += int(lonely.sum())
        ident, istats = dfc.filter_model(raw, *dfc.identity_tables(R)[:1], wr, shift)
        assert np.array_equal(ident, raw) and istats["n_changed"] == 0 == istats["sum_abs_change"]
        moved += stats["n_changed"]
    assert moved > 1000 and lonely_seen > 1000


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------------
def test_shared_header_under_sanitizers(tmp_path):
    """depth_filter_math.h as a g++ program of its own (ASan + UBSan, every block of exactly its size): df_pixel equals the loop
    byte for byte on every row, df_check_tables passes every row's tables and names the bound of every bad one."""
    exe = str(tmp_path / "depth_filter_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", HARNESS, "-o", exe])
    records, want = [], []
    for index, (name, raw, tables_of, R, _) in enumerate(dfc.rows()):
        for r in (dfc.RADII if raw.size <= LOOP_PIXELS else (R,)):
            records.append((raw, r, tables_of(r)))
            want.append((0, dfc.loop_of(index, r)[0]))
    for what, p in bad_params():
        if "rows" in what or "cols" in what:
            continue
        n = abs(2 * p.radius + 1)                                   # (what the harness reads for this radius)
        ws = np.zeros(n * n, np.uint8)
        ws[:min(n * n, 81)] = p.ws[:min(n * n, 81)]
        bound = {"radius": 1, "ws[": 2, "centre": 3, "wr[0]": 4, "shift": 5}[[k for k in ("radius", "ws[", "centre", "wr[0]", "shift") if k in what][0]]
        records.append((np.zeros((2, 2), np.uint16), p.radius, (ws, np.array(p.wr[:], np.uint8), np.array(p.shift[:], np.uint8))))
        want.append((bound, np.zeros((2, 2), np.uint16)))
    with open(tmp_path / "in.bin", "wb") as f:
        for raw, r, (ws, wr, shift) in records:
            f.write(np.array([raw.shape[0], raw.shape[1], r], np.int32).tobytes())
            for t in (ws, wr, shift):
                f.write(np.ascontiguousarray(t, np.uint8).tobytes())
            f.write(np.ascontiguousarray(raw, np.uint16).tobytes())
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert done.stdout.strip() == f"{len(records)} records"
    blob = open(tmp_path / "out.bin", "rb").read()
    at = 0
    for (raw, r, _), (check, out) in zip(records, want):
        got_check = int(np.frombuffer(blob, np.int32, 1, at)[0])
        got = np.frombuffer(blob, np.uint16, raw.size, at + 4).reshape(raw.shape)
        at += 4 + 2 * raw.size
        assert got_check == check, (raw.shape, r, got_check, check)
        assert got.tobytes() == np.ascontiguousarray(out).tobytes(), (raw.shape, r)
    assert at == len(blob)


# ---- tables ------------------------------------------------------------------------------------------------------------------------------
def test_default_tables():
    from odometry_amd import api
    ws, wr, shift = api.depth_filter_tables()
    assert ws.tolist() == [[3, 5, 7, 5, 3], [5, 10, 13, 10, 5], [7, 13, 16, 13, 7], [5, 10, 13, 10, 5], [3, 5, 7, 5, 3]]
    assert ws.dtype == wr.dtype == shift.dtype == np.uint8 and wr.shape == shift.shape == (256,)
    assert wr[0] == 255 and wr[8] == round(255 * np.exp(-0.5)) and (np.diff(wr.astype(int)) <= 0).all() and wr[255] == 0
    assert shift[0] == 0 and shift.max() == 4 and (np.diff(shift.astype(int)) >= 0).all()       # the noise grows with z beyond z0
    # the rule, restated per entry: sigma0 << shift[j] within a factor sqrt(2) of gain * sigma(z_j) in raw units where it is not clipped
    a, b, z0 = api.KINECT_AXIAL_NOISE
    for j in range(256):
        target = 3.0 * (a + b * ((256 * j + 128) / 1000.0 - z0) ** 2) * 1000.0
        if 0 < shift[j] < 4:
            assert 2 ** -0.5 <= (8.0 * 2 ** int(shift[j])) / target <= 2 ** 0.5, j
    for R in dfc.RADII:
        w = api.depth_filter_tables(radius=R)[0]
        assert w.shape == (2 * R + 1, 2 * R + 1) and w[R, R] == 16 and np.array_equal(w, w.T) and np.array_equal(w, w[::-1])


# ---- mutants -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant,row", [("le256", "step of 255 << 2 and 256 << 2"), ("toward_zero", "ties at W / 2 in both signs"),
                                        ("holes_count", "a hole at every tap, R = 2")])
def test_each_mutant_is_caught_by_its_row(mutant, row):
    index = dfc.row_ids().index(row)
    _, raw, tables_of, R, _ = dfc.rows()[index]
    want = dfc.model_of(index, R)[0]
    got = dfc.filter_loop(raw, *tables_of(R), **{mutant: True})[0]
    assert not np.array_equal(got, want), row
    if mutant == "holes_count":   # (and not by a row without holes)
        i = dfc.row_ids().index("all 65535")
        assert np.array_equal(dfc.filter_loop(dfc.rows()[i][1], *dfc.rows()[i][2](2), holes_count=True)[0], dfc.model_of(i, 2)[0])


# ---- synth -------------------------------------------------------------------------------------------------------------------------------
def _digest(seq, keys):
    h = hashlib.sha256()
    for k in keys:
        for a in seq[k]:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_sequences_without_noise_are_byte_identical_and_noise_is_seeded():
    """depth_noise=None is the code path of before: the frames equal sensor_depth of the rendering, byte for byte, and do not depend
    on the keyword being passed. With a seed the depth frames change, the grey frames and the ground truth do not."""
    from odometry_amd import synth
    kw = dict(rows=30, cols=40, f=synth.TUM_F / 16, cx=synth.TUM_CX / 16, cy=synth.TUM_CY / 16)
    plain, none = synth.make_rgbd_sequence(3, **kw), synth.make_rgbd_sequence(3, depth_noise=None, **kw)
    assert _digest(plain, ("gray", "depth")) == _digest(none, ("gray", "depth"))
    scene = synth.drive_scene("natural", 0)
    for T, d, g in zip(plain["poses"], plain["depth"], plain["gray"]):
        img, Z = scene.render(T, 30, 40, kw["f"], kw["cx"], kw["cy"], 0.0)
        assert d.tobytes() == synth.sensor_depth(Z, 1000.0, 30.0).tobytes() and g.tobytes() == img.tobytes()
    noisy, again = synth.make_rgbd_sequence(3, depth_noise=7, **kw), synth.make_rgbd_sequence(3, depth_noise=7, **kw)
    assert _digest(noisy, ("depth",)) == _digest(again, ("depth",)) != _digest(plain, ("depth",))
    assert _digest(noisy, ("gray",)) == _digest(plain, ("gray",))
    assert _digest(synth.make_rgbd_sequence(3, depth_noise=8, **kw), ("depth",)) != _digest(noisy, ("depth",))
    raw_plain = synth.make_raw_rgbd_sequence(2, **kw)
    raw_none = synth.make_raw_rgbd_sequence(2, depth_noise=None, **kw)
    keys = ("colour", "raw_depth", "gray", "depth_gt")
    assert _digest(raw_plain, keys) == _digest(raw_none, keys)
    assert raw_plain["raw_depth"][1].tobytes() == plain["depth"][1].tobytes()
    raw_noisy = synth.make_raw_rgbd_sequence(2, depth_noise=7, **kw)
    assert _digest(raw_noisy, ("colour", "gray", "depth_gt")) == _digest(raw_plain, ("colour", "gray", "depth_gt"))
    assert raw_noisy["raw_depth"][1].tobytes() == noisy["depth"][1].tobytes()


def test_sensor_noise_follows_its_model():
    from odometry_amd import synth
    rng = np.random.default_rng(3)
    for z in (0.4, 1.0, 3.0, 5.0):
        Z = np.full((200, 200), z)
        d = synth.sensor_noise(Z, rng) - Z
        sigma = 0.0012 + 0.0019 * (z - 0.4) ** 2
        assert abs(d.std() / sigma - 1.0) < 0.02 and abs(d.mean()) < 0.02 * sigma       # 40 000 samples: 3 sigma of the estimate is 1.1 %
    Z = np.array([[np.inf, 31.0, 0.5, 600.0]])
    out = synth.sensor_noise(Z, rng)
    assert out[0, 0] == np.inf and out[0, 1] == 31.0 and out[0, 3] == 600.0 and out[0, 2] != 0.5
    assert (synth.sensor_noise(np.full((50, 50), 1e-4), rng, noise=(1.0, 0.0, 0.0)) >= 0.0).all()
    half = synth.sensor_noise(np.full((300, 300), 2.0), rng, noise=(0.01, 0.0, 0.0)) - 2.0
    assert abs(half.std() / 0.01 - 1.0) < 0.02


# ---- what the filter is for ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sorted(MEASURED))
def test_filter_lowers_the_noise_of_the_ribbed_corridor(size):
    """Frame 1 of DESIGN.md section 9.8's ribbed corridor under the Kinect axial model (noise seed 7), default tables (R = 2,
    sigma0 = 8, gain = 3): the RMS error against the clean frame over Z <= 5 m is lower after the filter than before, by a ratio
    below the midpoint between the measured ratio and 1; the filter moves the clean frame by at most twice the measured RMS."""
    from odometry_amd import api
    tables = api.depth_filter_tables(radius=2, sigma0=8.0, gain=3.0)
    Z, clean = dfc.ribbed_frame(1, size)
    _, noisy = dfc.ribbed_frame(1, size, dfc.NOISE_SEED)
    filtered, stats = dfc.filter_model(noisy, *tables)
    clean_filtered, _ = dfc.filter_model(clean, *tables)
    before, after = dfc.rms_against_clean(noisy, clean, Z), dfc.rms_against_clean(filtered, clean, Z)
    moved = dfc.rms_against_clean(clean_filtered, clean, Z)
    m = MEASURED[size]
    print(f"{size}: RMS against the clean frame {before:.2f} -> {after:.2f} raw units (ratio {after / before:.3f}), the clean frame moved by "
          f"{moved:.2f}; {stats}")
    assert after < before
    assert after / before < 0.5 * (m["after"] / m["before"] + 1.0)
    assert moved <= 2.0 * m["clean"]
    assert abs(before - m["before"]) < 0.05 * m["before"] and abs(after - m["after"]) < 0.05 * m["after"]      # MEASURED is this model's


# ---- code object ---------------------------------------------------------------------------------------------------------------------------
def test_filter_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        m = re.search(r"depth_filter_kernelILi(\d)ELb([01])E", name)
        if m:
            found[(int(m.group(1)), int(m.group(2)))] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in (
                "vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"))
    print(found)
    assert sorted(found) == [(r, v) for r in dfc.RADII for v in (0, 1)]
    k = dfc.constants()
    stride = k["kDfTileW"] + 2 * k["kDfPad"]
    for (r, _), (vgprs, _, lds, vspill, sspill, scratch) in found.items():
        assert (vspill, sspill, scratch) == (0, 0, 0)
        assert vgprs <= 128                                                   # four waves per SIMD at the least
        tile = 2 * (k["kDfTileH"] + 2 * r) * stride                           # the staged tile, then the two tables and the reduction
        rest = 4 * k["kDfRangeWords"] + 256 + 12 * (k["kDfBlock"] // 64)
        assert tile + rest <= lds <= tile + rest + 32
