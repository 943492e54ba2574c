"""The speckle filter (odo_speckle_*, api.SpeckleFilter, api.StereoDepth.enable_speckle) without a GPU: the numpy model of the
specification (include/odometry_hip.h) pinned to the prose by a breadth-first flood fill on every row of
tests/speckle_cases.py small enough for it, every row held to the situation it is in the table for, four switches of the model each
caught by exactly its rows, the host + device header odometry_amd/csrc/speckle_math.h as a stand-alone g++ program under sanitizers,
the parameter refusals, the ABI, the kernels' code-object metadata, and what makes the method worth having: what it removes from the
matcher model's own output on the rendered scenes and on an untextured wall.

The model is the yardstick of tests/test_gpu_speckle.py, which asks the GPU for the same bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import speckle_cases as sc
import stereo_depth_cases as sdc

ROOT = sc.ROOT
HARNESS = os.path.join(ROOT, "tests", "speckle_math_harness.cpp")
NEW_SYMBOLS = ["odo_speckle_create", "odo_speckle_run_dev", "odo_speckle_stats", "odo_speckle_time_dev", "odo_speckle_destroy",
               "odo_stereo_depth_enable_speckle", "odo_stereo_depth_speckle_stats"]

# Measured with the two models, the matcher at A = 2, uniqueness 10, lr_max 1 (the tests below print them).
# wrong = matched pixels more than a pixel (rendered scenes) or a pixel's 16 sixteenths (wall) off the true disparity.
MEASURED = {"corridor": dict(matched=98830, wrong_before=197, wrong_after=4, good_removed=30),
            "natural": dict(matched=93585, wrong_before=228, wrong_after=47, good_removed=290),
            "wall": dict(matched=21626, wrong_before=335, wrong_after=3, good_removed=9, patch_matched=1902, patch_wrong=252)}


def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", header) and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert C.sizeof(_lib.SpeckleParams) == 4 * 4
    assert api.SpeckleFilter.STATS == sc.STATS and hasattr(api.StereoDepth, "enable_speckle") and hasattr(api.StereoDepth, "speckle_stats")
    import inspect
    assert list(inspect.signature(api.StereoDepth.__init__).parameters) == ["self", "ctx_or_tracker", "size", "fx", "baseline", "depth_scale",
                                                                           "min_disp", "max_disp", "agg_radius", "uniqueness", "lr_max",
                                                                           "max_depth"]


def c_params(rows=40, cols=60, max_diff=8, min_size=200):
    from odometry_amd import _lib
    p = _lib.SpeckleParams()
    p.rows, p.cols, p.max_diff, p.min_size = rows, cols, max_diff, min_size
    return p


def bad_params():
    """(what, params, number of the bound in sp_check_params, a word of the message) for every bound of odo_speckle_create."""
    return [(what, c_params(**kw), bound, word) for what, kw, bound, word in (
        ("rows 0", dict(rows=0), 1, "size"), ("cols 0", dict(cols=0), 1, "size"), ("rows -1", dict(rows=-1), 1, "size"),
        ("rows 8193", dict(rows=8193), 1, "size"), ("cols 8193", dict(cols=8193), 1, "size"), ("max_diff -1", dict(max_diff=-1), 2, "max_diff"),
        ("max_diff 65536", dict(max_diff=65536), 2, "max_diff"), ("min_size 0", dict(min_size=0), 3, "min_size"),
        ("min_size -5", dict(min_size=-5), 3, "min_size"), ("min_size 2^30 + 1", dict(min_size=(1 << 30) + 1), 3, "min_size"))]


def test_bad_arguments_are_refused_before_touching_a_device():
    """Every bound of create on a context handle that is never dereferenced; *out stays as it was and the message names the bound.
    NULLs everywhere."""
    from odometry_amd import _lib
    lib = _lib.load()
    fake_ctx = C.c_void_p(0x1000)
    for what, p, _, word in bad_params():
        h = C.c_void_p(0x5A5A)
        assert lib.odo_speckle_create(fake_ctx, C.byref(p), C.byref(h)) == -1, what
        assert h.value == 0x5A5A and "odo_speckle_create" in _lib.last_error() and word in _lib.last_error(), (what, _lib.last_error())
    h = C.c_void_p(0x5A5A)
    good = c_params()
    assert lib.odo_speckle_create(None, C.byref(good), C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_speckle_create(fake_ctx, None, C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_speckle_create(fake_ctx, C.byref(good), None) == -1
    out8, us = (C.c_long * 8)(*[7] * 8), (C.c_float * 5)(*[7.0] * 5)
    assert lib.odo_speckle_run_dev(None, C.c_void_p(8), C.c_void_p(16), C.c_void_p(32)) == -1
    assert lib.odo_speckle_stats(None, out8) == -1 and list(out8) == [7] * 8
    assert lib.odo_speckle_time_dev(None, C.c_void_p(8), C.c_void_p(16), None, 1, us) == -1 and list(us) == [7.0] * 5
    assert lib.odo_speckle_destroy(None) == 0
    assert lib.odo_stereo_depth_enable_speckle(None, 8, 200) == -1 and "odo_stereo_depth_enable_speckle" in _lib.last_error()
    assert lib.odo_stereo_depth_speckle_stats(None, out8) == -1 and list(out8) == [7] * 8


# ---- model, flood fill, rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(sc.rows())), ids=sc.row_ids())
def test_model_equals_the_flood_fill_and_the_row_reaches_its_situation(index):
    name, K, max_diff, min_size, pred = sc.rows()[index]
    M = sc.model_of(index)
    s = M["stats"]
    assert pred(M, K), (name, s)
    idx = np.arange(K.size).reshape(K.shape)
    assert np.array_equal(M["root"] >= 0, K != 0) and (M["root"] <= idx).all() and s["pixels"] == int(M["keep"].sum()) + s["removed_pixels"]
    assert s["removed_components"] <= s["components"] <= s["pixels"] and s["guard"] == 0
    assert int(M["size"][M["root"] == idx].sum()) == s["pixels"]
    if K.size <= sc.FLOOD_PIXELS:
        keep, stats, root, size = sc.speckle_flood(K, max_diff, min_size)
        assert np.array_equal(np.array(keep, bool).reshape(K.shape), M["keep"]) and stats == s, (name, stats, s)
        assert np.array_equal(np.array(root).reshape(K.shape), M["root"]) and np.array_equal(np.array(size).reshape(K.shape), M["size"]), name


def test_every_row_goes_through_the_flood_fill_and_stays_small():
    assert all(r[1].size <= sc.FLOOD_PIXELS for r in sc.rows()) and max(r[1].size for r in sc.rows()) <= 70 * 140


def test_rows_cover_the_launch_geometry():
    """One and several workgroups either way, frames with and without a seam, sizes either side of the tile, every cols % 4."""
    k = sc.constants()
    W, H = k["kSpTileW"], k["kSpTileH"]
    assert k["kSpBlock"] * k["kSpPerThread"] == W * H == k["kSpTile"] and k["kSpStages"] == 4 and k["kSpStatWords"] == 8
    shapes = {r[1].shape for r in sc.rows()}
    g = [sc.geometry(s, k) for s in shapes]
    assert {s[1] % 4 for s in shapes} == {0, 1, 2, 3}
    assert any(x["seam_pairs"] == 0 for x in g) and any(x["blocks_x"] == 3 and x["blocks_y"] == 3 for x in g)
    assert any(x["blocks_x"] > 1 and x["blocks_y"] == 1 for x in g) and any(x["blocks_x"] == 1 and x["blocks_y"] > 1 for x in g)
    for dr, dc in ((-1, -1), (0, 0), (1, 1)):
        assert (H + dr, W + dc) in shapes
    assert {(1, 1), (1, W + 3), (2 * H + 3, 1)} <= shapes
    assert {r[3] for r in sc.rows()} >= {1, 2, 1 << 30} and {r[2] for r in sc.rows()} >= {0, 65533, 65534, 65535}


@pytest.mark.parametrize("switch", sc.SWITCHES)
def test_each_switch_is_caught_by_exactly_its_rows(switch):
    placed = sc.CAUGHT_BY[switch]
    caught = [name for index, name in enumerate(sc.row_ids()) if sc.differs(index, switch)]
    want = [n for i, n in enumerate(sc.row_ids()) if placed(i)] if callable(placed) else [n for n in sc.row_ids() if n in placed]
    assert caught == want and len(caught) >= 2, (switch, set(caught) ^ set(want))
    if not callable(placed):
        assert len(want) == len(placed)


def test_the_rows_placed_for_a_switch_are_among_those_that_catch_it():
    caught = {sw: {n for i, n in enumerate(sc.row_ids()) if sc.differs(i, sw)} for sw in sc.SWITCHES}
    assert "diagonal-only contacts do not connect" in caught["eight"] and "checkerboard: every pixel its own component" in caught["eight"]
    assert {"ramp with steps of exactly max_diff", "keys 1 and 65535 with max_diff 65534",
            "two components that touch across a seam, both ways"} <= caught["strict"]
    assert "keys 1 and 65535 with max_diff 65533" not in caught["strict"]
    assert "components of min_size - 1, min_size and min_size + 1" in caught["gt"]
    assert "all zero" in caught["zeros_connect"] and "one component fills the frame" not in caught["zeros_connect"]


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------------
def test_shared_header_under_sanitizers(tmp_path):
    """speckle_math.h as a g++ program of its own (ASan + UBSan, every plane a heap block of exactly the frame): the reference
    labelling equals the model byte for byte on every row — both targets, the root and size planes, the counters — and
    sp_check_params names the bound of every bad parameter set and passes the outermost good ones."""
    exe = str(tmp_path / "speckle_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", HARNESS, "-o", exe])
    head = lambda rows, cols, max_diff, min_size: np.array([rows, cols, max_diff, min_size], np.int32).tobytes()
    with open(tmp_path / "in.bin", "wb") as f:
        for _, K, max_diff, min_size, _ in sc.rows():
            f.write(head(K.shape[0], K.shape[1], max_diff, min_size) + K.tobytes())
        for _, c, _, _ in bad_params():
            f.write(head(c.rows, c.cols, c.max_diff, c.min_size))
        f.write(head(1, 1, 0, 1) + np.array([9], np.uint16).tobytes())
        f.write(head(1, 2, 65535, 1 << 30) + np.array([1, 65535], np.uint16).tobytes())
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert done.stdout.strip() == f"{len(sc.rows()) + len(bad_params()) + 2} records"
    blob = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def record(K, M):
        nonlocal at
        n = K.size
        assert int(np.frombuffer(blob, np.int32, 1, at)[0]) == 0
        a = np.frombuffer(blob, np.uint16, n, at + 4).reshape(K.shape)
        b = np.frombuffer(blob, np.uint16, n, at + 4 + 2 * n).reshape(K.shape)
        parent = np.frombuffer(blob, np.int32, n, at + 4 + 4 * n).reshape(K.shape)
        size = np.frombuffer(blob, np.int32, n, at + 4 + 8 * n).reshape(K.shape)
        counts = np.frombuffer(blob, np.int64, 8, at + 4 + 12 * n)
        at += 4 + 12 * n + 64
        idx = np.arange(n).reshape(K.shape)
        assert np.array_equal(a, sc.apply_keep(K, M)) and np.array_equal(b, sc.apply_keep(np.full(K.shape, 0xABAB), M))
        assert np.array_equal(parent, M["root"]) and np.array_equal(size, np.where(M["root"] == idx, M["size"], 0))
        assert dict(zip(sc.STATS, counts[:6].tolist())) == M["stats"] and not counts[6:].any()

    for index, (name, K, _, _, _) in enumerate(sc.rows()):
        record(K, sc.model_of(index))
    for what, _, bound, _ in bad_params():
        assert int(np.frombuffer(blob, np.int32, 1, at)[0]) == bound, what
        at += 4
    record(np.array([[9]], np.uint16), sc.speckle_model([[9]], 0, 1))
    record(np.array([[1, 65535]], np.uint16), sc.speckle_model([[1, 65535]], 65535, 1 << 30))
    assert at == len(blob)


# ---- what the method gives -----------------------------------------------------------------------------------------------------------------
def _method(q, true_q, tol, max_diff, min_size):
    """(matched, wrong before, wrong after, good removed): wrong = a matched pixel more than tol sixteenths off true_q."""
    matched = q > 0
    wrong = matched & (np.abs(q.astype(np.float64) - true_q) > tol)
    keep = sc.speckle_model(q, max_diff, min_size)["keep"]
    return int(matched.sum()), int(wrong.sum()), int((wrong & keep).sum()), int((matched & ~wrong & ~keep).sum())


@pytest.mark.parametrize("drive", ["corridor", "natural"])
def test_what_the_filter_removes_on_the_rendered_scenes(drive):
    """The matcher model's q frame of the drive's frame 0 at 188 x 620 (candidates 1 .. 63, A = 2, uniqueness 10, lr_max 1) through
    the filter at max_diff 8, min_size 200, against the renderer's disparity f b / Z: of the matched pixels more than a pixel off at
    most half are left, and the correct pixels removed are at most 0.5 % of the matched."""
    left, right, Z, fx, baseline = sdc.rendered_pair(drive)
    if drive == "natural":
        q = sdc.model_of(sdc.row_ids().index("rendered pair natural 188 x 620, A = 2"))[1]
    else:
        q = sdc.stereo_model(left, right, sdc.rendered_params(2))[1]
    matched, before, after, good_removed = _method(q, 16.0 * fx * baseline / Z, 16.0, 8, 200)
    print(f"{drive}: matched {matched}, wrong before {before}, after {after}, good pixels removed {good_removed}")
    assert dict(matched=matched, wrong_before=before, wrong_after=after, good_removed=good_removed) == MEASURED[drive]
    assert 2 * after <= before and good_removed <= 0.005 * matched


def test_what_the_filter_removes_on_an_untextured_wall():
    """A textured scene at disparity 12 with an untextured patch, a grey level of noise on either image, the matcher at candidates
    1 .. 40, the filter at max_diff 16 and min_size 100: of the matched pixels more than a pixel off q = 192 at most 10 % are left,
    and the correct pixels removed are at most 1 % of the matched. Most of the wrong matches lie in the patch's 40 x 120 pixels."""
    q = sc.wall_match()[1]
    matched, before, after, good_removed = _method(q, 192.0, 16.0, 16, 100)
    patch = q[28:68, 120:240]
    patch_matched, patch_wrong = int((patch > 0).sum()), int(((patch > 0) & (np.abs(patch.astype(int) - 192) > 16)).sum())
    print(f"wall: matched {matched}, wrong before {before}, after {after}, good pixels removed {good_removed}; in the patch "
          f"{patch_matched} matched, {patch_wrong} wrong")
    assert dict(matched=matched, wrong_before=before, wrong_after=after, good_removed=good_removed, patch_matched=patch_matched,
                patch_wrong=patch_wrong) == MEASURED["wall"]
    assert 10 * after <= before and good_removed <= 0.01 * matched and 2 * patch_wrong > before


# ---- code object ---------------------------------------------------------------------------------------------------------------------------
def test_speckle_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        m = re.search(r"speckle_(label|seam|count|apply)_kernel", name)
        if m:
            found[m.group(1)] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in (
                "vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"))
    print(found)
    assert sorted(found) == ["apply", "count", "label", "seam"]
    k = sc.constants()
    for key, (vgprs, _, lds, vspill, sspill, scratch) in found.items():
        assert (vspill, sspill, scratch) == (0, 0, 0), key
        assert vgprs <= 64, key                                              # eight waves per SIMD
    assert found["label"][2] == k["kSpTile"] * (4 + 4 + 2) and found["seam"][2] == 0 and found["count"][2] == 0 and found["apply"][2] <= 128
