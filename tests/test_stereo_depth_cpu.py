"""The dense stereo matcher (odo_stereo_depth_*, api.StereoDepth) without a GPU: the numpy model of the specification
(include/odometry_hip.h) pinned to the prose by a plain loop on every row of tests/stereo_depth_cases.py small
enough for it, every row held to the situation it is in the table for, four switches of the model each caught by exactly its rows,
the host + device header odometry_amd/csrc/stereo_depth_math.h as a stand-alone g++ program under sanitizers, the parameter refusals,
the ABI, the kernels' code-object metadata, and what makes the method usable: the model's accuracy against the renderer's ground
truth and on the known-answer pair.

The model is the yardstick of tests/test_gpu_stereo_depth.py, which asks the GPU for the same bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import stereo_depth_cases as sdc

ROOT = sdc.ROOT
HARNESS = os.path.join(ROOT, "tests", "stereo_depth_math_harness.cpp")
NEW_SYMBOLS = ["odo_stereo_depth_create", "odo_stereo_depth_run_dev", "odo_stereo_depth_disparity_dev", "odo_stereo_depth_depth_dev",
               "odo_stereo_depth_stats", "odo_stereo_depth_time_dev", "odo_stereo_depth_destroy"]

# Measured with this model, A = 2, uniqueness 10, lr_max 1, candidates 1 .. 63 (the tests below print them). `passed` = matched +
# rejected by range: the pixels that pass uniqueness and the left-right check (on `natural` 970 of them lie beyond 65.535 m).
MEASURED = {"natural": dict(interior=108046, passed=94555, matched=93585), "corridor": dict(interior=108046, passed=99554, matched=98830),
            "integer": dict(interior=26402, matched=23215, core=15743, within8=15694)}


def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", header) and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert C.sizeof(_lib.StereoDepthParams) == 8 * 4 + 3 * 8
    assert hasattr(api, "StereoDepth") and api.StereoDepth.STATS == sdc.STATS


def c_params(rows=40, cols=60, **kw):
    from odometry_amd import _lib
    p = sdc.params(**kw)
    c = _lib.StereoDepthParams()
    c.rows, c.cols, c.dmin, c.dmax, c.agg_radius, c.uniqueness, c.lr_max, c.max_raw = (rows, cols, p["dmin"], p["dmax"], p["A"], p["uniq"],
                                                                                      p["lr_max"], p["max_raw"])
    c.fx, c.baseline, c.depth_scale = p["fx"], p["baseline"], p["depth_scale"]
    return c


def bad_params():
    """(what, params, number of the bound in sd_check_params) for every bound of odo_stereo_depth_create."""
    out = []
    for what, kw, bound in (("rows 0", dict(rows=0), 1), ("cols 0", dict(cols=0), 1), ("rows -1", dict(rows=-1), 1),
                            ("rows 8193", dict(rows=8193), 1), ("cols 8193", dict(cols=8193), 1), ("dmin 0", dict(dmin=0), 2),
                            ("dmin -3", dict(dmin=-3), 2), ("dmax 256", dict(dmax=256), 3), ("dmax dmin + 1", dict(dmin=7, dmax=8), 3),
                            ("dmax below dmin", dict(dmin=7, dmax=3), 3), ("agg_radius -1", dict(agg_radius=-1), 4),
                            ("agg_radius 4", dict(agg_radius=4), 4), ("uniqueness -1", dict(uniqueness=-1), 5),
                            ("uniqueness 100", dict(uniqueness=100), 5), ("lr_max -2", dict(lr_max=-2), 6), ("max_raw 0", dict(max_raw=0), 7),
                            ("max_raw 65536", dict(max_raw=65536), 7), ("fx 0", dict(fx=0.0), 8), ("baseline -1", dict(baseline=-1.0), 8),
                            ("depth_scale NaN", dict(depth_scale=float("nan")), 8), ("fx inf", dict(fx=float("inf")), 8),
                            ("k beyond fp32", dict(fx=1e30, depth_scale=1e30), 8)):
        p = c_params()
        for k, v in kw.items():
            setattr(p, k, v)
        out.append((what, p, bound))
    return out


def test_bad_arguments_are_refused_before_touching_a_device():
    """Every bound of create on a context handle that is never dereferenced; *out stays as it was. NULLs everywhere."""
    from odometry_amd import _lib
    lib = _lib.load()
    fake_ctx = C.c_void_p(0x1000)
    for what, p, _ in bad_params():
        h = C.c_void_p(0x5A5A)
        assert lib.odo_stereo_depth_create(fake_ctx, C.byref(p), C.byref(h)) == -1, what
        assert h.value == 0x5A5A and "odo_stereo_depth_create" in _lib.last_error(), what
    h = C.c_void_p(0x5A5A)
    good = c_params()
    assert lib.odo_stereo_depth_create(None, C.byref(good), C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_stereo_depth_create(fake_ctx, None, C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_stereo_depth_create(fake_ctx, C.byref(good), None) == -1
    out8, us, ptr = (C.c_long * 8)(*[7] * 8), (C.c_float * 3)(7.0, 7.0, 7.0), C.c_void_p(0x77)
    assert lib.odo_stereo_depth_run_dev(None, C.c_void_p(8), C.c_void_p(16), C.c_void_p(32)) == -1
    assert lib.odo_stereo_depth_stats(None, out8) == -1 and list(out8) == [7] * 8
    assert lib.odo_stereo_depth_time_dev(None, C.c_void_p(8), C.c_void_p(16), C.c_void_p(32), 1, us) == -1 and list(us) == [7.0] * 3
    assert lib.odo_stereo_depth_disparity_dev(None, C.byref(ptr)) == -1 and lib.odo_stereo_depth_depth_dev(None, C.byref(ptr)) == -1
    assert ptr.value == 0x77 and lib.odo_stereo_depth_destroy(None) == 0


# ---- model, loop, rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(sdc.rows())), ids=sdc.row_ids())
def test_model_equals_the_loop_and_the_row_reaches_its_situation(index):
    name, L, R, p, pred = sdc.rows()[index]
    depth, q, stats, T = sdc.model_of(index)
    assert pred(stats, T), (name, stats)
    assert stats["interior"] == stats["matched"] + stats["rej_unique"] + stats["rej_lr"] + stats["rej_range"]
    assert np.array_equal(q != 0, T["outcome"] == 1) and (depth[q == 0] == 0).all()
    assert T["f"].min() >= -8 and T["f"].max() <= 8 and (T["den"][(T["cm"] < sdc.BIG) & (T["cp"] < sdc.BIG) & (T["outcome"] > 0)] >= 1).all()
    if sdc.loop_work(index) <= sdc.LOOP_WORK:
        ld, lq, ls = sdc.stereo_loop(L, R, p)
        assert np.array_equal(depth, ld) and np.array_equal(q, lq), (name, np.argwhere(q != lq)[:4])
        assert stats == ls, (name, stats, ls)


def test_enough_rows_go_through_the_loop():
    looped = [n for i, n in enumerate(sdc.row_ids()) if sdc.loop_work(i) <= sdc.LOOP_WORK]
    assert len(looped) >= 25 and {sdc.rows()[sdc.row_ids().index(n)][3]["A"] for n in looped} >= {0, 1, 2}


def test_rows_cover_the_launch_geometry():
    """Both store paths, one and several workgroups in either direction, every cols % 4, sizes either side of the tile, every A."""
    k = sdc.constants()
    assert k["kSdBlock"] == 256 == k["kSdTileW"] * k["kSdTileH"] and k["kSdMaxSpan"] == 254 and k["kSdMaxAgg"] == 3
    lds = 8 * (k["kSdTileH"] + 2 * 3) * (2 * (k["kSdTileW"] + 2 * 3) + k["kSdMaxSpan"])
    assert lds < 64 * 1024
    shapes = {r[1].shape for r in sdc.rows()}
    g = [sdc.geometry(s, k) for s in shapes]
    assert {x["vec"] for x in g} == {True, False} and {s[1] % 4 for s in shapes} == {0, 1, 2, 3}
    assert any(x["blocks_x"] > 1 and x["blocks_y"] > 1 for x in g) and any(x["blocks_x"] == 1 for x in g)
    TW, TH = k["kSdTileW"], k["kSdTileH"]
    for dr, dc in ((0, -1), (0, 0), (0, 1), (-1, 0), (1, 0)):
        assert (3 * TH + dr, TW + dc) in shapes
    assert {r[3]["A"] for r in sdc.rows()} == {0, 1, 2, 3} and {r[3]["lr_max"] for r in sdc.rows()} == {-1, 0, 1, 3}


@pytest.mark.parametrize("switch", sdc.SWITCHES)
def test_each_switch_is_caught_by_exactly_its_rows(switch):
    placed = sdc.CAUGHT_BY[switch]
    caught = []
    for index, name in enumerate(sdc.row_ids()):
        depth, q, stats, _ = sdc.model_of(index)
        d2, q2, s2 = sdc.model_of(index, switch)
        if not (np.array_equal(depth, d2) and np.array_equal(q, q2) and stats == s2):
            caught.append(name)
    want = [n for i, n in enumerate(sdc.row_ids()) if placed(i)] if callable(placed) else [n for n in sdc.row_ids() if n in placed]
    assert caught == want and len(caught) >= 2, (switch, set(caught) ^ set(want))
    if not callable(placed):
        assert len(want) == len(placed)


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------------
SUBPIXEL_TRIPLES = [(5, 5, 5), (-1, 3, 9), (9, 3, -1), (4, 3, 4), (10, 3, 4), (4, 3, 10), (3, 3, 3038), (3038, 0, 3038), (3038, 0, 1),
                    (1, 0, 3038), (7, 6, 6), (6, 6, 7), (2, 5, 2), (100, 50, 51), (51, 50, 100)]


def _subpixel(cm, c0, cp):
    if cm < 0 or cp < 0 or cm - 2 * c0 + cp <= 0:
        return 0
    den, num = cm - 2 * c0 + cp, cm - cp
    f = (16 * abs(num) + den) // (2 * den)
    return -f if num < 0 else f


def test_shared_header_under_sanitizers(tmp_path):
    """stereo_depth_math.h as a g++ program of its own (ASan + UBSan, every block of exactly its size): sd_census, the walk and the
    rule's end equal the model byte for byte on every row, sd_check_params names the bound of every bad parameter set, and
    sd_subpixel gives the rule's f on triples that no winner can produce (den <= 0 among them)."""
    exe = str(tmp_path / "stereo_depth_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", HARNESS, "-o", exe])

    def head(rows, cols, p):
        return (np.array([rows, cols, p["dmin"], p["dmax"], p["A"], p["uniq"], p["lr_max"], p["max_raw"]], np.int32).tobytes()
                + np.array([p["fx"], p["baseline"], p["depth_scale"]], np.float64).tobytes())

    with open(tmp_path / "in.bin", "wb") as f:
        for _, L, R, p, _ in sdc.rows():
            f.write(head(L.shape[0], L.shape[1], p) + L.tobytes() + R.tobytes())
        for _, c, _ in bad_params():
            f.write(np.array([c.rows, c.cols, c.dmin, c.dmax, c.agg_radius, c.uniqueness, c.lr_max, c.max_raw], np.int32).tobytes()
                    + np.array([c.fx, c.baseline, c.depth_scale], np.float64).tobytes())
        f.write(head(-7777, len(SUBPIXEL_TRIPLES), sdc.params()) + np.array(SUBPIXEL_TRIPLES, np.int32).tobytes())
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert done.stdout.strip() == f"{len(sdc.rows()) + len(bad_params()) + 1} records"
    blob = open(tmp_path / "out.bin", "rb").read()
    at = 0
    for index, (name, L, _, _, _) in enumerate(sdc.rows()):
        depth, q, stats, _ = sdc.model_of(index)
        assert int(np.frombuffer(blob, np.int32, 1, at)[0]) == 0, name
        got_d = np.frombuffer(blob, np.uint16, L.size, at + 4).reshape(L.shape)
        got_q = np.frombuffer(blob, np.uint16, L.size, at + 4 + 2 * L.size).reshape(L.shape)
        counts = np.frombuffer(blob, np.int64, 6, at + 4 + 4 * L.size)
        at += 4 + 4 * L.size + 48
        assert np.array_equal(got_q, q) and np.array_equal(got_d, depth), (name, np.argwhere(got_q != q)[:4])
        assert dict(zip(sdc.STATS, counts.tolist())) == stats, name
    for what, _, bound in bad_params():
        assert int(np.frombuffer(blob, np.int32, 1, at)[0]) == bound, what
        at += 4
    fs = np.frombuffer(blob, np.int32, len(SUBPIXEL_TRIPLES), at)
    at += 4 * len(SUBPIXEL_TRIPLES)
    assert fs.tolist() == [_subpixel(*t) for t in SUBPIXEL_TRIPLES] and set(fs.tolist()) >= {-8, 0, 8}
    assert at == len(blob)


# ---- what the method is good for -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drive", ["natural", "corridor"])
def test_accuracy_against_the_renderers_ground_truth(drive):
    """Frame 0 of the drive at 188 x 620, candidates 1 .. 63, A = 2, uniqueness 10, lr_max 1, against the true disparity f b / Z.
    Floors with a margin over the measured figures (MEASURED): matched >= 80 % of interior, within one pixel
    >= 99 % of matched."""
    left, right, Z, fx, baseline = sdc.rendered_pair(drive)
    p = sdc.rendered_params(2)
    depth, q, stats = sdc.stereo_model(left, right, p) if drive != "natural" else sdc.model_of(sdc.row_ids().index("rendered pair natural 188 x 620, A = 2"))[:3]
    m = q > 0
    true_d = fx * baseline / Z[m]
    err = np.abs(q[m] / 16.0 - true_d)
    z_err = np.abs(depth[m] / 1000.0 - Z[m]) / Z[m]
    near = Z[m] < 10.0
    print(f"{drive}: {stats}; within 0.5 px {100 * (err <= 0.5).mean():.2f} %, within 1 px {100 * (err <= 1.0).mean():.2f} %; depth error median "
          f"{100 * np.median(z_err):.2f} % of range, 99th percentile below 10 m {100 * np.percentile(z_err[near], 99):.2f} %")
    assert stats["interior"] == MEASURED[drive]["interior"]
    assert stats["matched"] + stats["rej_range"] == MEASURED[drive]["passed"] and stats["matched"] == MEASURED[drive]["matched"]
    assert stats["matched"] >= 0.80 * stats["interior"]
    assert (err <= 1.0).mean() >= 0.99


def test_known_answers_on_the_integer_disparity_pair():
    """Away from the band edges (at least A + 3 rows inside a band) every matched pixel lies within a pixel of its band's disparity
    and 99 % within half a pixel; the rest are exact ties between neighbouring candidates in flat tiles."""
    index = sdc.row_ids().index("integer disparity pair 96 x 320")
    _, q, stats, _ = sdc.model_of(index)
    disp = sdc.integer_pair()[2]
    A = sdc.rows()[index][3]["A"]
    y = np.arange(q.shape[0]) % 24
    core = ((y >= A + 3) & (y < 24 - (A + 3)))[:, None] & (q > 0)
    e = np.abs(q.astype(int) - 16 * disp)[core]
    print(stats, int(core.sum()), int((e <= 8).sum()))
    assert (e <= 16).all() and (e <= 8).mean() >= 0.99
    m = MEASURED["integer"]
    assert (stats["interior"], stats["matched"], int(core.sum()), int((e <= 8).sum())) == (m["interior"], m["matched"], m["core"], m["within8"])


# ---- code object ---------------------------------------------------------------------------------------------------------------------------
def test_stereo_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        m = re.search(r"stereo_match_kernelILi(\d)ELb([01])ELb([01])E", name)
        key = (int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else ("census" if "stereo_census_kernel" in name else None)
        if key is not None:
            found[key] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in (
                "vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"))
    print(found)
    assert sorted(k for k in found if k != "census") == [(a, r, v) for a in range(4) for r, v in ((0, 0), (0, 1), (1, 0))] and "census" in found
    k = sdc.constants()
    for key, (vgprs, _, lds, vspill, sspill, scratch) in found.items():
        assert (vspill, sspill, scratch) == (0, 0, 0), key
        assert vgprs <= 256, key                                             # two waves per SIMD at the least
        if key != "census":
            a = key[0]
            words = (k["kSdTileH"] + 2 * a) * (2 * (k["kSdTileW"] + 2 * a) + k["kSdMaxSpan"])
            assert 8 * words <= lds <= 8 * words + 128 and lds < 64 * 1024, (key, lds)
