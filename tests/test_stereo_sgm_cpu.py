"""The dense stereo matcher's semi-global mode (odo_stereo_depth_enable_sgm, api.StereoDepth.enable_sgm) without a GPU: the numpy
model of the specification (include/odometry_hip.h) pinned to the prose by a plain loop on every row of
tests/stereo_sgm_cases.py small enough for it, every row held to the situation it is in the table for, four switches of the model
each caught by exactly the rows that its unswitched path costs name, the host + device header odometry_amd/csrc/stereo_sgm_math.h as a
stand-alone g++ program under sanitizers, the refusals that the arguments alone decide, the ABI, the kernels' code-object metadata,
and what the method gives: matched and wrong pixels against the renderer's ground truth beside the box matcher's.

The model is the yardstick of tests/test_gpu_stereo_sgm.py, which asks the GPU for the same bits."""
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
import stereo_sgm_cases as sgc

ROOT = sgc.ROOT
HARNESS = os.path.join(ROOT, "tests", "stereo_sgm_math_harness.cpp")
NEW_SYMBOLS = ["odo_stereo_depth_enable_sgm", "odo_stereo_depth_sgm_time_dev", "odo_debug_sgm_volume"]

# Measured with this model at 188 x 620, rendered_params(2) (candidates 1 .. 63, A = 2, uniqueness 10, lr_max 1), P1 100, P2 600;
# "wrong" = more than a pixel off the renderer's f b / Z. box = stereo_depth_cases.stereo_model on the same pair. The integer pair:
# candidates 1 .. 63, A = 2, far = more than 16 sixteenths off the band's disparity. The wall (speckle_cases.wall_pair): wrong = more
# than a pixel off disparity 12, patch = inside the untextured patch, after = behind speckle_model(q, 16, 100).
MEASURED = {
    "natural": dict(box=(93585, 228), sgm8=(100784, 170), sgm4=(100838, 194)),
    "corridor": dict(box=(98830, 197), sgm8=(100777, 191), sgm4=(100736, 201)),
    "integer": dict(box=(23215, 151), sgm8=(23633, 79)),
    "wall": dict(box=dict(wrong=335, patch_wrong=252, after=3), sgm8=dict(wrong=777, patch_wrong=520, after=241)),
}


def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b" + n + r"\s*\(", header) and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert "TEST ONLY" in header[:header.index("int odo_debug_sgm_volume(")].rsplit("/*", 1)[1]
    assert "odo_debug_sgm_volume" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in ("enable_sgm", "disable_sgm", "sgm_time", "sgm_volume"):
        assert hasattr(api.StereoDepth, n), n
    units = open(os.path.join(ROOT, "odometry_amd", "build.py")).read()
    assert "stereo_sgm_kernels.hip" in units


def bad_sgm(live):
    """(what, p1, p2, paths, bound) for every bound of odo_stereo_depth_enable_sgm. live=False: the cases that the arguments alone
    decide, whatever the matcher (A = 0 is the weakest case of the aggregate's bound). live=True: also those that need the matcher's
    A — given for a matcher with agg_radius 2."""
    out = [("P1 0", 0, 10, 8, 1), ("P1 -5", -5, 10, 8, 1), ("P1 above P2", 11, 10, 8, 1), ("P2 0", 1, 0, 4, 1), ("paths 1", 1, 10, 1, 2),
           ("paths 5", 1, 10, 5, 2), ("paths 16", 1, 10, 16, 2), ("paths -4", 1, 10, -4, 2), ("P2 8130 at 8 paths", 10, 8130, 8, 3),
           ("P2 16322 at 4 paths", 10, 16322, 4, 3), ("P2 INT_MAX", 1, 2 ** 31 - 1, 8, 3)]
    if live:
        out += [("P2 one above the bound at A = 2, 8 paths", 10, 65534 // 8 - 62 * 25 + 1, 8, 3),
                ("P2 one above the bound at A = 2, 4 paths", 10, 65534 // 4 - 62 * 25 + 1, 4, 3)]
    return out


def test_bad_arguments_are_refused_before_the_matcher_is_read():
    """Every refusal that the arguments alone decide, on a matcher handle that is never dereferenced; the bounds that need the
    matcher's A and size are reached by the harness below (sgm_check_params) and on a live matcher by the GPU suite."""
    from odometry_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    for what, p1, p2, paths, bound in bad_sgm(False):
        assert sgc.check_params(40, 60, sdc.params(A=0), dict(p1=p1, p2=p2, paths=paths)) == bound, what
        assert lib.odo_stereo_depth_enable_sgm(fake, p1, p2, paths) == -1, what
        msg = _lib.last_error()
        assert "odo_stereo_depth_enable_sgm" in msg and ("P1", "paths", "aggregate")[bound - 1] in msg, (what, msg)
    us, vol = (C.c_float * 5)(*[7.0] * 5), (C.c_uint16 * 4)(9, 9, 9, 9)
    assert lib.odo_stereo_depth_enable_sgm(None, 100, 600, 8) == -1 and lib.odo_stereo_depth_enable_sgm(None, 0, 0, 0) == -1
    assert lib.odo_stereo_depth_sgm_time_dev(None, C.c_void_p(8), C.c_void_p(16), C.c_void_p(32), 1, us) == -1 and list(us) == [7.0] * 5
    assert lib.odo_debug_sgm_volume(None, vol) == -1 and list(vol) == [9] * 4


# ---- model, loop, rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(sgc.rows())), ids=sgc.row_ids())
def test_model_equals_the_loop_and_the_row_reaches_its_situation(index):
    name, L, R, p, sg, pred = sgc.rows()[index]
    depth, q, stats, S, T = sgc.model_of(index)
    assert pred(stats, T, sg), (name, stats)
    assert stats["interior"] == stats["matched"] + stats["rej_unique"] + stats["rej_lr"] + stats["rej_range"] == int(T["adm"].any(axis=2).sum())
    assert np.array_equal(q != 0, T["outcome"] == 1) and (depth[q == 0] == 0).all()
    a = T["adm"]
    assert np.array_equal(S != sgc.NONE, a) and a[..., 0].sum() == stats["interior"]          # contiguous from dmin
    assert np.array_equal(a, np.arange(a.shape[2])[None, None] < T["n_cand"][..., None])
    cmax = int(T["C"][a].max(initial=0))
    assert int(S[a].max(initial=0)) <= sg["paths"] * (cmax + sg["p2"]) <= 65534
    if T["L"] is not None:
        for Lr in T["L"]:
            assert ((Lr[a] >= T["C"][a]) & (Lr[a] <= T["C"][a] + sg["p2"])).all()
    if sgc.loop_work(index) <= sgc.LOOP_WORK:
        ld, lq, ls, lS = sgc.sgm_loop(L, R, p, sg)
        assert np.array_equal(S, lS), (name, np.argwhere(S != lS)[:4])
        assert np.array_equal(depth, ld) and np.array_equal(q, lq), (name, np.argwhere(q != lq)[:4])
        assert stats == ls, (name, stats, ls)


def test_enough_rows_go_through_the_loop():
    looped = [r for i, r in enumerate(sgc.rows()) if sgc.loop_work(i) <= sgc.LOOP_WORK]
    assert len(looped) >= 25 and {r[3]["A"] for r in looped} == {0, 1, 2, 3} and {r[4]["paths"] for r in looped} == {4, 8}
    assert {r[3]["dmax"] - r[3]["dmin"] + 1 for r in looped} >= {3, 64}


def test_rows_cover_the_launch_geometry_and_the_seams():
    """Sizes either side of the tile and of the lines per workgroup at every cols % 4, candidate counts either side of a lane's slot
    and of the selection's chunk, rows > cols and cols > rows, both path counts at every A."""
    k = sgc.constants()
    TW, TH, LPB, CH = k["kSdTileW"], k["kSdTileH"], k["kSgmLinesPerBlock"], k["kSgmChunk"]
    assert k["kSgmBlock"] == 64 * LPB and 64 * k["kSgmSlots"] >= k["kSdMaxDisp"] and k["kSgmChunkStride"] == CH + 1
    assert k["kSgmNone"] == sgc.NONE and k["kSgmMaxSum"] == 65534
    shapes = {r[1].shape for r in sgc.rows()}
    assert {s[1] % 4 for s in shapes} == {0, 1, 2, 3}
    for dr, dc in ((0, -1), (0, 0), (0, 1), (-1, 0), (1, 0)):
        assert (3 * TH + dr, TW + dc) in shapes
    lines, lengths = set(), set()                                             # of a launch; of a line
    for _, L, _, p, sg, _ in sgc.rows():
        x0, x1, y0, y1 = sgc.rect(L.shape[0], L.shape[1], p)
        if x1 > x0 and y1 > y0:
            w, h = x1 - x0, y1 - y0
            lines |= {w, h} | ({w + h - 1} if sg["paths"] == 8 else set())
            lengths |= {w, h} | (set(range(1, min(w, h) + 1)) if sg["paths"] == 8 else set())
    AH = k["kSgmAhead"]
    assert {LPB - 1, LPB, LPB + 1, 1} <= lines and any(n > 16 * LPB for n in lines)
    assert set(range(1, 3 * AH + 2)) <= lengths and any(n > 16 * AH for n in lengths)
    D = {r[3]["dmax"] - r[3]["dmin"] + 1 for r in sgc.rows()}
    assert {3, CH, CH + 1, 2 * CH, 2 * CH + 1, 255} <= D
    assert {(r[3]["A"], r[4]["paths"]) for r in sgc.rows()} == {(a, n) for a in range(4) for n in (4, 8)}


@pytest.mark.parametrize("switch", sgc.SWITCHES)
def test_each_switch_is_caught_by_exactly_its_rows(switch):
    caught, want = [], []
    for index, name in enumerate(sgc.row_ids()):
        depth, q, stats, S, _ = sgc.model_of(index)
        d2, q2, s2, S2 = sgc.model_of(index, switch)
        same_S = np.array_equal(S.astype(np.int64), np.where(S2 >= sgc.INF, sgc.NONE, S2))
        if not (same_S and np.array_equal(depth, d2) and np.array_equal(q, q2) and stats == s2):
            caught.append(name)
        if sgc.caught_by(index, switch):
            want.append(name)
    assert caught == want, (switch, set(caught) ^ set(want))
    assert set(sgc.PLACED[switch]) <= set(caught) and len(caught) < len(sgc.rows()), switch


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------------
def harness_bad():
    """Every bound through sgm_check_params: (what, rows, cols, params, sgm, bound)."""
    out = [(what, 40, 60, sdc.params(A=2), dict(p1=p1, p2=p2, paths=paths), bound) for what, p1, p2, paths, bound in bad_sgm(True)]
    out.append(("paths 0", 40, 60, sdc.params(), dict(p1=1, p2=2, paths=0), 2))
    for A in range(4):
        for paths in (4, 8):
            out.append((f"P2 above the bound at A = {A}, {paths} paths", 40, 60, sdc.params(A=A),
                        dict(p1=1, p2=65534 // paths - 62 * (2 * A + 1) ** 2 + 1, paths=paths), 3))
    out.append(("volume of 2^30 + 8192 entries", 8192, 8192, sdc.params(dmin=1, dmax=17), sgc.sgm(), 4))
    out.append(("volume 4096 x 8192 x 33", 4096, 8192, sdc.params(dmin=8, dmax=40), sgc.sgm(), 4))
    return out


def test_shared_header_under_sanitizers(tmp_path):
    """stereo_sgm_math.h as a g++ program of its own (ASan + UBSan, every volume a heap block of exactly its size): the cost volume,
    the aggregation line by line and the selection equal the model byte for byte on every row, S included; the largest aggregate
    stays within paths (Cmax + P2); sgm_check_params names the bound of every bad parameter set and passes each bound's last good
    value."""
    exe = str(tmp_path / "stereo_sgm_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", HARNESS, "-o", exe])

    def head(rows, cols, p, sg):
        return (np.array([rows, cols, p["dmin"], p["dmax"], p["A"], p["uniq"], p["lr_max"], p["max_raw"], sg["p1"], sg["p2"], sg["paths"]],
                         np.int32).tobytes() + np.array([p["fx"], p["baseline"], p["depth_scale"]], np.float64).tobytes())

    for what, r, c, p, sg, bound in harness_bad():
        assert sgc.check_params(r, c, p, sg) == bound, what
    with open(tmp_path / "in.bin", "wb") as f:
        for _, L, R, p, sg, _ in sgc.rows():
            f.write(head(L.shape[0], L.shape[1], p, sg) + L.tobytes() + R.tobytes())
        for _, r, c, p, sg, _ in harness_bad():
            f.write(head(r, c, p, sg))
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert done.stdout.strip() == f"{len(sgc.rows()) + len(harness_bad())} records"
    blob = open(tmp_path / "out.bin", "rb").read()
    at = 0
    for index, (name, L, _, p, sg, _) in enumerate(sgc.rows()):
        depth, q, stats, S, T = sgc.model_of(index)
        assert int(np.frombuffer(blob, np.int32, 1, at)[0]) == 0, name
        got_d = np.frombuffer(blob, np.uint16, L.size, at + 4).reshape(L.shape)
        got_q = np.frombuffer(blob, np.uint16, L.size, at + 4 + 2 * L.size).reshape(L.shape)
        counts = np.frombuffer(blob, np.int64, 8, at + 4 + 4 * L.size)
        got_S = np.frombuffer(blob, np.uint16, S.size, at + 4 + 4 * L.size + 64).reshape(S.shape)
        at += 4 + 4 * L.size + 64 + 2 * S.size
        assert np.array_equal(got_S, S), (name, np.argwhere(got_S != S)[:4])
        assert np.array_equal(got_q, q) and np.array_equal(got_d, depth), (name, np.argwhere(got_q != q)[:4])
        assert dict(zip(sdc.STATS, counts[:6].tolist())) == stats, name
        assert int(counts[6]) == int(S[T["adm"]].max(initial=0)) and int(counts[7]) == int(T["C"][T["adm"]].max(initial=0)), name
        assert counts[6] <= sg["paths"] * (counts[7] + sg["p2"]), name
    for what, _, _, _, _, bound in harness_bad():
        assert int(np.frombuffer(blob, np.int32, 1, at)[0]) == bound, what
        at += 4
    assert at == len(blob)


# ---- what the method gives -----------------------------------------------------------------------------------------------------------------
def _wrong(q, truth):
    m = q > 0
    err = np.abs(q[m] / 16.0 - truth[m])
    return int(m.sum()), int((err > 1.0).sum()), float((err <= 1.0).mean()), float((err <= 0.5).mean())


@pytest.mark.parametrize("drive", ["natural", "corridor"])
def test_density_and_accuracy_against_the_renderers_ground_truth(drive):
    """Frame 0 of the drive at 188 x 620, rendered_params(2), default penalties: the counts of DESIGN.md section 9.18, more matched
    pixels than the box matcher (on `natural` at least 5 % more), and at least 99.5 % of them within a pixel of f b / Z — the cap
    that keeps density from being bought with wrong pixels."""
    left, right, Z, fx, baseline = sdc.rendered_pair(drive)
    p = sdc.rendered_params(2)
    truth = fx * baseline / Z
    box = _wrong(sdc.stereo_model(left, right, p)[1], truth)
    s8 = _wrong(sgc.sgm_model(left, right, p, sgc.sgm(paths=8))[1], truth)
    s4 = _wrong(sgc.sgm_model(left, right, p, sgc.sgm(paths=4))[1], truth)
    for tag, r in (("box", box), ("8 paths", s8), ("4 paths", s4)):
        print(f"{drive}, {tag}: matched {r[0]}, wrong {r[1]}, within 1 px {100 * r[2]:.2f} %, within 0.5 px {100 * r[3]:.2f} %")
    assert (box[:2], s8[:2], s4[:2]) == tuple(MEASURED[drive][k] for k in ("box", "sgm8", "sgm4"))
    assert s8[0] > box[0] and s8[2] >= 0.995
    if drive == "natural":
        assert s8[0] >= 1.05 * box[0]


def test_known_answers_on_the_integer_disparity_pair():
    L, R, disp = sdc.integer_pair()[:3]
    p = sdc.params(dmin=1, dmax=63)
    far = lambda q: (int((q > 0).sum()), int((np.abs(q.astype(int) - 16 * disp)[q > 0] > 16).sum()))
    box = far(sdc.model_of(sdc.row_ids().index("integer disparity pair 96 x 320"))[1])
    s8 = far(sgc.model_of(sgc.row_ids().index("integer disparity pair 96 x 320, A = 2, 8 paths"))[1])
    print("integer pair: box", box, "8 paths", s8)
    assert (box, s8) == (MEASURED["integer"]["box"], MEASURED["integer"]["sgm8"])


def test_the_wall_scene_where_the_mode_loses():
    """Recorded, not asserted as a property: on the untextured wall the census bits are the sign of the noise, no path has a signal
    to propagate, and the semi-global mode matches MORE wrong pixels than the box matcher, before and after the speckle filter
    (DESIGN.md section 9.18). Only the figures' reproduction is held."""
    L, R = sc.wall_pair()
    p = sc.wall_params()

    def figures(q):
        wrong = (q > 0) & (np.abs(q.astype(int) - 192) > 16)
        kept = sc.apply_keep(q, sc.speckle_model(q, 16, 100))
        return dict(wrong=int(wrong.sum()), patch_wrong=int(wrong[28:68, 120:240].sum()),
                    after=int(((kept > 0) & (np.abs(kept.astype(int) - 192) > 16)).sum()))
    got = dict(box=figures(sc.wall_match()[1]), sgm8=figures(sgc.sgm_model(L, R, p, sgc.sgm())[1]))
    print("wall:", got)
    assert got == MEASURED["wall"]


# ---- code object ---------------------------------------------------------------------------------------------------------------------------
def test_sgm_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
    num = lambda s: -int(s[1:]) if s.startswith("n") else int(s)
    found = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        key = None
        if m := re.search(r"sgm_cost_kernelILi(\d)EE", name):
            key = ("cost", int(m.group(1)))
        elif m := re.search(r"sgm_path_kernelILi(n?\d)ELi(n?\d)ELi(\d)ELb([01])EE", name):
            key = ("path", num(m.group(1)), num(m.group(2)), int(m.group(3)), int(m.group(4)))
        elif m := re.search(r"sgm_select_kernelILb([01])EE", name):
            key = ("select", int(m.group(1)))
        if key is not None:
            found[key] = tuple(int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in (
                "vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"))
    print(found)
    k = sgc.constants()
    assert sorted(found) == sorted([("cost", a) for a in range(4)] + [("path", dx, dy, ns, int((dx, dy) == sgc.DIRS[0])) for dx, dy in sgc.DIRS for ns in range(1, k["kSgmSlots"] + 1)] + [("select", 0), ("select", 1)])
    for key, (vgprs, _, lds, vspill, sspill, scratch) in found.items():
        assert (vspill, sspill, scratch) == (0, 0, 0), key
        assert vgprs <= 128, key                                             # four waves per SIMD at the least
        if key[0] == "path":
            assert lds == 0, key                                             # a line is one wave's registers
        elif key[0] == "select":
            words = k["kSdTileH"] * k["kSgmChunk"] * k["kSgmChunkStride"]
            assert 2 * words <= lds <= 2 * words + 128, (key, lds)
        else:
            a = key[1]
            words = (k["kSdTileH"] + 2 * a) * (2 * (k["kSdTileW"] + 2 * a) + k["kSdMaxSpan"])
            out = 2 * k["kSdTileH"] * k["kSdTileW"] * k["kSgmCostStride"]      # the block the tile's costs leave through
            assert 8 * words + out <= lds <= 8 * words + out + 128 and lds < 64 * 1024, (key, lds)
