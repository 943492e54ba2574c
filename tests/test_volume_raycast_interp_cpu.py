"""The trilinear colour sampling of the volume's ray-cast (odo_volume_set_colour_sampling, odo_volume_colour_sampling,
api.TsdfVolume.set_colour_sampling) without a GPU: the ABI and the refusals, the numpy model of the rule (include/odometry_hip.h,
DESIGN.md section 9.11) pinned to the prose by a plain loop that does one fp32 operation at a time, every branch reached by a row
made for it, a property on random grids, rc_colour_interp of odometry_amd/csrc/volume_raycast_math.h compiled by g++ with sanitizers,
the photometric alignment of the two pinned cases against model frames coloured by the rule, and the kernel's code-object metadata.

The model (tests/volume_raycast_interp_cases.py) is the yardstick of tests/test_gpu_volume_raycast_interp.py, which asks the GPU for
the same bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import volume_icp_photo_cases as pc
import volume_raycast_interp_cases as ic
from test_volume_icp_cpu import build_host_library, host_step, icp, pose_error
from test_volume_raycast_cpu import TALLIES, default_view, frames_equal, raycast_model, tiny_volumes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

NEW_SYMBOLS = ["odo_volume_set_colour_sampling", "odo_volume_colour_sampling", "odo_volume_raycast_time"]
# Measured with this model at the default photometric parameters (test_ground_truth_under_trilinear_sampling prints them): the largest
# error of the six frames of either case with the model frames coloured by the trilinear rule. The assertions there and in
# tests/test_gpu_volume_raycast_interp.py are twice these.
MEASURED_CORRIDOR_T_M = 0.011934      # frame 5 (nearest mode: 0.031702, frame 1)
MEASURED_CORRIDOR_R_DEG = 0.0951      # frame 3 (nearest mode: 0.1738, frame 3)
MEASURED_RIBBED_T_M = 0.007364        # frames 5 and 6 (nearest mode: 0.012642, frame 6)
MEASURED_RIBBED_R_DEG = 0.1624        # frame 1 (nearest mode: 0.2359, frame 6)
# The twelve lines that test prints for the trilinear mode. tests/test_gpu_volume_raycast_interp.py asks the GPU's track(grey=...) for
# the same lines, digit for digit.
TRILINEAR_LINES = dict(
    corridor=["corridor frame 1: 3.26 mm 0.028 deg, pairs 3210 + 2612, steps 16",
              "corridor frame 2: 2.25 mm 0.033 deg, pairs 5267 + 4557, steps 16",
              "corridor frame 3: 9.52 mm 0.095 deg, pairs 6583 + 6018, steps 19",
              "corridor frame 4: 8.09 mm 0.061 deg, pairs 6872 + 6247, steps 15",
              "corridor frame 5: 11.93 mm 0.082 deg, pairs 7115 + 6895, steps 16",
              "corridor frame 6: 6.07 mm 0.053 deg, pairs 6904 + 6488, steps 19"],
    ribbed=["ribbed frame 1: 6.71 mm 0.162 deg, pairs 11805 + 10361, steps 19",
            "ribbed frame 2: 2.60 mm 0.042 deg, pairs 11895 + 10343, steps 18",
            "ribbed frame 3: 3.79 mm 0.040 deg, pairs 13294 + 11747, steps 19",
            "ribbed frame 4: 1.70 mm 0.019 deg, pairs 13284 + 12223, steps 19",
            "ribbed frame 5: 7.36 mm 0.140 deg, pairs 13091 + 12026, steps 18",
            "ribbed frame 6: 7.36 mm 0.160 deg, pairs 13095 + 11986, steps 19"])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    assert callable(api.TsdfVolume.set_colour_sampling) and isinstance(api.TsdfVolume.colour_sampling, property)
    assert api.TsdfVolume.COLOUR_SAMPLING == ("nearest", "trilinear")


def test_bad_arguments_are_refused_before_touching_a_device():
    from odometry_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(8)   # never dereferenced: every case below is refused by the argument checks
    for mode in (2, -1, 3, 1 << 20):
        assert lib.odo_volume_set_colour_sampling(fake, mode) == -1 and "odo_volume_set_colour_sampling:" in L.last_error(), mode
    for mode in (0, 1, 2):
        assert lib.odo_volume_set_colour_sampling(None, mode) == -1 and "NULL" in L.last_error()
    assert lib.odo_volume_colour_sampling(None) == -1 and "odo_volume_colour_sampling:" in L.last_error()
    rp = L.RaycastParams(48, 64, 50.0, 32.0, 24.0, 0.0, 0.05, 100)
    pose = (C.c_float * 16)(*np.eye(4, dtype=f32).ravel())
    us = C.c_float(0)
    for reps in (0, -1, 10001):
        assert lib.odo_volume_raycast_time(fake, C.byref(rp), pose, 1, reps, C.byref(us)) == -1 and "reps" in L.last_error()
    assert lib.odo_volume_raycast_time(fake, C.byref(L.RaycastParams(0, 64, 50.0, 32.0, 24.0, 0.0, 0.05, 100)), pose, 0, 5, C.byref(us)) == -1
    assert "odo_volume_raycast_time:" in L.last_error()
    for args in ((None, C.byref(rp), pose, C.byref(us)), (fake, None, pose, C.byref(us)), (fake, C.byref(rp), None, C.byref(us)),
                 (fake, C.byref(rp), pose, None)):
        assert lib.odo_volume_raycast_time(*args[:3], 0, 5, args[3]) == -1 and "NULL" in L.last_error()


# ---- the model against the prose -------------------------------------------------------------------------------------------------
def _add(total, met):
    for k, v in met.items():
        total[k] = total.get(k, 0) + v


def test_vectorised_model_equals_the_loop_model_bit_for_bit():
    """On the four tiny volumes, coloured, from their own poses, and on the random grids; depth, raw and nrmw are raycast_model's. Per
    channel the output lies between the smallest and the largest value among the cell's coloured corners."""
    total, spans, views = {}, [], 0
    for p, q, w, col, poses in tiny_volumes():
        for pose in poses:
            rp = default_view(p, n_steps=30)
            got = ic.raycast_interp_model(q, w, col, pose, p, rp)
            *want, met, imet = ic.raycast_interp_loop(q, w, col, pose, p, rp, spans)
            frames_equal(got, want, "tiny")
            frames_equal(got[:3], raycast_model(q, w, col, pose, p, rp)[:3], "tiny, against the nearest mode")
            _add(total, imet)
            views += 1
    for tag, p, q, w, col, pose, rp in ic.random_views():
        assert (w == 0).any() and (col[..., 3] == 0).any()
        got = ic.raycast_interp_model(q, w, col, pose, p, rp)
        *want, met, imet = ic.raycast_interp_loop(q, w, col, pose, p, rp, spans)
        frames_equal(got, want, tag)
        frames_equal(got[:3], raycast_model(q, w, col, pose, p, rp)[:3], tag + ", against the nearest mode")
        _add(total, imet)
        views += 1
    print(views, "views:", total)
    for k in ("hit", "invalid_cell", "coloured", "partial", "all8", "m_one"):   # (a cell with one or no coloured corner: the branch rows)
        assert total[k] > 0, (k, total)
    assert total["m_one"] >= total["all8"] and len(spans) == total["coloured"]
    for rgb, lo, hi in spans:
        assert all(lo[k] <= rgb[k] <= hi[k] for k in range(3)), (rgb, lo, hi)


@pytest.mark.parametrize("row", ic.interp_branch_rows(), ids=lambda r: r[0])
def test_every_branch_is_reached_by_the_row_made_for_it(row):
    name, p, q, w, col, pose, rp, predicate, check = row
    *got, more = ic.raycast_interp_model(q, w, col, pose, p, rp, detail=True)
    *want, met, imet = ic.raycast_interp_loop(q, w, col, pose, p, rp)
    frames_equal(got, want, name)
    assert predicate(imet), (name, imet)
    near = raycast_model(q, w, col, pose, p, rp)
    frames_equal(got[:3], near[:3], name)
    if check is not None:
        assert check(got[3], near[3], more), (name, got[3].tolist())


def test_last_cell_views_end_on_the_grids_last_word():
    """The views that tests/test_gpu_volume_raycast_interp.py uses for the last pair load: every ray hits, in the last cell of all
    three axes, whose corner 7 is the grid's last voxel."""
    for tag, p, q, w, col, pose, rp, cell in ic.last_cell_views():
        *got, more = ic.raycast_interp_model(q, w, col, pose, p, rp, detail=True)
        *want, met, imet = ic.raycast_interp_loop(q, w, col, pose, p, rp)
        frames_equal(got, want, tag)
        nx, ny, nz = p["dims"]
        assert cell == (nx - 2, ny - 2, nz - 2) and imet["all8"] == imet["hit"] == 15, (tag, imet)
        assert all((more["bi"][c] == cell[c]).all() for c in range(3)) and more["ok"].all(), tag
        assert ((cell[2] + 1) * ny + cell[1] + 1) * nx + cell[0] + 1 == q.size - 1


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------
REC = np.dtype([("vox", "<u4", 8), ("col", "<u4", 8), ("e", "<f4", 3), ("g", "<f4", 3), ("t_min", "<f4"), ("step", "<f4"),
                ("n_steps", "<i4"), ("scale", "<f4")])
OUT = np.dtype([("hit", "<i4"), ("z", "<f4"), ("rgba", "u1", 4)])


def test_shared_header_equals_the_loop_model_under_sanitizers(tmp_path):
    """rc_colour_interp of odometry_amd/csrc/volume_raycast_math.h — the lines the device compiles — as a stand-alone g++ program with
    AddressSanitizer and UBSan, behind rc_march and rc_cell through bounds-checked loaders, on 20 000 random rays through coloured
    2 x 2 x 2 grids with colour holes (half of them a plane that the rays cross)."""
    exe = str(tmp_path / "volume_raycast_interp_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "volume_raycast_interp_harness.cpp"), "-o", exe])
    rng = np.random.default_rng(21)
    n = 20000
    rec = np.zeros(n, REC)
    nrm = rng.normal(size=(n, 3))
    off = rng.uniform(0.2, 0.8, n)
    corner = np.array([[d & 1, (d >> 1) & 1, d >> 2] for d in range(8)], float)
    plane = np.clip(((corner[None] * nrm[:, None, :]).sum(2) - (nrm * off[:, None]).sum(1)[:, None]) * 20000, -32767, 32767)
    qv = np.where((rng.uniform(size=n) < 0.8)[:, None], np.rint(plane).astype(np.int64), rng.integers(-32767, 32768, (n, 8)))
    wv = rng.integers(1, 65536, (n, 8))
    gone = np.nonzero(rng.uniform(size=n) < 0.05)[0]                        # one corner never observed: the whole grid is invalid
    wv[gone, rng.integers(0, 8, len(gone))] = 0
    rec["vox"] = (wv.astype(np.uint32) << 16) | (qv.astype(np.int16).view(np.uint16).astype(np.uint32))
    cv = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64).astype(np.uint32)
    cv[rng.uniform(size=(n, 8)) < rng.choice([0.0, 0.3, 0.8, 1.0], n)[:, None]] &= np.uint32(0x00ffffff)   # wc == 0: holes, up to all eight
    edge = rng.uniform(size=n) < 0.2                                        # channels at 0 and 255: the clamp
    cv[edge] = np.where(rng.uniform(size=(int(edge.sum()), 8)) < 0.5, cv[edge] | np.uint32(0x00ffffff), cv[edge] & np.uint32(0xff000000))
    rec["col"] = cv
    rec["step"] = rng.uniform(0.01, 0.3, n)
    rec["n_steps"] = rng.integers(2, 60, n)
    e = rng.uniform(-0.3, 1.3, (n, 3))
    g = (rng.uniform(0.0, 1.0, (n, 3)) - e) / (rec["step"] * rec["n_steps"] * rng.uniform(0.3, 1.2, n))[:, None]
    g[rng.uniform(size=(n, 3)) < 0.1] = 0.0
    rec["e"], rec["g"] = e, g
    rec["t_min"] = np.where(rng.uniform(size=n) < 0.5, 0.0, rng.uniform(0, 0.5, n))
    rec["scale"] = 1000.0
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rec.tofile(src)
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
    got = np.fromfile(dst, OUT)
    assert len(got) == n
    met, imet = {k: 0 for k in TALLIES}, {k: 0 for k in ic.INTERP_TALLIES}
    for i in range(n):
        q = (rec["vox"][i] & 0xffff).astype(np.uint16).view(np.int16).reshape(2, 2, 2)
        w = (rec["vox"][i] >> 16).astype(np.uint16).reshape(2, 2, 2)
        col = rec["col"][i].copy().view(np.uint8).reshape(2, 2, 2, 4)
        before = met["hit"]
        z, _, _, rgba = ic.ray_interp_loop(q, w, col, rec["e"][i], list(rec["g"][i]), rec["t_min"][i], rec["step"][i], int(rec["n_steps"][i]),
                                           rec["scale"][i], met, imet)
        want = np.zeros(1, OUT)
        want["hit"], want["z"], want["rgba"] = met["hit"] - before, z, rgba
        assert got[i].tobytes() == want[0].tobytes(), (i, got[i], want[0])
    print(imet)
    assert imet["hit"] > 1000 and imet["coloured"] > 500 and imet["none"] > 100 and imet["partial"] > 200 and imet["all8"] > 100
    assert imet["one"] > 0 and imet["clamp"] > 50 and imet["m_one"] >= imet["all8"]


# ---- the alignment against the ground truth, model frames coloured by the rule -------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_library(tmp_path_factory.mktemp("icp_host"))


def ground_truth_lines(name, seq, res):
    """The six lines of a case as section 9.10 prints them, and the largest translation and rotation error."""
    lines, wt, wr = [], 0.0, 0.0
    for k in sorted(res):
        r = res[k]
        et, er = pose_error(r["abs_pose"], seq["poses"][k])
        wt, wr = max(wt, et), max(wr, er)
        lines.append(f"{name} frame {k}: {et * 1e3:.2f} mm {er:.3f} deg, pairs {r['pairs']:.0f} + {r['photo_pairs']:.0f}, steps {r['iterations']}")
    return lines, wt, wr


def test_ground_truth_under_trilinear_sampling(host):
    """Section 9.10's two pinned cases at 120 x 160, frames 1 .. 6, default photometric parameters, each frame against the volume of
    the frames before it at true poses, the model frame's colours by the trilinear rule. Conditions: every frame reaches status 0,
    and each case's largest translation error is at most that of the nearest mode, computed here from the same volumes. Measured
    bounds: MEASURED_* (DESIGN.md section 9.11), asserted at twice their value."""
    step = host_step(host)
    measured = dict(corridor=(MEASURED_CORRIDOR_T_M, MEASURED_CORRIDOR_R_DEG), ribbed=(MEASURED_RIBBED_T_M, MEASURED_RIBBED_R_DEG))
    worst = {}
    for name, make in (("corridor", pc.corridor_photo_sequence), ("ribbed", pc.ribbed_photo_sequence)):
        seq = make()
        both = ic.photo_models_both(seq)
        par = icp(p=seq["p"], min_eig_ratio=0.0)
        res = pc.photo_frame_to_model(seq, {k: (d, n, tri) for k, (d, n, _, tri) in both.items()}, par, pc.photo(), step=step)
        near = pc.photo_frame_to_model(seq, {k: (d, n, nr) for k, (d, n, nr, _) in both.items()}, par, pc.photo(), step=step)
        lines, wt, wr = ground_truth_lines(name, seq, res)
        near_lines, nt, nr = ground_truth_lines(name + " (nearest)", seq, near)
        print("\n".join(lines + near_lines))
        print(f"{name}: largest {wt * 1e3:.3f} mm {wr:.4f} deg (nearest {nt * 1e3:.3f} mm {nr:.4f} deg)")
        assert all(res[k]["status"] == 0 for k in res), (name, [res[k]["status"] for k in sorted(res)])
        worst[name] = (wt, wr, nt, lines)
    for name, (wt, wr, nt, lines) in worst.items():   # (behind the loop: both cases' lines are printed whichever fails)
        assert lines == TRILINEAR_LINES[name], name
        assert wt <= nt, (name, wt, nt)
        assert wt <= 2 * measured[name][0] and wr <= 2 * measured[name][1], (name, wt, wr)


# ---- code object ------------------------------------------------------------------------------------------------------------------
def test_interp_kernel_is_in_the_gfx950_code_object_without_spills_or_scratch():
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
        for k in ("volume_raycast_kernel", "volume_raycast_interp_kernel"):
            if k in name:
                found[k] = tuple(int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1)) for key in
                                 ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"))
                print(k, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
    assert sorted(found) == ["volume_raycast_interp_kernel", "volume_raycast_kernel"], found
    assert all(v == (0, 0, 0, 0) for v in found.values()), found
