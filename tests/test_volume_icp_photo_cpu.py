"""The photometric term of frame-to-model tracking (odo_volume_icp_photo_eval_dev, odo_volume_icp_photo_align_dev,
odo_volume_track_photo_dev, api.TsdfVolume.icp_eval / align / track with grey=) without a GPU: the ABI and the argument checks, the
numpy model of the specification (include/odometry_hip.h) pinned to the prose by a plain loop that does one
fp32 operation at a time, every branch reached by a row made for it, the host + device header
odometry_amd/csrc/volume_icp_photo_math.h compiled by g++ as a library and, with sanitizers, as a program, the rule of the defaults,
the model against the ground truth of the two pinned cases, and the kernels' code-object metadata.

The model (tests/volume_icp_photo_cases.py) is the yardstick of tests/test_gpu_volume_icp_photo.py, which asks the GPU for the same
bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import volume_icp_photo_cases as pc
from test_volume_cpu import bits
from test_volume_icp_cpu import build_host_library, good_params, host_step, icp, icp_align_model, icp_frame, pose_error, rows_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

NEW_SYMBOLS = ["odo_volume_icp_photo_eval_dev", "odo_volume_icp_photo_align_dev", "odo_volume_track_photo_dev",
               "odo_volume_icp_photo_time_dev"]
# The instantiations for 31 sums of the kernel templates of volume_icp_kernels.hip, as the code object names them.
PHOTO_KERNELS = ["volume_icp_rows_kernelILi31E", "volume_icp_step_kernelILi31E", "volume_icp_init_kernelILi31E"]
# Measured with this model at the defaults (test_ground_truth_with_the_photometric_term prints them): the largest error of the six
# frames of either case. The assertions there and in tests/test_gpu_volume_icp_photo.py are twice these.
MEASURED_CORRIDOR_T_M = 0.031702      # frame 1 (geometric only: 0.56718, frame 1)
MEASURED_CORRIDOR_R_DEG = 0.1739      # frame 3 (geometric only: 4.602, frame 1)
MEASURED_RIBBED_T_M = 0.012643        # frame 6 (geometric only: 0.004357, frame 3): the term costs this case accuracy
MEASURED_RIBBED_R_DEG = 0.2360        # frame 6 (geometric only: 0.2253, frame 1)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    assert C.sizeof(_lib.IcpPhotoParams) == 8 and C.sizeof(_lib.IcpPhotoResult) == 120 and C.sizeof(_lib.IcpPhotoTraceRow) == 344
    for t in ("odo_icp_photo_params", "odo_icp_photo_result", "odo_icp_photo_trace_row"):
        assert t in hdr
    for name in ("photo_params", "icp_photo_time"):
        assert callable(getattr(api.TsdfVolume, name))
    ph = api.TsdfVolume.photo_params(api.TsdfVolume)
    assert (ph.weight, ph.huber_delta) == (f32(api.TsdfVolume.ICP_PHOTO_WEIGHT), f32(api.TsdfVolume.ICP_PHOTO_HUBER))


def test_bad_arguments_are_refused_before_touching_a_device():
    from odometry_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(64)   # never dereferenced: every case below is refused by the argument checks
    nan, inf = float("nan"), float("inf")
    eye = (C.c_float * 16)(*np.eye(4, dtype=f32).ravel())
    out = (C.c_float * 16)()
    acc = (C.c_double * pc.NACC)()
    us = (C.c_float * 2)()
    res = L.IcpPhotoResult()
    good, ph = good_params(), L.IcpPhotoParams(0.003, 12.0)

    def align(p=good, photo=ph, frames=(fake,) * 5, P_m=eye, P_i=eye, result=res, trace=None, cap=0, v=fake):
        d, n, c, r, g = frames
        return lib.odo_volume_icp_photo_align_dev(v, C.byref(p) if p else None, C.byref(photo) if photo else None, d, n, c, P_m, r, g, P_i, out,
                                                  C.byref(result) if result else None, trace, cap, None)

    def evaluate(frames=(fake,) * 5, P_m=eye, Cm=eye, stride=1, dist_max=0.1, huber=0.0, photo=ph, a=acc, rows=None):
        d, n, c, r, g = frames
        return lib.odo_volume_icp_photo_eval_dev(fake, d, n, c, P_m, r, g, Cm, stride, dist_max, huber, C.byref(photo) if photo else None, a, rows)

    from test_volume_icp_cpu import bad_params
    for kw, p in bad_params():
        assert align(p=p) == -1 and "odo_volume_icp_photo_align_dev:" in L.last_error(), (kw, L.last_error())
        assert lib.odo_volume_track_photo_dev(fake, C.byref(p), C.byref(ph), fake, fake, eye, out, C.byref(res)) == -1, kw
        assert "odo_volume_track_photo_dev:" in L.last_error(), (kw, L.last_error())
    for w, h in ((0.0, 0.0), (-1.0, 0.0), (nan, 0.0), (inf, 0.0), (0.01, -1.0), (0.01, nan), (0.01, inf)):
        bad = L.IcpPhotoParams(w, h)
        assert align(photo=bad) == -1 and "photometric" in L.last_error(), (w, h)
        assert evaluate(photo=bad) == -1 and "photometric" in L.last_error(), (w, h)
        assert lib.odo_volume_track_photo_dev(fake, C.byref(good), C.byref(bad), fake, fake, eye, out, C.byref(res)) == -1
        assert "photometric" in L.last_error()
        assert lib.odo_volume_icp_photo_time_dev(fake, fake, fake, fake, eye, fake, fake, eye, 1, 0.1, 0.0, C.byref(bad), 5, us) == -1
    for i in (0, 5, 12, 15):
        for v in (nan, inf, -inf):
            A = (C.c_float * 16)(*np.eye(4, dtype=f32).ravel())
            A[i] = v
            assert align(P_m=A) == -1 and align(P_i=A) == -1 and "pose" in L.last_error()
            assert evaluate(P_m=A) == -1 and evaluate(Cm=A) == -1 and "pose" in L.last_error()
            assert lib.odo_volume_track_photo_dev(fake, C.byref(good), C.byref(ph), fake, fake, A, out, C.byref(res)) == -1
    for args in (dict(stride=0), dict(stride=17), dict(dist_max=0.0), dict(dist_max=nan), dict(dist_max=inf), dict(huber=-1.0), dict(huber=nan)):
        assert evaluate(**args) == -1 and "odo_volume_icp_photo_eval_dev:" in L.last_error(), args
    for k, addr in enumerate((2, 8, 2, 1, 2)):                  # depth 4, nrmw 16, rgba 4, raw 2, grey 4
        frames = [fake] * 5
        frames[k] = C.c_void_p(addr)
        assert evaluate(frames=frames) == -1 and "misaligned" in L.last_error(), k
        assert align(frames=frames) == -1 and "misaligned" in L.last_error(), k
        frames[k] = None
        assert evaluate(frames=frames) == -1 and align(frames=frames) == -1
    assert evaluate(rows=C.c_void_p(8)) == -1 and "misaligned" in L.last_error()
    assert lib.odo_volume_track_photo_dev(fake, C.byref(good), C.byref(ph), C.c_void_p(1), fake, eye, out, C.byref(res)) == -1
    assert lib.odo_volume_track_photo_dev(fake, C.byref(good), C.byref(ph), fake, C.c_void_p(2), eye, out, C.byref(res)) == -1
    assert "misaligned" in L.last_error()
    trace = (L.IcpPhotoTraceRow * 1)()
    assert align(trace=trace, cap=0) == -1
    assert align(v=None) == -1 and align(p=None) == -1 and align(photo=None) == -1 and align(result=None) == -1
    assert evaluate(a=None) == -1 and evaluate(photo=None) == -1
    for args in ((None, good, ph, fake, fake), (fake, None, ph, fake, fake), (fake, good, None, fake, fake), (fake, good, ph, None, fake),
                 (fake, good, ph, fake, None)):
        v, p, photo, r, g = args
        assert lib.odo_volume_track_photo_dev(v, C.byref(p) if p else None, C.byref(photo) if photo else None, r, g, eye, out, C.byref(res)) == -1
    for reps in (0, 10001):
        assert lib.odo_volume_icp_photo_time_dev(fake, fake, fake, fake, eye, fake, fake, eye, 1, 0.1, 0.0, C.byref(ph), reps, us) == -1


# ---- the model against the prose -------------------------------------------------------------------------------------------------
def model_cases():
    cases = [(fr, s, 0.3, h, 0.01, ph) for seed in range(3) for fr in [pc.random_photo_frames(seed)]
             for s, h, ph in ((1, 0.0, 0.0), (2, 0.02, 4.0), (3, 0.0, 12.0), (4, 0.005, 1.0))]
    cases += [(fr, s, 2 * float(f32(fr[0]["mu"])), 0.01, 0.003, 12.0) for fr in pc.tiny_photo_views() for s in (1, 3)]
    return cases


def test_vectorised_rows_equal_the_loop_bit_for_bit():
    total = {k: 0 for k in pc.PHOTO_TALLIES}
    cases = model_cases()
    for (p, raw, grey, depth, nrmw, rgba, P_m, P_init), stride, dist_max, huber, weight, ph in cases:
        M, Cm = icp_frame(P_m, P_init)
        got, mg, mp = pc.icp_photo_rows_model(raw, grey, depth, nrmw, rgba, M, Cm, p, stride, dist_max, huber, weight, ph)
        want, acc, met = pc.icp_photo_rows_loop(raw, grey, depth, nrmw, rgba, M, Cm, p, stride, dist_max, huber, weight, ph)
        rows_equal(got, want, (stride, dist_max))
        assert mp.sum() == met["pairs"] and (got[..., 8:][~mp] == 0).all() and mg.sum() == met["both"] + met["geo_only"]
        s, mag, n = pc.icp_photo_acc(got, mg, mp)
        assert (np.abs(s - acc) <= max(1, n) * 2.0 ** -52 * mag)[np.isfinite(mag)].all()
        assert np.array_equal(s[28:30], acc[28:30]) or not np.isfinite(mag).all()
        for k, v in met.items():
            total[k] += v
    print(len(cases), "evaluations:", total)
    for k in ("no_point", "off_left", "off_top", "model_hole", "gated", "tap00", "tap01", "tap10", "tap11", "huber_below", "huber_above",
              "pairs", "geo_only", "photo_only", "both", "neither"):
        assert total[k] > 0, (k, total)


def test_the_kernels_order_of_the_sums_is_one_of_the_orders():
    """icp_photo_acc_kernel_order, which tests/test_gpu_volume_icp_photo.py holds the GPU to bit for bit: inside the bound of any order
    round the pairwise sums and both counts exact, on one block, on several, with two partials per lane and with more than 64 blocks."""
    for size, stride in (((2, 2), 1), ((17, 23), 1), ((65, 33), 1), ((65, 33), 4), ((120, 160), 1)):
        K = (1.3 * max(*size, 8), (size[1] - 1) / 2, (size[0] - 1) / 2)
        p, raw, grey, depth, nrmw, rgba, P_m, P_init = pc.random_photo_frames(0, size, K)
        rows16, mg, mp = pc.icp_photo_rows_model(raw, grey, depth, nrmw, rgba, *icp_frame(P_m, P_init), p, stride, 0.3, 0.01, 0.01, 6.0)
        s, mag, n = pc.icp_photo_acc(rows16, mg, mp)
        order = pc.icp_photo_acc_kernel_order(rows16, mg, mp, stride)
        assert n > 0 and order[28] == mg.sum() and order[29] == mp.sum(), (size, stride)
        assert (np.abs(order - s) <= n * 2.0 ** -52 * mag).all(), (size, stride)


@pytest.mark.parametrize("row", pc.photo_branch_rows(), ids=lambda r: r[0])
def test_every_branch_is_reached_by_the_row_made_for_it(row):
    name, p, raw, grey, depth, nrmw, rgba, M, Cm, stride, dist_max, huber, weight, ph, predicate = row
    got, mg, mp = pc.icp_photo_rows_model(raw, grey, depth, nrmw, rgba, M, Cm, p, stride, dist_max, huber, weight, ph)
    want, acc, met = pc.icp_photo_rows_loop(raw, grey, depth, nrmw, rgba, M, Cm, p, stride, dist_max, huber, weight, ph)
    rows_equal(got, want, name)
    assert predicate(met), (name, met)
    assert mp.sum() == met["pairs"] and acc[29] == met["pairs"] and acc[28] == mg.sum()
    if name == "a flat patch":                                 # cost and count only: res = lambda (77 - 50), J = 0
        assert (got[..., 8:14] == 0).all() and (got[..., 14] == f32(0.25 * 27)).all() and acc[30] == 24 * (0.25 * 27) ** 2
        assert not acc[:27].any() or mg.any()
    if name.startswith("photo_huber"):
        assert got[0, 0, 15] == 1.0 and got[0, 1, 15] == 1.0 and got[0, 2, 15] == 0.5, got[0, :, 14:]
    if name.startswith("|pm_z"):
        assert not mp[:, :1].any() and mp[:, 4:].all()
    if name.startswith("colours on"):                          # the integer rule, not a float one
        c = rgba.reshape(-1, 4).astype(np.float64)
        exact = (c[:, 0] * 4899 + c[:, 1] * 9617 + c[:, 2] * 1868) / 16384
        assert (np.abs(exact - np.floor(exact) - 0.5) < 1e-4).all() and (pc.grey_of(rgba).reshape(-1) == np.floor(exact + 0.5)).all()


# ---- the shared header on the host -------------------------------------------------------------------------------------------------
HARNESS = os.path.join(ROOT, "tests", "volume_icp_photo_math_harness.cpp")
HEAD = np.dtype([("rows", "<i4"), ("cols", "<i4"), ("stride", "<i4"), ("f", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("depth_scale", "<f4"),
                 ("max_depth", "<f4"), ("dist_max", "<f4"), ("huber_delta", "<f4"), ("photo_weight", "<f4"), ("photo_huber", "<f4"),
                 ("M", "<f4", 16), ("C", "<f4", 16)])
STEP_REC = np.dtype([("acc", "<f8", pc.NACC), ("C", "<f4", 16), ("min_pairs", "<i4"), ("eps_t", "<f4"), ("eps_r", "<f4"), ("pad", "<i4")])
STEP_OUT = np.dtype([("failed", "<i4"), ("converged", "<i4"), ("delta", "<f4", 6), ("C", "<f4", 16)])


def build_photo_library(directory):
    so = os.path.join(str(directory), "volume_icp_photo_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-DICP_HARNESS_LIBRARY", "-shared", "-fPIC",
                           HARNESS, "-o", so])
    return C.CDLL(so)


def build_sanitized_program(directory):
    exe = os.path.join(str(directory), "volume_icp_photo_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", HARNESS, "-o", exe])
    return exe


def head_of(p, M, Cm, stride, dist_max, huber, weight, ph):
    h = np.zeros(1, HEAD)
    h["rows"], h["cols"], h["stride"] = p["size"][0], p["size"][1], stride
    h["f"], h["cx"], h["cy"] = p["K"]
    h["depth_scale"], h["max_depth"], h["dist_max"], h["huber_delta"] = p["depth_scale"], p["max_depth"], dist_max, huber
    h["photo_weight"], h["photo_huber"] = weight, ph
    with np.errstate(all="ignore"):
        h["M"], h["C"] = np.asarray(M, f32).T.reshape(16), np.asarray(Cm, f32).T.reshape(16)
    return h


def frames_of(raw, grey, depth, nrmw, rgba):
    return (np.ascontiguousarray(raw, np.uint16), np.ascontiguousarray(grey, f32), np.ascontiguousarray(depth, f32),
            np.ascontiguousarray(nrmw, f32), np.ascontiguousarray(rgba, np.uint8))


def host_rows(lib, raw, grey, depth, nrmw, rgba, M, Cm, p, stride, dist_max, huber, weight, ph):
    h = head_of(p, M, Cm, stride, dist_max, huber, weight, ph)
    fr = frames_of(raw, grey, depth, nrmw, rgba)
    out = np.zeros(p["size"] + (16,), f32)
    acc = np.zeros(pc.NACC)
    lib.icp_photo_host_rows(h.ctypes.data_as(C.c_void_p), *[a.ctypes.data_as(C.c_void_p) for a in fr], out.ctypes.data_as(C.c_void_p),
                            acc.ctypes.data_as(C.c_void_p))
    return out, acc


def host_cases():
    """(frames, M, C, stride, dist_max, huber, weight, photo_huber) of the host builds: random frames, tiny views, every branch row."""
    out = []
    for fr, stride, dist_max, huber, weight, ph in model_cases()[::3]:
        M, Cm = icp_frame(fr[6], fr[7])
        out.append((fr[:6], M, Cm, stride, dist_max, huber, weight, ph))
    for row in pc.photo_branch_rows():
        out.append((row[1:7], row[7], row[8]) + row[9:14])
    return out


@pytest.fixture(scope="module")
def photo_host(tmp_path_factory):
    return build_photo_library(tmp_path_factory.mktemp("icp_photo_host"))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_library(tmp_path_factory.mktemp("icp_host"))


def test_host_library_rows_and_sums_equal_the_loop(photo_host):
    for (p, raw, grey, depth, nrmw, rgba), M, Cm, stride, dist_max, huber, weight, ph in host_cases():
        got, acc = host_rows(photo_host, raw, grey, depth, nrmw, rgba, M, Cm, p, stride, dist_max, huber, weight, ph)
        want, acc_loop, _ = pc.icp_photo_rows_loop(raw, grey, depth, nrmw, rgba, M, Cm, p, stride, dist_max, huber, weight, ph)
        rows_equal(got, want)
        assert np.array_equal(acc.view(np.uint64), acc_loop.view(np.uint64)) or not np.isfinite(acc_loop).all()


def test_shared_header_under_sanitizers(tmp_path, photo_host, host):
    """The stand-alone program (AddressSanitizer, UBSan) gives the library's bytes on rows and sums, and the step on 31 sums is the
    step of tests/test_volume_icp_cpu.py's library on the first 29."""
    exe = build_sanitized_program(tmp_path)

    def run(mode, blob):
        src, dst = str(tmp_path / (mode + ".in")), str(tmp_path / (mode + ".out"))
        open(src, "wb").write(blob)
        out = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
        return open(dst, "rb").read()

    for (p, raw, grey, depth, nrmw, rgba), M, Cm, stride, dist_max, huber, weight, ph in host_cases():
        blob = head_of(p, M, Cm, stride, dist_max, huber, weight, ph).tobytes() + b"".join(a.tobytes() for a in frames_of(raw, grey, depth, nrmw, rgba))
        want_rows, want_acc = host_rows(photo_host, raw, grey, depth, nrmw, rgba, M, Cm, p, stride, dist_max, huber, weight, ph)
        assert run("rows", blob) == want_rows.tobytes() + want_acc.tobytes()
    from test_volume_icp_cpu import step_cases
    cases = step_cases()
    rec = np.zeros(len(cases), STEP_REC)
    for i, (acc, Cm, mp, et, er) in enumerate(cases):
        rec["acc"][i, :29], rec["acc"][i, 29:] = acc, (7.0, 0.5)
        rec["C"][i], rec["min_pairs"][i], rec["eps_t"][i], rec["eps_r"][i] = Cm.T.reshape(16), mp, et, er
    got = np.frombuffer(run("step", rec.tobytes()), STEP_OUT)
    step = host_step(host)
    for i, (acc, Cm, mp, et, er) in enumerate(cases):
        a = step(acc, Cm, mp, et, er)
        assert (int(got["failed"][i]), int(got["converged"][i])) == a[:2]
        assert np.array_equal(bits(got["delta"][i]), bits(a[2])) and np.array_equal(bits(got["C"][i].reshape(4, 4).T), bits(a[3]))


# ---- the model against the ground truth, and the defaults -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sequences():
    out = {}
    for name, make in (("corridor", pc.corridor_photo_sequence), ("ribbed", pc.ribbed_photo_sequence)):
        seq = make()
        out[name] = (seq, pc.photo_models(seq))
    return out


def worst(seq, results):
    errs = [pose_error(results[k]["abs_pose"], seq["poses"][k]) for k in sorted(results)]
    return max(e[0] for e in errs), max(e[1] for e in errs), errs


def test_ground_truth_with_the_photometric_term(sequences, host):
    """Both pinned cases at the defaults, frames 1 .. 6, each against the coloured volume of the frames before it at true poses.
    Conditions: every frame reaches status 0, and on the corridor every frame's translation error is at most half of the
    geometric-only alignment's. Measured bounds: MEASURED_* (DESIGN.md section 9.10), asserted at twice their value."""
    step = host_step(host)
    measured = dict(corridor=(MEASURED_CORRIDOR_T_M, MEASURED_CORRIDOR_R_DEG), ribbed=(MEASURED_RIBBED_T_M, MEASURED_RIBBED_R_DEG))
    for name, (seq, models) in sequences.items():
        ic = icp(p=seq["p"], min_eig_ratio=0.0)
        res = pc.photo_frame_to_model(seq, models, ic, pc.photo(), step=step)
        wt, wr, errs = worst(seq, res)
        for k, (et, er) in zip(sorted(res), errs):
            r = res[k]
            g = icp_align_model(seq["depth"][k], models[k][0], models[k][1], seq["poses"][k - 1], seq["poses"][k - 1], seq["p"], ic, step=step)
            gt, gr = pose_error(g["abs_pose"], seq["poses"][k])
            print(f"{name} frame {k}: {et * 1e3:.2f} mm {er:.3f} deg (geometric only {gt * 1e3:.2f} mm {gr:.3f} deg), pairs {r['pairs']:.0f} + "
                  f"{r['photo_pairs']:.0f}, photometric share of the cost {r['photo_cost'] / r['cost']:.2f}, ratio "
                  f"{r['eig_min'] / r['eig_max']:.2e}, steps {r['iterations']}")
            assert r["status"] == 0, (name, k, r["status"])
            if name == "corridor":
                assert et <= 0.5 * gt, (k, et, gt)
        print(f"{name}: largest {wt * 1e3:.3f} mm {wr:.4f} deg")
        assert wt <= 2 * measured[name][0] and wr <= 2 * measured[name][1], (name, wt, wr)


def test_default_photo_params_follow_the_rule_of_the_grid(sequences, host):
    """The defaults are the pair of the grid WEIGHTS x HUBERS with the smallest sum of the two cases' worst translation errors over
    frames 1 .. 6 (DESIGN.md section 9.10 holds the grid this prints)."""
    from odometry_amd import api
    step = host_step(host)
    total = {}
    for weight in pc.WEIGHTS:
        for huber in pc.HUBERS:
            parts = []
            for name, (seq, models) in sequences.items():
                res = pc.photo_frame_to_model(seq, models, icp(p=seq["p"], min_eig_ratio=0.0), pc.photo(weight, huber), step=step)
                wt = worst(seq, res)[0]
                parts.append(wt if np.isfinite(wt) else np.inf)                  # (a refused frame's pose is NaN: never the best)
            total[(weight, huber)] = sum(parts)
            print(f"weight {weight} huber {huber}: corridor {parts[0] * 1e3:.2f} mm, ribbed {parts[1] * 1e3:.2f} mm, sum {sum(parts) * 1e3:.2f} mm")
    best = min(total, key=total.get)
    assert (api.TsdfVolume.ICP_PHOTO_WEIGHT, api.TsdfVolume.ICP_PHOTO_HUBER) == best, (best, total[best])


# ---- code object ------------------------------------------------------------------------------------------------------------------
def test_photo_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        for k in PHOTO_KERNELS:
            if k in name:
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
                print(k, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1),
                      "lds", re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert sorted(found) == sorted(PHOTO_KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found
