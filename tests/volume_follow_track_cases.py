"""The closed loop of the TSDF volume: TsdfVolume.track(..., integrate=True) on a volume with set_follow on, every frame started from the
pose that the frame before it returned (DESIGN.md sections 9.8 and 9.9). The two drives, and the loop composed from the models that
each of its links is already held to:

  ray-cast   test_volume_raycast_cpu.raycast_model on test_volume_shift_cpu.window(p, off)
  alignment  test_volume_icp_cpu.icp_align_model (rows: icp_rows_model; sums: icp_acc_kernel_order; step: the host build's)
  window     test_volume_shift_cpu.follow_model, shift_model, offset_model
  stores     test_volume_shift_cpu.spill_model through volume_stores_cases.points_append, volume_reentry_cases.reentry_model
  fusion     test_volume_cpu.integrate_model

drive_model re-implements none of them. It is the yardstick of tests/test_gpu_volume_follow_track.py, which asks the GPU for the same
bits frame by frame; tests/test_volume_follow_track_cpu.py holds what the drives are there for on the model."""
import atexit
import functools
import shutil
import tempfile

import numpy as np

import volume_reentry_cases as R
import volume_stores_cases as V
from test_volume_cpu import empty_grid, integrate_model, params
from test_volume_icp_cpu import (RIBBED_SCENE, SMALL, build_host_library, host_step, icp, icp_acc, icp_acc_kernel_order, icp_align_model,
                                 small_K)
from test_volume_raycast_cpu import default_view, raycast_model
from test_volume_shift_cpu import follow_model, offset_model, origin_model, shift_model, spill_model, window

f32 = np.float32

# The window: 3.4 x 2.6 x 3.0 m of 5 cm voxels (212 160 of them) that starts 2 m in front of the camera, where this field of view
# first meets the walls and the floor, and follows the point 3.5 m in front of it (the window's centre at frame 0) once that is two
# voxels off on some axis.
WINDOW = dict(dims=(68, 52, 60), vs=0.05, origin=(-1.7, -1.3, 2.0), mu=0.15, max_depth=5.0, max_weight=65535)
FOLLOW = dict(focus=3.5, threshold=2)
# A ("leaves"): 26 frames, frame 9 blind (all zeros); the window ends deeper than it is long, so every voxel of the first window has
# left. B ("out and back"): 10 frames, then the same frames and poses in reverse; the window returns to where it started.
DRIVES = dict(A=dict(n=26, back=False, blind=(9,)), B=dict(n=10, back=True, blind=()))
# The frames behind which the model keeps its grid: A's first tracked frame, the frames round the blind one and the last; B's last.
CHECKPOINTS = dict(A=(1, 8, 9, 10, 25), B=(18,), fine=())
# The same corridor in 2.5 cm voxels (the same box, the follow threshold the same 10 cm): what a closed loop needs min_eig_ratio for.
# CPU only; see tests/test_volume_follow_track_cpu.py.
FINE_WINDOW = dict(dims=(136, 104, 120), vs=0.025, origin=(-1.7, -1.3, 2.0), mu=0.075, max_depth=5.0, max_weight=65535)
DRIVES["fine"] = dict(n=8, back=False, blind=(), window=FINE_WINDOW, follow=dict(focus=3.5, threshold=4))
SPILL_CAPACITY = 1 << 18
REENTRY_CAPACITY = 1 << 19


@functools.lru_cache(maxsize=None)
def drive(name):
    """depth, gray (Scene.render's grey frames, for the photometric path) and the true poses of a drive, the volume parameters p, the
    follow rule and the model's ICP parameters (min_eig_ratio 0: nothing is refused as rank-deficient)."""
    from odometry_amd import synth
    c = DRIVES[name]
    scene = synth.Scene(0, **RIBBED_SCENE)
    poses = list(synth.trajectory(c["n"], 0, fwd_range=(0.1, 0.2), max_offset=1.0))
    f, cx, cy = small_K()
    frames = [scene.render(T, SMALL[0], SMALL[1], f, cx, cy) for T in poses]
    depth = [synth.sensor_depth(Z, 1000.0, 30.0) for _, Z in frames]
    gray = [img for img, _ in frames]
    if c["back"]:
        poses, depth, gray = poses + poses[-2::-1], depth + depth[-2::-1], gray + gray[-2::-1]
    for k in c["blind"]:
        depth[k] = np.zeros_like(depth[k])
    p = params((f, cx, cy), 1000.0, SMALL, **c.get("window", WINDOW))
    return dict(name=name, depth=depth, gray=gray, poses=[np.asarray(T, f32) for T in poses], p=p, follow=dict(c.get("follow", FOLLOW)),
                blind=c["blind"], ic=icp(p=p, min_eig_ratio=0.0), checkpoints=CHECKPOINTS[name])


_HOST = []


def default_step():
    """The host build's icp_step (test_volume_icp_cpu.build_host_library), built once per process."""
    if not _HOST:
        d = tempfile.mkdtemp(prefix="follow_track_host_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        _HOST.append(host_step(build_host_library(d)))
    return _HOST[0]


def kernel_sums(worst):
    """The kernels' order of the sums as icp_align_model's strided_sums. worst[0] becomes the largest |kernel order - fp64 pairwise|
    over the bound of any summation order, n 2^-52 sum |terms|, met by the sums it is asked for."""
    def sums(rows8, mask, stride):
        acc = icp_acc_kernel_order(rows8, mask, stride)
        s, mag = icp_acc(rows8, mask)
        bound = int(mask.sum()) * 2.0 ** -52 * mag
        if (bound > 0).any():
            worst[0] = max(worst[0], float(np.max(np.abs(acc - s)[bound > 0] / bound[bound > 0])))
        assert np.array_equal(acc[bound == 0], s[bound == 0])
        return acc
    return sums


def shift_step(p, st, d, capacities):
    """The follow step's shift by d != 0 on the state st (q, w, off, points, reentry), in the product's order: the point spill reads
    the grid as it is, then the grid moves, with the re-entry store's restore, keep and save round the shift."""
    q, w, off = st["q"], st["w"], st["off"]
    if st["points"] is not None:
        st["points"], _ = V.points_append(st["points"], spill_model(q, w, None, window(p, off), d), capacities["points"])
    if st["reentry"] is not None:
        st["q"], st["w"], _, st["off"], st["reentry"] = R.reentry_model(q, w, None, off, st["reentry"], d, capacities["reentry"])
    else:
        (st["q"], st["w"], _), st["off"] = shift_model(q, w, None, d), offset_model(off, d)


def drive_model(name, reentry=False, spill=False, step=None, sums="kernel", frames=None):
    """The closed loop on the model, for a drive by name or a drive dict with drive()'s keys (depth, poses, p, follow, ic, checkpoints:
    tests/stereo_drive_cases.py brings the frames of a stereo matcher). Frame 0: the follow step for the first true pose, then its
    integration. Frame k: the ray-cast of window(p, off) from the last good pose, the alignment from that pose, and on status 0 the follow step for the returned pose, the
    shift it asks for, and the integration into the window as it then is; on any other status nothing changes and the good pose stays.
    sums: "kernel" (the device's bits) or "pairwise" (fp64, numpy's order). frames: stop behind that many.

    Returns dict(frames, q, w, off, points, reentry, shifts). frames[k]: status, iterations, pairs, cost, eig_min, eig_max, C, pose (what
    track returns: NaNs when refused), good (the pose the next frame starts from), d, off, origin, fused (stats()["frames"]), hits (the
    ray-cast's pixels with a surface), sum_ratio (see kernel_sums) and, at the drive's checkpoints, grid = (q, w)."""
    c = drive(name) if isinstance(name, str) else name
    p, ic, fo = c["p"], c["ic"], c["follow"]
    step = step or default_step()
    caps = dict(points=SPILL_CAPACITY, reentry=REENTRY_CAPACITY)
    q, w = empty_grid(p)
    st = dict(q=q, w=w, off=(0, 0, 0), points=V.empty_points(False) if spill else None, reentry=R.empty_store(False) if reentry else None)
    n = len(c["depth"]) if frames is None else frames
    good, fused, shifts, out = c["poses"][0], 0, 0, []
    for k in range(n):
        row = dict(status=0, d=(0, 0, 0), hits=0, sum_ratio=0.0)
        if k == 0:
            pose = good
        else:
            pw = window(p, st["off"])
            dm, _, nrmw, _ = raycast_model(st["q"], st["w"], None, good, pw, default_view(pw))
            worst = [0.0]
            how = dict(strided_sums=kernel_sums(worst)) if sums == "kernel" else {}
            r = icp_align_model(c["depth"][k], dm, nrmw, good, good, pw, ic, step=step, **how)
            pose = np.asarray(r["abs_pose"], f32)
            row.update({key: r[key] for key in ("status", "iterations", "pairs", "cost", "eig_min", "eig_max", "C")},
                       hits=int((dm > 0).sum()), sum_ratio=worst[0])
        if row["status"] == 0:
            d = follow_model(pose, p, st["off"], fo["focus"], fo["threshold"])
            if d != (0, 0, 0):
                shift_step(p, st, d, caps)
                shifts += 1
            st["q"], st["w"], _, _ = integrate_model(st["q"], st["w"], c["depth"][k], pose, window(p, st["off"]))
            good, fused = pose, fused + 1
            row["d"] = d
        row.update(pose=pose, good=good, off=st["off"], origin=origin_model(p["origin"], st["off"], p["vs"]), fused=fused)
        if k in c["checkpoints"]:
            row["grid"] = (st["q"], st["w"])
        out.append(row)
    return dict(frames=out, q=st["q"], w=st["w"], off=st["off"], points=st["points"], reentry=st["reentry"], shifts=shifts)


@functools.lru_cache(maxsize=None)
def model(name, reentry=False, spill=False):
    """drive_model with the device's sums and the host build's step, once per process."""
    return drive_model(name, reentry=reentry, spill=spill)
