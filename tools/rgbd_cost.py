"""What RGB-D tracking (odo_tracker_create_rgbd) costs: bench.py's tracked loop (next frame announced with its depth frame, back and
forth over the drive) on
  tum      the TUM-shaped RGB-D drive (640 x 480, f = 525, RealSense-like 1000 units/m up to 30 m; synth.make_rgbd_sequence),
  kitti    a 1241 x 376 RGB-D rendering of the natural drive (KITTI intrinsics, 1000 units/m up to 30 m), and
  stereo   the stereo tracker on the same 1241 x 376 drive (the left images are the RGB-D drive's grey frames),
runs interleaved mode by mode. Prints frames/s per mode (median, spread), the stream-B job's host time per frame
(odo_tracker_timing out[2]) and the depth jobs run again after a give-up of the depth LM's persistent launch.

  python tools/rgbd_cost.py [--runs 5] [--steps 200] [--warmup 20] [--frames 100] [--modes tum,kitti,stereo]
"""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_scenes = {}


def _render(job):
    from odometry_amd import synth
    T, rows, cols, f, cx, cy, stereo = job
    if "s" not in _scenes:
        _scenes["s"] = synth.drive_scene("natural", 0)
    sc = _scenes["s"]
    img, Z = sc.render(T, rows, cols, f, cx, cy, 0.0)
    right = sc.render(T, rows, cols, f, cx, cy, synth.KITTI_BASELINE)[0] if stereo else None
    return img, synth.sensor_depth(Z, 1000.0, 30.0), right


def render(n, shape):
    from odometry_amd import synth
    if shape == "tum":
        poses = synth.trajectory(n, 0, fwd_range=(0.1, 0.2), max_offset=1.0)
        geo = (synth.TUM_ROWS, synth.TUM_COLS, synth.TUM_F, synth.TUM_CX, synth.TUM_CY, False)
    else:
        poses = synth.drive_trajectory("natural", n, 0)
        geo = (synth.KITTI_ROWS, synth.KITTI_COLS, synth.KITTI_F, synth.KITTI_CX, synth.KITTI_CY, True)
    with cf.ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        frames = list(ex.map(_render, [(T,) + geo for T in poses], chunksize=4))
    return dict(gray=[f[0] for f in frames], depth=[f[1] for f in frames], right=[f[2] for f in frames], rows=geo[0], cols=geo[1],
                K=geo[2:5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--modes", default="tum,kitti,stereo")
    args = ap.parse_args()
    from odometry_amd import api
    modes = args.modes.split(",")
    drives = {}
    if "tum" in modes:
        drives["tum"] = render(args.frames, "tum")
    if "kitti" in modes or "stereo" in modes:
        drives["kitti"] = render(args.frames, "kitti")
    trackers = {}
    for mode in modes:
        d = drives["tum" if mode == "tum" else "kitti"]
        if mode == "stereo":
            trk = api.Tracker(0)
            dev = [(trk.upload_frame(g), trk.upload_frame(r)) for g, r in zip(d["gray"], d["right"])]
        else:
            trk = api.RgbdTracker(0, depth_scale=1000.0, max_depth_step=0.05, rows=d["rows"], cols=d["cols"], K=d["K"])
            dev = [(trk.upload_frame(g), trk.upload_depth(r)) for g, r in zip(d["gray"], d["depth"])]
        trackers[mode] = (trk, dev)
    T = np.zeros(16, np.float32)
    A = np.zeros(16, np.float32)
    res = {m: [] for m in modes}
    jobs = {m: [] for m in modes}
    for run in range(args.runs):
        for mode in modes:
            trk, dev = trackers[mode]
            n = len(dev)
            order = [k % (2 * n - 2) for k in range(args.warmup + args.steps + 1)]
            order = [k if k < n else 2 * n - 2 - k for k in order]   # back and forth over the drive, as bench.py does
            _, djob0 = trk.depth_persistent_stats()
            trk.init(*dev[order[0]])
            kf = 0
            t0 = None
            for k in range(1, args.warmup + args.steps + 1):
                if k == args.warmup + 1:
                    trk._sync()
                    trk.timing()   # (resets the averages)
                    t0 = time.perf_counter()
                if k + 1 <= args.warmup + args.steps and k + 1 != args.warmup + 1:
                    trk.hint_next(*dev[order[k + 1]])
                kf += trk.track_into(*dev[order[k]], T, A)
            trk._sync()
            fps = args.steps / (time.perf_counter() - t0)
            tm = trk.timing()
            persist_on, djob1 = trk.depth_persistent_stats()
            res[mode].append(fps)
            jobs[mode].append(tm["depth_job_us"])
            print(json.dumps(dict(run=run, mode=mode, fps=round(fps, 1), keyframes=kf + 1, depth_job_us=round(tm["depth_job_us"], 1),
                                  depth_persistent_on=persist_on, depth_jobs_redone=djob1 - djob0, n_valid_last=trk.stats()["n_valid_depth"])),
                  flush=True)
    print(json.dumps(dict(summary=True, **{m: dict(median_fps=round(float(np.median(res[m])), 1),
                                                   spread=[round(min(res[m]), 1), round(max(res[m]), 1)],
                                                   median_depth_job_us=round(float(np.median(jobs[m])), 1)) for m in modes})))
    for trk, _ in trackers.values():
        trk.close()


if __name__ == "__main__":
    main()
