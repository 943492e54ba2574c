"""What an attached keyframe map (odo_tracker_attach_map) costs the headline drive: bench.py's tracked loop (natural drive, next
pair announced with hint_next), timed with and without a map, interleaved run by run. Prints frames/s per mode (median, spread),
the map's size and counters, and the persistent launches' redo counts (pose LM: Solves redone on the step launches; depth LM:
jobs run again), which would show whether the short insertion kernels on the shared CUs disturb the co-resident launches.

  python tools/map_cost.py [--runs 10] [--steps 200] [--warmup 20] [--frames 200] [--voxel 0.05] [--capacity 4000000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--voxel", type=float, default=0.05)
    ap.add_argument("--capacity", type=int, default=4_000_000)
    args = ap.parse_args()
    import bench
    from odometry_amd import api
    seq = bench.render_sequence(args.frames, 0, min(8, os.cpu_count() or 1), drive="natural")
    trk = api.Tracker(0)
    dev = [(trk.upload_frame(l), trk.upload_frame(r)) for l, r in zip(seq["left"], seq["right"])]
    m = api.PointMap(trk, 376, 1241, args.capacity, args.voxel)
    n = len(dev)
    order = [k % (2 * n - 2) for k in range(args.warmup + args.steps + 1)]
    order = [k if k < n else 2 * n - 2 - k for k in order]   # back and forth over the drive, as bench.py does
    T = np.zeros(16, np.float32)
    A = np.zeros(16, np.float32)
    res = {"off": [], "on": []}
    info = {}
    for run in range(2 * args.runs):
        mode = "on" if run % 2 else "off"
        if mode == "on":
            m.clear()
            trk.attach_map(m)
        pk0, redo0 = trk.persistent_stats()
        _, djob0 = trk.depth_persistent_stats()
        trk.init(*dev[order[0]])
        kf = 0
        t0 = None
        for k in range(1, args.warmup + args.steps + 1):
            if k == args.warmup + 1:
                trk._sync()
                t0 = time.perf_counter()
            if k + 1 <= args.warmup + args.steps and k + 1 != args.warmup + 1:
                trk.hint_next(*dev[order[k + 1]])
            kf += trk.track_into(*dev[order[k]], T, A)
        trk._sync()
        fps = args.steps / (time.perf_counter() - t0)
        res[mode].append(fps)
        _, redo1 = trk.persistent_stats()
        _, djob1 = trk.depth_persistent_stats()
        row = dict(run=run, mode=mode, fps=round(fps, 1), keyframes=kf + 1, lm_redone=redo1 - redo0, depth_redone=djob1 - djob0)
        if mode == "on":
            trk.attach_map(None)
            row["map"] = m.stats()
            info = row["map"]
        print(json.dumps(row), flush=True)
    med = {k: float(np.median(v)) for k, v in res.items()}
    print(json.dumps(dict(summary=True, median_fps_off=round(med["off"], 1), median_fps_on=round(med["on"], 1),
                          spread_off=[round(min(res["off"]), 1), round(max(res["off"]), 1)],
                          spread_on=[round(min(res["on"]), 1), round(max(res["on"]), 1)],
                          on_vs_off=round(med["on"] / med["off"] - 1.0, 4), last_map=info)))
    m.close()
    trk.close()


if __name__ == "__main__":
    main()
