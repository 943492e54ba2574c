#!/usr/bin/env python
"""Event times of the dense stereo matcher's semi-global mode (odo_stereo_depth_sgm_time_dev), as tools/stereo_depth_cost.py takes
the box matcher's: medians of 5 batches of 20 repetitions of each of the five groups (census, cost, all path launches of one run,
right selection, left selection) between two events on the context's stream, at 376 x 1241, A = 2, for 64 / 128 / 255 candidates
(dmin = 1) and 4 / 8 paths, and the box matcher's three kernels on the same frames in the same process as the yardstick. Beside the
path group's time the least its traffic could take: per direction every admissible entry of C is read and every one of S written,
and all but the first direction read S as well, 2 bytes each, at 6.3 TB/s (the HBM rate a streaming kernel reaches on this chip).

    python tools/stereo_sgm_cost.py [--out times.json] [--batches 5] [--reps 20]

The pair is synth.integer_disparity_pair at 376 x 1241, as in tools/stereo_depth_cost.py: the work depends on the frame's size, the
candidates and the paths alone, not on what the images show."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_SECOND = 6.3e12


def admissible(rows, cols, A, dmin, dmax):
    """Admissible (pixel, candidate) pairs of a frame: the entries of C and S that the path launches touch."""
    x = np.arange(cols)
    per_row = np.clip(np.minimum(dmax, x - A - 4) - dmin + 1, 0, None)[(x >= A + 4) & (x < cols - A - 4)].sum()
    return int(per_row) * max(rows - 2 * (A + 3), 0)


def path_bytes(entries, paths):
    return 2 * entries * (paths + paths + paths - 1)


def median(runs):
    return {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--agg-radius", type=int, default=2)
    args = ap.parse_args()
    from odometry_amd import api, synth
    rows, cols, A = synth.KITTI_ROWS, synth.KITTI_COLS, args.agg_radius
    left, right, _ = synth.integer_disparity_pair(seed=0, rows=rows, cols=cols)
    ctx = api.Context(0)
    dl, dr, out = ctx.upload(left), ctx.upload(right), ctx.alloc(2 * rows * cols)
    results = []
    for dmax in (64, 128, 255):
        sd = api.StereoDepth(ctx, (rows, cols), synth.KITTI_F, synth.KITTI_BASELINE, min_disp=1, max_disp=dmax, agg_radius=A)
        box = median([sd.time(dl, dr, out, reps=args.reps) for _ in range(args.batches)])
        box_total, box_stats = sum(box.values()), sd.stats()
        entries = admissible(rows, cols, A, 1, dmax)
        for paths in (4, 8):
            sd.enable_sgm(paths=paths)
            us = median([sd.sgm_time(dl, dr, out, reps=args.reps) for _ in range(args.batches)])
            total, stats = sum(us.values()), sd.stats()
            floor = path_bytes(entries, paths) / HBM_BYTES_PER_SECOND * 1e6
            results.append(dict(rows=rows, cols=cols, agg_radius=A, candidates=dmax, paths=paths, us=us, us_total=total, box_us=box,
                                box_us_total=box_total, ratio=total / box_total, admissible_entries=entries,
                                path_bytes=path_bytes(entries, paths), path_us_at_hbm_rate=floor, volume_bytes=4 * rows * cols * dmax,
                                matched=stats["matched"], box_matched=box_stats["matched"], interior=stats["interior"]))
            print(f"{rows} x {cols}  A = {A}  {dmax:3d} candidates  {paths} paths: " + "  ".join(f"{k} {v:7.1f}" for k, v in us.items())
                  + f"  total {total:8.1f} us   box {box_total:7.1f} us   ratio {total / box_total:5.2f}   paths move "
                  f"{path_bytes(entries, paths) / 1e9:5.2f} GB = {floor:6.1f} us at the HBM rate ({us['paths'] / floor:4.1f} x)   "
                  f"matched {stats['matched']} (box {box_stats['matched']}) of {stats['interior']}")
        sd.close()
    for p in (dl, dr, out):
        ctx.free(p)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
