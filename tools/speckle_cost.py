#!/usr/bin/env python
"""Event times of the speckle filter's four kernels and of the whole filter (odo_speckle_time_dev), as tools/stereo_depth_cost.py
takes the matcher's: medians of 5 batches of 20 repeats between two events on the context's stream. A kernel's time is the difference
of two prefixes of the run (label; label + seams; ...), because only a prefix can be repeated: the label launch rewrites the planes
that the others build on.

    python tools/speckle_cost.py [--out times.json] [--batches 5] [--reps 20]

Two key frames, both the matcher's own q frame, made on the device: synth.integer_disparity_pair at 376 x 1241 (the matcher's
defaults, 128 candidates, A = 2: the shape of its measured 481 us per pair) and the rendered `natural` pair
of the tests at 188 x 620 (63 candidates). The filter runs at max_diff 8, min_size 200. Beside the filter the matcher's own three
kernels are timed on the same visit."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MATCHER_US_9_16 = 481.0   # a pair at 376 x 1241, A = 2, 128 candidates


def median(runs):
    return {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-diff", type=int, default=8)
    ap.add_argument("--min-size", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    from odometry_amd import api, synth
    ctx = api.Context(0)
    results = []

    def measure(what, left, right, fx, max_disp):
        rows, cols = left.shape
        dl, dr = ctx.upload(np.asarray(left, np.float32)), ctx.upload(np.asarray(right, np.float32))
        sd = api.StereoDepth(ctx, (rows, cols), fx, synth.KITTI_BASELINE, min_disp=1, max_disp=max_disp)
        match = median([sd.time(dl, dr, reps=args.reps) for _ in range(args.batches)])
        depth = sd.run(dl, dr)
        q_host = sd.disparity()
        q, a = ctx.upload(q_host), ctx.upload(q_host)                    # the key, the matcher's q frame, stays unfiltered: every batch sees it
        flt = api.SpeckleFilter(ctx, (rows, cols), args.max_diff, args.min_size)
        us = median([flt.time(q, a, depth, reps=args.reps) for _ in range(args.batches)])
        stats = flt.stats()
        pair = sum(match.values())
        results.append(dict(what=what, rows=rows, cols=cols, max_disp=max_disp, us=us, matcher_us=match, matcher_pair_us=pair, **stats))
        print(f"{what} {rows} x {cols}: label {us['label']:.1f} us, seams {us['seams']:.1f}, count {us['count']:.1f}, apply {us['apply']:.1f}; "
              f"the filter {us['run']:.1f} us beside the matcher's {pair:.1f} us on this visit"
              + (f" ({MATCHER_US_9_16:.0f} in section 9.16)" if (rows, cols, max_disp) == (synth.KITTI_ROWS, synth.KITTI_COLS, 128) else "")
              + f"; {stats}")
        assert stats["guard"] == 0, stats
        flt.close()
        sd.close()
        for p in (dl, dr, q, a):
            ctx.free(p)

    left, right, _ = synth.integer_disparity_pair(seed=0, rows=synth.KITTI_ROWS, cols=synth.KITTI_COLS)
    measure("integer disparity pair", left, right, synth.KITTI_F, 128)
    scene = synth.drive_scene("natural", 0)
    T = synth.drive_trajectory("natural", 1, 0)[0]
    f, cx, cy = synth.KITTI_F / 2, synth.KITTI_CX / 2, synth.KITTI_CY / 2
    left, _ = scene.render(T, 188, 620, f, cx, cy, 0.0)
    right, _ = scene.render(T, 188, 620, f, cx, cy, synth.KITTI_BASELINE)
    measure("rendered natural pair", left, right, f, 63)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
