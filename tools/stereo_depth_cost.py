#!/usr/bin/env python
"""Event times of the dense stereo matcher's three kernels (odo_stereo_depth_time_dev), as tools/depth_filter_cost.py takes the
depth filter's: medians of 5 batches of 20 launches of each kernel between two events on the context's stream, at 376 x 1241, for
A = 0 .. 3 and 64 / 128 / 255 candidates (dmin = 1). Beside each time the arithmetic's estimate: a candidate of a pixel costs
(2A + 1)^2 taps of about 5 vector instructions (two XORs, two population counts with their adds, the LDS read's share) and about 12
for the walk's step; a match launch is that times the pixels and candidates it walks, spread over 256 CUs x 64 lanes at 2.4 GHz.

    python tools/stereo_depth_cost.py [--out times.json] [--batches 5] [--reps 20]

The pair is synth.integer_disparity_pair at 376 x 1241 (bands of integer disparity 3 .. 96): the walk's length depends on the frame's
size and the candidates alone, not on what the images show."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LANES_PER_SECOND = 256 * 64 * 2.4e9
TAP_INSTRUCTIONS, STEP_INSTRUCTIONS = 5, 12


def walked(rows, cols, A, dmin, dmax):
    """(left, right): pixel-candidates a match launch walks — per interior row, the admissible candidates of every column."""
    x = np.arange(cols)
    left = np.clip(np.minimum(dmax, x - A - 4) - dmin + 1, 0, None)[(x >= A + 4) & (x < cols - A - 4)].sum()
    right = np.clip(np.minimum(dmax, cols - A - 5 - x) - dmin + 1, 0, None)[x >= A + 4].sum()
    n_rows = max(rows - 2 * (A + 3), 0)
    return int(left) * n_rows, int(right) * n_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from odometry_amd import api, synth
    rows, cols = synth.KITTI_ROWS, synth.KITTI_COLS
    left, right, _ = synth.integer_disparity_pair(seed=0, rows=rows, cols=cols)
    ctx = api.Context(0)
    dl, dr, out = ctx.upload(left), ctx.upload(right), ctx.alloc(2 * rows * cols)
    results = []
    for A in (0, 1, 2, 3):
        for dmax in (64, 128, 255):
            sd = api.StereoDepth(ctx, (rows, cols), synth.KITTI_F, synth.KITTI_BASELINE, min_disp=1, max_disp=dmax, agg_radius=A)
            runs = [sd.time(dl, dr, out, reps=args.reps) for _ in range(args.batches)]
            med = {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}
            per = (2 * A + 1) ** 2 * TAP_INSTRUCTIONS + STEP_INSTRUCTIONS
            wl, wr = walked(rows, cols, A, 1, dmax)
            est = dict(left=wl * per / LANES_PER_SECOND * 1e6, right=wr * per / LANES_PER_SECOND * 1e6)
            stats = sd.stats()
            results.append(dict(rows=rows, cols=cols, agg_radius=A, candidates=dmax, us=med, instructions_per_candidate=per,
                                instructions_per_pixel=per * dmax, walked_left=wl, walked_right=wr, us_estimate=est, **stats))
            print(f"{rows} x {cols}  A = {A}  {dmax:3d} candidates: census {med['census']:6.1f} us   right {med['match_right']:8.1f} us "
                  f"(arithmetic {est['right']:7.1f})   left {med['match_left']:8.1f} us (arithmetic {est['left']:7.1f})   "
                  f"{per * dmax:6d} instructions / pixel   matched {stats['matched']} of {stats['interior']}")
            sd.close()
    for p in (dl, dr, out):
        ctx.free(p)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
