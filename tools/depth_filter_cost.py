#!/usr/bin/env python
"""Event times of the bilateral depth filter's kernel (odo_depth_filter_time_dev), as tools/volume_cost.py takes the volume's: medians
of 7 batches of 50 launches between two events on the context's stream, at 480 x 640 and 120 x 160, for R = 1 .. 4, the default
tables. Beside each time its work: 4 B of traffic per pixel (one uint16 read, one written; the halo is re-read out of cache) and
(2R + 1)^2 taps per pixel.

    python tools/depth_filter_cost.py [--out times.json] [--batches 7] [--reps 50]

The frame is a slanted wall with a step across it, between 1 and 4 m, under the Kinect axial noise model, 2 % holes."""
import argparse
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def frame(size):
    from odometry_amd import synth
    rows, cols = size
    y, x = np.mgrid[0:rows, 0:cols]
    Z = 1.0 + 2.5 * x / cols + 0.3 * y / rows + 0.5 * (x > cols // 2)
    rng = np.random.default_rng(11)
    raw = synth.sensor_depth(synth.sensor_noise(Z, rng), 1000.0, 30.0)
    raw[rng.random(size) < 0.02] = 0
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    from odometry_amd import api
    header = open(os.path.join(os.path.dirname(os.path.abspath(api.__file__)), "csrc", "depth_filter.hip.h")).read()
    tile_w, tile_h = (int(re.search(r"constexpr int " + k + r" = (\d+);", header).group(1)) for k in ("kDfTileW", "kDfTileH"))
    ctx = api.Context(0)
    results = []
    for size in ((480, 640), (120, 160)):
        raw = frame(size)
        src = ctx.upload(raw)
        dst = ctx.alloc(raw.nbytes)
        for R in (1, 2, 3, 4):
            flt = api.DepthFilter(ctx, size, radius=R)
            us = sorted(flt.time(src, dst, reps=args.reps) for _ in range(args.batches))
            med = us[len(us) // 2]
            stats = flt.stats()
            pixels, taps = size[0] * size[1], (2 * R + 1) ** 2
            row = dict(rows=size[0], cols=size[1], radius=R, us_median=med, us_min=us[0], us_max=us[-1], bytes=4 * pixels,
                       gb_per_s=4 * pixels / med * 1e-3, taps_per_pixel=taps, gtaps_per_s=pixels * taps / med * 1e-3,
                       workgroups=-(-size[0] // tile_h) * -(-size[1] // tile_w), **stats)
            results.append(row)
            print(f"{size[0]} x {size[1]}  R = {R}: {med:7.2f} us ({us[0]:.2f} - {us[-1]:.2f})   {4 * pixels / 1e3:7.1f} KB -> "
                  f"{row['gb_per_s']:7.1f} GB/s   {taps:2d} taps / pixel -> {row['gtaps_per_s']:6.1f} Gtap/s   "
                  f"{row['workgroups']} workgroups   changed {stats['n_changed']} of {stats['n_valid']}")
            flt.close()
        ctx.free(src)
        ctx.free(dst)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
