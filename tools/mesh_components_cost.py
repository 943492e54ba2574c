#!/usr/bin/env python
"""Event times of the mesh component filter's six groups of launches and of their sum (odo_mesh_components_time_dev), as
tools/mesh_weld_cost.py takes the welder's: medians of 5 batches of 20 repeats between two events on the context's stream. Each group
is repeated in place (a group repeated gives the same bytes: the unions start from parent[i] = i, the sizes are zeroed by the launch
that flattens, the edge table is cleared inside its group).

    python tools/mesh_components_cost.py [--out times.json] [--batches 5] [--reps 20]

Two meshes, each with and without edge statistics:
  the drive's welded mesh   tools/mesh_weld_cost.py's drive mesh, made on the device, welded on the device at eight grids; the filter
                            reads the welder's result where it lies. min_triangles = 128.
  one fan                   the same vertex and triangle counts with every triangle (0, i, i + 1): one component whose every union
                            meets vertex 0, one size word, 2 n_t edges at vertex 0. The worst case for contention.
Beside each group the bytes it moves at least (the arrays it reads and writes, the clears included) and the time those would take at
6.3 TB/s, the rate a streaming kernel reaches here."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STREAM_TBS = 6.3


def median(runs):
    return {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}


def group_bytes(n_v, n_t, eslots):
    """The least bytes the groups move for n_v vertices and n_t triangles in (the outputs counted as large as the inputs): the arrays
    each kernel reads and writes once, the clears of the edge table and of the reference bytes; no walk or probe beyond the first
    word."""
    return dict(union=n_v * 4 + n_t * (12 + 3 * 4), sizes=n_v * (4 + 4 + 4) + n_t * (12 + 4 + 4) + n_v * (4 + 4),
                edges=12 * eslots + n_t * (12 + 3 * 12) + eslots * (12 + 4), survivors=n_v + n_t * (4 + 4 + 12 + 3) + n_v * (4 + 4 + 1),
                scans=(n_v + n_t) // 256 * 12, scatters=n_v * (4 + 4 + 1 + 4 + 2 * 32) + n_t * (4 + 4 + 12 + 12 + 12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    from mesh_weld_cost import DRIVE, drive_mesh
    from odometry_amd import api
    ctx = api.Context(0)
    results = []
    (xyz0, nrmw, tri), shifts = drive_mesh(ctx)
    d_in = [ctx.upload(a) for a in (xyz0, nrmw, tri)]
    w = api.MeshWeld(ctx, len(xyz0), len(tri))
    w.run_dev(len(xyz0), len(tri), *d_in, eps=np.float32(DRIVE["vs"]) / np.float32(64.0), origin=DRIVE["origin"], grids=8)
    x, n, _, t, n_v, n_t = w.result_dev()
    print(f"the drive mesh: {shifts} shifts, {len(xyz0)} vertices, {len(tri)} triangles; welded at eight grids: {n_v} vertices, {n_t} triangles")
    i = np.arange(n_t, dtype=np.int64) % (n_v - 2)
    d_fan = ctx.upload(np.stack([np.zeros(n_t, np.int64), 1 + i, 2 + i], 1).astype(np.int32))
    eslots = 2
    while eslots < 6 * n_t:
        eslots *= 2
    for edge_stats in (True, False):
        f = api.MeshComponents(ctx, n_v, n_t, edge_stats=edge_stats)
        for what, d_tri in (("the drive's welded mesh", t), ("one fan", d_fan)):
            us = median([f.time(n_v, n_t, x, n, d_tri, min_triangles=128, reps=args.reps) for _ in range(args.batches)])
            stats = f.stats()
            assert stats["guard"] == 0, stats
            floor = {k: 1e-6 * b / STREAM_TBS for k, b in group_bytes(n_v, n_t, eslots if edge_stats else 0).items()}
            results.append(dict(what=what, edge_stats=edge_stats, vertices=n_v, triangles=n_t, us=us, stream_us=floor, **stats))
            print(f"{what}, edge_stats {int(edge_stats)}: " + ", ".join(f"{k} {v:.1f}" for k, v in us.items()) + f" us; the bytes at {STREAM_TBS} TB/s: " +
                  ", ".join(f"{k} {v:.1f}" for k, v in floor.items()) + f" us; {stats}")
        f.close()
    w.close()
    for d in d_in + [d_fan]:
        ctx.free(d)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1, default=float)
    ctx.close()


if __name__ == "__main__":
    main()
