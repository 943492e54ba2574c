#!/usr/bin/env python
"""Event times of the mesh welder's six groups of launches and of their sum (odo_mesh_weld_time_dev), as tools/speckle_cost.py takes
the speckle filter's: medians of 5 batches of 20 repeats between two events on the context's stream. Within a pass each group is
repeated in place (a group repeated gives the same bytes: the tables are cleared inside the groups that fill them); a group's time
is summed over the passes.

    python tools/mesh_weld_cost.py [--out times.json] [--batches 5] [--reps 20]

Two meshes, at one grid and at eight:
  the drive mesh   DESIGN.md section 9.9's drive, which leaves its box, made on the device: a 112 x 64 x 56 volume at 0.1 m with a
                   mesh store follows the `natural` corridor for 30 frames; the mesh is the store in front of the final window's
                   mesh, as save_mesh_ply(spill=True) writes it. eps = voxel_size / 64, the origin the volume's.
  one cell         the same vertex and triangle counts with every vertex in one cell: one slot of the vertex table, every thread
                   contending for it; every triangle becomes degenerate. The worst case for contention.
Beside each group the bytes it moves at least (the arrays it reads and writes, the table clears included) and the time those would
take at 6.3 TB/s, the rate a streaming kernel reaches here."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.3
DRIVE = dict(frames=30, size=(120, 160), fwd_range=(0.45, 0.7), dims=(112, 64, 56), vs=0.1, origin=(-5.6, -3.23, 3.0), mu=0.3,
             max_depth=8.0, focus=5.8, threshold=10)


def median(runs):
    return {k: sorted(r[k] for r in runs)[len(runs) // 2] for k in runs[0]}


def group_bytes(n_v, n_t, vslots, tslots, colour=False):
    """The least bytes a pass's groups move for n_v vertices and n_t triangles in (the outputs counted as large as the inputs): the
    arrays each kernel reads and writes once, the clears of the tables and of the reference bytes; no probe beyond the first."""
    v = 36 if colour else 32
    return dict(vertex_table=12 * vslots + n_v * (16 + 8 + 4 + 4), representatives=n_v * (4 + 4 + 4),
                triangle_table=4 * tslots + n_t * (12 + 12 + 12 + 12 + 4 + 4), survivors=n_v + n_t * (4 + 4 + 12 + 3) + n_v * (4 + 1),
                scans=(n_v + n_t) // 256 * 12, scatters=n_v * (4 + 1 + 4 + 2 * v) + n_t * (12 + 4 + 4 + 12 + 12))


def drive_mesh(ctx):
    import numpy as np
    from odometry_amd import api, synth
    rows, cols = DRIVE["size"]
    K = (525.0 * cols / 640.0, (cols - 1) / 2.0, (rows - 1) / 2.0)
    scene = synth.drive_scene("natural", 0)
    poses = synth.trajectory(DRIVE["frames"], 0, fwd_range=DRIVE["fwd_range"], max_offset=1.0)
    vol = api.TsdfVolume(ctx, DRIVE["dims"], DRIVE["vs"], DRIVE["origin"], DRIVE["mu"], DRIVE["max_depth"], 65535, DRIVE["size"], K, 1000.0)
    vol.enable_spill_mesh(1 << 18, 1 << 18)
    vol.set_follow(DRIVE["focus"], DRIVE["threshold"])
    shifts = 0
    for T in poses:
        raw = synth.sensor_depth(scene.render(T, rows, cols, *K)[1], 1000.0, 30.0)
        shifts += vol.follow(T) != (0, 0, 0)
        vol.integrate(raw, T)
    store, win = vol.spilled_mesh(), vol.mesh()
    vol.close()
    mesh = (np.concatenate([store[0], win[0]]), np.concatenate([store[1], win[1]]),
            np.concatenate([store[2], win[2] + len(store[0])]).astype(np.int32))
    return mesh, shifts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    from odometry_amd import api
    ctx = api.Context(0)
    results = []
    (xyz0, nrmw, tri), shifts = drive_mesh(ctx)
    n_v, n_t = len(xyz0), len(tri)
    eps, origin = np.float32(DRIVE["vs"]) / np.float32(64.0), DRIVE["origin"]
    print(f"the drive mesh: {shifts} shifts, {n_v} vertices, {n_t} triangles")
    one = xyz0.copy()
    one[:, :3] = np.asarray(origin, np.float32) + np.float32(0.25) * eps
    w = api.MeshWeld(ctx, n_v, n_t)
    slots = [2, 2]
    for k, n in enumerate((n_v, n_t)):
        while slots[k] < 2 * n:
            slots[k] *= 2
    d_n, d_t = ctx.upload(nrmw), ctx.upload(tri)
    for what, pos in (("the drive mesh", xyz0), ("one cell", one)):
        d_x = ctx.upload(pos)
        for grids in (1, 8):
            us = median([w.time(n_v, n_t, d_x, d_n, d_t, eps=eps, origin=origin, grids=grids, reps=args.reps) for _ in range(args.batches)])
            stats = w.stats()
            assert stats["guard"] == 0 and stats["passes"] == grids, stats
            floor = {k: 1e-6 * b / STREAM_TBS for k, b in group_bytes(n_v, n_t, *slots).items()}     # microseconds of the FIRST pass
            results.append(dict(what=what, grids=grids, vertices=n_v, triangles=n_t, us=us, first_pass_stream_us=floor, **stats))
            print(f"{what}, grids {grids}: " + ", ".join(f"{k} {v:.1f}" for k, v in us.items()) + " us; a pass's bytes at "
                  f"{STREAM_TBS} TB/s: " + ", ".join(f"{k} {v:.1f}" for k, v in floor.items()) + f" us; {stats}")
        ctx.free(d_x)
    w.close()
    ctx.free(d_n)
    ctx.free(d_t)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1, default=float)
    ctx.close()


if __name__ == "__main__":
    main()
