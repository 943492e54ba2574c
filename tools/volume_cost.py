"""What the TSDF volume (odo_volume_*) costs.

  kernels   the workload for a kernel trace: the first frames of the TUM-shaped RGB-D drive integrated with their true poses into the
            pinned grid (240 x 128 x 200 voxels of 4 cm, 24.6 MB: resident in the Infinity Cache) and into a 512 x 256 x 512 grid of
            the same voxel size (268 MB: it is not), each followed by extractions and meshes (api.TsdfVolume.mesh(): count + scan
            for the totals, then count + scan + vertices + triangles with exact capacities). Each grid is then done once more as a
            COLOURED volume (odo_volume_enable_colour): the same frames through integrate(colour=...) — volume_integrate_colour_kernel
            beside volume_integrate_kernel in one trace — followed by coloured extractions and meshes (one colour launch behind each).
            Every leg ends with ray-casts (api.TsdfVolume.raycast: one volume_raycast_kernel launch each) at 480 x 640 with the
            volume's K from the first and the last pose of the drive, t_min = 0, step = mu / 2, samples up to max_depth + mu; the
            coloured legs ask for the colour frame as well, and then time the ray-cast with its colour frame under both sampling
            modes of odo_volume_set_colour_sampling (volume_raycast_kernel and volume_raycast_interp_kernel), alternating in the one
            call: medians over `runs` batches of `reps` launches between two events (api.TsdfVolume.raycast_time), in the line's
            `raycast_colour_us`.
            Run it under the profiler, in a run of its own (no counters in that run), then summarise:
              rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/volume_cost.py kernels
              python tools/volume_cost.py summary <dir>
            It prints one JSON line per grid with the counters the algorithmic bytes are made of; --json FILE keeps them for
            `summary` (without it `summary` prints the times alone).
  summary   medians of the volume's kernels per grid out of the trace, with the algorithmic bytes
              integrate = 8 B per updated voxel (load + store) + 2 B per depth pixel
              coloured  = the same + 8 B per in-band voxel (colour word load + store) + 3 B per in-band voxel (its pixel)
              colours   = extraction: 4 B per voxel (the ballots aside) + 20 B per point (two voxel words, two colour words, one
                          store); mesh: 5 B per voxel + 20 B per vertex
              extract   = 4 B per voxel + 32 B per point
              mesh      = count 4 + 1 B per voxel; vertices 1 + 4 B per voxel + 32 B per vertex; triangles 4 B per voxel + 12 B
                          per triangle
            and their share of the achievable HBM bandwidth (6.3 TB/s).
  track     tools/rgbd_cost.py's tracked loop over the TUM-shaped drive (next frame announced with its depth frame, back and forth
            over the drive) with no volume, the pinned grid and the large grid attached, runs interleaved mode by mode: frames/s
            (median, spread), the tracker's host timing, Solves redone on the step launches and depth jobs redone. Mode `coloured` is
            the pinned grid with a colour grid, every frame's colour named with odo_tracker_frame_colour (the price of colour:
            --modes coloured,pinned,none alternating in one call). Mode `follow` is the pinned grid with a spill store of 2^22 points
            and api.TsdfVolume.set_follow's defaults (focus max_depth / 2, threshold min(dims) // 8): the window moves with the
            camera; its lines carry `shifts`, the times the window moved during the timed frames (the window is read after every
            frame, a host call without a wait, in this mode only). `follow_none` is the same without a store and `follow_mesh`
            the same with a mesh store (2^22 vertices, 2^23 triangles) in place of the point store, `follow_reentry` with a
            re-entry store of 2^23 voxels in its place (the price of re-entry: --modes follow_none,follow_reentry alternating).

  icp       the frame-to-model alignment's two kernels timed with events (api.TsdfVolume.icp_time: `reps` launches of
            volume_icp_rows_kernel<29>, then of volume_icp_step_kernel<29>'s fold, each batch between two events on the volume's stream):
            the pinned grid after `frames` integrations at their true poses, the ray-cast from the last pose but one as the model
            frame, the last frame as the sensor frame, at 480 x 640 and strides 4, 2 and 1. One JSON line per stride with the medians
            over `runs` batches, the pairs and the blocks, then the wall time of whole api.TsdfVolume.track calls (ray-cast, the
            alignment's launches, its allocations and its one wait). With --photo the volume has a colour grid (every frame fused
            with its grey replicated into R, G and B), the ray-cast includes the colours, and each line carries the two kernels of
            the alignment with the photometric term (api.TsdfVolume.icp_photo_time: volume_icp_rows_kernel<31> and
            volume_icp_step_kernel<31>, the same templates instantiated for 31 sums) beside the geometric two, timed in alternating
            batches of the same call; the last line gives the wall time of track(grey=...) beside the geometric track's.
            --sampling nearest | trilinear | both sets the colour sampling of the model frame for those whole track(grey=...) calls
            (both: the two modes alternating in the same loop, a line for each).

  shift     the moving volume's launches timed with events (api.TsdfVolume.shift_time: batches of `reps` between two events on the
            volume's stream, the shift not applied): the pinned and the large grid after `frames` integrations at their true poses,
            without and with a colour grid, each with a spill store, for a one-layer shift d = (0, 0, 1) and a quarter-grid shift
            d = (0, 0, nz / 4). One JSON line per case with the medians over `runs` batches of the shift, of a device-to-device
            hipMemcpyAsync of the same bytes, of a hipMemsetAsync of the same bytes, and of the spill's count, scan and scatter,
            with the bytes moved and the points that shift spills.
            --mesh: each volume has both stores; a one-layer shift on each axis, the quarter-grid shift and a whole-grid shift
            (d = (0, 0, nz): every voxel is near the slab, the mesh's whole work through the spill's kernels); one line per case with
            the mesh spill's five stages (api.TsdfVolume.spill_mesh_time) beside the shift and the point spill's three stages from
            alternating batches, then the counts each shift really spills.
            --reentry: each volume has a point store and a re-entry store that holds 0, 10^5, 10^6 or 10^7 live entries (whole grids
            of observed voxels pushed out of the window first); one line per case with the re-entry store's five stages
            (api.TsdfVolume.reentry_time: save count, save scan, save scatter, the store pass, advance) beside the shift and the
            point spill's three stages from alternating batches, then what each shift really saves and its way back restores.

  python tools/volume_cost.py kernels [--frames 10] [--extractions 3] [--runs 7] [--reps 20] [--json FILE]
  python tools/volume_cost.py icp [--frames 10] [--runs 7] [--reps 50] [--photo [--sampling nearest|trilinear|both]]
  python tools/volume_cost.py shift [--frames 10] [--runs 7] [--reps 20] [--mesh | --reentry]
  python tools/volume_cost.py summary DIR [--json FILE]
  python tools/volume_cost.py track [--runs 3] [--steps 200] [--warmup 20] [--frames 100]
                                    [--modes none,pinned,large[,coloured][,follow][,follow_none][,follow_mesh][,follow_reentry]]

A build without the volume is measured with tools/rgbd_cost.py --modes tum (the same drive and loop as `track`'s mode `none`).
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 6.3e12   # achievable, not peak (the micro-architecture notes)
VS, MU, MAX_DEPTH = 0.04, 0.12, 8.0
GRIDS = dict(pinned=dict(dims=(240, 128, 200), origin=(-4.8, -3.3, 0.4)),
             large=dict(dims=(512, 256, 512), origin=(-10.24, -5.86, 0.4)))   # the same corridor, the same voxel size


def make_volume(owner, grid, size, K, colour=False):
    from odometry_amd import api
    g = GRIDS["pinned" if grid == "coloured" or grid.startswith("follow") else grid]
    vol = api.TsdfVolume(owner, g["dims"], VS, g["origin"], MU, MAX_DEPTH, 65535, size, K, 1000.0)
    if colour or grid == "coloured":
        vol.enable_colour(3, False, 255)
    if grid == "follow":
        vol.enable_spill(1 << 22)
    if grid == "follow_mesh":
        vol.enable_spill_mesh(1 << 22, 1 << 23)
    if grid == "follow_reentry":
        vol.enable_reentry(1 << 23)
    if grid.startswith("follow"):
        vol.set_follow(MAX_DEPTH / 2, min(g["dims"]) // 8)
    return vol


def kernels(args):
    from odometry_amd import api, synth
    seq = synth.make_rgbd_sequence(args.frames, seed=0)
    K = (seq["K"]["f0"], seq["K"]["cx0"], seq["K"]["cy0"])
    ctx = api.Context(0)
    dev = [ctx.upload(d) for d in seq["depth"]]
    cdev = [ctx.upload(synth.colour_from_gray(g, 3, False, tint_seed=1)) for g in seq["gray"]]
    out = {}
    for grid in ("pinned", "large"):
        for coloured in (False, True):    # the plain leg, then the same grid and frames as a coloured volume
            vol = make_volume(ctx, grid, (synth.TUM_ROWS, synth.TUM_COLS), K, colour=coloured)
            upd, band = [], []
            for d, c, A in zip(dev, cdev, seq["poses"]):
                vol.integrate(d, A, colour=c if coloured else None)
                st = vol.stats()
                upd.append(st["updated"])
                band.append(st["in_band"])
            t0 = time.perf_counter()
            for d, c, A in zip(dev, cdev, seq["poses"]):    # once more without a host wait between the frames (weights differ, the work does not)
                vol.integrate(d, A, colour=c if coloured else None)
            vol.sync()
            host_us = 1e6 * (time.perf_counter() - t0) / len(dev)
            n = 0
            for _ in range(args.extractions):
                n = len(vol.extract(1 << 21, colour=coloured)[0])
            nv = nt = 0
            for _ in range(args.extractions):
                got = vol.mesh(colour=coloured)
                nv, nt = len(got[0]), len(got[2])
            hits = []
            for _ in range(args.extractions):
                for k in (0, len(seq["poses"]) - 1):
                    hits.append(int((vol.raycast(seq["poses"][k], step=MU / 2, raw=True, colour=coloured)[0] > 0).sum()))
            cast = {}
            if coloured:                      # the ray-cast with its colour frame under both sampling modes, alternating, between events
                for _ in range(args.runs):
                    for k in (0, len(seq["poses"]) - 1):
                        for m in api.TsdfVolume.COLOUR_SAMPLING:
                            vol.set_colour_sampling(m)
                            cast.setdefault(f"pose {k} {m}", []).append(vol.raycast_time(seq["poses"][k], step=MU / 2, colour=True, reps=args.reps))
                vol.set_colour_sampling("nearest")
                cast = {k: _med(v) for k, v in cast.items()}
            nx, ny, nz = GRIDS[grid]["dims"]
            row = dict(raycast_hits=hits[:2], voxels=nx * ny * nz, updated_per_frame=int(np.median(upd)), in_band_per_frame=int(np.median(band)), points=n,
                       vertices=nv, triangles=nt, pixels=synth.TUM_ROWS * synth.TUM_COLS, integrate_host_us_back_to_back=round(host_us, 1))
            if coloured:
                out[grid]["coloured_integrate_host_us_back_to_back"] = row["integrate_host_us_back_to_back"]
            else:
                out[grid] = row
            print(json.dumps(dict(grid=grid, coloured=coloured, **row, **({"raycast_colour_us": cast} if cast else {}))), flush=True)
            vol.close()
    for d in dev + cdev:
        ctx.free(d)
    ctx.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f)


def summary(args):
    work = json.load(open(args.json)) if args.json else None
    rows = []
    for f in glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("odo::", "")
        if name.startswith("volume_"):
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name in sorted(per):
        half = len(per[name]) // 2    # `kernels` does the same launches on the pinned grid first, then on the large one
        for which, d in (("pinned", per[name][:half]), ("large", per[name][half:])):
            d = np.array(d)
            line = f"{name:26s} {which:7s} n={len(d):3d}  median {np.median(d):8.2f} us  min {d.min():8.2f}  max {d.max():8.2f}"
            if work and which in work:
                w = work[which]
                b = None
                if name == "volume_integrate_kernel":
                    b = 8 * w["updated_per_frame"] + 2 * w["pixels"]
                elif name == "volume_integrate_colour_kernel":
                    b = 8 * w["updated_per_frame"] + 2 * w["pixels"] + 11 * w.get("in_band_per_frame", 0)
                elif name == "volume_extract_colour_kernel":
                    b = 4 * w["voxels"] + 20 * w["points"]
                elif name == "volume_mesh_colour_kernel" and "vertices" in w:
                    b = 5 * w["voxels"] + 20 * w["vertices"]
                elif name == "volume_count_kernel":
                    b = 4 * w["voxels"]
                elif name == "volume_scatter_kernel":
                    b = 32 * w["points"]
                elif name == "volume_mesh_count_kernel":
                    b = 5 * w["voxels"]
                elif name == "volume_mesh_vertex_kernel" and "vertices" in w:
                    b = 5 * w["voxels"] + 32 * w["vertices"]
                elif name == "volume_mesh_triangle_kernel" and "triangles" in w:
                    b = 4 * w["voxels"] + 12 * w["triangles"]
                if b is not None:
                    bw = b / (np.median(d) * 1e-6)
                    line += f"  algorithmic {b / 1e6:8.2f} MB -> {bw / 1e12:5.2f} TB/s = {100 * bw / HBM_BYTES_PER_S:5.1f} % of 6.3 TB/s"
            print(line)


def track(args):
    import rgbd_cost
    from odometry_amd import api, synth
    modes = args.modes.split(",")
    d = rgbd_cost.render(args.frames, "tum")
    trk = api.RgbdTracker(0, depth_scale=1000.0, max_depth_step=0.05, rows=d["rows"], cols=d["cols"], K=d["K"])
    dev = [(trk.upload_frame(g), trk.upload_depth(r)) for g, r in zip(d["gray"], d["depth"])]
    vols = {m: make_volume(trk, m, (d["rows"], d["cols"]), d["K"]) for m in modes if m != "none"}
    cdev = [trk.upload_colour(synth.colour_from_gray(g, 3, False, tint_seed=1)) for g in d["gray"]] if "coloured" in modes else None
    T = np.zeros(16, np.float32)
    A = np.zeros(16, np.float32)
    res = {m: [] for m in modes}
    n = len(dev)
    last = args.warmup + args.steps
    order = [k % (2 * n - 2) for k in range(last + 1)]
    order = [k if k < n else 2 * n - 2 - k for k in order]   # back and forth over the drive, as bench.py does
    for run in range(args.runs):
        for mode in modes:
            vol = vols.get(mode)
            if vol is not None:
                vol.clear()
            trk.attach_volume(vol)
            _, djob0 = trk.depth_persistent_stats()
            _, redo0 = trk.persistent_stats()
            coloured = mode == "coloured"
            if coloured:
                trk.frame_colour(cdev[order[0]])
            trk.init(*dev[order[0]])
            kf = shifts = 0
            t0 = None
            win = vol.window()[0] if mode.startswith("follow") else None
            for k in range(1, last + 1):
                if k == args.warmup + 1:
                    trk._sync()
                    trk.timing()   # (resets the averages)
                    t0 = time.perf_counter()
                if k + 1 <= last and k + 1 != args.warmup + 1:
                    trk.hint_next(*dev[order[k + 1]])
                if coloured:
                    trk.frame_colour(cdev[order[k]])
                kf += trk.track_into(*dev[order[k]], T, A)
                if win is not None:
                    now = vol.window()[0]
                    shifts += t0 is not None and now != win
                    win = now
            trk._sync()            # (waits for the pending integrations as well)
            fps = args.steps / (time.perf_counter() - t0)
            tm = trk.timing()
            _, djob1 = trk.depth_persistent_stats()
            groups, redo1 = trk.persistent_stats()
            res[mode].append(fps)
            st = vol.stats() if vol is not None else {}
            if mode.startswith("follow"):
                st = dict(st, shifts=int(shifts), window=list(win))
            if mode == "follow":
                st = dict(st, spilled=len(vol.spilled(clear=True)[0]))
            if mode == "follow_mesh":
                got = vol.spilled_mesh(clear=True, with_dropped=True)
                st = dict(st, spilled_vertices=len(got[0]), spilled_triangles=len(got[2]), spilled_dropped=list(got[3]))
            if mode == "follow_reentry":
                st = dict(st, reentry=vol.reentry_stats())
            print(json.dumps(dict(run=run, mode=mode, fps=round(fps, 1), keyframes=kf + 1, lm_persistent_groups=groups,
                                  solves_redone=redo1 - redo0, depth_jobs_redone=djob1 - djob0, frames_integrated=st.get("frames"),
                                  updated_last=st.get("updated"), in_band_last=st.get("in_band"),
                                  **{k_: st[k_] for k_ in ("shifts", "window", "spilled", "spilled_vertices", "spilled_triangles", "spilled_dropped", "reentry") if k_ in st}, **{k_: round(v, 1) for k_, v in tm.items()})), flush=True)
    trk.attach_volume(None)
    print(json.dumps(dict(summary=True, **{m: dict(median_fps=round(float(np.median(res[m])), 1),
                                                   spread=[round(min(res[m]), 1), round(max(res[m]), 1)]) for m in modes})))
    for v in vols.values():
        v.close()
    trk.close()


def icp(args):
    from odometry_amd import api, synth
    seq = synth.make_rgbd_sequence(args.frames, seed=0)
    K = (seq["K"]["f0"], seq["K"]["cx0"], seq["K"]["cy0"])
    ctx = api.Context(0)
    vol = make_volume(ctx, "pinned", (synth.TUM_ROWS, synth.TUM_COLS), K)
    for d, A in zip(seq["depth"][:-1], seq["poses"][:-1]):
        vol.integrate(d, A)
    P_m = seq["poses"][-2]
    depth, nrmw = vol.raycast(P_m)
    raw = seq["depth"][-1]
    for stride in (4, 2, 1):
        acc = vol.icp_eval(raw, depth, nrmw, P_m, np.eye(4), stride=stride)
        us = np.array([vol.icp_time(raw, depth, nrmw, P_m, np.eye(4), stride=stride, reps=args.reps) for _ in range(args.runs)])
        lattice = (-(-synth.TUM_ROWS // stride)) * (-(-synth.TUM_COLS // stride))
        print(json.dumps(dict(stride=stride, lattice=lattice, pairs=int(acc[28]), blocks=(-(-(-(-synth.TUM_ROWS // stride)) // 16)) * (-(-(-(-synth.TUM_COLS // stride)) // 16)),
                              rows_us_median=round(float(np.median(us[:, 0])), 2), rows_us_min_max=[round(float(us[:, 0].min()), 2), round(float(us[:, 0].max()), 2)],
                              step_fold_us_median=round(float(np.median(us[:, 1])), 2),
                              step_fold_us_min_max=[round(float(us[:, 1].min()), 2), round(float(us[:, 1].max()), 2)])), flush=True)
    wall = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        pose, res = vol.track(raw, P_m)
        wall.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(track_call_ms_median=round(float(np.median(wall)), 3), track_call_ms_min_max=[round(min(wall), 3), round(max(wall), 3)],
                          status=res["status"], iterations=res["iterations"], pairs=res["pairs"], eig_ratio=res["eig_min"] / res["eig_max"] if res["eig_max"] else None)),
          flush=True)
    vol.close()
    ctx.close()


def _med(a):
    return dict(median=round(float(np.median(a)), 2), min_max=[round(float(np.min(a)), 2), round(float(np.max(a)), 2)])


def icp_photo(args):
    """`icp --photo`: the geometric and the photometric kernels in alternating batches on one coloured volume."""
    from odometry_amd import api, synth
    seq = synth.make_rgbd_sequence(args.frames, seed=0)
    K = (seq["K"]["f0"], seq["K"]["cx0"], seq["K"]["cy0"])
    ctx = api.Context(0)
    vol = make_volume(ctx, "pinned", (synth.TUM_ROWS, synth.TUM_COLS), K, colour=True)
    for d, g, A in zip(seq["depth"][:-1], seq["gray"][:-1], seq["poses"][:-1]):
        vol.integrate(d, A, colour=synth.colour_from_gray(g))
    P_m = seq["poses"][-2]
    depth, nrmw, rgba = vol.raycast(P_m, colour=True)
    raw, grey = seq["depth"][-1], seq["gray"][-1]
    for stride in (4, 2, 1):
        acc = vol.icp_eval(raw, depth, nrmw, P_m, np.eye(4), stride=stride, grey=grey, model_rgba=rgba)
        geo, photo = [], []
        for _ in range(args.runs):
            geo.append(vol.icp_time(raw, depth, nrmw, P_m, np.eye(4), stride=stride, reps=args.reps))
            photo.append(vol.icp_photo_time(raw, grey, depth, nrmw, rgba, P_m, np.eye(4), stride=stride, reps=args.reps))
        geo, photo = np.array(geo), np.array(photo)
        lx, ly = -(-synth.TUM_COLS // stride), -(-synth.TUM_ROWS // stride)
        print(json.dumps(dict(stride=stride, lattice=lx * ly, pairs=int(acc[28]), photo_pairs=int(acc[29]), blocks=(-(-lx // 16)) * (-(-ly // 16)),
                              rows_us=_med(geo[:, 0]), photo_rows_us=_med(photo[:, 0]), step_fold_us=_med(geo[:, 1]),
                              photo_step_fold_us=_med(photo[:, 1]))), flush=True)
    modes = list(api.TsdfVolume.COLOUR_SAMPLING) if args.sampling == "both" else [args.sampling]
    wall = dict(geo=[], **{m: [] for m in modes})
    p_res = {}
    for _ in range(args.runs):
        t0 = time.perf_counter()
        _, g_res = vol.track(raw, P_m)
        wall["geo"].append(1e3 * (time.perf_counter() - t0))
        for m in modes:                   # the whole call under each sampling mode of the model's colour frame, alternating
            vol.set_colour_sampling(m)
            t1 = time.perf_counter()
            _, p_res[m] = vol.track(raw, P_m, grey=grey)
            wall[m].append(1e3 * (time.perf_counter() - t1))
    for m in modes:
        r = p_res[m]
        print(json.dumps(dict(sampling=m, track_call_ms=_med(wall["geo"]), track_photo_call_ms=_med(wall[m]), status=[g_res["status"], r["status"]],
                              iterations=[g_res["iterations"], r["iterations"]], pairs=r["pairs"], photo_pairs=r["photo_pairs"])), flush=True)
    vol.close()
    ctx.close()


def shift(args):
    from odometry_amd import api, synth
    seq = synth.make_rgbd_sequence(args.frames, seed=0)
    K = (seq["K"]["f0"], seq["K"]["cx0"], seq["K"]["cy0"])
    ctx = api.Context(0)
    names = ("shift", "copy", "memset", "spill_count", "spill_scan", "spill_scatter")
    for grid in ("pinned", "large"):
        nx, ny, nz = GRIDS[grid]["dims"]
        for coloured in (False, True):
            vol = make_volume(ctx, grid, (synth.TUM_ROWS, synth.TUM_COLS), K, colour=coloured)
            cdev = [synth.colour_from_gray(g, 3, False, tint_seed=1) for g in seq["gray"]]
            for d, c, A in zip(seq["depth"], cdev, seq["poses"]):
                vol.integrate(d, A, colour=c if coloured else None)
            vol.enable_spill(1 << 22)
            points = len(vol.extract(1 << 22)[0])
            for tag, d in (("one layer", (0, 0, 1)), ("quarter grid", (0, 0, nz // 4))):
                us = np.array([vol.shift_time(d, reps=args.reps) for _ in range(args.runs)])
                row = dict(grid=grid, coloured=coloured, shift=tag, d=list(d), voxels=nx * ny * nz, extraction_points=points,
                           bytes_read_and_written=2 * (8 if coloured else 4) * nx * ny * nz)
                for k, n in enumerate(names):
                    row[n + "_us_median"] = round(float(np.median(us[:, k])), 2)
                    row[n + "_us_min_max"] = [round(float(us[:, k].min()), 2), round(float(us[:, k].max()), 2)]
                print(json.dumps(row), flush=True)
            for tag, d in (("one layer", (0, 0, 1)), ("quarter grid", (0, 0, nz // 4))):   # what either really spills, applied in turn
                vol.shift(d)
                got = vol.spilled(clear=True, with_dropped=True)
                print(json.dumps(dict(grid=grid, coloured=coloured, shift=tag, applied=True, spilled=len(got[0]), dropped=got[-1])), flush=True)
            vol.close()
    ctx.close()


def shift_mesh(args):
    """`shift --mesh`: the mesh spill's five stages beside the point spill's three and the shift, one visit."""
    from odometry_amd import api, synth
    seq = synth.make_rgbd_sequence(args.frames, seed=0)
    K = (seq["K"]["f0"], seq["K"]["cx0"], seq["K"]["cy0"])
    ctx = api.Context(0)
    names = ("count", "scan", "vertices", "triangles", "colour")
    for grid in ("pinned", "large"):
        nx, ny, nz = GRIDS[grid]["dims"]
        for coloured in (False, True):
            vol = make_volume(ctx, grid, (synth.TUM_ROWS, synth.TUM_COLS), K, colour=coloured)
            cdev = [synth.colour_from_gray(g, 3, False, tint_seed=1) for g in seq["gray"]]
            for d, c, A in zip(seq["depth"], cdev, seq["poses"]):
                vol.integrate(d, A, colour=c if coloured else None)
            vol.enable_spill(1 << 22)
            vol.enable_spill_mesh(1 << 23, 1 << 24)
            nv, nt = vol.mesh_counts()
            shifts = (("one layer x", (1, 0, 0)), ("one layer y", (0, 1, 0)), ("one layer z", (0, 0, 1)), ("quarter grid", (0, 0, nz // 4)),
                      ("whole grid", (0, 0, nz)))
            for tag, d in shifts:
                us = np.array([vol.spill_mesh_time(d, reps=args.reps) for _ in range(args.runs)])
                pt = np.array([vol.shift_time(d, reps=args.reps) for _ in range(args.runs)])
                row = dict(grid=grid, coloured=coloured, shift=tag, d=list(d), voxels=nx * ny * nz, mesh_vertices=nv, mesh_triangles=nt)
                for k, n in enumerate(names):
                    row["mesh_" + n + "_us_median"] = round(float(np.median(us[:, k])), 2)
                    row["mesh_" + n + "_us_min_max"] = [round(float(us[:, k].min()), 2), round(float(us[:, k].max()), 2)]
                row["mesh_stages_us_median_sum"] = round(float(np.median(us, 0).sum()), 2)
                for k, n in ((0, "shift"), (3, "spill_count"), (4, "spill_scan"), (5, "spill_scatter")):
                    row[n + "_us_median"] = round(float(np.median(pt[:, k])), 2)
                print(json.dumps(row), flush=True)
            for tag, d in shifts[:4]:   # what each really spills, applied in turn
                vol.shift(d)
                got = vol.spilled_mesh(clear=True, with_dropped=True)
                print(json.dumps(dict(grid=grid, coloured=coloured, shift=tag, applied=True, spilled_vertices=len(got[0]),
                                      spilled_triangles=len(got[2]), dropped=list(got[3]), spilled_points=len(vol.spilled(clear=True)[0]))), flush=True)
            vol.close()
    ctx.close()


def shift_reentry(args):
    """`shift --reentry`: the re-entry store's five stages beside the shift and the point spill's three, in alternating batches, with
    stores of 10^5, 10^6 and 10^7 live entries; then what each shift really saves and, on the way back, restores."""
    from odometry_amd import api, synth
    seq = synth.make_rgbd_sequence(args.frames, seed=0)
    K = (seq["K"]["f0"], seq["K"]["cx0"], seq["K"]["cy0"])
    ctx = api.Context(0)
    names = ("save_count", "save_scan", "save_scatter", "store_pass", "advance")
    for grid in ("pinned", "large"):
        nx, ny, nz = GRIDS[grid]["dims"]
        n = nx * ny * nz
        for coloured in ((False, True) if grid == "pinned" else (False,)):
            src = make_volume(ctx, grid, (synth.TUM_ROWS, synth.TUM_COLS), K, colour=coloured)
            cdev = [synth.colour_from_gray(g, 3, False, tint_seed=1) for g in seq["gray"]]
            for d, c, A in zip(seq["depth"], cdev, seq["poses"]):
                src.integrate(d, A, colour=c if coloured else None)
            q, w = src.grid()
            col = src.colour_grid() if coloured else None
            src.close()
            for live in (0, 10 ** 5, 10 ** 6, 10 ** 7):
                vol = make_volume(ctx, grid, (synth.TUM_ROWS, synth.TUM_COLS), K, colour=coloured)
                vol.enable_spill(1 << 22)
                vol.enable_reentry(live + n)
                fq, fw = np.zeros_like(q), np.zeros_like(w)
                left = live
                while left > 0:   # whole grids of `left` observed voxels, pushed out of the window: exactly `live` entries
                    fw.reshape(-1)[:] = 0
                    fw.reshape(-1)[:min(left, n)] = 1
                    vol.upload(fq, fw)
                    vol.shift((0, 0, nz))
                    left -= min(left, n)
                vol.spilled(clear=True)
                assert vol.reentry_stats()["live"] == live
                vol.upload(q, w)
                if coloured:
                    vol.upload_colour(col)
                shifts = (("one layer", (0, 0, 1)), ("quarter grid", (0, 0, nz // 4)))
                for tag, d in shifts:
                    re, pt = [], []
                    for _ in range(args.runs):   # alternating
                        re.append(vol.reentry_time(d, reps=args.reps))
                        pt.append(vol.shift_time(d, reps=args.reps))
                    re, pt = np.array(re), np.array(pt)
                    row = dict(grid=grid, coloured=coloured, shift=tag, d=list(d), voxels=n, live_entries=live,
                               observed_voxels=int((w > 0).sum()))
                    for k, nm in enumerate(names):
                        row[nm + "_us_median"] = round(float(np.median(re[:, k])), 2)
                        row[nm + "_us_min_max"] = [round(float(re[:, k].min()), 2), round(float(re[:, k].max()), 2)]
                    row["reentry_stages_us_median_sum"] = round(float(np.median(re, 0).sum()), 2)
                    for k, nm in ((0, "shift"), (3, "spill_count"), (4, "spill_scan"), (5, "spill_scatter")):
                        row[nm + "_us_median"] = round(float(np.median(pt[:, k])), 2)
                    print(json.dumps(row), flush=True)
                for tag, d in shifts:   # what each really saves, and what the way back restores
                    s0 = vol.reentry_stats()
                    vol.shift(d)
                    s1 = vol.reentry_stats()
                    vol.shift(tuple(-x for x in d))
                    s2 = vol.reentry_stats()
                    print(json.dumps(dict(grid=grid, coloured=coloured, shift=tag, applied=True, live_entries=live, saved=s1["saved"] - s0["saved"],
                                          restored_on_the_way_back=s2["restored"] - s1["restored"], dropped=s2["dropped"],
                                          grid_restored=bool(np.array_equal(vol.grid()[1], w)))), flush=True)
                vol.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    k = sub.add_parser("kernels")
    k.add_argument("--frames", type=int, default=10)
    k.add_argument("--extractions", type=int, default=3)
    k.add_argument("--json", default=None)
    k.add_argument("--runs", type=int, default=7)
    k.add_argument("--reps", type=int, default=20)
    s = sub.add_parser("summary")
    s.add_argument("dir")
    s.add_argument("--json", default=None)
    t = sub.add_parser("track")
    t.add_argument("--runs", type=int, default=3)
    t.add_argument("--steps", type=int, default=200)
    t.add_argument("--warmup", type=int, default=20)
    t.add_argument("--frames", type=int, default=100)
    t.add_argument("--modes", default="none,pinned,large")
    i = sub.add_parser("icp")
    i.add_argument("--frames", type=int, default=10)
    i.add_argument("--runs", type=int, default=7)
    i.add_argument("--reps", type=int, default=50)
    i.add_argument("--photo", action="store_true")
    i.add_argument("--sampling", choices=("nearest", "trilinear", "both"), default="nearest")
    h = sub.add_parser("shift")
    h.add_argument("--frames", type=int, default=10)
    h.add_argument("--runs", type=int, default=7)
    h.add_argument("--reps", type=int, default=20)
    h.add_argument("--mesh", action="store_true")
    h.add_argument("--reentry", action="store_true")
    args = ap.parse_args()
    if args.cmd == "icp" and args.photo:
        return icp_photo(args)
    if args.cmd == "shift" and args.mesh:
        return shift_mesh(args)
    if args.cmd == "shift" and args.reentry:
        return shift_reentry(args)
    dict(kernels=kernels, summary=summary, track=track, icp=icp, shift=shift)[args.cmd](args)


if __name__ == "__main__":
    main()
