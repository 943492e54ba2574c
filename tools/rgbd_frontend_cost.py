"""What the RGB-D front end (odo_rgbd_frontend_*) costs the tracker it feeds: tools/rgbd_cost.py's tracked loop over the TUM-shaped
drive (next frame announced with its depth frame, back and forth over the drive), with the tracker's inputs coming from
  premade  device buffers made beforehand (the loop of tools/rgbd_cost.py: no front end in the clock),
  dev      the front end, raw frames (interleaved uint8 colour + the depth imager's uint16 frame) device-resident, submitted two
           frames ahead of the tracker (an announced frame must be complete),
  host     the same from host memory through a context of the front end's own: the uploads are inside the clock,
runs interleaved mode by mode. All three feed the tracker byte-equal frames (the premade buffers are the front end's own results),
so keyframes and valid-depth counts must agree between the modes. Prints frames/s per mode (median, spread), the host time of a
submit and of the waits per frame, and the tracker's own timing (odo_tracker_timing).

  python tools/rgbd_frontend_cost.py [--runs 3] [--steps 200] [--warmup 20] [--frames 100] [--rig identity|A] [--modes premade,dev[,host]]

`premade` is tools/rgbd_cost.py's `tum` mode (same drive, same loop): a build without the front end is measured with that tool.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def rigs():
    from odometry_amd import synth
    return dict(identity=dict(depth_size=(480, 640), depth_K=(525.0, 525.0, 319.5, 239.5), E=np.eye(4)),
                A=dict(depth_size=(480, 640), depth_K=(385.0, 385.0, 319.5, 239.5),
                       E=synth.rig_extrinsic((0.015, 0.0005, -0.0003), (0.002, -0.003, 0.001))))


def render_raw(n, r):
    """The drive of rgbd_cost.py's `tum` mode as the sensor of rig r delivers it: [(colour uint8 rows x cols x 3, raw depth)]."""
    import concurrent.futures as cf
    from odometry_amd import synth
    poses = synth.trajectory(n, 0, fwd_range=(0.1, 0.2), max_offset=1.0)
    jobs = [(T, r) for T in poses]
    with cf.ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(_render, jobs, chunksize=4))


_scenes = {}


def _render(job):
    from odometry_amd import synth
    T, r = job
    if "s" not in _scenes:
        _scenes["s"] = synth.drive_scene("natural", 0)
    sc = _scenes["s"]
    img, _ = sc.render(T, synth.TUM_ROWS, synth.TUM_COLS, synth.TUM_F, synth.TUM_CX, synth.TUM_CY, 0.0)
    (dr, dc), (fx, _, cx, cy) = r["depth_size"], r["depth_K"]
    _, Zd = sc.render(T @ r["E"], dr, dc, fx, cx, cy, 0.0)
    return synth.colour_from_gray(img, 3, False, None), synth.sensor_depth(Zd, 1000.0, 30.0)


class Premade:
    """Frames that are device buffers already."""

    def __init__(self, dev):
        self.dev = dev
        self.submit_s = self.wait_s = 0.0

    def request(self, k, idx):
        pass

    def get(self, k, idx):
        return self.dev[idx]


class Fed:
    """Frames prepared by the front end: request(k) submits, get(k) waits for the slot."""

    def __init__(self, fe, raw):
        self.fe, self.raw, self.slot = fe, raw, {}
        self.submit_s = self.wait_s = 0.0

    def request(self, k, idx):
        t0 = time.perf_counter()
        self.slot[k] = self.fe.submit(*self.raw[idx])
        self.submit_s += time.perf_counter() - t0
        self.slot.pop(k - 4, None)

    def get(self, k, idx):
        t0 = time.perf_counter()
        self.fe.wait(self.slot[k][0])
        self.wait_s += time.perf_counter() - t0
        return self.slot[k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rig", default="identity")
    ap.add_argument("--modes", default="premade,dev")
    args = ap.parse_args()
    from odometry_amd import api, synth
    modes = args.modes.split(",")
    r = rigs()[args.rig]
    raw = render_raw(args.frames, r)
    K = (synth.TUM_F, synth.TUM_CX, synth.TUM_CY)
    size = (synth.TUM_ROWS, synth.TUM_COLS)
    trk = api.RgbdTracker(0, depth_scale=1000.0, max_depth_step=0.05, rows=size[0], cols=size[1], K=K)

    def frontend(ctx):
        return api.RgbdFrontend(ctx, r["depth_size"], r["depth_K"], 1000.0, size, K, 1000.0, r["E"], 3, False, 4)
    # Only what the requested modes need is created: every front end and context is one more stream, and streams beyond the
    # process's hardware queues (GPU_MAX_HW_QUEUES, HIP's default 4; the tracker has three) share a queue with the tracker's.
    fe_dev = frontend(trk)
    raw_dev = [(fe_dev.upload(c), fe_dev.upload(d)) for c, d in raw]
    made = [fe_dev.download(*fe_dev.submit(c, d)) for c, d in raw_dev]
    feeders = dict(dev=Fed(fe_dev, raw_dev), premade=Premade([(trk.upload_frame(g), trk.upload_depth(d)) for g, d in made]))
    own_ctx = fe_host = None
    if "host" in modes:
        own_ctx = api.Context(0)
        fe_host = frontend(own_ctx)
        feeders["host"] = Fed(fe_host, raw)
    T = np.zeros(16, np.float32)
    A = np.zeros(16, np.float32)
    res = {m: [] for m in modes}
    n = len(raw)
    last = args.warmup + args.steps
    order = [k % (2 * n - 2) for k in range(last + 3)]
    order = [k if k < n else 2 * n - 2 - k for k in order]   # back and forth over the drive, as bench.py does
    for run in range(args.runs):
        for mode in modes:
            fd = feeders[mode]
            _, djob0 = trk.depth_persistent_stats()
            for k in range(3):
                fd.request(k, order[k])
            trk.init(*fd.get(0, order[0]))
            kf = 0
            t0 = None
            for k in range(1, last + 1):
                if k == args.warmup + 1:
                    trk._sync()
                    trk.timing()   # (resets the averages)
                    fd.submit_s = fd.wait_s = 0.0
                    t0 = time.perf_counter()
                if k + 2 <= last:
                    fd.request(k + 2, order[k + 2])
                if k + 1 <= last and k + 1 != args.warmup + 1:
                    trk.hint_next(*fd.get(k + 1, order[k + 1]))
                kf += trk.track_into(*fd.get(k, order[k]), T, A)
            trk._sync()
            fps = args.steps / (time.perf_counter() - t0)
            tm = trk.timing()
            _, djob1 = trk.depth_persistent_stats()
            res[mode].append(fps)
            print(json.dumps(dict(run=run, mode=mode, rig=args.rig, fps=round(fps, 1), keyframes=kf + 1,
                                  submit_us=round(1e6 * fd.submit_s / args.steps, 2), wait_us=round(1e6 * fd.wait_s / args.steps, 2),
                                  depth_jobs_redone=djob1 - djob0, n_valid_last=trk.stats()["n_valid_depth"],
                                  **{k_: round(v, 1) for k_, v in tm.items()})), flush=True)
    print(json.dumps(dict(summary=True, rig=args.rig, **{m: dict(median_fps=round(float(np.median(res[m])), 1),
                                                                  spread=[round(min(res[m]), 1), round(max(res[m]), 1)]) for m in modes})))
    fe_dev.close()
    if fe_host is not None:
        fe_host.close()
    trk.close()
    if own_ctx is not None:
        own_ctx.close()


if __name__ == "__main__":
    main()
