"""Frame sizes and pyramid depths the whole trackers are held to (tests/test_shapes_cpu.py, tests/test_gpu_shapes.py): the table of
shapes, the synthetic drives rendered at each of them, and the CPU side of every comparison — oracle/runner.py's OracleRunner for the
stereo rows, tests/test_rgbd_cpu.py's RgbdModelRunner for the RGB-D rows. Nothing here imports the GPU library.

Intrinsics scale with the width and the principal point is the image centre; every drive is the `natural` drive at seed 0 unless a
seed is given. A row is rendered and run through its CPU runner in a worker process (at most 16, started with `spawn`: a worker never
inherits a process that has opened a device), once per test session."""
import concurrent.futures as cf
import multiprocessing as mp
import os

import numpy as np

STEREO_BASELINE = 0.537
RGBD = dict(depth_scale=1000.0, fwd_range=(0.1, 0.2), max_depth_step=0.05, max_range=30.0)


def case(kind, rows, cols, levels, frames, why=""):
    return dict(kind=kind, rows=rows, cols=cols, levels=levels, frames=frames, why=why, seed=0)


# rows x cols, levels, frames — and what the row is in the table for. The frame counts are the shortest at which the CPU runner
# switches keyframe at least once.
STEREO = [
    case("stereo", 120, 160, 3, 20, "tiles of 4x7 pixels, 6 blocks of 256 points at level 0"),
    case("stereo", 240, 320, 3, 20),
    case("stereo", 480, 640, 4, 16),
    case("stereo", 370, 1226, 4, 12, "KITTI's other rectified size"),
    case("stereo", 375, 1242, 4, 12, "KITTI raw"),
    case("stereo", 361, 1243, 4, 12, "rows odd, cols % 4 == 3"),
    case("stereo", 376, 1241, 3, 12),
    case("stereo", 376, 1241, 5, 12, "level-by-level pyramid kernels"),
    case("stereo", 1080, 1920, 4, 12, "selection tile 59x67 = 3 953 pixels"),
    case("stereo", 1032, 2056, 4, 10, "selection tile 64x64 = 4 096 pixels, the bound itself"),
]
RGBD_ROWS = [
    case("rgbd", 120, 160, 3, 40),
    case("rgbd", 240, 424, 4, 40, "RealSense"),
    case("rgbd", 363, 643, 4, 40, "rows odd, cols % 4 == 3"),
    case("rgbd", 479, 641, 4, 40),
    case("rgbd", 480, 848, 4, 40, "RealSense"),
    case("rgbd", 720, 1280, 4, 30, "RealSense; level 0 takes two passes of the persistent launch"),
    case("rgbd", 480, 640, 3, 40),
    case("rgbd", 480, 640, 5, 40),
]
TABLE = STEREO + RGBD_ROWS


def case_id(c):
    tag = f"{c['kind']}-{c['rows']}x{c['cols']}-L{c['levels']}"
    return tag if c.get("seed", 0) == 0 else f"{tag}-seed{c['seed']}"


def find(kind, rows, cols, levels, seed=0):
    """The table's row, or (another seed, a shape of the bounds tests) a case of the same form with the row's frame count."""
    for c in TABLE:
        if (c["kind"], c["rows"], c["cols"], c["levels"]) == (kind, rows, cols, levels):
            return dict(c, seed=seed)
    raise KeyError((kind, rows, cols, levels))


def intrinsics(c):
    """(f0, cx0, cy0): the focal length of KITTI-00 / of a 640-wide RGB-D sensor scaled with the width, the image centre."""
    f = (718.856 if c["kind"] == "stereo" else 525.0) * c["cols"] / (1241.0 if c["kind"] == "stereo" else 640.0)
    return (f, (c["cols"] - 1) / 2.0, (c["rows"] - 1) / 2.0)


def lm_max_iters(levels):
    """The runner's (10, 20, 30, 30), cut to 3 levels or extended by one more 30 for 5."""
    return ((10, 20, 30, 30) + (30,) * 4)[:levels]


def tracker_args(c, **kw):
    """Keyword overrides of api.Tracker / api.RgbdTracker / api.TrackerBatch for the case."""
    args = dict(rows=c["rows"], cols=c["cols"], levels=c["levels"], lm_max_iters=lm_max_iters(c["levels"]), K=intrinsics(c), any_size=1)
    if c["kind"] == "stereo":
        args["baseline"] = STEREO_BASELINE
    else:
        args.update(depth_scale=RGBD["depth_scale"], max_depth_step=RGBD["max_depth_step"])
    args.update(kw)
    return args


# ---- renderer calls -------------------------------------------------------------------------------------------------------------
def render(c):
    from odometry_amd import synth
    f, cx, cy = intrinsics(c)
    if c["kind"] == "stereo":
        return synth.make_sequence(c["frames"], seed=c["seed"], rows=c["rows"], cols=c["cols"], f=f, cx=cx, cy=cy,
                                   baseline=STEREO_BASELINE, drive="natural")
    return synth.make_rgbd_sequence(c["frames"], seed=c["seed"], drive="natural", fwd_range=RGBD["fwd_range"],
                                    depth_scale=RGBD["depth_scale"], max_range=RGBD["max_range"], rows=c["rows"], cols=c["cols"],
                                    f=f, cx=cx, cy=cy)


# ---- the two runner loops -------------------------------------------------------------------------------------------------------
STRIDE = 5   # stereo: masks / disparities / inverse depths are kept on every STRIDE-th frame, at frame 0 and at every switch


def tolerant_runner():
    """OracleRunner for a drive on which Solves fail. The reference's Solve then returns the pseudo-identity, whose last row is zero
    (src/lm_optimizer.cpp:48-52), and its runner inverts it; OracleRunner raises there. This variant does not invert a failed pose:
    the frame's abs_pose is None, the rest of the loop — keyframe test on the returned pose, Reset with it — goes on as the runner's."""
    from oracle import oracle as O
    from oracle import runner as orunner

    class Tolerant(orunner.OracleRunner):
        def track(self, left, right):
            r = O.track_frame(self.kf_img, self.kf_dep, left, right, self.lp, self.dp, self.init_pose)
            if r["status"] == -2:
                raise RuntimeError("    depth failed!")
            T = r["pose"]
            cur = None
            if r["status"] == 0:
                cur = orunner.matmul4_f32(self.kf_abs, np.linalg.inv(T.astype(np.float64)).astype(np.float32))
            mot = np.concatenate([np.abs(orunner.motion_angles(T)), np.abs(T[:3, 3])]).astype(np.float32)
            mag = np.float32(0)
            for m, w in zip(mot, orunner.KEYFRAME_WEIGHT):
                mag = np.float32(mag + np.float32(m * w))
            new_kf = bool(mag > self.motion_th) and cur is not None
            if new_kf:
                self.kf_img, self.kf_dep, self.kf_abs = r["img_pyr"], r["dep_pyr"], cur
                self.n_keyframes += 1
            self.init_pose = T
            return dict(pose_to_keyframe=T, abs_pose=cur, new_keyframe=new_kf, motion=float(mag), solve_status=r["status"],
                        val=r["val"], disp=r["disp"], dep=r["dep"], n_valid=r["n_valid"])
    return Tolerant


def stereo_params(c):
    from oracle import oracle as O
    f, cx, cy = intrinsics(c)
    lp = O.lm_params(max_iters=lm_max_iters(c["levels"]), K=dict(f0=f, cx0=cx, cy0=cy))
    dp = O.depth_params(baseline=STEREO_BASELINE, f0=f, any_size=1, boundary=c.get("boundary", 4))
    return lp, dp


def run_stereo(c, seq, runner=None):
    """OracleRunner over the drive: rows[0] = init (depth outputs only), rows[k] = frame k; the keyframe count."""
    from oracle import runner as orunner
    lp, dp = stereo_params(c)
    ref = (runner or orunner.OracleRunner)(lm_params=lp, depth_params=dp)
    d = ref.init(seq["left"][0], seq["right"][0])
    rows = [dict(n_valid=d["n_valid"], val=d["val"], disp=d["disp"], dep=d["dep"])]
    for k in range(1, c["frames"]):
        r = ref.track(seq["left"][k], seq["right"][k])
        if not (k % STRIDE == 0 or r["new_keyframe"]):
            r.update(val=None, disp=None, dep=None)
        rows.append(r)
    return rows, ref.n_keyframes


def run_rgbd(c, seq):
    """RgbdModelRunner over the drive: rows[0] = init, rows[k] = frame k (mask and inverse depth of every frame); the keyframe count."""
    from oracle import oracle as O
    from test_rgbd_cpu import RgbdModelRunner
    m = RgbdModelRunner(seq["K"], seq["depth_scale"], max_depth_step=RGBD["max_depth_step"], boundary=c.get("boundary", 4),
                        levels=c["levels"])
    m.lp = O.lm_params(K=seq["K"], max_iters=lm_max_iters(c["levels"]))
    rows = [m.init(seq["gray"][0], seq["depth"][0])]
    for k in range(1, c["frames"]):
        rows.append(m.track(seq["gray"][k], seq["depth"][k]))
    return rows, m.n_keyframes


def _job(job):
    c, with_ref = job
    seq = render(c)
    if not with_ref:
        return seq, None, None
    rows, n_kf = (run_stereo if c["kind"] == "stereo" else run_rgbd)(c, seq)
    return seq, rows, n_kf


# ---- once per session -----------------------------------------------------------------------------------------------------------
_cache = {}


def prepare(cases, with_ref=True):
    """Renders the cases (and runs their CPU runner) in worker processes; returns {case_id: dict(case, seq, rows, n_keyframes)} for
    them. A case is computed once per process."""
    from oracle import oracle as O
    O.lib()   # builds the oracle's library once, here, not in every worker
    todo = [c for c in cases if (case_id(c), with_ref) not in _cache and (case_id(c), True) not in _cache]
    if todo:
        todo.sort(key=lambda c: -c["rows"] * c["cols"] * c["frames"])   # the long rows first
        workers = max(1, min(16, os.cpu_count() or 1, len(todo)))
        if workers == 1:
            results = [_job((c, with_ref)) for c in todo]
        else:
            with cf.ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
                results = list(ex.map(_job, [(c, with_ref) for c in todo]))
        for c, (seq, rows, n_kf) in zip(todo, results):
            _cache[(case_id(c), with_ref)] = dict(case=c, seq=seq, rows=rows, n_keyframes=n_kf)
    return {case_id(c): _cache.get((case_id(c), True)) or _cache[(case_id(c), with_ref)] for c in cases}
