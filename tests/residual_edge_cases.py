"""Frames, initial poses and the child process of tests/test_gpu_residual_edges.py.

A two-level pyramid of a 32 x 40 image (levels 32 x 40 and 16 x 20) whose every pixel carries a valid inverse depth, so that
every interior pixel of both levels is a keyframe point and the points reach the image borders' scale. The initial poses put the
warped points on and across every edge the residual tests: u in [cols - 1, cols), u in [-1, 0), the same for v, everything out,
everything behind the camera, a NaN and an infinity in the pose.

    python tests/residual_edge_cases.py OUT.npz NAME:KEY=VALUE,... [NAME:KEY=VALUE,...]

runs, per route NAME (the variables are set while that route's optimisers are created) and per initial pose, one Solve on a
recording optimiser (trace rows: the N of every evaluation) and one on a lean one (what the trackers run), and writes poses,
statuses, evaluation counts, point counts, persistent-launch statistics and trace rows to OUT.npz. ODO_COARSE_MAX and
ODO_LM_FINE_K are read once per process by the library: they come with the child's environment.
"""
import os
import sys

import numpy as np

ROWS, COLS, LEVELS = 32, 40, 2
K = dict(f0=40.0, cx0=20.0, cy0=16.0)
ITERS = [6, 6]
ROBUST = 1
HUBER = 28.0
TRACE_INT = ("level", "iter", "n_res", "accepted", "stop")


def _texture(x, y):
    return 128.0 + 50.0 * np.sin(0.23 * x + 0.11 * y) + 40.0 * np.cos(0.17 * y - 0.05 * x) + 25.0 * np.sin(0.31 * x) * np.cos(0.27 * y)


def frames(rows=ROWS, cols=COLS, valid=None):
    """(keyframe image, inverse depth — valid everywhere, two values in a checkerboard of 2 x 2 cells so that a translation moves
    neighbouring points by different amounts —, current image), float32. Other sizes and `valid` = (row0, row1, col0, col1), the
    only window that keeps its inverse depth, are for tests/batch_chain_cases.py."""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img0 = _texture(x, y).astype(np.float32)
    img1 = _texture(x + 1.0, y + 1.0).astype(np.float32)
    inv = np.where(((x // 2) + (y // 2)) % 2 == 0, 0.125, 0.25).astype(np.float32)
    if valid is not None:
        keep = np.zeros((rows, cols), bool)
        keep[valid[0]:valid[1], valid[2]:valid[3]] = True
        inv[~keep] = 0.0
    return img0, inv, img1


def _translation(tx=0.0, ty=0.0):
    T = np.eye(4, dtype=np.float32)
    T[0, 3], T[1, 3] = tx, ty
    return T


def _half_turn_y():
    T = np.eye(4, dtype=np.float32)
    T[0, 0] = T[2, 2] = -1.0
    return T


def _with_entry(r, c, v):
    T = np.eye(4, dtype=np.float32)
    T[r, c] = v
    return T


# A translation t moves a point of inverse depth d by fl * t * d pixels: on the coarsest level (fl = 20, the level of a Solve's first
# evaluation) tx = 1.9 is 4.75 px for d = 0.125 and 9.5 px for d = 0.25 — the interior columns 4 .. 15 go to 8.75 .. 19.75 (the last
# one in [cols - 1, cols) = [19, 20)) and to 13.5 .. 24.5 (partly beyond cols). The negative shifts: 4 .. 15 to -0.75 .. 10.25 (the
# first one in [-1, 0)) and to -5.5 .. 5.5. The same with ty and the rows (4 .. 11 of 16: ty = 1.5 is 3.75 and 7.5 px).
POSES = {
    "identity": _translation(),
    "u_high": _translation(tx=1.9),
    "u_low": _translation(tx=-1.9),
    "v_high": _translation(ty=1.5),
    "v_low": _translation(ty=-1.5),
    "all_out": _translation(tx=40.0),      # 100 px and more on the coarsest level, 200 and more on the finest: beyond cols
    "behind": _half_turn_y(),              # every t2 = -Z <= 0
    "nan": _with_entry(0, 3, np.float32("nan")),
    "inf": _with_entry(1, 3, np.float32("inf")),
}
PARTLY_OUT = ("u_high", "u_low", "v_high", "v_low")
ALL_OUT = ("all_out", "behind", "nan", "inf")


def first_eval_coordinates(T):
    """(u, v) of the coarsest level's keyframe points warped by T, in float64 — where the first evaluation of a Solve samples."""
    lvl = LEVELS - 1
    rows, cols, fl = ROWS >> lvl, COLS >> lvl, K["f0"] / 2 ** lvl
    cx, cy = K["cx0"], K["cy0"]
    for _ in range(lvl):
        cx, cy = (cx + 0.5) / 2.0 + 0.5, (cy + 0.5) / 2.0 + 0.5
    from oracle import oracle
    inv = oracle.depth_pyramid(frames()[1], LEVELS)[lvl].astype(np.float64)
    y, x = np.mgrid[4:rows - 4, 4:cols - 4].astype(np.float64)
    z = 1.0 / inv[4:rows - 4, 4:cols - 4]
    P = np.stack([z * (x - cx) / fl, z * (y - cy) / fl, z, np.ones_like(z)], -1) @ np.asarray(T, np.float64).T
    with np.errstate(all="ignore"):
        return fl * P[..., 0] / P[..., 2] + cx, fl * P[..., 1] / P[..., 2] + cy, P[..., 2]


def parse_route(arg):
    name, _, rest = arg.partition(":")
    return name, dict(kv.split("=", 1) for kv in rest.split(",") if kv)


def main(out, routes):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from odometry_amd import api
    api.default_context()
    img0, inv, img1 = frames()
    p0, d0, p1 = api.ImagePyramid(LEVELS, img0, True), api.DepthPyramid(LEVELS, inv, False), api.ImagePyramid(LEVELS, img1, True)
    res = {}
    for route, env in routes:
        for pose_name, T0 in POSES.items():
            for record in (True, False):
                os.environ.update(env)
                lm = api.LevenbergMarquardtOptimizer(0.01, 0.995, ITERS, T0, None, ROBUST, HUBER, intrinsics=(K["f0"], K["cx0"], K["cy0"]))
                for k in env:
                    os.environ.pop(k, None)
                lm.set_record(record)
                T = lm.Solve(p0, d0, p1)
                key = f"{route}_{pose_name}_{'rec' if record else 'lean'}"
                res[key + "_pose"] = np.asarray(T, np.float32)
                res[key + "_meta"] = np.array([lm.last_status, lm.launch_stats()[0], *lm.persistent_stats()], np.int64)
                res[key + "_points"] = np.array(lm.points()[0], np.int64)
                if record:
                    rows = lm.trace()
                    res[key + "_trace_i"] = np.array([[r[f] for f in TRACE_INT] for r in rows], np.int64).reshape(-1, len(TRACE_INT))
                    res[key + "_trace_f"] = np.array([[r["err"], r["lambda_after"], *r["delta"]] for r in rows], np.float64).reshape(-1, 8)
                    if route == routes[0][0]:   # the in-library reference's 29 sums of the first evaluation (coarsest level, the initial pose)
                        st, acc = lm.accumulate(p0, d0, p1, LEVELS - 1, T0)
                        res[f"{pose_name}_acc"] = acc
                        res[f"{pose_name}_acc_status"] = np.array([st], np.int64)
                lm.close()
    for o in (p0, d0, p1):
        o.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], [parse_route(a) for a in sys.argv[2:]])
