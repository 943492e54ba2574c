"""Frames and the child process of tests/test_gpu_fine_gather.py.

The persistent launch's row gather (lm_fine_body, step (c)) takes one of two paths by the level's number of virtual blocks
(256 points each). The frames here are 96 x 128, one pyramid level, with an inverse-depth image of exactly N valid pixels, so a
test chooses the block count. ODO_COARSE_MAX and ODO_HOME_XCD are read once per process by the library, hence the child:

    python tests/fine_gather_cases.py OUT.npz N [N ...]

runs one Solve per N and weight mode (Huber 1, L2 0, t-distribution 2) on the persistent launch and one with ODO_LM_NO_FINE=1
(step launches), and writes poses, statuses, evaluation counts, point counts and persistent-launch statistics to OUT.npz.

    python tests/fine_gather_cases.py OUT.npz --under coarse:ODO_LM_NO_FINE=1 --base step:ODO_LM_NO_FINE=1,ODO_LM_NO_COARSE=1 --trace N ...

chooses the two environments itself — the launch under test and its baseline, here the one-workgroup coarse launch (which, with
ODO_COARSE_MAX unset and no persistent launch, takes levels of up to kCoarseMaxPoints points) against the step launches — and with
--trace also writes every trace row of both (tests/test_gpu_coarse_rounds.py).
"""
import os
import sys

import numpy as np

ROWS, COLS = 96, 128
K = dict(f0=120.0, cx0=64.0, cy0=48.0)
MARGIN = 8
INTERIOR = (ROWS - 2 * MARGIN) * (COLS - 2 * MARGIN)
MODES = (1, 0, 2)
ITERS = [10]


def _texture(x, y):
    return 128.0 + 50.0 * np.sin(0.23 * x + 0.11 * y) + 40.0 * np.cos(0.17 * y - 0.05 * x) + 25.0 * np.sin(0.31 * x) * np.cos(0.27 * y)


def frames(n_points):
    """(keyframe image, inverse depth with exactly n_points valid interior pixels, current image), float32."""
    assert 1 <= n_points <= INTERIOR
    y, x = np.mgrid[0:ROWS, 0:COLS].astype(np.float64)
    img0 = _texture(x, y).astype(np.float32)
    img1 = _texture(x + 2.0, y + 1.0).astype(np.float32)   # (whole pixels: the LM samples at floor coordinates)
    inv = np.zeros((ROWS, COLS), np.float32)
    inner = inv[MARGIN:ROWS - MARGIN, MARGIN:COLS - MARGIN]
    i = np.arange(n_points)
    flat = np.zeros(INTERIOR, np.float32)
    flat[(i * 37) % INTERIOR] = (0.1 + 0.05 * ((i * 7) % 11) / 11.0).astype(np.float32)   # (37 and INTERIOR are coprime: n_points distinct pixels)
    inner[...] = flat.reshape(inner.shape)
    return img0, inv, img1


PATHS = (("fine", {}), ("step", {"ODO_LM_NO_FINE": "1"}))     # (name, environment of the optimiser): the launch under test, the baseline
TRACE_INT = ("level", "iter", "n_res", "accepted", "stop")


def parse_path(arg):
    """NAME:KEY=VALUE,KEY=VALUE -> (name, environment); the variables are set while that path's optimiser is created (the library
    reads ODO_LM_NO_FINE and ODO_LM_NO_COARSE per optimiser)."""
    name, _, rest = arg.partition(":")
    return name, dict(kv.split("=", 1) for kv in rest.split(",") if kv)


def main(out, counts, paths=PATHS, trace=False):
    """trace: the optimisers record (set_record), and every trace row is written out as well: `_trace_i` [rows, 5] (TRACE_INT) and
    `_trace_f` [rows, 8] float64 (err, lambda_after, delta[6]); `_launches`: the launches of the Solve."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from odometry_amd import api
    api.default_context()
    res = {}
    for n in counts:
        img0, inv, img1 = frames(n)
        p0, d0, p1 = api.ImagePyramid(1, img0, False), api.DepthPyramid(1, inv, False), api.ImagePyramid(1, img1, False)
        for mode in MODES:
            for path, env in paths:
                os.environ.update(env)
                lm = api.LevenbergMarquardtOptimizer(0.01, 0.995, ITERS, np.eye(4), None, mode, 28.0,
                                                     intrinsics=(K["f0"], K["cx0"], K["cy0"]))
                if trace:
                    lm.set_record(True)
                T = lm.Solve(p0, d0, p1)
                key = f"{n}_{mode}_{path}"
                res[key + "_pose"] = np.asarray(T, np.float32)
                res[key + "_meta"] = np.array([lm.last_status, lm.launch_stats()[0], lm.points()[0][0], *lm.persistent_stats()], np.int64)
                res[key + "_launches"] = np.array([lm.launch_stats()[1]], np.int64)
                if trace:
                    rows = lm.trace()
                    res[key + "_trace_i"] = np.array([[r[f] for f in TRACE_INT] for r in rows], np.int64).reshape(-1, len(TRACE_INT))
                    res[key + "_trace_f"] = np.array([[r["err"], r["lambda_after"], *r["delta"]] for r in rows], np.float64).reshape(-1, 8)
                lm.close()
                for k in env:
                    os.environ.pop(k, None)
        for o in (p0, d0, p1):
            o.close()
    np.savez(out, **res)


if __name__ == "__main__":
    args = sys.argv[2:]
    opts = {"paths": list(PATHS), "trace": False}
    while args and args[0].startswith("--"):
        flag = args.pop(0)
        if flag == "--trace":
            opts["trace"] = True
        else:
            opts["paths"][{"--under": 0, "--base": 1}[flag]] = parse_path(args.pop(0))
    main(sys.argv[1], [int(a) for a in args], tuple(opts["paths"]), opts["trace"])
