"""The table and the child process of tests/test_gpu_state_machine_branches.py: every exit of the pose LM's decision
(lm_state_machine_hot, kernels.hip.h) at the smallest geometry that reaches it.

The frames are those of tests/residual_edge_cases.py — a 32 x 40 image, two levels, every interior pixel a keyframe point: 768 and
96 points, so the coarsest level runs in the coarse launch's one-virtual-block path and the finest one through its fold. A row of
the table is (frames, initial pose, lambda0, max_iters per level); what exit it takes was read off the oracle's trace on the CPU
when the table was written and is asserted by the test from the recorded rows.

    python tests/state_machine_cases.py OUT.npz NAME:KEY=VALUE,... [NAME:KEY=VALUE,...]

runs, per route NAME (residual_edge_cases.py's scheme: the variables are set while that route's optimisers are created;
ODO_COARSE_MAX and ODO_LM_FINE_K come with the child's environment) and per row, one Solve on a recording optimiser and one on
a lean one, and writes poses, statuses, evaluation counts, persistent-launch statistics and trace rows to OUT.npz.
"""
import os
import sys

import numpy as np

import residual_edge_cases as base

ROWS, COLS, LEVELS, K, ROBUST, HUBER = base.ROWS, base.COLS, base.LEVELS, base.K, base.ROBUST, base.HUBER
PRECISION = 0.995
TRACE_INT = base.TRACE_INT
# An error above the 1e10 a level starts from (lm_begin_level's err_last) rejects the level's FIRST evaluation: with Huber weights the
# error is about 28 |r|, so the images are scaled until |r| is of the order 1e10.
HUGE = 1e9


def frames(kind):
    img0, inv, img1 = base.frames()
    if kind == "same":
        return img0, inv, img0
    if kind == "huge":
        return img0 * np.float32(HUGE), inv, img1 * np.float32(HUGE)
    return img0, inv, img1


def _case(kind="shifted", T=None, lam=0.01, iters=(6, 6)):
    return dict(kind=kind, T=base._translation() if T is None else T, lam=lam, iters=list(iters))


# max_iters is indexed by level: (finest, coarsest). The Solve walks the coarsest level first.
CASES = {
    "identical": _case(kind="same"),                                   # err = 0 in every evaluation of the coarsest level: accepted, 0 / 0 is no stop
    "precision": _case(T=base._translation(0.05, 0.025), lam=3e4),     # accept, then accept with err / err_last > precision on both levels
    "reject_x5": _case(),                                              # two rejected steps (lambda x 5) at the end of the coarsest level
    "lambda_stop": _case(T=base._translation(1.2, 0.6), lam=3e4),      # accept, accept, reject, reject, reject over 1e5
    "iters_1_2": _case(iters=(1, 2)),
    "iters_2_1": _case(iters=(2, 1)),
    "no_finest": _case(iters=(0, 6)),                                  # a level with max_iters 0 at the end of the walk
    "no_coarsest": _case(iters=(6, 0)),                                # ... and at its start
    "no_residual": _case(T=base.POSES["all_out"]),
    "reject_first": _case(kind="huge"),                                # every evaluation rejected, the first one of each level included
    "reject_first_stop": _case(kind="huge", lam=3e4),                  # lambda over 1e5 in a level's first evaluation: no step at all
    "reject_stop_3rd": _case(kind="huge", lam=1e3),                    # reject, reject, reject over 1e5: a level ends on a rejected step
}


def main(out, routes):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from odometry_amd import api
    api.default_context()
    pyr = {}
    for kind in sorted({c["kind"] for c in CASES.values()}):
        img0, inv, img1 = frames(kind)
        pyr[kind] = (api.ImagePyramid(LEVELS, img0, True), api.DepthPyramid(LEVELS, inv, False), api.ImagePyramid(LEVELS, img1, True))
    res = {}
    for route, env in routes:
        for name, c in CASES.items():
            p0, d0, p1 = pyr[c["kind"]]
            for record in (True, False):
                os.environ.update(env)
                lm = api.LevenbergMarquardtOptimizer(c["lam"], PRECISION, c["iters"], c["T"], None, ROBUST, HUBER,
                                                     intrinsics=(K["f0"], K["cx0"], K["cy0"]))
                for k in env:
                    os.environ.pop(k, None)
                lm.set_record(record)
                T = lm.Solve(p0, d0, p1)
                key = f"{route}_{name}_{'rec' if record else 'lean'}"
                res[key + "_pose"] = np.asarray(T, np.float32)
                res[key + "_meta"] = np.array([lm.last_status, lm.launch_stats()[0], *lm.persistent_stats()], np.int64)
                if record:
                    rows = lm.trace()
                    res[key + "_trace_i"] = np.array([[r[f] for f in TRACE_INT] for r in rows], np.int64).reshape(-1, len(TRACE_INT))
                    res[key + "_trace_f"] = np.array([[r["err"], r["lambda_after"], *r["delta"]] for r in rows], np.float32).reshape(-1, 8)
                lm.close()
    for objs in pyr.values():
        for o in objs:
            o.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], [base.parse_route(a) for a in sys.argv[2:]])
