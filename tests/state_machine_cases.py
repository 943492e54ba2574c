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


COARSEST, FINEST = LEVELS - 1, 0


def check_exits(trace_i, trace_f):
    """Every row of CASES takes the exit it is named for. trace_i[case]: the recorded (level, iter, n_res, accepted, stop) rows of the
    row's Solve, trace_f[case]: their (err, lambda after, delta[6]) — of a single Solve or of one sequence of a batched one."""
    def _rows(case):
        return [tuple(int(x) for x in r) for r in trace_i[case]], [float(x) for x in trace_f[case][:, 1]]

    def _of_level(rows, level):
        return [r for r in rows if r[0] == level]

    # identical frames: err == 0 on the coarsest level, every step accepted (0 / 0 > precision is false), the level ends at max_iters
    # on an ACCEPTED step and the walk goes on
    rows, lam = _rows("identical")
    co = _of_level(rows, COARSEST)
    assert len(co) == 6 and all(r[3] == 1 and r[4] == 0 for r in co) and rows[6][:2] == (FINEST, 0)
    assert (trace_f["identical"][:6, 0] == 0).all()
    # accept, then the precision stop — on the coarsest level (the level changes on an accepted step) and on the finest (the Solve ends)
    rows, lam = _rows("precision")
    for level in (COARSEST, FINEST):
        lv = _of_level(rows, level)
        assert lv[0][3:] == (1, 0) and lv[-1][3:] == (1, 1) and len(lv) < 6
    assert rows[-1][0] == FINEST and rows[len(_of_level(rows, COARSEST))][:2] == (FINEST, 0)
    # reject with lambda x 5 and a step from the unchanged estimate; the coarsest level ends at max_iters on a REJECTED step
    rows, lam = _rows("reject_x5")
    rej = [i for i, r in enumerate(rows) if r[3:] == (0, 0)]
    assert rej and all(np.float32(lam[i]) == np.float32(lam[i - 1]) * np.float32(5.0) for i in rej if rows[i][1] > 0)
    co = _of_level(rows, COARSEST)
    assert len(co) == 6 and co[-1][3] == 0 and rows[6][:2] == (FINEST, 0)
    # lambda over 1e5: the level stops on a rejected step, the next level begins
    rows, lam = _rows("lambda_stop")
    stops = [i for i, r in enumerate(rows) if r[4] == 2]
    assert len(stops) == 1 and rows[stops[0]][3] == 0 and lam[stops[0]] > 1e5 and rows[stops[0]][0] == COARSEST
    assert rows[stops[0] + 1][:2] == (FINEST, 0) and rows[stops[0] - 1][3:] == (0, 0)
    # max_iters 1 and 2
    for case, n_fine, n_coarse in (("iters_1_2", 1, 2), ("iters_2_1", 2, 1)):
        rows, lam = _rows(case)
        assert [r[:2] for r in rows] == [(COARSEST, i) for i in range(n_coarse)] + [(FINEST, i) for i in range(n_fine)]
        assert all(r[4] == 0 for r in rows)
    # a level with max_iters 0: walked over, at the end and at the start of the pyramid
    rows, lam = _rows("no_finest")
    assert len(rows) == 6 and all(r[0] == COARSEST for r in rows)
    rows, lam = _rows("no_coarsest")
    assert len(rows) == 6 and all(r[0] == FINEST for r in rows)
    # a reject as the first evaluation of a level (the step starts from the level's initial estimate)
    rows, lam = _rows("reject_first")
    assert len(rows) == 12 and all(r[3:] == (0, 0) for r in rows)
    # ... and lambda over 1e5 there: one evaluation per level, no step
    rows, lam = _rows("reject_first_stop")
    assert [r[:2] + r[3:] for r in rows] == [(COARSEST, 0, 0, 2), (FINEST, 0, 0, 2)]
    assert (trace_f["reject_first_stop"][:, 2:] == 0).all()
    # ... and after two rejected steps
    rows, lam = _rows("reject_stop_3rd")
    assert [r[:2] + r[3:] for r in rows] == [(l, i, 0, 2 if i == 2 else 0) for l in (COARSEST, FINEST) for i in range(3)]


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
