"""Every exit of the pose LM's decision (lm_state_machine_hot, kernels.hip.h: accept / reject, the lambda rule, the three stops, the
level walk) on the chain kernels, whose state machine runs on wave-uniform branches and writes what an exit changes under that exit
only. The rows of tests/state_machine_cases.py at the 32 x 40 two-level pyramid (768 and 96 points), through the four routes of
tests/test_gpu_residual_edges.py — the step launches (the in-library reference: lm_state_machine, not the hot one), the coarse
launch, the persistent launch at its default number of workgroups and at two — on a recording and on a lean optimiser each.

Asserted: the same bits from every route (pose, status, evaluations, trace rows); the recorded rows against the oracle's lm_solve
trace; and that every row of the table takes the exit it is named for, read from the recorded `accepted` and `stop` fields.

(Identical frames do not reach the precision stop: their error is 0 on the coarsest level, 0 / 0 compares false with the precision
and the level runs to max_iters on accepted steps — the row `identical` holds that; the stop itself is the row `precision`, a small
translation with lambda0 = 3e4, whose second step changes the error by less than the precision on both levels.)

Against the oracle the integer fields and lambda (x 5, / 5 and max of fp32 values: exact in both) are equal, err = float(sum 27 /
sum 28) of sums held to 1e-11 is one fp32 rounding apart at the most, and the step is held to a perturbation bound: device and
oracle solve (A + lambda diag A) d = -b in fp64 by the same elimination, from sums of poses that may differ in the last bit of an
fp32 entry, so |d_device - d_oracle| <= (cond(A + lambda diag A) + 1) 2^-22 |d_oracle| in the 2-norm, the condition number taken
from the oracle's sums at the row's pose."""
import os
import subprocess
import sys

import numpy as np
import pytest

import state_machine_cases as cases
from test_gpu_residual_edges import ROUTES, _KNOBS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COARSEST, FINEST = cases.COARSEST, cases.FINEST


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every Solve of this module: one child process per process-wide setting (ODO_COARSE_MAX, ODO_LM_FINE_K are read once)."""
    tmp = tmp_path_factory.mktemp("state_machine")
    children = {}
    for route, (child, env, _) in ROUTES.items():
        children.setdefault(child, (env, []))[1].append(route)
    out = {}
    for child, (env, routes) in children.items():
        path = os.path.join(str(tmp), child + ".npz")
        e = {k: v for k, v in os.environ.items() if k not in _KNOBS}
        e.update(env)
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "state_machine_cases.py"), path] +
                       [f"{r}:{ROUTES[r][2]}" for r in routes], check=True, env=e, timeout=300)
        out.update(np.load(path))
    return out


def oracle_reference(O, pyr, c, robust=cases.ROBUST):
    """(the oracle's Solve of the row c, per recorded evaluation the condition number of the damped system it solved). pyr: a cache of
    the oracle's pyramids per kind of frames."""
    flat = lambda levels: np.concatenate([l.ravel() for l in levels])
    if c["kind"] not in pyr:
        img0, inv, img1 = cases.frames(c["kind"])
        pyr[c["kind"]] = (O.image_pyramid(img0, cases.LEVELS, True), O.depth_pyramid(inv, cases.LEVELS),
                          O.image_pyramid(img1, cases.LEVELS, True))
    r0, rd, r1 = pyr[c["kind"]]
    params = O.lm_params(lam=c["lam"], precision=cases.PRECISION, max_iters=tuple(c["iters"]), robust=robust,
                         huber_delta=cases.HUBER, K=cases.K)
    solve = O.lm_solve(flat(r0), flat(rd), flat(r1), cases.ROWS, cases.COLS, params, init=c["T"])
    conds = []
    for row in solve["trace"]:
        cond = 0.0
        if np.any(row["delta"] != 0):
            l = row["level"]
            acc = O.lm_accumulate(r0[l], r1[l], rd[l], l, row["pose"], robust=robust, huber_delta=cases.HUBER, K=cases.K)["acc"]
            A = np.zeros((6, 6))
            for i in range(6):
                for j in range(i, 6):
                    A[i, j] = A[j, i] = acc[i * 6 - (i * (i - 1)) // 2 + (j - i)]
            A[np.diag_indices(6)] += np.float64(np.float32(row["lambda_after"])) * np.diag(A)
            cond = float(np.linalg.cond(A))
        conds.append(cond)
    return solve, conds


@pytest.fixture(scope="module")
def refs(O):
    """The oracle's Solve of every row, and per recorded evaluation the condition number of the damped system it solved."""
    pyr = {}
    return {name: oracle_reference(O, pyr, c) for name, c in cases.CASES.items()}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_routes_are_the_ones_meant(runs):
    for case in cases.CASES:
        for kind in ("rec", "lean"):
            assert tuple(runs[f"step_{case}_{kind}_meta"][2:]) == (0, 0) == tuple(runs[f"coarse_{case}_{kind}_meta"][2:])
            for route in ("fine", "fine_k2"):
                k, redone = (int(v) for v in runs[f"{route}_{case}_{kind}_meta"][2:])
                assert k > 0 and redone == 0, "the Solve did not run on the persistent launch"
            assert int(runs[f"fine_k2_{case}_{kind}_meta"][2]) == 2


@pytest.mark.parametrize("case", list(cases.CASES))
def test_every_route_gives_the_same_bits(runs, case):
    base_pose, base_meta = runs[f"step_{case}_rec_pose"], runs[f"step_{case}_rec_meta"]
    ti, tf = runs[f"step_{case}_rec_trace_i"], runs[f"step_{case}_rec_trace_f"]
    for route in ROUTES:
        for kind in ("rec", "lean"):
            key = f"{route}_{case}_{kind}"
            assert np.array_equal(_bits(runs[key + "_pose"]), _bits(base_pose)), key
            assert tuple(runs[key + "_meta"][:2]) == tuple(base_meta[:2]), key    # status, evaluations
        key = f"{route}_{case}_rec"
        assert runs[key + "_trace_i"].shape == ti.shape and np.array_equal(runs[key + "_trace_i"], ti), key
        assert np.array_equal(_bits(runs[key + "_trace_f"]), _bits(tf)), key


@pytest.mark.parametrize("case", list(cases.CASES))
def test_the_recorded_rows_are_the_oracles(runs, refs, case):
    solve, conds = refs[case]
    for route in ROUTES:
        key = f"{route}_{case}_rec"
        status, n_evals = (int(x) for x in runs[key + "_meta"][:2])
        ti, tf = runs[key + "_trace_i"], runs[key + "_trace_f"]
        assert status == solve["status"], key
        assert np.array_equal(_bits(runs[key + "_pose"]), _bits(runs[f"step_{case}_rec_pose"]))
        if case == "no_residual":
            # the reference fails in its first evaluation (N == 0) and records nothing; what the device recorded of it holds N == 0
            assert solve["n_evals"] == 0 and len(ti) <= 1 and (ti[:, 2] == 0).all(), key
            continue
        assert n_evals == solve["n_evals"] == len(ti), key
        assert_rows_are_the_oracles(key, ti, tf, solve, conds)


def assert_rows_are_the_oracles(key, ti, tf, solve, conds):
    """Recorded rows against the oracle's: integer fields and lambda exact, err one fp32 rounding, the step within the perturbation
    bound of the module's docstring."""
    for row, f, b, cond in zip(ti, tf, solve["trace"], conds):
        d_dev, d_ref = f[2:].astype(np.float64), b["delta"].astype(np.float64)
        bound = (cond + 1.0) * 2.0 ** -22 * np.linalg.norm(d_ref)
        print(key, "level", row[0], "iter", row[1], "N", row[2], "accepted", row[3], "stop", row[4], "err", f[0], "oracle", b["err"],
              "lambda", f[1], "oracle", b["lambda_after"], "|d - oracle's|", np.linalg.norm(d_dev - d_ref), "bound", bound)
        assert tuple(int(x) for x in row) == (b["level"], b["iter"], b["n_res"], b["accepted"], b["stop"]), key
        assert abs(np.float64(f[0]) - b["err"]) <= 2.0 ** -23 * abs(b["err"]), key
        assert np.float32(f[1]) == np.float32(b["lambda_after"]), key
        assert np.linalg.norm(d_dev - d_ref) <= bound, key


def test_each_row_of_the_table_takes_its_exit(runs):
    # the checks themselves: state_machine_cases.check_exits (shared with tests/test_gpu_batch_chain_cases.py), on the in-library
    # reference's recording run (every route equals it)
    cases.check_exits({c: runs[f"step_{c}_rec_trace_i"] for c in cases.CASES}, {c: runs[f"step_{c}_rec_trace_f"] for c in cases.CASES})
    # no residual at all
    for route in ROUTES:
        for kind in ("rec", "lean"):
            assert int(runs[f"{route}_no_residual_{kind}_meta"][0]) == -1
