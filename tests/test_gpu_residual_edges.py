"""The residual of the LM chain kernels at the edges of its validity test (point_residual_g, kernels.hip.h): ONE predicate — the lane
holds a point, t2 > 0, 0 <= floor(u) < cols, 0 <= floor(v) < rows, a NaN failing every comparison — selects the taps' pixel and the
row's r and J instead of a nest of early returns, in the coarse launch and the persistent launch. This module runs their recording and
their lean builds on single Solves with Huber weights; the batched builds run the same poses as sequences of one batched Solve in
tests/test_gpu_batch_chain_cases.py, and no test issues these poses with t-distribution weights. The step launches keep the branching
point_residual: they are the in-library reference here.

A two-level pyramid of a 32 x 40 image with a valid inverse depth everywhere, so every interior pixel is a keyframe point (the
library's interior keeps 4 pixels from each border: 24 x 32 = 768 and 8 x 12 = 96 points, three virtual blocks and one), solved from
initial poses that put points ON each border ([cols - 1, cols), [-1, 0), the same for rows), all of them out, all of them behind the
camera, and from poses with a NaN and an infinity. Three routes — the coarse launch, the persistent launch (at its default number of
workgroups, where the second half of every workgroup has no virtual block, and at two, where workgroup 0's second half has one and
workgroup 1's has none) and the step launches — must give the same bits; the N of every evaluation must be the oracle's, the 29 sums
of the first evaluation the oracle's at the parity tests' tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import residual_edge_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_KNOBS = ("ODO_HOME_XCD", "ODO_NO_HOME_XCD", "ODO_LM_NO_FINE", "ODO_LM_FINE_K", "ODO_LM_NO_COARSE", "ODO_COARSE_MAX")
# route -> (child process, environment of the child, environment while the route's optimisers are created)
ROUTES = {
    "step": ("plain", {}, "ODO_LM_NO_FINE=1,ODO_LM_NO_COARSE=1"),
    "coarse": ("plain", {}, "ODO_LM_NO_FINE=1"),                       # ODO_COARSE_MAX unset: the coarse launch takes both levels
    "fine": ("fine", {"ODO_COARSE_MAX": "0"}, ""),                     # the persistent launch takes both levels, default workgroups
    "fine_k2": ("fine_k2", {"ODO_COARSE_MAX": "0", "ODO_LM_FINE_K": "2"}, ""),
}


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every Solve of this module: one child process per process-wide setting (ODO_COARSE_MAX, ODO_LM_FINE_K are read once)."""
    tmp = tmp_path_factory.mktemp("residual_edges")
    children = {}
    for route, (child, env, _) in ROUTES.items():
        children.setdefault(child, (env, []))[1].append(route)
    out = {}
    for child, (env, routes) in children.items():
        path = os.path.join(str(tmp), child + ".npz")
        e = {k: v for k, v in os.environ.items() if k not in _KNOBS}
        e.update(env)
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "residual_edge_cases.py"), path] +
                       [f"{r}:{ROUTES[r][2]}" for r in routes], check=True, env=e, timeout=300)
        out.update(np.load(path))
    return out


@pytest.fixture(scope="module")
def refs(O):
    """The oracle's Solve from every initial pose and its sums of the first evaluation (coarsest level), computed once."""
    img0, inv, img1 = cases.frames()
    r0, r1 = O.image_pyramid(img0, cases.LEVELS, True), O.image_pyramid(img1, cases.LEVELS, True)
    rd = O.depth_pyramid(inv, cases.LEVELS)
    flat = lambda levels: np.concatenate([l.ravel() for l in levels])
    params = O.lm_params(max_iters=tuple(cases.ITERS), robust=cases.ROBUST, huber_delta=cases.HUBER, K=cases.K)
    out = {}
    for name, T in cases.POSES.items():
        solve = O.lm_solve(flat(r0), flat(rd), flat(r1), cases.ROWS, cases.COLS, params, init=T)
        lvl = cases.LEVELS - 1
        first = O.lm_accumulate(r0[lvl], r1[lvl], rd[lvl], lvl, T, robust=cases.ROBUST, huber_delta=cases.HUBER, K=cases.K)
        out[name] = (solve, first)
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_routes_are_the_ones_meant(runs):
    for pose in cases.POSES:
        for kind in ("rec", "lean"):
            assert tuple(runs[f"step_{pose}_{kind}_meta"][2:]) == (0, 0) == tuple(runs[f"coarse_{pose}_{kind}_meta"][2:])
            for route in ("fine", "fine_k2"):
                k, redone = (int(v) for v in runs[f"{route}_{pose}_{kind}_meta"][2:])
                assert k > 0 and redone == 0, "the Solve did not run on the persistent launch"
            assert int(runs[f"fine_k2_{pose}_{kind}_meta"][2]) == 2
            # default: more workgroups than the finest level has virtual blocks (the second halves have none)
            assert int(runs[f"fine_{pose}_{kind}_meta"][2]) >= 3
        assert list(runs[f"step_{pose}_rec_points"]) == [24 * 32, 8 * 12]


@pytest.mark.parametrize("pose", list(cases.POSES))
def test_three_routes_give_the_same_bits(runs, pose):
    base_pose, base_meta = runs[f"step_{pose}_rec_pose"], runs[f"step_{pose}_rec_meta"]
    ti, tf = runs[f"step_{pose}_rec_trace_i"], runs[f"step_{pose}_rec_trace_f"]
    for route in ROUTES:
        for kind in ("rec", "lean"):
            key = f"{route}_{pose}_{kind}"
            assert np.array_equal(_bits(runs[key + "_pose"]), _bits(base_pose)), key
            assert tuple(runs[key + "_meta"][:2]) == tuple(base_meta[:2]), key    # status, evaluations
        key = f"{route}_{pose}_rec"
        assert runs[key + "_trace_i"].shape == ti.shape and np.array_equal(runs[key + "_trace_i"], ti), key
        assert np.array_equal(runs[key + "_trace_f"].view(np.uint64), tf.view(np.uint64)), key


@pytest.mark.parametrize("pose", list(cases.POSES))
def test_every_evaluations_count_and_the_first_sums_are_the_oracles(runs, refs, pose):
    solve, first = refs[pose]
    n_coarsest = 8 * 12
    u, v, z = cases.first_eval_coordinates(cases.POSES[pose])
    rows, cols = cases.ROWS >> (cases.LEVELS - 1), cases.COLS >> (cases.LEVELS - 1)
    # the case is what it is meant to be (chosen with the oracle; asserted so that it cannot pass vacuously)
    if pose in cases.PARTLY_OUT:
        assert 0 < solve["trace"][0]["n_res"] < n_coarsest and solve["trace"][0]["level"] == cases.LEVELS - 1
        band = {"u_high": (u >= cols - 1) & (u < cols), "u_low": (u >= -1) & (u < 0),
                "v_high": (v >= rows - 1) & (v < rows), "v_low": (v >= -1) & (v < 0)}[pose]
        beyond = {"u_high": u >= cols, "u_low": u < -1, "v_high": v >= rows, "v_low": v < -1}[pose]
        assert band.any() and beyond.any()
    elif pose in cases.ALL_OUT:
        assert first["acc"][28] == 0 and solve["status"] != 0
        if pose == "behind":
            assert (z <= 0).all()
    else:
        assert solve["trace"][0]["n_res"] == n_coarsest
    for route in ROUTES:
        key = f"{route}_{pose}_rec"
        status, n_evals = (int(x) for x in runs[key + "_meta"][:2])
        ti, tf = runs[key + "_trace_i"], runs[key + "_trace_f"]
        assert status == solve["status"], key
        if pose in cases.ALL_OUT:
            # the reference fails in its first evaluation (N == 0) and records nothing; what the device recorded of it holds N == 0
            assert (ti[:, 2] == 0).all() and len(ti) <= 1, key
            continue
        assert n_evals == solve["n_evals"] == len(ti), key
        for row, f, b in zip(ti, tf, solve["trace"]):
            print(key, "level", row[0], "iter", row[1], "N", row[2], "oracle N", b["n_res"], "err", f[0], "oracle err", b["err"])
            assert tuple(int(x) for x in row) == (b["level"], b["iter"], b["n_res"], b["accepted"], b["stop"]), key
            # err = float(sum 27 / sum 28) of sums held to 1e-11: one rounding to fp32 apart at the most
            assert abs(f[0] - b["err"]) <= 2.0 ** -23 * abs(b["err"]), key
    # the 29 sums of the first evaluation: the in-library reference (whose Solve the routes above equal bit for bit) against the oracle
    assert runs[f"{pose}_acc"][28] == first["acc"][28]
    np.testing.assert_allclose(runs[f"{pose}_acc"], first["acc"], rtol=1e-11, atol=1e-9)
