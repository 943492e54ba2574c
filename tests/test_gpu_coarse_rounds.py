"""The one-workgroup coarse launch at the edges of its rounds (lm_coarse_body). It is the point lists' first consumer, and its shape
changes with the level's point count: one virtual block of 256 points with the short fold, one round on both halves of the
workgroup, a second round on half 0 only, two full rounds up to kCoarseMaxPoints; one point more and the level goes to the step
launches. tests/test_gpu_fine_gather.py runs with ODO_COARSE_MAX=0, where the coarse launch takes nothing; here ODO_COARSE_MAX is
unset and ODO_LM_NO_FINE=1 keeps the persistent launch away, so the coarse launch takes every level it can hold. It must give what
the step launches give (ODO_LM_NO_FINE=1 ODO_LM_NO_COARSE=1) bit for bit — pose, status, evaluation count and every trace row."""
import os
import re

import numpy as np
import pytest

from conftest import se3_log_norm
import fine_gather_cases as cases
from test_gpu_fine_gather import ROOT, _child

pytestmark = pytest.mark.gpu


def _constant(pattern):
    src = open(os.path.join(ROOT, "odometry_amd", "csrc", "kernels.hip.h")).read()
    m = re.search(pattern, src)
    assert m, "kernels.hip.h no longer holds `%s`: the cases here are placed around that constant" % pattern
    return int(m.group(1))


MAX_POINTS, BLOCK = _constant(r"constexpr int kCoarseMaxPoints = (\d+);"), _constant(r"#define ODO_COARSE_BLOCK (\d+)\n")
# points -> shape of the launch: 1 .. 256 one virtual block; 257 .. 512 one round, both halves; 513 .. 768 a second round on half 0
# only; 769 .. 1024 two full rounds; 1025: not the coarse launch's any more. And the wave edges of the first block.
COUNTS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025]


def test_counts_sit_on_the_round_edges():
    assert (MAX_POINTS, BLOCK) == (1024, 512)
    assert {BLOCK // 2, BLOCK, BLOCK + BLOCK // 2, MAX_POINTS} <= set(COUNTS)
    assert all(n - 1 in COUNTS and n + 1 in COUNTS for n in (BLOCK // 2, BLOCK, BLOCK + BLOCK // 2, MAX_POINTS))
    assert max(COUNTS) <= cases.INTERIOR


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every Solve of this module in one child process, ODO_COARSE_MAX unset."""
    tmp = tmp_path_factory.mktemp("coarse_rounds")
    return _child(tmp, "coarse", COUNTS, {}, ["--under", "coarse:ODO_LM_NO_FINE=1", "--base", "step:ODO_LM_NO_FINE=1,ODO_LM_NO_COARSE=1",
                                              "--trace"])


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("n", COUNTS)
def test_coarse_launch_equals_step_launches_and_oracle(runs, O, n, mode):
    pose, meta = runs[f"{n}_{mode}_coarse_pose"], runs[f"{n}_{mode}_coarse_meta"]
    pose_s, meta_s = runs[f"{n}_{mode}_step_pose"], runs[f"{n}_{mode}_step_meta"]
    status, n_evals, n_pts, k_fine, redone = (int(v) for v in meta)
    assert n_pts == n == int(meta_s[2]), "the inverse-depth image does not give the point count this case is about"
    assert (k_fine, redone) == (0, 0) == tuple(int(v) for v in meta_s[3:]), "a persistent launch took part"
    # the coarse launch did the level in ONE launch; one point above its reach it did not
    launches, launches_s = int(runs[f"{n}_{mode}_coarse_launches"][0]), int(runs[f"{n}_{mode}_step_launches"][0])
    if n <= MAX_POINTS:
        assert launches == 1, "%d launches: the coarse launch did not run the level alone" % launches
        assert launches_s > 1 or int(meta_s[1]) <= 1
    else:
        assert launches > 1 and launches_s > 1
    # (a) the step launches: bit for bit, trace rows field for field
    assert np.array_equal(pose.view(np.uint32), pose_s.view(np.uint32)) and (status, n_evals) == (int(meta_s[0]), int(meta_s[1]))
    ti, ti_s = runs[f"{n}_{mode}_coarse_trace_i"], runs[f"{n}_{mode}_step_trace_i"]
    tf, tf_s = runs[f"{n}_{mode}_coarse_trace_f"], runs[f"{n}_{mode}_step_trace_f"]
    assert len(ti) > 0 and ti.shape == ti_s.shape, "%d trace rows against %d" % (len(ti), len(ti_s))
    assert np.array_equal(ti, ti_s), "trace rows differ in %s" % [cases.TRACE_INT[c] for c in np.unique(np.argwhere(ti != ti_s)[:, 1])]
    assert np.array_equal(tf.view(np.uint64), tf_s.view(np.uint64)), "trace rows differ in err / lambda / delta"
    assert (ti[:, 2] <= n).all()
    # (b) the oracle, as the parity tests hold it
    img0, inv, img1 = cases.frames(n)
    ref = O.lm_solve(img0.ravel(), inv.ravel(), img1.ravel(), cases.ROWS, cases.COLS,
                     O.lm_params(max_iters=tuple(cases.ITERS), robust=mode, K=cases.K))
    assert status == ref["status"] and n_evals == ref["n_evals"]
    if status == 0:
        assert se3_log_norm(ref["pose"], pose) < 1e-5
