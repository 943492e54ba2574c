"""The persistent launch's row gather at the edges of its row map (lm_fine_body, step (c)): levels of at most kFineSoloRows virtual
blocks are gathered by wave 0 alone and folded in registers, larger ones by four waves through LDS. Both must give the sums of
the step launches bit for bit — the additions and their order are the same — at every block count where a lane, a segment or a
path comes into or goes out of use."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import se3_log_norm
import fine_gather_cases as cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _solo_rows():
    src = open(os.path.join(ROOT, "odometry_amd", "csrc", "kernels.hip.h")).read()
    m = re.search(r"constexpr int kFineSoloRows = (\d+);", src)
    assert m, "kernels.hip.h no longer declares `constexpr int kFineSoloRows = <n>;`: the cases here are placed around that constant"
    return int(m.group(1))


S = _solo_rows()
# N -> virtual blocks: 1 (segments 1-7 empty: their + 0.0 stays), 2 and 4 (lower-half segments only), 5 and 8 (first use of the
# upper-half lanes; every segment one row), 9 (first segment with two rows), S (the solo path's last size), S + 1 (the four-wave
# path's first)
COUNTS = [n for n in sorted({1, 255, 256, 257, 1024, 1025, 2048, 2049, 256 * S, 256 * S + 1}) if n <= cases.INTERIOR]


def _child(tmp, name, counts, env, options=()):
    out = os.path.join(str(tmp), name + ".npz")
    e = {k: v for k, v in os.environ.items() if k not in ("ODO_HOME_XCD", "ODO_NO_HOME_XCD", "ODO_LM_NO_FINE", "ODO_LM_FINE_K",
                                                          "ODO_LM_NO_COARSE", "ODO_COARSE_MAX")}
    e.update(env)
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fine_gather_cases.py"), out] + list(options) + [str(n) for n in counts],
                   check=True, env=e, timeout=300)
    return np.load(out)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every Solve of this module, in two child processes: the library reads ODO_COARSE_MAX (0: the persistent launch takes a level
    of any size) and ODO_HOME_XCD (home XCDs on: no placement handshake) once per process."""
    tmp = tmp_path_factory.mktemp("fine_gather")
    roam = _child(tmp, "roam", COUNTS, {"ODO_COARSE_MAX": "0"})                          # ODO_HOME_XCD unset: home < 0, the handshake
    home = _child(tmp, "home", [256, 2049, 256 * S + 1], {"ODO_COARSE_MAX": "0", "ODO_HOME_XCD": "1"})
    return roam, home


@pytest.mark.parametrize("mode", cases.MODES)
@pytest.mark.parametrize("n", COUNTS)
def test_gather_paths_equal_step_launches_and_oracle(runs, O, n, mode):
    roam, _ = runs
    pose, meta = roam[f"{n}_{mode}_fine_pose"], roam[f"{n}_{mode}_fine_meta"]
    pose_s, meta_s = roam[f"{n}_{mode}_step_pose"], roam[f"{n}_{mode}_step_meta"]
    status, n_evals, n_pts, k_fine, redone = (int(v) for v in meta)
    assert n_pts == n, "the inverse-depth image does not give the block count this case is about"
    assert k_fine > 0 and redone == 0, "the Solve did not run on the persistent launch"
    assert tuple(int(v) for v in meta_s[3:]) == (0, 0)
    # (a) the step launches: bit for bit
    assert np.array_equal(pose, pose_s) and (status, n_evals) == (int(meta_s[0]), int(meta_s[1]))
    # (b) the oracle, as the parity tests hold it
    img0, inv, img1 = cases.frames(n)
    ref = O.lm_solve(img0.ravel(), inv.ravel(), img1.ravel(), cases.ROWS, cases.COLS,
                     O.lm_params(max_iters=tuple(cases.ITERS), robust=mode, K=cases.K))
    assert status == ref["status"] and n_evals == ref["n_evals"]
    if status == 0:
        assert se3_log_norm(ref["pose"], pose) < 1e-5


@pytest.mark.parametrize("mode", cases.MODES)
def test_no_placement_handshake_on_a_home_xcd(runs, mode):
    """ODO_HOME_XCD=1: every workgroup that takes part found itself on the optimiser's home XCD, so the launch skips the exchange of
    XCC ids; without it (the default) the workgroups ask each other. Same pose either way, on both gather paths.
    (What this cannot see: the library hands out homes only if its probe finds eight distinct XCC ids — on a device where it does
    not, home stays < 0 under ODO_HOME_XCD=1 as well and both children take the handshake. No statistic of the API tells the two
    apart; a whole MI355X shows eight ids.)"""
    roam, home = runs
    for n in (256, 2049, 256 * S + 1):
        assert int(home[f"{n}_{mode}_fine_meta"][3]) > 0 and int(home[f"{n}_{mode}_fine_meta"][4]) == 0
        assert np.array_equal(home[f"{n}_{mode}_fine_pose"], roam[f"{n}_{mode}_fine_pose"])
        assert np.array_equal(home[f"{n}_{mode}_fine_meta"][:3], roam[f"{n}_{mode}_fine_meta"][:3])


def test_batched_launch_gathers_small_levels_like_the_single_tracker(kitti_seq):
    """Two sequences in lock step (lm_fine_kernel_batch shares lm_fine_body): sequence 0 equals the single tracker on a keyframe
    whose levels take both gathers inside one launch (this fixture's keyframe: 7 virtual blocks on level 2, 28 and 113 below)."""
    from odometry_amd import api
    n_frames = 3
    trk = api.Tracker()
    L = [trk.upload_frame(f) for f in kitti_seq["left"][:n_frames]]
    R = [trk.upload_frame(f) for f in kitti_seq["right"][:n_frames]]
    trk.init(L[0], R[0])
    single = [trk.track(L[k], R[k]) for k in range(1, n_frames)]
    pts = trk.lm_points()[0]
    assert trk.persistent_stats()[0] > 0 and trk.persistent_stats()[1] == 0
    trk.close()
    blocks = [(p + 255) // 256 for p in pts]
    assert blocks[2] <= S < blocks[1] <= 64, blocks   # level 2: the solo gather; level 1: the four-wave gather, points resident
    tb = api.TrackerBatch(2)
    Lb = [tb.upload_frame(f) for f in kitti_seq["left"][:n_frames]]
    Rb = [tb.upload_frame(f) for f in kitti_seq["right"][:n_frames]]
    tb.init([Lb[0], Lb[0]], [Rb[0], Rb[0]])
    for k in range(1, n_frames):
        res = tb.track([Lb[k], Lb[k]], [Rb[k], Rb[k]])
        assert res[0]["status"] == 0
        assert np.array_equal(res[0]["pose_to_keyframe"], single[k - 1]["pose_to_keyframe"]), k
        assert np.array_equal(res[0]["abs_pose"], single[k - 1]["abs_pose"]), k
    tb.close()
