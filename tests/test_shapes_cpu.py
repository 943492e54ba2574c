"""Every row of tests/shape_cases.py's table is a valid input, shown with the CPU runners alone (the oracle for the stereo rows, the
RGB-D model runner for the others): every frame's Solve succeeds, every frame has at least 500 valid depths (what ComputeDepth and
the sensor-depth conversion require), and the runner switches keyframe at least once. tests/test_gpu_shapes.py holds the trackers to
the same runs."""
import numpy as np
import pytest

import shape_cases as S


@pytest.fixture(scope="module")
def runs():
    return S.prepare(S.TABLE)


def test_the_table_holds_the_shapes_it_is_there_for():
    ids = [S.case_id(c) for c in S.TABLE]
    assert len(ids) == len(set(ids)) >= 18   # the table may grow
    tile = lambda c: ((c["cols"] - 8) // 32) * ((c["rows"] - 8) // 16)   # noqa: E731  (boundary 4)
    assert max(tile(c) for c in S.TABLE) == 4096                          # the selection's bound itself
    assert any(c["cols"] % 4 == 3 and c["rows"] % 2 == 1 for c in S.STEREO) and any(c["cols"] % 4 == 3 and c["rows"] % 2 == 1 for c in S.RGBD_ROWS)
    assert {c["levels"] for c in S.STEREO} == {c["levels"] for c in S.RGBD_ROWS} == {3, 4, 5}
    assert S.lm_max_iters(3) == (10, 20, 30) and S.lm_max_iters(4) == (10, 20, 30, 30) and S.lm_max_iters(5) == (10, 20, 30, 30, 30)
    f, cx, cy = S.intrinsics(S.find("rgbd", 240, 424, 4))
    assert (f, cx, cy) == (525.0 * 424 / 640, 211.5, 119.5)


@pytest.mark.parametrize("cid", [S.case_id(c) for c in S.TABLE])
def test_row_is_a_valid_input(runs, cid):
    r = runs[cid]
    c, rows = r["case"], r["rows"]
    assert len(rows) == c["frames"] and len(r["seq"]["left" if c["kind"] == "stereo" else "gray"]) == c["frames"]
    assert r["seq"]["left" if c["kind"] == "stereo" else "gray"][0].shape == (c["rows"], c["cols"])
    for k, row in enumerate(rows):
        assert row["n_valid"] >= 500, f"frame {k}: {row['n_valid']} valid depths"
        if k:
            assert row["solve_status"] == 0, f"frame {k}: Solve status {row['solve_status']}"
            assert np.isfinite(row["abs_pose"]).all()
    assert r["n_keyframes"] >= 2, "the runner never switches keyframe"
    err = [float(np.linalg.norm(row["abs_pose"][:3, 3].astype(np.float64) - np.asarray(P)[:3, 3]))
           for row, P in zip(rows[1:], r["seq"]["poses"][1:])]
    print(f"{cid}: {c['frames']} frames, min valid depths {min(row['n_valid'] for row in rows)}, keyframes {r['n_keyframes']}, "
          f"translation error against the drive's poses (not asserted) max {max(err):.3f} m")


def test_stereo_120x160_with_four_levels_is_not_a_valid_input():
    """Level 3 is 15x20 with a 7x12 interior: the oracle's Solve fails on frames of this drive, and OracleRunner, which inverts the
    returned pseudo-identity, raises. The runner variant that does not invert a failed pose gets through; the GPU test of this case
    compares the tracker's solve_status with it frame by frame."""
    from oracle import runner as orunner
    c = dict(S.find("stereo", 120, 160, 3), levels=4)
    seq = S.render(c)
    with pytest.raises(np.linalg.LinAlgError):
        S.run_stereo(c, seq, orunner.OracleRunner)
    rows, _ = S.run_stereo(c, seq, S.tolerant_runner())
    status = [r["solve_status"] for r in rows[1:]]
    assert any(s != 0 for s in status), status
    assert all((r["abs_pose"] is None) == (r["solve_status"] != 0) for r in rows[1:])
