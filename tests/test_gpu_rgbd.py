"""RGB-D tracking on the GPU (odo_tracker_create_rgbd, api.RgbdTracker) against the numpy model of the spec and the model runner of
tests/test_rgbd_cpu.py: the sensor-depth conversion bit for bit, the frame loop over the pinned drive for every overlap mode and
announcement style, depth failure, mismatched entry points, lifecycle, an attached map and the absence of redone depth jobs."""
import numpy as np
import pytest

from conftest import se3_log_norm
from test_rgbd_cpu import DRIVE, MAX_DEPTH_STEP, N_FRAMES, drive, rgbd_depth_model, run_model, select_model, translation_errors

pytestmark = pytest.mark.gpu
TOL = 1e-5   # SE(3) log-map norm: the pose parity tolerance of every tracker test (the oracle's LM sums in its own order)


def _K(seq):
    k = seq["K"]
    return (k["f0"], k["cx0"], k["cy0"])


@pytest.fixture(scope="module")
def seq():
    return drive()


@pytest.fixture(scope="module")
def model(seq):
    return run_model(seq)


def _tracker(seq, **kw):
    from odometry_amd import api
    args = dict(depth_scale=seq["depth_scale"], max_depth_step=MAX_DEPTH_STEP, rows=480, cols=640, K=_K(seq))
    args.update(kw)
    return api.RgbdTracker(0, **args)


def _outputs_equal(trk, want, tag):
    val, disp, dep = trk.outputs(480, 640)
    assert np.array_equal(val, want["val"]), f"{tag}: mask differs at {int((val != want['val']).sum())} pixels"
    assert np.array_equal(dep.view(np.uint32), want["dep"].view(np.uint32)), f"{tag}: inverse depth differs"
    assert not disp.any(), f"{tag}: disparity is not zero"


# ---- conversion ---------------------------------------------------------------------------------------------------------------
def _hard_depth(seq, scale):
    """The drive's first depth frame at `scale`, with holes, out-of-range values, saturated readings and steps either side of the
    edge guard's bound written onto selected pixels."""
    from odometry_amd import synth
    gray = seq["gray"][0]
    Z = synth.Scene(DRIVE["seed"], **synth.DRIVES["natural"]["scene"]).render(seq["poses"][0], 480, 640, *_K(seq), 0.0)[1]
    raw = synth.sensor_depth(Z, scale, 1e9 if scale == 1000.0 else 10.0).astype(np.int64)
    sel = np.argwhere(select_model(gray, 1) != 0)
    rng = np.random.default_rng(5)
    pick = sel[rng.permutation(len(sel))]
    for k, (y, x) in enumerate(pick[:3000]):
        kind = k % 6
        if kind == 0:
            raw[y, x] = 0
        elif kind == 1:
            raw[y, x] = 65535
        elif kind == 2:
            raw[y, x] = int(0.05 * scale)               # 5 cm: nearer than min_depth
        elif kind in (3, 4) and 0 < x < 639 and raw[y, x] > 100:
            r = int(raw[y, x])
            lim = np.float32(MAX_DEPTH_STEP) * np.float32(r)
            step = int(np.floor(lim)) + (1 if kind == 4 else 0)   # exactly at the bound (kept) / one unit past it (dropped)
            raw[y, x + 1] = min(65535, r + step)
    return np.clip(raw, 0, 65535).astype(np.uint16)


@pytest.mark.parametrize("scale,step,boundary", [(1000.0, MAX_DEPTH_STEP, 1), (5000.0, MAX_DEPTH_STEP, 4), (1000.0, np.inf, 4),
                                                 (5000.0, 0.0, 2)])
def test_conversion_matches_the_model_bit_for_bit(seq, scale, step, boundary):
    gray, raw = seq["gray"][0], _hard_depth(seq, scale)
    val, dep, st = rgbd_depth_model(gray, raw, scale, step, boundary)
    trk = _tracker(seq, depth_scale=scale, max_depth_step=step, boundary=boundary)
    g, d = trk.upload_frame(gray), trk.upload_depth(raw)
    if st["status"] == 0:
        trk.init(g, d)
    else:
        with pytest.raises(Exception):
            trk.init(g, d)
    _outputs_equal(trk, dict(val=val, dep=dep), f"scale {scale} step {step} boundary {boundary}")
    rep = trk.depth_report()
    assert rep == dict(iters=0, cost=0.0, n_selected=st["n_selected"], n_matched=st["n_matched"], n_valid=st["n_valid"]), (rep, st)
    assert trk.stats()["depth_iters"] == 0
    trk.close()


# ---- tracking -----------------------------------------------------------------------------------------------------------------
def _check_row(k, g, c):
    assert g["solve_status"] == c["solve_status"], f"frame {k}: Solve status"
    assert g["new_keyframe"] == c["new_keyframe"], f"frame {k}: keyframe decision differs"
    d_kf = se3_log_norm(c["pose_to_keyframe"], g["pose_to_keyframe"])
    d_abs = se3_log_norm(c["abs_pose"], g["abs_pose"])
    assert d_kf < TOL and d_abs < TOL, f"frame {k}: pose log-norms {d_kf} {d_abs}"
    assert abs(g["motion"] - c["motion"]) < 1e-5, f"frame {k}: motion score"


@pytest.mark.parametrize("hints", ["none", "gray", "rgbd"])
@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_tracking_matches_the_model_runner(seq, model, overlap, hints):
    rows, n_kf = model
    trk = _tracker(seq, overlap_depth=overlap)
    dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])]
    trk.init(*dev[0])
    _outputs_equal(trk, rows[0], "frame 0")
    got = [None]
    for k in range(1, N_FRAMES):
        if k + 1 < N_FRAMES and hints == "gray":
            trk.hint_next(dev[k + 1][0])
        elif k + 1 < N_FRAMES and hints == "rgbd":
            trk.hint_next(*dev[k + 1])
        g = trk.track(*dev[k])
        _check_row(k, g, rows[k])
        _outputs_equal(trk, rows[k], f"frame {k}")
        assert trk.stats()["n_valid_depth"] == rows[k]["n_valid"]
        got.append(g)
    assert trk.stats()["n_keyframes"] == n_kf >= 3
    assert trk.depth_persistent_stats() == (0, 0)   # the stereo depth LM's persistent launch is never issued: nothing to redo
    trk.close()
    err = translation_errors(got, seq["poses"])
    assert np.mean(err < 0.05) >= 0.9, np.round(err, 3)


# ---- depth failure ------------------------------------------------------------------------------------------------------------
def test_depth_failure_at_init_and_in_track(seq):
    from odometry_amd import _lib as L
    sparse = np.zeros_like(seq["depth"][1])
    sparse[::40, ::40] = seq["depth"][1][::40, ::40]          # a few hundred readings: < 500 valid
    trk = _tracker(seq)
    g0, g1 = trk.upload_frame(seq["gray"][0]), trk.upload_frame(seq["gray"][1])
    d0, d_sparse = trk.upload_depth(seq["depth"][0]), trk.upload_depth(sparse)
    with pytest.raises(L.OdoError, match="Init 0-th frame failed!"):
        trk.init(g0, d_sparse)
    trk.init(g0, d0)
    T = np.zeros(16, np.float32)
    A = np.full(16, np.nan, np.float32)
    import ctypes as C
    nk, ss, mag = C.c_int(7), C.c_int(7), C.c_float(7)
    rc = trk.lib.odo_tracker_track_rgbd(trk.h, g1, d_sparse, T.ctypes.data_as(C.POINTER(C.c_float)), A.ctypes.data_as(C.POINTER(C.c_float)),
                                        C.byref(nk), C.byref(mag), C.byref(ss))
    assert rc == -1 and "depth failed" in L.last_error()
    assert np.isfinite(A).all() and abs(A[14] - seq["poses"][1][2, 3]) < 0.05   # the pose is still written (ref: :218 before :230)
    assert trk.depth_report()["n_valid"] < 500
    trk.close()


# ---- entry points -------------------------------------------------------------------------------------------------------------
def test_mismatched_entry_points_are_refused_and_change_nothing(seq, model):
    from odometry_amd import _lib as L, api
    import ctypes as C
    rows, _ = model
    trk = _tracker(seq)
    st = api.Tracker(0)
    g = [trk.upload_frame(x) for x in seq["gray"][:4]]
    d = [trk.upload_depth(x) for x in seq["depth"][:4]]
    pose = np.eye(4, dtype=np.float32).reshape(-1)
    fp = pose.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros(16, np.float32)
    T = out.ctypes.data_as(C.POINTER(C.c_float))
    assert trk.lib.odo_tracker_init(trk.h, g[0], d[0], fp) == -1 and "odo_tracker_init_rgbd" in L.last_error()
    assert trk.lib.odo_tracker_track(trk.h, g[0], d[0], T, T, None, None, None) == -1 and "odo_tracker_track_rgbd" in L.last_error()
    assert trk.lib.odo_tracker_hint_next_pair(trk.h, g[1], d[1]) == -1 and "odo_tracker_hint_next_rgbd" in L.last_error()
    assert st.lib.odo_tracker_init_rgbd(st.h, g[0], d[0], fp) == -1 and "odo_tracker_init" in L.last_error()
    assert st.lib.odo_tracker_track_rgbd(st.h, g[0], d[0], T, T, None, None, None) == -1 and "odo_tracker_track" in L.last_error()
    assert st.lib.odo_tracker_hint_next_rgbd(st.h, g[1], d[1]) == -1 and "odo_tracker_hint_next_pair" in L.last_error()
    st.close()
    # the RGB-D tracker still tracks as a fresh one, and a re-init with another sequence behaves like a fresh tracker
    for start in (0, 0):
        trk.init(g[start], d[start])
        for k in (1, 2, 3):
            _check_row(k, trk.track(g[k], d[k]), rows[k])
            _outputs_equal(trk, rows[k], f"frame {k}")
    trk.close()


def test_reinit_with_a_new_sequence_behaves_like_a_fresh_tracker(seq):
    from odometry_amd import synth
    seq2 = synth.make_rgbd_sequence(4, **dict(DRIVE, seed=1))
    rows2, _ = run_model(seq2)
    trk = _tracker(seq)
    g = [trk.upload_frame(x) for x in seq["gray"][:3]]
    d = [trk.upload_depth(x) for x in seq["depth"][:3]]
    trk.init(g[0], d[0])
    trk.hint_next(g[2], d[2])
    trk.track(g[1], d[1])   # leaves an announced frame behind
    g2 = [trk.upload_frame(x) for x in seq2["gray"]]
    d2 = [trk.upload_depth(x) for x in seq2["depth"]]
    trk.init(g2[0], d2[0])
    _outputs_equal(trk, rows2[0], "re-init")
    for k in (1, 2, 3):
        if k + 1 < 4:
            trk.hint_next(g2[k + 1], d2[k + 1])
        _check_row(k, trk.track(g2[k], d2[k]), rows2[k])
        _outputs_equal(trk, rows2[k], f"frame {k}")
    trk.close()


def test_quiesce_and_destroy_after_an_announced_pair_that_was_never_tracked(seq):
    trk = _tracker(seq)
    g = [trk.upload_frame(x) for x in seq["gray"][:3]]
    d = [trk.upload_depth(x) for x in seq["depth"][:3]]
    trk.init(g[0], d[0])
    trk.hint_next(g[1], d[1])
    trk.track(g[1], d[1])
    trk.hint_next(g[2], d[2])          # announced, never tracked
    trk.close()                         # quiesce + free + destroy
    trk2 = _tracker(seq)
    g = [trk2.upload_frame(x) for x in seq["gray"][:2]]
    d = [trk2.upload_depth(x) for x in seq["depth"][:2]]
    trk2.init(g[0], d[0])
    trk2.hint_next(g[1], d[1])
    trk2._sync()
    trk2.close()


# ---- map ----------------------------------------------------------------------------------------------------------------------
def test_attached_map_equals_standalone_insertion_of_the_keyframes(seq, model):
    from odometry_amd import api
    rows, n_kf = model
    trk = _tracker(seq)
    m = api.PointMap(trk, 480, 640, 4_000_000, 0.05)
    trk.attach_map(m)
    dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])]
    trk.init(*dev[0])
    kfs = [(rows[0]["val"], rows[0]["dep"], 0, np.eye(4, dtype=np.float32))]
    for k in range(1, N_FRAMES):
        if k + 1 < N_FRAMES:
            trk.hint_next(*dev[k + 1])
        g = trk.track(*dev[k])
        if g["new_keyframe"]:
            val, _, dep = trk.outputs(480, 640)
            kfs.append((val, dep, k, g["abs_pose"]))
    trk.attach_map(None)
    got = m.points()
    st = m.stats()
    ref = api.PointMap(trk, 480, 640, 4_000_000, 0.05)
    for val, dep, k, A in kfs:   # mask, inverse depth, level-0 pyramid image, abs_pose
        ref.insert(val, dep, api.ImagePyramid(4, seq["gray"][k], True).GetPyramidImage(0), _K(seq), A)
    want = ref.points()
    assert len(kfs) == n_kf and st["insertions"] == n_kf
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert st == ref.stats()
    ref.close()
    m.close()
    trk.close()
