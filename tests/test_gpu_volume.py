"""The TSDF volume on the GPU (odo_volume_*, api.TsdfVolume) against the numpy model of tests/test_volume_cpu.py: the grid and the
counters after every integration and the extracted surface bit for bit on two rigs, capacity / clear / empty volumes, and a volume
attached to an RgbdTracker over the pinned drive: the tracker's results unchanged, the volume equal to a standalone one fed the same
frames and poses, the integration rule for failed frames, lifecycle, and the front end's ring as the source of the depth frames."""
import ctypes as C

import numpy as np
import pytest

from test_rgbd_cpu import MAX_DEPTH_STEP, N_FRAMES, drive, translation_errors
from test_volume_cpu import _pose, bits, empty_grid, extract_model, integrate_model, params, plane_errors, report

pytestmark = pytest.mark.gpu


def _K(seq):
    k = seq["K"]
    return (k["f0"], k["cx0"], k["cy0"])


def _volume(owner, p):
    from odometry_amd import api
    return api.TsdfVolume(owner, p["dims"], p["vs"], p["origin"], p["mu"], p["max_depth"], p["max_weight"], p["size"], p["K"],
                          p["depth_scale"])


def _tracker(seq, **kw):
    from odometry_amd import api
    args = dict(depth_scale=seq["depth_scale"], max_depth_step=MAX_DEPTH_STEP, rows=480, cols=640, K=_K(seq))
    args.update(kw)
    return api.RgbdTracker(0, **args)


def _grid_equal(vol, q, w, tag):
    gq, gw = vol.grid()
    assert np.array_equal(gw, w), f"{tag}: weights differ at {int((gw != w).sum())} voxels"
    assert np.array_equal(gq, q), f"{tag}: distances differ at {int((gq != q).sum())} voxels"


def _points_equal(got, want, tag):
    assert got[0].shape == want[0].shape, f"{tag}: {len(got[0])} points, the model has {len(want[0])}"
    assert np.array_equal(bits(got[0]), bits(want[0])), f"{tag}: positions differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{tag}: normals / weights differ"


@pytest.fixture(scope="module")
def seq():
    return drive()


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def second_rig():
    """What the pinned case does not exercise: a pose with real rotation about all three axes and a start away from the origin, a
    grid the camera sits inside (voxels behind it), dimensions that are no multiples of 64 / 4, a depth frame with holes and 65535s,
    max_weight 3 over six frames, TUM's 5000 units per metre."""
    from odometry_amd import synth
    rows, cols, K = 300, 420, (310.0, 207.3, 151.8)
    scene = synth.drive_scene("natural", 0)
    p = params(K, 5000.0, (rows, cols), dims=(101, 75, 83), vs=0.07, origin=(-3.1, -3.2, 1.0), mu=0.2, max_depth=8.0, max_weight=3)
    rng = np.random.default_rng(11)
    frames = []
    for n in range(6):
        A = _pose((0.25 - 0.03 * n, -0.35 + 0.05 * n, 0.15 + 0.02 * n), (0.4 - 0.1 * n, -0.3 + 0.02 * n, 3.0 - 0.2 * n))
        Z = scene.render(A, rows, cols, *K, 0.0)[1]
        raw = synth.sensor_depth(Z, 5000.0, 30.0)          # beyond 13.1 m: no reading
        raw[rng.uniform(size=raw.shape) < 0.03] = 0
        raw[rng.uniform(size=raw.shape) < 0.02] = 65535
        raw[40:80, 100:180] = 0
        frames.append((raw, A))
    return p, frames


# ---- integration and extraction against the model ------------------------------------------------------------------------------
def _run_rig(ctx, p, frames, check_at, tag):
    vol = _volume(ctx, p)
    q, w = empty_grid(p)
    assert vol.stats() == dict(frames=0, updated=0, in_band=0, cumulative=0)
    assert [len(a) for a in vol.extract(100)] == [0, 0]                       # an empty volume yields no point
    total = 0
    for n, (raw, A) in enumerate(frames):
        vol.integrate(raw, A)
        q, w, upd, band = integrate_model(q, w, raw, A, p)
        total += upd
        st = vol.stats()
        print(f"{tag} frame {n}: updated {st['updated']} in band {st['in_band']}")
        assert st == dict(frames=n + 1, updated=upd, in_band=band, cumulative=total), (tag, n, st, upd, band)
        if n + 1 in check_at:
            _grid_equal(vol, q, w, f"{tag} after {n + 1} integrations")
    want = extract_model(q, w, p)
    cap = len(want[0]) + 1000
    got = vol.extract(cap, with_dropped=True)
    _points_equal(got, want, tag)
    assert got[2] == 0 and len(want[0]) > 1000
    _grid_equal(vol, q, w, f"{tag} after the extraction")                     # extraction does not modify the grid
    few = len(want[0]) // 3
    part = vol.extract(few, with_dropped=True)                                # below the count: the first points, the rest dropped
    _points_equal(part, (want[0][:few], want[1][:few]), f"{tag} capacity {few}")
    assert part[2] == len(want[0]) - few
    n = C.c_long(-1)
    d = C.c_long(-1)
    assert vol.lib.odo_volume_extract(vol.h, 0, None, None, C.byref(n), C.byref(d)) == 0 and (n.value, d.value) == (0, len(want[0]))
    _points_equal(vol.extract(cap), want, f"{tag} again")                     # a pure function of the volume
    return vol, (q, w), want


def test_pinned_case_matches_the_model_bit_for_bit(ctx, seq):
    p = params(seq)
    frames = [(seq["depth"][k], seq["poses"][k]) for k in range(10)]
    vol, _, want = _run_rig(ctx, p, frames, (1, 2, 10), "pinned")
    dist, dots, ln, zero = plane_errors(*want, p["vs"])
    report("true poses, GPU", dist, dots, ln, zero)
    # clear restarts from nothing
    vol.clear()
    assert vol.stats() == dict(frames=0, updated=0, in_band=0, cumulative=0)
    assert [len(a) for a in vol.extract(100)] == [0, 0]
    q, w = empty_grid(p)
    _grid_equal(vol, q, w, "cleared")
    vol.integrate(*frames[3])
    q, w, upd, band = integrate_model(q, w, *frames[3], p)
    _grid_equal(vol, q, w, "after clear + 1")
    assert vol.stats() == dict(frames=1, updated=upd, in_band=band, cumulative=upd)
    vol.close()


def test_second_rig_matches_the_model_bit_for_bit(ctx):
    p, frames = second_rig()
    vol, (q, w), _ = _run_rig(ctx, p, frames, (1, 2, 6), "second rig")
    assert w.max() == 3 and (w == 3).sum() > 1000                             # the weight saturated
    vol.close()


def test_non_finite_poses_and_bad_arguments_are_refused(ctx, seq):
    from odometry_amd import _lib as L
    p = params(seq, dims=(32, 16, 24), vs=0.08, origin=(-1.28, 0.9, 3.6))   # the ground, 3.6 to 5.5 m ahead, crosses it
    vol = _volume(ctx, p)
    vol.integrate(seq["depth"][0], seq["poses"][0])
    q, w, upd, band = integrate_model(*empty_grid(p), seq["depth"][0], seq["poses"][0], p)
    _grid_equal(vol, q, w, "32 x 16 x 24 after one integration")
    assert vol.stats() == dict(frames=1, updated=upd, in_band=band, cumulative=upd) and upd > 0
    before = vol.stats(), vol.grid()
    d = ctx.upload(seq["depth"][1])
    for bad in (np.nan, np.inf, -np.inf):
        A = np.array(seq["poses"][1], np.float32)
        A[1, 3] = bad
        with pytest.raises(L.OdoError, match="non-finite"):
            vol.integrate(d, A)
    assert vol.lib.odo_volume_integrate_dev(vol.h, None, None) == -1
    assert vol.lib.odo_volume_extract(vol.h, 10, None, None, None, None) == -1
    after = vol.stats(), vol.grid()
    assert before[0] == after[0] and np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
    _grid_equal(vol, q, w, "32 x 16 x 24 after the refused calls")
    ctx.free(d)
    vol.close()


# ---- attached to a tracker -----------------------------------------------------------------------------------------------------
def _row(trk, res):
    val, _, dep = trk.outputs(480, 640)
    return dict(res, val=val, dep=dep)


def _run(trk, dev, hints):
    trk.init(*dev[0])
    rows = [_row(trk, dict(abs_pose=np.eye(4, dtype=np.float32), solve_status=0))]
    for k in range(1, len(dev)):
        if k + 1 < len(dev) and hints:
            trk.hint_next(*dev[k + 1])
        rows.append(_row(trk, trk.track(*dev[k])))
    return rows


def _rows_equal(a, b, tag):
    assert len(a) == len(b)
    for k, (g, c) in enumerate(zip(a, b)):
        assert np.array_equal(g["val"], c["val"]), f"{tag} frame {k}: mask differs"
        assert np.array_equal(bits(g["dep"]), bits(c["dep"])), f"{tag} frame {k}: inverse depth differs"
        if k == 0:
            continue
        assert g["new_keyframe"] == c["new_keyframe"] and g["solve_status"] == c["solve_status"], f"{tag} frame {k}: decisions differ"
        for key in ("pose_to_keyframe", "abs_pose"):
            assert np.array_equal(bits(g[key]), bits(c[key])), f"{tag} frame {k}: {key} differs"
        assert g["motion"] == c["motion"], f"{tag} frame {k}: motion score differs"


def _standalone(trk, p, dev, rows):
    """A volume of its own fed the device frames and the poses the tracker returned."""
    ref = _volume(trk, p)
    for (_, d), r in zip(dev, rows):
        ref.integrate(d, r["abs_pose"])
    return ref


def _volumes_equal(a, b, tag):
    qa, wa = a.grid()
    _grid_equal(b, qa, wa, tag)
    assert a.stats() == b.stats(), (tag, a.stats(), b.stats())


@pytest.mark.parametrize("hints", [False, True])
@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_attached_volume_changes_nothing_and_equals_a_standalone_volume(seq, overlap, hints):
    p = params(seq)
    plain = _tracker(seq, overlap_depth=overlap)
    want = _run(plain, [(plain.upload_frame(g), plain.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])], hints)
    plain.close()
    trk = _tracker(seq, overlap_depth=overlap)
    vol = _volume(trk, p)
    trk.attach_volume(vol)
    dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])]
    got = _run(trk, dev, hints)
    _rows_equal(got, want, f"overlap {overlap} hints {hints}")
    assert all(g["solve_status"] == 0 for g in got) and sum(1 for g in got[1:] if g["new_keyframe"]) >= 2
    st = vol.stats()
    assert st["frames"] == N_FRAMES and st["cumulative"] > 10_000_000, st
    ref = _standalone(trk, p, dev, got)
    _volumes_equal(vol, ref, f"overlap {overlap} hints {hints}")
    ref.close()
    vol.close()     # detaches
    trk.close()


def test_tracked_poses_against_the_corridors_planes(seq):
    """DESIGN.md section 9.4 quotes these figures beside the true-pose ones. There is no reference to derive a bound for them from:
    the test asserts the absence of failed frames and that the attached volume is the standalone one."""
    p = params(seq)
    for n in (10, N_FRAMES):
        trk = _tracker(seq)
        vol = _volume(trk, p)
        trk.attach_volume(vol)
        dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"][:n], seq["depth"][:n])]
        got = _run(trk, dev, True)
        assert all(g["solve_status"] == 0 for g in got)
        err = translation_errors(got, seq["poses"][:n])
        print(f"{n} frames: translation error of the tracked poses mean {err.mean():.4f} max {err.max():.4f} m")
        pts = vol.extract(1 << 20)
        dist, dots, ln, zero = plane_errors(*pts, p["vs"])
        report(f"tracked poses, {n} frames", dist, dots, ln, zero)
        print(f"tracked poses, {n} frames: points with z in [0.4, 4), [4, 6), [6, 7), [7, 8.4): "
              f"{np.histogram(pts[0][:, 2], [0.4, 4.0, 6.0, 7.0, 8.4])[0].tolist()}")
        print(f"tracked poses, {n} frames: points beyond half a voxel {int((dist > 0.5).sum())}, normals with a dot product <= 0 "
              f"{int((dots[~zero] <= 0).sum())}")
        if n == N_FRAMES:
            true = _volume(trk, p)
            for k in range(n):
                true.integrate(dev[k][1], seq["poses"][k])
            pts = true.extract(1 << 20)
            dist, dots, ln, zero = plane_errors(*pts, p["vs"])
            report(f"true poses, {n} frames", dist, dots, ln, zero)
            print(f"true poses, {n} frames: points with z in [0.4, 4), [4, 6), [6, 7), [7, 8.4): "
                  f"{np.histogram(pts[0][:, 2], [0.4, 4.0, 6.0, 7.0, 8.4])[0].tolist()}")
            true.close()
        ref = _standalone(trk, p, dev, got)
        _volumes_equal(vol, ref, f"{n} frames")
        ref.close()
        vol.close()
        trk.close()


def test_failed_frames_and_the_integration_rule(seq):
    """A frame is integrated iff its Solve succeeded. A constant grey frame is tracked and the rule is checked against the status the
    tracker reports for it, whichever it is. On the MI355X that Solve SUCCEEDS (solve_status 0, a finite pose; only the frame's depth
    job fails, there being nothing to select), so a failed Solve is not reached deterministically this way: the not-integrated side
    of the rule is covered by the refusal of a non-finite pose — what a failed Solve returns — in
    test_non_finite_poses_and_bad_arguments_are_refused, through the same pose check the tracker applies. A frame whose depth JOB
    failed has a good pose and is integrated."""
    from odometry_amd import _lib as L
    p = params(seq)
    trk = _tracker(seq)
    vol = _volume(trk, p)
    trk.attach_volume(vol)
    g = [trk.upload_frame(x) for x in seq["gray"][:3]]
    d = [trk.upload_depth(x) for x in seq["depth"][:3]]
    sparse = np.zeros_like(seq["depth"][1])
    sparse[::40, ::40] = seq["depth"][1][::40, ::40]            # a few hundred readings: the depth job fails
    d_sparse = trk.upload_depth(sparse)
    flat = trk.upload_frame(np.full((480, 640), 128.0, np.float32))
    trk.init(g[0], d[0])
    T = np.zeros(16, np.float32)
    A = np.full(16, np.nan, np.float32)
    fp = C.POINTER(C.c_float)
    rc = trk.lib.odo_tracker_track_rgbd(trk.h, g[1], d_sparse, T.ctypes.data_as(fp), A.ctypes.data_as(fp), None, None, None)
    assert rc == -1 and "depth failed" in L.last_error() and np.isfinite(A).all()
    assert vol.stats()["frames"] == 2
    ref = _volume(trk, p)
    ref.integrate(d[0], np.eye(4))
    ref.integrate(d_sparse, A.reshape(4, 4).T)
    _volumes_equal(vol, ref, "after a failed depth job")
    # a fresh sequence, then a frame without any texture
    trk.init(g[0], d[0])
    assert vol.stats()["frames"] == 3                            # re-init integrates its frame 0 again: the volume is the caller's to clear
    ss = C.c_int(-7)
    A[:] = 0.0
    rc = trk.lib.odo_tracker_track_rgbd(trk.h, flat, d[1], T.ctypes.data_as(fp), A.ctypes.data_as(fp), None, None, C.byref(ss))
    print("constant grey frame: return", rc, "solve_status", ss.value, "abs_pose finite", bool(np.isfinite(A).all()))
    assert rc == -1 and ss.value != -7       # (nothing to select on a frame without gradients: its depth job fails as well)
    if ss.value != 0:
        assert not np.isfinite(A).all()
        assert vol.stats()["frames"] == 3                        # not integrated
    else:
        assert np.isfinite(A).all() and vol.stats()["frames"] == 4
    ref.close()
    vol.close()
    trk.close()


def test_attach_detach_and_lifecycle(seq):
    from odometry_amd import _lib as L, api
    p = params(seq)
    trk = _tracker(seq)
    vol = _volume(trk, p)
    # a stereo tracker is refused, nothing enqueued
    stereo = api.Tracker(0)
    assert stereo.lib.odo_tracker_attach_volume(stereo.h, vol.h) == -1 and "RGB-D" in L.last_error()
    stereo.close()
    # another frame size is refused
    small = _volume(trk, params(seq, size=(240, 320)))
    assert trk.lib.odo_tracker_attach_volume(trk.h, small.h) == -1 and "does not match" in L.last_error()
    small.close()
    trk.attach_volume(vol)
    other = _tracker(seq)
    assert other.lib.odo_tracker_attach_volume(other.h, vol.h) == -1 and "another tracker" in L.last_error()
    other.close()
    assert vol.lib.odo_volume_destroy(vol.h) == -1 and "attached" in L.last_error()   # destroy while attached
    g = [trk.upload_frame(x) for x in seq["gray"][:4]]
    d = [trk.upload_depth(x) for x in seq["depth"][:4]]
    trk.init(g[0], d[0])
    r1 = trk.track(g[1], d[1])
    assert vol.stats()["frames"] == 2
    trk.attach_volume(None)                                      # detach: pending integrations complete, later frames stay out
    r2 = trk.track(g[2], d[2])
    assert vol.stats()["frames"] == 2
    trk.attach_volume(vol)
    r3 = trk.track(g[3], d[3])
    assert vol.stats()["frames"] == 3
    ref = _volume(trk, p)
    for k, A in ((0, np.eye(4)), (1, r1["abs_pose"]), (3, r3["abs_pose"])):
        ref.integrate(d[k], A)
    _volumes_equal(vol, ref, "attach / detach / attach")
    assert r2["solve_status"] == 0
    ref.close()
    # the tracker goes first: the volume is detached by it and lives on
    trk.close()
    assert vol.stats()["frames"] == 3
    assert len(vol.extract(1 << 20)[0]) > 1000
    vol.close()


def test_fed_from_the_front_ends_ring_the_result_is_the_same(seq):
    """The front end's ring with four slots used two frames ahead keeps every depth frame unchanged for as
    long as an attached volume needs it."""
    from odometry_amd import api
    from test_rgbd_frontend_cpu import RIGS, raw_sequence
    r = RIGS()["identity"]
    raw = raw_sequence(r, N_FRAMES)
    p = params(seq)
    a = _tracker(seq)
    va = _volume(a, p)
    a.attach_volume(va)
    want = _run(a, [(a.upload_frame(g), a.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])], True)
    b = _tracker(seq)
    vb = _volume(b, p)
    b.attach_volume(vb)
    fe = api.RgbdFrontend(b, r["depth_size"], r["depth_K"], 1000.0, r["size"], r["K"], 1000.0, r["E"], 3, False, 4)
    frames = [(fe.upload(c), fe.upload(d)) for c, d in zip(raw["colour"], raw["raw_depth"])]
    n = len(frames)
    slot = [fe.submit(*frames[k]) for k in range(3)]
    fe.wait(slot[0][0])
    b.init(*slot[0])
    got = [_row(b, dict(abs_pose=np.eye(4, dtype=np.float32), solve_status=0))]
    for k in range(1, n):
        if k + 2 < n:
            slot.append(fe.submit(*frames[k + 2]))
        fe.wait(slot[k][0])
        if k + 1 < n:
            fe.wait(slot[k + 1][0])
            b.hint_next(*slot[k + 1])
        got.append(_row(b, b.track(*slot[k])))
    _rows_equal(got, want, "front end")
    _volumes_equal(va, vb, "front end")
    fe.close()
    vb.close()
    b.close()
    va.close()
    a.close()
