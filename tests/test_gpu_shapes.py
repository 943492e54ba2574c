"""The whole trackers at the frame sizes and pyramid depths of tests/shape_cases.py (api.Tracker, api.TrackerBatch, api.RgbdTracker,
and the RGB-D front end, map and volume attached together): every row of the table against its CPU runner frame by frame with the
assertions and numbers the pinned shapes get (tests/test_gpu_sequence200.py, tests/test_gpu_rgbd.py), the trackers' own invariants
bit for bit at unpinned shapes, the bounds of the supported sizes, and one unpinned RGB-D shape end to end. Every expected value comes
from oracle/ and the numpy models, computed at test time; tests/test_shapes_cpu.py shows with those alone that each row is a valid
input."""
import numpy as np
import pytest

import shape_cases as S
from conftest import se3_log_norm

pytestmark = pytest.mark.gpu
TOL = 1e-5   # SE(3) log-map norm, BASELINE.json north_star: the pose parity tolerance of every tracker test


@pytest.fixture(scope="module")
def runs():
    return S.prepare(S.TABLE)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- driving a tracker ------------------------------------------------------------------------------------------------------------
def _make(c, **kw):
    from odometry_amd import api
    args = S.tracker_args(c, **kw)
    return api.Tracker(0, **args) if c["kind"] == "stereo" else api.RgbdTracker(0, **args)


def _upload(trk, c, seq):
    if c["kind"] == "stereo":
        return [(trk.upload_frame(l), trk.upload_frame(r)) for l, r in zip(seq["left"], seq["right"])]
    return [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])]


def _drive(c, seq, hints, overlap=2, keep=lambda k, g: True):
    """The tracker over the case's drive. Returns (rows, info): rows[0] = init, rows[k] = track's result of frame k with
    n_valid and — where keep(k, result) — the depth outputs; info = the statistics the tests print and assert on."""
    trk = _make(c, overlap_depth=overlap)
    dev = _upload(trk, c, seq)
    n = c["frames"]

    def row(k, g):
        g = dict(g, n_valid=trk.stats()["n_valid_depth"])
        if keep(k, g):
            g["val"], g["disp"], g["dep"] = trk.outputs(c["rows"], c["cols"])
        return g

    trk.init(*dev[0])
    rows = [row(0, {})]
    points, switched = {}, False
    for k in range(1, n):
        if hints and k + 1 < n:
            trk.hint_next(*dev[k + 1])   # the pair / grey and depth: pyramid prefetch, the depth stream a frame ahead, early and armed Solves
        g = trk.track(*dev[k])
        rows.append(row(k, g))
        if k == 1:
            points["first Solve"] = trk.lm_points()
        if switched and "after the first switch" not in points:
            points["after the first switch"] = trk.lm_points()
        switched = switched or g["new_keyframe"]
    info = dict(points=points, persistent=trk.persistent_stats(), arm=trk.arm_stats(), depth_persistent=trk.depth_persistent_stats(),
                n_keyframes=trk.stats()["n_keyframes"])
    trk.close()
    return rows, info


def _describe(tag, info, worst):
    pts = "; ".join(f"{k}: points per level {v[0]}, launches {v[1]}" for k, v in info["points"].items())
    print(f"{tag}: {pts}; persistent workgroups {info['persistent'][0]}, Solves redone {info['persistent'][1]}, armed / told to return "
          f"{info['arm']}, keyframes {info['n_keyframes']}, worst log-norm {worst:.3g}")


# ---- 2a: every row against its CPU runner -----------------------------------------------------------------------------------------
def _check_pose_row(k, g, c):
    assert g["solve_status"] == c["solve_status"] == 0, f"frame {k}: Solve status {g['solve_status']} vs {c['solve_status']}"
    assert g["new_keyframe"] == c["new_keyframe"], f"frame {k}: keyframe decision differs"
    d_kf = se3_log_norm(c["pose_to_keyframe"], g["pose_to_keyframe"])
    d_abs = se3_log_norm(c["abs_pose"], g["abs_pose"])
    assert d_kf < TOL, f"frame {k}: pose_to_keyframe log-norm {d_kf}"
    assert d_abs < TOL, f"frame {k}: abs_pose log-norm {d_abs}"
    assert abs(g["motion"] - c["motion"]) < 1e-5, f"frame {k}: motion score {g['motion']} vs {c['motion']}"
    assert g["n_valid"] == c["n_valid"], f"frame {k}: valid-depth count {g['n_valid']} vs {c['n_valid']}"
    return max(d_kf, d_abs)


def _check_stereo_outputs(k, g, c):
    assert np.array_equal(g["val"], c["val"]), f"frame {k}: mask differs at {int((g['val'] != c['val']).sum())} pixels"
    assert np.array_equal(g["disp"], c["disp"]), f"frame {k}: disparity"
    np.testing.assert_allclose(g["dep"], c["dep"], rtol=0, atol=1e-7, err_msg=f"frame {k}: inverse depth")


def _check_rgbd_outputs(k, g, c):
    assert np.array_equal(g["val"], c["val"]), f"frame {k}: mask differs at {int((g['val'] != c['val']).sum())} pixels"
    assert np.array_equal(_bits(g["dep"]), _bits(c["dep"])), f"frame {k}: inverse depth differs"
    assert not g["disp"].any(), f"frame {k}: disparity is not zero"


@pytest.mark.parametrize("hints", [True, False])
@pytest.mark.parametrize("cid", [S.case_id(c) for c in S.STEREO])
def test_stereo_row_matches_the_oracle_runner(runs, cid, hints):
    r = runs[cid]
    c, ref = r["case"], r["rows"]
    rows, info = _drive(c, r["seq"], hints, keep=lambda k, g: ref[k]["val"] is not None)
    assert rows[0]["n_valid"] == ref[0]["n_valid"], f"frame 0: valid-depth count {rows[0]['n_valid']} vs {ref[0]['n_valid']}"
    _check_stereo_outputs(0, rows[0], ref[0])
    worst = 0.0
    for k in range(1, c["frames"]):
        worst = max(worst, _check_pose_row(k, rows[k], ref[k]))
        if ref[k]["val"] is not None:   # on a stride of frames and at every switch
            _check_stereo_outputs(k, rows[k], ref[k])
    _describe(f"{cid} hints={hints}", info, worst)
    assert info["n_keyframes"] == r["n_keyframes"] >= 2
    assert info["persistent"][1] == 0, "a pose Solve was redone on the step launches"


@pytest.mark.parametrize("hints", [True, False])
@pytest.mark.parametrize("cid", [S.case_id(c) for c in S.RGBD_ROWS])
def test_rgbd_row_matches_the_model_runner(runs, cid, hints):
    r = runs[cid]
    c, ref = r["case"], r["rows"]
    rows, info = _drive(c, r["seq"], hints)
    assert rows[0]["n_valid"] == ref[0]["n_valid"]
    _check_rgbd_outputs(0, rows[0], ref[0])
    worst = 0.0
    for k in range(1, c["frames"]):
        worst = max(worst, _check_pose_row(k, rows[k], ref[k]))
        _check_rgbd_outputs(k, rows[k], ref[k])   # every frame, bit for bit
    _describe(f"{cid} hints={hints}", info, worst)
    assert info["n_keyframes"] == r["n_keyframes"] >= 2
    assert info["persistent"][1] == 0, "a pose Solve was redone on the step launches"
    assert info["depth_persistent"] == (0, 0)   # the stereo depth LM's persistent launch is never issued


@pytest.mark.parametrize("key,boundary", [((363, 643, 4), 4), ((120, 160, 3), 2), ((720, 1280, 4), 1)])
def test_conversion_with_holes_and_steps_at_the_guards_bound_matches_the_model(runs, key, boundary):
    """The drives' own depth frames have next to no depth steps at selected pixels (a guard that never fires changes four pixels of
    frame 0 at 120 x 160 and none at 240 x 424 or 363 x 643): here holes, saturated and too-near readings, and steps exactly at the
    edge guard's bound and one unit past it are written beside selected pixels, to the right and below, last column and row included."""
    from test_rgbd_cpu import rgbd_depth_model, select_model
    r = runs[S.case_id(S.find("rgbd", *key))]
    c = r["case"]
    gray = r["seq"]["gray"][0]
    raw = r["seq"]["depth"][0].astype(np.int64)
    step = np.float32(S.RGBD["max_depth_step"])
    sel = np.argwhere(select_model(gray, boundary) != 0)
    pick = sel[np.random.default_rng(5).permutation(len(sel))][:min(3000, len(sel) // 2)]
    for n, (y, x) in enumerate(pick):
        kind = n % 8
        if kind == 0:
            raw[y, x] = 0
        elif kind == 1:
            raw[y, x] = 65535
        elif kind == 2:
            raw[y, x] = 50                              # 5 cm at 1000 units per metre: nearer than min_depth
        elif kind >= 4 and raw[y, x] > 100:
            dy, dx = ((0, 1), (0, -1), (1, 0), (-1, 0))[kind - 4]
            if 0 <= y + dy < c["rows"] and 0 <= x + dx < c["cols"]:
                lim = step * np.float32(raw[y, x])
                past = (n // 8) % 2                     # exactly at the bound (kept) / one unit past it (dropped)
                raw[y + dy, x + dx] = min(65535, int(raw[y, x]) + int(np.floor(lim)) + past)
    raw = np.clip(raw, 0, 65535).astype(np.uint16)
    val, dep, st = rgbd_depth_model(gray, raw, S.RGBD["depth_scale"], S.RGBD["max_depth_step"], boundary)
    plain = rgbd_depth_model(gray, raw, S.RGBD["depth_scale"], np.inf, boundary)[2]
    assert st["status"] == 0 and plain["n_valid"] - st["n_valid"] > 100   # the guard drops points here
    trk = _make(c, boundary=boundary)
    trk.init(trk.upload_frame(gray), trk.upload_depth(raw))
    g = dict(zip(("val", "disp", "dep"), trk.outputs(c["rows"], c["cols"])))
    _check_rgbd_outputs(0, g, dict(val=val, dep=dep))
    rep = trk.depth_report()
    assert (rep["n_selected"], rep["n_matched"], rep["n_valid"]) == (st["n_selected"], st["n_matched"], st["n_valid"]), (rep, st)
    trk.close()


# ---- 2b: the schedule must not matter, at unpinned shapes ---------------------------------------------------------------------------
def _rows_identical(a, b, tag):
    assert len(a) == len(b)
    for k, (g, c) in enumerate(zip(a, b)):
        assert g["n_valid"] == c["n_valid"], f"{tag} frame {k}: valid-depth count"
        assert np.array_equal(g["val"], c["val"]), f"{tag} frame {k}: mask differs"
        assert np.array_equal(_bits(g["dep"]), _bits(c["dep"])), f"{tag} frame {k}: inverse depth differs"
        assert np.array_equal(_bits(g["disp"]), _bits(c["disp"])), f"{tag} frame {k}: disparity differs"
        if k == 0:
            continue
        assert g["new_keyframe"] == c["new_keyframe"] and g["solve_status"] == c["solve_status"], f"{tag} frame {k}: decisions differ"
        for key in ("pose_to_keyframe", "abs_pose"):
            assert np.array_equal(_bits(g[key]), _bits(c[key])), f"{tag} frame {k}: {key} differs"
        assert g["motion"] == c["motion"], f"{tag} frame {k}: motion score differs"


@pytest.mark.parametrize("key", [("stereo", 120, 160, 3), ("stereo", 361, 1243, 4), ("rgbd", 240, 424, 4), ("rgbd", 720, 1280, 4)],
                         ids=lambda k: f"{k[0]}-{k[1]}x{k[2]}-L{k[3]}")
def test_results_do_not_depend_on_the_schedule(runs, key):
    """overlap_depth 0 (serial) / 1 (two streams, one host thread) / 2 (helper thread) x next frame announced or not: the same bits."""
    r = runs[S.case_id(S.find(*key))]
    c = r["case"]
    want, _ = _drive(c, r["seq"], False, overlap=0)
    assert all(g["solve_status"] == 0 for g in want[1:])
    for overlap in (0, 1, 2):
        for hints in (False, True):
            if (overlap, hints) != (0, False):
                got, _ = _drive(c, r["seq"], hints, overlap=overlap)
                _rows_identical(got, want, f"overlap {overlap} hints {hints}")


def _track_single(c, seq):
    from odometry_amd import api
    trk = api.Tracker(0, **S.tracker_args(c))
    dev = _upload(trk, c, seq)
    trk.init(*dev[0])
    out = []
    for k in range(1, c["frames"]):
        g = trk.track(*dev[k])
        g["stats"] = trk.stats()
        out.append(g)
    maps = trk.outputs(c["rows"], c["cols"])
    trk.close()
    return out, maps


@pytest.mark.parametrize("shape,n_seq,pairs", [((480, 640), 3, True), ((480, 640), 3, False), ((370, 1226), 2, True), ((370, 1226), 2, False)])
def test_batched_tracker_is_bit_identical_to_separate_trackers(runs, shape, n_seq, pairs):
    from odometry_amd import api
    cases = [S.find("stereo", shape[0], shape[1], 4, seed=s) for s in range(n_seq)]
    assert runs[S.case_id(cases[0])]["n_keyframes"] >= 2          # the comparison covers a keyframe switch (the oracle's count)
    drives = S.prepare(cases, with_ref=False)
    seqs = [drives[S.case_id(c)]["seq"] for c in cases]
    n_frames = cases[0]["frames"]
    singles = [_track_single(c, s) for c, s in zip(cases, seqs)]
    tb = api.TrackerBatch(n_seq, 0, **S.tracker_args(cases[0]))
    L = [[tb.upload_frame(f) for f in s["left"]] for s in seqs]
    R = [[tb.upload_frame(f) for f in s["right"]] for s in seqs]
    tb.init([L[i][0] for i in range(n_seq)], [R[i][0] for i in range(n_seq)])
    for k in range(1, n_frames):
        if pairs and k + 1 < n_frames:
            tb.hint_next([L[i][k + 1] for i in range(n_seq)], [R[i][k + 1] for i in range(n_seq)])
        res = tb.track([L[i][k] for i in range(n_seq)], [R[i][k] for i in range(n_seq)])
        st = tb.stats()
        for i in range(n_seq):
            ref = singles[i][0][k - 1]
            assert res[i]["status"] == ref["solve_status"] == 0
            assert np.array_equal(res[i]["pose_to_keyframe"], ref["pose_to_keyframe"]), f"sequence {i} frame {k}"
            assert np.array_equal(res[i]["abs_pose"], ref["abs_pose"]), f"sequence {i} frame {k}"
            assert res[i]["new_keyframe"] == ref["new_keyframe"], f"sequence {i} frame {k}"
            assert res[i]["motion"] == ref["motion"]
            assert st[i] == ref["stats"], f"sequence {i} frame {k}"
    for i in range(n_seq):
        for a, b in zip(tb.outputs(i, *shape), singles[i][1]):
            assert np.array_equal(a, b)
    tb.close()


def test_batched_tracker_refuses_five_levels_at_create():
    from odometry_amd import _lib as L
    from odometry_amd import api
    with pytest.raises(L.OdoError, match="at most 4 pyramid levels"):
        api.TrackerBatch(2, 0, **S.tracker_args(S.find("stereo", 376, 1241, 5)))


# ---- 2c: the bounds -----------------------------------------------------------------------------------------------------------------
def test_one_step_past_the_selection_bound_is_refused_at_init_and_the_device_stays_usable(runs):
    """1048 x 2056 with boundary 4: tiles of 64 x 65 = 4 160 pixels, past the selection kernel's 4 096. depth_check_size is the first
    statement of tracker_job_begin, the one place a tracker's depth launches start from (init, track at every overlap_depth, the helper
    thread's job posted ahead); the batched tracker asks at create."""
    from odometry_amd import _lib as L
    from odometry_amd import api
    big = dict(rows=1048, cols=2056, levels=4, frames=1)
    img = np.zeros((1048, 2056), np.float32)
    for kind in ("stereo", "rgbd"):
        c = dict(big, kind=kind)
        trk = _make(c)
        a = trk.upload_frame(img)
        b = trk.upload_frame(img) if kind == "stereo" else trk.upload_depth(np.zeros((1048, 2056), np.uint16))
        with pytest.raises(L.OdoError, match="selection block 64x65 exceeds 4096"):
            trk.init(a, b)
        assert trk.stats()["n_keyframes"] == 0 and trk.stats()["n_valid_depth"] == 0
        trk.close()
    with pytest.raises(L.OdoError, match="selection block 64x65 exceeds 4096"):
        api.TrackerBatch(2, 0, **S.tracker_args(dict(big, kind="stereo")))
    # a tracker created afterwards tracks normally
    r = runs[S.case_id(S.find("stereo", 480, 640, 4))]
    c = dict(r["case"], frames=6)
    rows, _ = _drive(c, r["seq"], True, keep=lambda k, g: False)
    for k in range(1, 6):
        _check_pose_row(k, rows[k], r["rows"][k])


@pytest.mark.parametrize("kind", ["stereo", "rgbd"])
def test_one_pixel_per_tile_fails_its_depth_like_the_model(kind):
    """24 x 40 with boundary 4: the selection grid's tiles are one pixel, at most 512 pixels can be selected and fewer than 500 depths
    are valid: init refuses with the runner's message, the counts are the oracle's / the model's."""
    from odometry_amd import _lib as L
    from odometry_amd import api
    c = dict(kind=kind, rows=24, cols=40, levels=3, frames=1, seed=0)
    seq = S.render(c)
    if kind == "stereo":
        from oracle import oracle as O
        want = O.compute_depth(seq["left"][0], seq["right"][0], S.stereo_params(c)[1])
    else:
        from test_rgbd_cpu import rgbd_depth_model
        want = rgbd_depth_model(seq["gray"][0], seq["depth"][0], S.RGBD["depth_scale"], S.RGBD["max_depth_step"], 4)[2]
    assert want["status"] != 0 and want["n_valid"] < 500 and want["n_selected"] <= 512
    trk = _make(c)
    dev = _upload(trk, c, seq)
    with pytest.raises(L.OdoError, match="Init 0-th frame failed!"):
        trk.init(*dev[0])
    rep = api.RgbdTracker.depth_report(trk)
    print(f"24x40 {kind}: selected / matched / valid {rep['n_selected']} / {rep['n_matched']} / {rep['n_valid']}")
    assert (rep["n_selected"], rep["n_matched"], rep["n_valid"]) == (want["n_selected"], want["n_matched"], want["n_valid"])
    trk.close()


@pytest.mark.parametrize("hints", [True, False])
def test_stereo_120x160_with_four_levels_reports_the_oracles_solve_status(hints):
    """Level 3 is 15 x 20 with a 7 x 12 interior: Solves of this drive fail in the oracle. The tracker reports the oracle's status
    frame by frame and stays usable (no exception, every good frame a finite pose)."""
    c = dict(S.find("stereo", 120, 160, 3), levels=4)
    seq = S.render(c)
    ref, _ = S.run_stereo(c, seq, S.tolerant_runner())
    want = [r["solve_status"] for r in ref[1:]]
    assert any(s != 0 for s in want)
    rows, info = _drive(c, seq, hints, keep=lambda k, g: False)
    got = [g["solve_status"] for g in rows[1:]]
    worst = max([se3_log_norm(r["pose_to_keyframe"], g["pose_to_keyframe"]) for r, g in zip(ref[1:], rows[1:])
                 if r["solve_status"] == 0 and g["solve_status"] == 0] or [0.0])
    print(f"120x160, 4 levels, hints={hints}: solve_status {got}, the oracle's {want}; worst pose_to_keyframe log-norm on good frames {worst:.3g}")
    assert got == want
    assert all(np.isfinite(g["abs_pose"]).all() for g in rows[1:] if g["solve_status"] == 0)
    assert all(g["n_valid"] == r["n_valid"] for g, r in zip(rows, ref))


def test_any_size_0_refuses_another_size_with_the_references_message(runs):
    from odometry_amd import _lib as L
    r = runs[S.case_id(S.find("stereo", 480, 640, 4))]
    trk = _make(r["case"], any_size=0)
    a, b = trk.upload_frame(r["seq"]["left"][0]), trk.upload_frame(r["seq"]["right"][0])
    with pytest.raises(L.OdoError, match="rows != 480 or cols != 640."):   # ref: src/depth_estimate.cpp:46-49
        trk.init(a, b)
    trk.close()


# ---- 2d: one unpinned RGB-D shape with everything attached --------------------------------------------------------------------------
def test_frontend_tracker_map_and_volume_together_at_240x424():
    """Colour 240 x 424, the depth imager 240 x 320 with its own focal length and a small extrinsic: RgbdFrontend (ring of 4, two frames
    ahead) -> RgbdTracker with a PointMap and a TsdfVolume attached together. The front end against frontend_model, the tracker against
    the same tracker fed the model's frames (and the model runner on them), the map against RefMap fed the keyframes, the volume against
    integrate_model / extract_model fed the returned poses."""
    from odometry_amd import api
    from oracle import oracle as O
    from test_gpu_map import RefMap, assert_same
    from test_rgbd_frontend_cpu import STAT_KEYS, frontend_model, raw_sequence, rig
    from test_volume_cpu import bits, empty_grid, extract_model, integrate_model, params
    c = S.find("rgbd", 240, 424, 4)
    n = c["frames"]
    K = S.intrinsics(c)
    r = rig((240, 320), 250.0, (240, 424), K[0], (15.0, 0.5, -0.3), (2.0, -3.0, 1.0))
    assert r["K"] == K
    raw = raw_sequence(r, n, tint_seed=5)
    model = [frontend_model(col, d, r, 1000.0, 1000.0) for col, d in zip(raw["colour"], raw["raw_depth"])]
    mseq = dict(gray=[m[0] for m in model], depth=[m[1] for m in model], K=dict(f0=K[0], cx0=K[1], cy0=K[2]), depth_scale=1000.0)
    ref_rows, ref_kf = S.run_rgbd(c, mseq)
    assert ref_kf >= 2 and all(row["solve_status"] == 0 for row in ref_rows[1:]) and all(row["n_valid"] >= 500 for row in ref_rows)
    want, _ = _drive(c, mseq, True)                                     # the same tracker fed the model's frames
    # a grid round the corridor's first eight metres; dimensions that are no multiples of 64 or 4
    p = params(K, 1000.0, size=(240, 424), dims=(121, 67, 99), vs=0.08, origin=(-4.8, -3.3, 0.4), mu=0.24, max_depth=8.0, max_weight=65535)
    trk = _make(c)
    fe = api.RgbdFrontend(trk, r["depth_size"], r["depth_K"], 1000.0, r["size"], r["K"], 1000.0, r["E"], 3, False, 4)
    pm = api.PointMap(trk, 240, 424, 2_000_000, 0.05)
    vol = api.TsdfVolume(trk, p["dims"], p["vs"], p["origin"], p["mu"], p["max_depth"], p["max_weight"], p["size"], p["K"], p["depth_scale"])
    trk.attach_map(pm)
    trk.attach_volume(vol)
    frames = [(fe.upload(col), fe.upload(d)) for col, d in zip(raw["colour"], raw["raw_depth"])]

    def row(k, g, slot):
        gray, dep = fe.download(*slot)
        st = fe.stats(slot[0])
        assert np.array_equal(_bits(gray), _bits(model[k][0])), f"frame {k}: the front end's grey differs"
        assert np.array_equal(dep, model[k][1]), f"frame {k}: the front end's registered depth differs"
        assert {key: st[key] for key in STAT_KEYS} == model[k][2], f"frame {k}: {st}"
        g = dict(g, n_valid=trk.stats()["n_valid_depth"])
        g["val"], g["disp"], g["dep"] = trk.outputs(240, 424)
        return g

    slot = [fe.submit(*frames[k]) for k in range(3)]
    fe.wait(slot[0][0])
    trk.init(*slot[0])
    got = [row(0, {}, slot[0])]
    for k in range(1, n):
        if k + 2 < n:
            slot.append(fe.submit(*frames[k + 2]))
        fe.wait(slot[k][0])
        if k + 1 < n:
            fe.wait(slot[k + 1][0])
            trk.hint_next(*slot[k + 1])
        got.append(row(k, trk.track(*slot[k]), slot[k]))
    # the tracker
    _rows_identical(got, want, "front end + map + volume against the plain tracker")
    worst = 0.0
    _check_rgbd_outputs(0, got[0], ref_rows[0])
    for k in range(1, n):
        worst = max(worst, _check_pose_row(k, got[k], ref_rows[k]))
        _check_rgbd_outputs(k, got[k], ref_rows[k])
    assert trk.stats()["n_keyframes"] == ref_kf
    # the map
    trk.attach_map(None)
    ref_map = RefMap(2_000_000, 0.05, cols=424, k=K)
    poses = [np.eye(4, dtype=np.float32)] + [g["abs_pose"] for g in got[1:]]
    for k in range(n):
        if k == 0 or got[k]["new_keyframe"]:
            ref_map.insert(got[k]["val"], got[k]["dep"], O.image_pyramid(model[k][0], 4, True)[0], poses[k])
    assert ref_map.st["insertions"] == ref_kf and ref_map.st["size"] > 5_000
    assert_same(pm, ref_map)
    # the volume
    trk.attach_volume(None)
    q, w = empty_grid(p)
    total = 0
    for k in range(n):
        q, w, upd, band = integrate_model(q, w, model[k][1], poses[k], p)
        total += upd
    st = vol.stats()
    assert st == dict(frames=n, updated=upd, in_band=band, cumulative=total), (st, upd, band, total)
    gq, gw = vol.grid()
    assert np.array_equal(gw, w), f"weights differ at {int((gw != w).sum())} voxels"
    assert np.array_equal(gq, q), f"distances differ at {int((gq != q).sum())} voxels"
    pts = extract_model(q, w, p)
    got_pts = vol.extract(len(pts[0]) + 1000, with_dropped=True)
    assert got_pts[0].shape == pts[0].shape and len(pts[0]) > 1000 and got_pts[2] == 0
    assert np.array_equal(bits(got_pts[0]), bits(pts[0])) and np.array_equal(bits(got_pts[1]), bits(pts[1]))
    print(f"240x424 end to end: {n} frames, {ref_kf} keyframes, map {ref_map.st['size']} points, volume {total} updates, "
          f"{len(pts[0])} surface points, worst log-norm {worst:.3g}")
    vol.close()
    pm.close()
    fe.close()
    trk.close()
