"""The RGB-D front end on the GPU (odo_rgbd_frontend_*, api.RgbdFrontend) against the numpy model of tests/test_rgbd_frontend_cpu.py:
grey and registered depth bit for bit with their statistics on three sensor rigs and the corner cases, both submit paths, order
independence, the ring's contract, and an RgbdTracker fed from the front end against the same tracker fed pre-made buffers."""
import numpy as np
import pytest

from test_rgbd_cpu import MAX_DEPTH_STEP, N_FRAMES, translation_errors
from test_rgbd_frontend_cpu import DRIVE, RIGS, STAT_KEYS, frontend_model, raw_sequence, rig

pytestmark = pytest.mark.gpu


def _frontend(ctx, r, scale_in=1000.0, scale_out=1000.0, channels=3, bgr=False, slots=3):
    from odometry_amd import api
    return api.RgbdFrontend(ctx, r["depth_size"], r["depth_K"], scale_in, r["size"], r["K"], scale_out, r["E"], channels, bgr, slots)


def _pitched(a, pad):
    """The same array inside a wider allocation: rows `pad` elements longer than the frame's."""
    wide = np.zeros((a.shape[0], a.shape[1] + pad) + a.shape[2:], a.dtype)
    wide[:, :a.shape[1]] = a
    view = wide[:, :a.shape[1]]
    assert view.strides[0] > a.strides[0]
    return view


def _check(fe, slot, want, tag):
    gray, dep = fe.download(*slot)
    st = fe.stats(slot[0])
    wg, wd, ws = want
    assert np.array_equal(gray.view(np.uint32), wg.view(np.uint32)), f"{tag}: grey differs at {int((gray != wg).sum())} pixels"
    assert np.array_equal(dep, wd), f"{tag}: registered depth differs at {int((dep != wd).sum())} pixels"
    assert {k: st[k] for k in STAT_KEYS} == ws, f"{tag}: {st} != {ws}"
    return gray, dep


def _both_paths(r, colour, raw, scale_in=1000.0, scale_out=1000.0, channels=3, bgr=False):
    """One frame through the device path and through the host path (pitched rows): both equal to the model."""
    from odometry_amd import api
    want = frontend_model(colour, raw, r, scale_in, scale_out, bgr)
    ctx = api.Context(0)
    fe = _frontend(ctx, r, scale_in, scale_out, channels, bgr)
    try:
        s0 = fe.submit(fe.upload(colour), fe.upload(raw))
        s1 = fe.submit(_pitched(colour, 5), _pitched(raw, 3))
        assert s0[0].value != s1[0].value and s0[1].value != s1[1].value
        _check(fe, s0, want, "device path")
        _check(fe, s1, want, "host path")
        assert fe.stats(s0[0])["frame"] == 0 and fe.stats(s1[0])["frame"] == 1
    finally:
        fe.close()
        ctx.close()
    return want


# ---- against the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "identity"])
def test_rigs_match_the_model_bit_for_bit(name):
    r = RIGS()[name]
    seq = raw_sequence(r, 6, frames=[0, 5], tint_seed=None if name == "identity" else 3)
    for colour, raw in zip(seq["colour"], seq["raw_depth"]):
        gray, dep, st = _both_paths(r, colour, raw)
        assert st["n_filled"] > 200000 and st["dropped_splat"] == 0
        if name == "identity":
            assert np.array_equal(dep, raw)


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("bgr", [False, True])
def test_colour_layouts_match_the_model(channels, bgr):
    r = RIGS()["A"]
    seq = raw_sequence(r, 6, frames=[5], channels=channels, bgr=bgr, tint_seed=7)
    colour = seq["colour"][0]
    assert not np.array_equal(colour[..., 0], colour[..., 2])
    gray, _, _ = _both_paths(r, colour, seq["raw_depth"][0], channels=channels, bgr=bgr)
    rgb = raw_sequence(r, 6, frames=[5], channels=3, bgr=False, tint_seed=7)["colour"][0]
    from test_rgbd_frontend_cpu import grey_model
    assert np.array_equal(gray, grey_model(rgb))            # the layout does not change the grey image


@pytest.mark.parametrize("size", [(479, 641), (480, 641), (3, 5)])
@pytest.mark.parametrize("channels", [3, 4])
def test_frames_that_are_not_a_multiple_of_four_wide(size, channels):
    """The four-pixel groups run over the flat frame: its last one to three pixels take the tail path (479 x 641 and 3 x 5 leave
    three), and a 641-wide frame whose size is a multiple of four has none."""
    rows, cols = size
    r = rig((480, 640), 385.0, size, 525.0 * cols / 640.0, (15.0, 0.5, -0.3), (2.0, -3.0, 1.0))
    rng = np.random.default_rng(rows * cols + channels)
    colour = rng.integers(0, 256, (rows, cols, channels)).astype(np.uint8)
    raw = raw_sequence(RIGS()["A"], 6, frames=[5])["raw_depth"][0]
    _, dep, st = _both_paths(r, colour, raw, channels=channels)
    assert st["n_filled"] > rows * cols // 2


def test_corner_cases_match_the_model():
    from odometry_amd import synth
    R = RIGS()
    a = R["A"]
    seq = raw_sequence(a, 6, frames=[5])
    colour, raw = seq["colour"][0], seq["raw_depth"][0]
    n = int((raw != 0).sum())
    # no readings at all / every reading saturated
    _, dep, st = _both_paths(a, colour, np.zeros_like(raw))
    assert not dep.any() and st == dict(n_depth=0, n_filled=0, dropped_behind=0, dropped_range=0, dropped_splat=0)
    _, dep, st = _both_paths(a, colour, np.full_like(raw, 65535))
    assert st["n_depth"] == raw.size and st["dropped_range"] > 0          # 65.5 m seen from 0.3 mm further back: q > 65535
    _, dep, st = _both_paths(R["identity"], colour, np.full_like(raw, 65535))
    assert np.all(dep == 65535) and st["n_filled"] == raw.size
    # the depth imager looking the other way: everything behind the colour camera
    flipped = dict(a, E=synth.rig_extrinsic((0.015, 0.0, 0.0), (0.0, np.pi, 0.0)))
    _, dep, st = _both_paths(flipped, colour, raw)
    assert not dep.any() and st["dropped_behind"] == n and st["n_filled"] == 0
    # an output scale that pushes q past 65535
    _, dep, st = _both_paths(a, colour, raw, scale_out=10000.0)
    assert 0 < st["dropped_range"] < n and st["n_filled"] > 0
    # a strongly magnifying rig: footprints wider than four pixels
    magnify = rig((480, 640), 120.0, (480, 640), 525.0, (15.0, 0.5, -0.3), (2.0, -3.0, 1.0))
    _, dep, st = _both_paths(magnify, colour, raw)
    assert st["dropped_splat"] > 0
    # in between: footprints on both sides of the bound
    edge = rig((480, 640), 131.0, (480, 640), 525.0, (15.0, 0.5, -0.3), (2.0, -3.0, 1.0))
    _, dep, st = _both_paths(edge, colour, raw)
    assert 0 < st["dropped_splat"] < n and st["n_filled"] > 0


def test_the_same_frame_twenty_times_round_the_ring_gives_identical_bytes():
    from odometry_amd import api
    r = RIGS()["C"]            # the rig with the most writes per target pixel
    seq = raw_sequence(r, 6, frames=[5], tint_seed=2)
    want = frontend_model(seq["colour"][0], seq["raw_depth"][0], r, 1000.0, 1000.0)
    ctx = api.Context(0)
    fe = _frontend(ctx, r, slots=3)
    c, d = fe.upload(seq["colour"][0]), fe.upload(seq["raw_depth"][0])
    slots = []
    for k in range(20):
        slots.append(fe.submit(c, d))
        if k >= 2:             # two frames in flight behind the one checked
            _check(fe, slots[k - 2], want, f"submit {k - 2}")
            assert fe.stats(slots[k - 2][0])["frame"] == k - 2
    _check(fe, slots[18], want, "submit 18")
    _check(fe, slots[19], want, "submit 19")
    assert len({s[0].value for s in slots}) == 3
    fe.close()
    ctx.close()


# ---- the ring --------------------------------------------------------------------------------------------------------------------
def test_ring_contract():
    from odometry_amd import _lib as L
    from odometry_amd import api
    r = RIGS()["A"]
    seq = raw_sequence(r, 6, frames=[0, 1, 2, 3, 4])
    want = [frontend_model(c, d, r, 1000.0, 1000.0) for c, d in zip(seq["colour"], seq["raw_depth"])]
    assert not np.array_equal(want[0][1], want[1][1])
    ctx = api.Context(0)
    fe = _frontend(ctx, r, slots=3)
    dev = [(ctx.upload(c), ctx.upload(d)) for c, d in zip(seq["colour"], seq["raw_depth"])]   # the context's: they outlive a front end
    with pytest.raises(L.OdoError):
        fe.wait(dev[0][0])                                  # not a slot
    s = [fe.submit(*dev[k]) for k in range(3)]              # `slots` submits without a wait
    with pytest.raises(L.OdoError, match="outstanding"):
        fe.submit(*dev[3])
    with pytest.raises(L.OdoError, match="outstanding"):
        fe.submit(seq["colour"][3], seq["raw_depth"][3])
    for k in range(3):                                      # the refused submits enqueued nothing
        _check(fe, s[k], want[k], f"frame {k}")
        assert fe.stats(s[k][0])["frame"] == k
    fe.close()
    fe = _frontend(ctx, r, slots=3)
    s = [fe.submit(*dev[k]) for k in range(3)]
    with pytest.raises(L.OdoError, match="outstanding"):
        fe.submit(*dev[3])
    fe.wait(s[0][0])                                        # frame 0 accounted for: its slot may come round
    s.append(fe.submit(*dev[3]))
    assert s[3][0].value == s[0][0].value and s[3][1].value == s[0][1].value
    with pytest.raises(L.OdoError, match="outstanding"):
        fe.submit(*dev[4])
    _check(fe, s[1], want[1], "frame 1 after its neighbour's slot was reused")
    _check(fe, s[2], want[2], "frame 2")
    _check(fe, s[3], want[3], "frame 3 in frame 0's slot")
    assert fe.stats(s[3][0])["frame"] == 3                  # the refused submits did not count
    s.append(fe.submit(seq["colour"][4], seq["raw_depth"][4]))
    assert s[4][0].value == s[1][0].value
    _check(fe, s[4], want[4], "frame 4, host path")
    _check(fe, s[2], want[2], "frame 2 again")
    # destroy with frames in flight drains them
    for k in range(3):
        fe.submit(*dev[k])
    fe.close()
    fe = _frontend(ctx, r, slots=2)
    _check(fe, fe.submit(*dev[1]), want[1], "a new front end after the drained one")
    fe.submit(seq["colour"][0], seq["raw_depth"][0])
    fe.close()
    for c, d in dev:
        ctx.free(c)
        ctx.free(d)
    ctx.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def _tracker(K, **kw):
    from odometry_amd import api
    return api.RgbdTracker(0, depth_scale=1000.0, max_depth_step=MAX_DEPTH_STEP, rows=480, cols=640, K=K, **kw)


def _row(trk, res):
    val, disp, dep = trk.outputs(480, 640)
    return dict(res, val=val, dep=dep, n_valid=trk.depth_report()["n_valid"])


def _run_premade(trk, dev, hints):
    """The tracker over pre-made device buffers [(grey, depth), ...]."""
    trk.init(*dev[0])
    rows = [_row(trk, {})]
    for k in range(1, len(dev)):
        if hints and k + 1 < len(dev):
            trk.hint_next(*dev[k + 1])
        rows.append(_row(trk, trk.track(*dev[k])))
    return rows


def _run_from_frontend(trk, fe, raw, hints):
    """The same loop with the front end working ahead of the tracker: submit k + 1, wait k, track k — with announcements one frame
    further ahead (submit k + 2, wait k + 1, announce k + 1, track k), since an announced frame must be complete."""
    n = len(raw)
    ahead = 2 if hints else 1
    slot = [fe.submit(*raw[k]) for k in range(min(ahead + 1, n))]
    fe.wait(slot[0][0])
    trk.init(*slot[0])
    rows = [_row(trk, {})]
    for k in range(1, n):
        if k + ahead < n:
            slot.append(fe.submit(*raw[k + ahead]))
        fe.wait(slot[k][0])
        if hints and k + 1 < n:
            fe.wait(slot[k + 1][0])
            trk.hint_next(*slot[k + 1])
        rows.append(_row(trk, trk.track(*slot[k])))
    return rows


def _rows_equal(a, b, tag):
    assert len(a) == len(b)
    for k, (g, c) in enumerate(zip(a, b)):
        assert np.array_equal(g["val"], c["val"]), f"{tag} frame {k}: mask differs"
        assert np.array_equal(g["dep"].view(np.uint32), c["dep"].view(np.uint32)), f"{tag} frame {k}: inverse depth differs"
        if k == 0:
            continue
        assert g["new_keyframe"] == c["new_keyframe"] and g["solve_status"] == c["solve_status"], f"{tag} frame {k}: decisions differ"
        for key in ("pose_to_keyframe", "abs_pose"):
            assert np.array_equal(g[key].view(np.uint32), c[key].view(np.uint32)), f"{tag} frame {k}: {key} differs"
        assert g["motion"] == c["motion"], f"{tag} frame {k}: motion score differs"


@pytest.fixture(scope="module")
def identity_drive():
    from odometry_amd import synth
    ref = synth.make_rgbd_sequence(N_FRAMES, **DRIVE)
    raw = raw_sequence(RIGS()["identity"], N_FRAMES)
    return ref, raw


@pytest.mark.parametrize("hints", [False, True])
@pytest.mark.parametrize("overlap", [0, 1, 2])
def test_tracker_fed_from_the_front_end_equals_the_tracker_fed_premade_buffers(identity_drive, overlap, hints):
    ref, raw = identity_drive
    r = RIGS()["identity"]
    a = _tracker(r["K"], overlap_depth=overlap)
    want = _run_premade(a, [(a.upload_frame(g), a.upload_depth(d)) for g, d in zip(ref["gray"], ref["depth"])], hints)
    a.close()
    b = _tracker(r["K"], overlap_depth=overlap)
    fe = _frontend(b, r, slots=4)
    got = _run_from_frontend(b, fe, [(fe.upload(c), fe.upload(d)) for c, d in zip(raw["colour"], raw["raw_depth"])], hints)
    n_kf = b.stats()["n_keyframes"]
    fe.close()
    b.close()
    _rows_equal(got, want, f"overlap {overlap} hints {hints}")
    assert n_kf >= 3 and all(g["solve_status"] == 0 for g in got[1:])


def test_rig_a_tracker_fed_from_the_front_end_equals_the_tracker_fed_the_models_frames():
    """Rig A over the pinned drive: the front end's frames are the model's, so the tracker's results are equal. The translation errors
    against the drive's true poses are printed beside those of the tracker fed ground-truth-registered depth;
    there is no reference to derive a bound for their difference from, so only failures are asserted: no frame's Solve or depth
    fails on either."""
    r = RIGS()["A"]
    raw = raw_sequence(r, N_FRAMES, tint_seed=5)
    model = [frontend_model(c, d, r, 1000.0, 1000.0) for c, d in zip(raw["colour"], raw["raw_depth"])]
    runs = {}
    for name, frames in (("model", [(m[0], m[1]) for m in model]), ("ground truth", list(zip([m[0] for m in model], raw["depth_gt"])))):
        t = _tracker(r["K"], overlap_depth=2)
        runs[name] = _run_premade(t, [(t.upload_frame(g), t.upload_depth(d)) for g, d in frames], True)
        t.close()
    t = _tracker(r["K"], overlap_depth=2)
    fe = _frontend(t, r, slots=4)
    runs["front end"] = _run_from_frontend(t, fe, list(zip(raw["colour"], raw["raw_depth"])), True)   # host path
    fe.close()
    t.close()
    _rows_equal(runs["front end"], runs["model"], "rig A")
    for name in ("front end", "ground truth"):
        err = translation_errors(runs[name], raw["poses"])
        print(f"rig A, tracker fed by {name}: translation error per frame (m): " + " ".join(f"{e:.4f}" for e in err))
        print(f"rig A, tracker fed by {name}: mean {err.mean():.4f} max {err.max():.4f} m, "
              f"keyframes {sum(1 for g in runs[name][1:] if g['new_keyframe']) + 1}")
        assert all(g["solve_status"] == 0 for g in runs[name][1:]), name
        assert all(g["n_valid"] >= 500 for g in runs[name]), name
