"""Dense stereo depth on the GPU (odo_stereo_depth_*, api.StereoDepth) against the numpy model of tests/stereo_depth_cases.py: every
row of the table bit for bit — depth frame, q frame and all counters, no tolerance — into a buffer pre-filled with 0xAB with guarded
margins, two runs, both store paths on one pair, the internal and the caller's output frame, disparity() and download(), every
refusal with the outputs and the statistics unchanged after it, two matchers on one context, destroy with a run in flight, the timing
call, and the hand-over: the matcher's device frame straight into TsdfVolume.integrate and into RgbdTracker.init / track, equal to
the same consumers fed the model's frames from the host."""
import ctypes as C

import numpy as np
import pytest

import stereo_depth_cases as sdc
from test_gpu_depth_filter import Guarded

pytestmark = pytest.mark.gpu
ZERO = dict.fromkeys(sdc.STATS, 0)


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _matcher(owner, size, p):
    from odometry_amd import api
    return api.StereoDepth(owner, size, p["fx"], p["baseline"], p["depth_scale"], p["dmin"], p["dmax"], p["A"], p["uniq"], p["lr_max"],
                           None if p["max_raw"] == 65535 else p["max_raw"] / p["depth_scale"])      # (the rows with a max_raw have depth_scale 1)


def _run(ctx, sd, L, R, offset=0):
    """One run of the pair into a guarded buffer: (depth, q, statistics)."""
    left, right = ctx.upload(L), ctx.upload(R)
    dst = Guarded(ctx, 2 * L.size, offset)
    assert sd.run(left, right, dst.p).value == dst.p.value
    depth, q, stats = dst.frame(L.shape).copy(), sd.disparity(), sd.stats()
    for b in (left, right):
        ctx.free(b)
    dst.free()
    return depth, q, stats


@pytest.mark.parametrize("index", range(len(sdc.rows())), ids=sdc.row_ids())
def test_every_row_bit_for_bit(ctx, index):
    name, L, R, p, _ = sdc.rows()[index]
    want_d, want_q, want_s, _ = sdc.model_of(index)
    sd = _matcher(ctx, L.shape, p)
    assert sd.params.max_raw == p["max_raw"] and sd.stats() == ZERO and not sd.disparity().any()          # before the first run
    depth, q, stats = _run(ctx, sd, L, R)
    assert np.array_equal(q, want_q), (name, np.argwhere(q != want_q)[:4])
    assert np.array_equal(depth, want_d), (name, np.argwhere(depth != want_d)[:4])
    assert stats == want_s, (name, stats, want_s)
    d2, q2, s2 = _run(ctx, sd, L, R)
    assert d2.tobytes() == depth.tobytes() and q2.tobytes() == q.tobytes() and s2 == stats, name
    sd.close()


@pytest.mark.parametrize("size", [(12, 64), (13, 68), (30, 132)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_store_paths_give_the_same_frame(ctx, size):
    """cols % 4 == 0 with an 8-byte aligned output takes the 8-byte stores; the same pair into a frame 2, 4 and 6 bytes off that
    alignment takes the guarded pixel path: all equal the model."""
    L, R = sdc.shifted_pair(21, size, 6)
    for A in (0, 3):
        p = sdc.params(A=A, dmax=30)
        want_d, want_q, want_s = sdc.stereo_model(L, R, p)
        assert want_s["matched"] > 0 or size[0] < 2 * A + 7
        sd = _matcher(ctx, size, p)
        for off in (0, 2, 4, 6):
            depth, q, stats = _run(ctx, sd, L, R, off)
            assert np.array_equal(depth, want_d) and np.array_equal(q, want_q) and stats == want_s, (size, A, off)
        sd.close()


def test_internal_and_callers_output_frame_disparity_and_download(ctx):
    from odometry_amd import api
    L, R = sdc.shifted_pair(22, (40, 100), 9)
    p = sdc.params(dmax=40)
    want_d, want_q, want_s = sdc.stereo_model(L, R, p)
    sd = api.StereoDepth(ctx, L.shape, p["fx"], p["baseline"], min_disp=1, max_disp=40, max_depth=None)       # the defaults are the rest
    assert (sd.params.agg_radius, sd.params.uniqueness, sd.params.lr_max, sd.params.max_raw, sd.params.depth_scale) == (2, 10, 1, 65535, 1000.0)
    for kw, max_raw in ((dict(max_depth=30.0), 30000), (dict(depth_scale=5000.0, max_depth=20.0), 65535), (dict(depth_scale=5000.0, max_depth=2.5), 12500)):
        other = api.StereoDepth(ctx, L.shape, 100.0, 0.5, **kw)
        assert other.params.max_raw == max_raw, kw
        other.close()
    left, right = ctx.upload(L), ctx.upload(R)
    own = sd.run(left, right)
    assert own.value == sd.run(left, right).value                                   # the same internal frame every time
    assert np.array_equal(sd.download(), want_d) and np.array_equal(sd.disparity(), want_q) and sd.stats() == want_s
    assert np.array_equal(ctx.download(own, L.shape, np.uint16), want_d)
    # a caller's frame leaves the internal one as it was; the q frame is the matcher's own either way
    L2, R2 = sdc.shifted_pair(23, (40, 100), 4)
    d2, q2, s2 = sdc.stereo_model(L2, R2, p)
    left2, right2 = ctx.upload(L2), ctx.upload(R2)
    dst = Guarded(ctx, 2 * L.size)
    sd.run(left2, right2, dst.p)
    assert np.array_equal(dst.frame(L.shape), d2) and np.array_equal(sd.download(dst.p), d2) and np.array_equal(sd.download(), want_d)
    assert np.array_equal(sd.disparity(), q2) and sd.stats() == s2 and s2 != want_s
    sd.close()
    sd.close()                                                                      # twice is harmless
    dst.free()
    for b in (left, right, left2, right2):
        ctx.free(b)


def test_refusals_leave_the_outputs_and_the_statistics_unchanged(ctx):
    """Every bound of create with a live context, NULL and misaligned frames, an output that overlaps an input, a bad reps: -1 with a
    message, and the last run's depth frame, q frame and statistics are what they were."""
    from odometry_amd import _lib as L_
    from test_stereo_depth_cpu import bad_params, c_params
    lib = L_.load()
    L, R = sdc.shifted_pair(24, (30, 80), 5)
    p = sdc.params()
    want_d, want_q, want_s = sdc.stereo_model(L, R, p)
    sd = _matcher(ctx, L.shape, p)
    left, right = ctx.upload(L), ctx.upload(R)
    dst = Guarded(ctx, 2 * L.size)
    sd.run(left, right, dst.p)

    def unchanged(what):
        assert np.array_equal(dst.frame(L.shape), want_d) and np.array_equal(sd.disparity(), want_q) and sd.stats() == want_s, what
        assert np.array_equal(ctx.download(left, L.shape, np.float32), L) and np.array_equal(ctx.download(right, L.shape, np.float32), R), what

    unchanged("the run itself")
    for what, bad, _ in bad_params():
        h = C.c_void_p(0x5A5A)
        assert lib.odo_stereo_depth_create(ctx.h, C.byref(bad), C.byref(h)) == -1 and h.value == 0x5A5A, what
        assert "odo_stereo_depth_create" in L_.last_error(), what
        unchanged(what)
    h = C.c_void_p(0x5A5A)
    assert lib.odo_stereo_depth_create(None, C.byref(c_params()), C.byref(h)) == -1 and h.value == 0x5A5A
    us = (C.c_float * 3)(7.0, 7.0, 7.0)
    off = lambda ptr, n: C.c_void_p(ptr.value + n)
    calls = [("left NULL", lambda: lib.odo_stereo_depth_run_dev(sd.h, None, right, dst.p)),
             ("right NULL", lambda: lib.odo_stereo_depth_run_dev(sd.h, left, None, dst.p)),
             ("matcher NULL", lambda: lib.odo_stereo_depth_run_dev(None, left, right, dst.p)),
             ("odd output", lambda: lib.odo_stereo_depth_run_dev(sd.h, left, right, off(dst.p, 1))),
             ("left off by two bytes", lambda: lib.odo_stereo_depth_run_dev(sd.h, off(left, 2), right, dst.p)),
             ("output == left", lambda: lib.odo_stereo_depth_run_dev(sd.h, left, right, left)),
             ("output inside right", lambda: lib.odo_stereo_depth_run_dev(sd.h, left, right, off(right, 4 * L.size - 2))),
             ("time: left NULL", lambda: lib.odo_stereo_depth_time_dev(sd.h, None, right, dst.p, 3, us)),
             ("time: us NULL", lambda: lib.odo_stereo_depth_time_dev(sd.h, left, right, dst.p, 3, None)),
             ("time: reps 0", lambda: lib.odo_stereo_depth_time_dev(sd.h, left, right, dst.p, 0, us)),
             ("time: reps 10001", lambda: lib.odo_stereo_depth_time_dev(sd.h, left, right, dst.p, 10001, us)),
             ("time: output == right", lambda: lib.odo_stereo_depth_time_dev(sd.h, left, right, right, 3, us)),
             ("stats NULL", lambda: lib.odo_stereo_depth_stats(sd.h, None)),
             ("disparity NULL", lambda: lib.odo_stereo_depth_disparity_dev(sd.h, None)),
             ("depth NULL", lambda: lib.odo_stereo_depth_depth_dev(sd.h, None))]
    for what, call in calls:
        assert call() == -1 and L_.last_error(), what
        assert list(us) == [7.0] * 3, what
        unchanged(what)
    with pytest.raises(L_.OdoError):
        sd.run(left, right, left)
    unchanged("api")
    sd.close()
    dst.free()
    for b in (left, right):
        ctx.free(b)


def test_two_matchers_on_one_context(ctx):
    """Enqueued alternately, nothing waited for in between: each has its own planes, q frame and statistics."""
    L, R = sdc.shifted_pair(25, (50, 140), 11)
    pa, pb = sdc.params(A=0, dmax=30, lr_max=0), sdc.params(A=3, dmin=4, dmax=60, uniq=25)
    a, b = _matcher(ctx, L.shape, pa), _matcher(ctx, L.shape, pb)
    left, right = ctx.upload(L), ctx.upload(R)
    da, db = Guarded(ctx, 2 * L.size), Guarded(ctx, 2 * L.size)
    for _ in range(2):
        a.run(left, right, da.p)
        b.run(left, right, db.p)
    wa, wb = sdc.stereo_model(L, R, pa), sdc.stereo_model(L, R, pb)
    assert np.array_equal(da.frame(L.shape), wa[0]) and np.array_equal(db.frame(L.shape), wb[0])
    assert np.array_equal(a.disparity(), wa[1]) and np.array_equal(b.disparity(), wb[1])
    assert a.stats() == wa[2] and b.stats() == wb[2] and wa[2] != wb[2]
    for x in (a, b):
        x.close()
    for x in (da, db):
        x.free()
    for x in (left, right):
        ctx.free(x)


def test_destroy_with_a_run_in_flight(ctx):
    index = sdc.row_ids().index("rendered pair natural 188 x 620, A = 3")
    _, L, R, p, _ = sdc.rows()[index]
    sd = _matcher(ctx, L.shape, p)
    left, right = ctx.upload(L), ctx.upload(R)
    dst = Guarded(ctx, 2 * L.size)
    for _ in range(10):
        sd.run(left, right, dst.p)
    sd.close()                                              # waits for the runs, then frees the planes they read and write
    assert np.array_equal(dst.frame(L.shape), sdc.model_of(index)[0])
    dst.free()
    for x in (left, right):
        ctx.free(x)


def test_timing_call_leaves_the_outputs_of_one_run(ctx):
    index = sdc.row_ids().index("rendered pair natural 188 x 620, A = 2")
    _, L, R, p, _ = sdc.rows()[index]
    want_d, want_q, want_s, _ = sdc.model_of(index)
    sd = _matcher(ctx, L.shape, p)
    left, right = ctx.upload(L), ctx.upload(R)
    dst = Guarded(ctx, 2 * L.size)
    us = sd.time(left, right, dst.p, reps=3)
    print("188 x 620, 63 candidates, A = 2:", ", ".join(f"{k} {v:.1f} us" for k, v in us.items()),
          "(3 launches each between two events; tools/stereo_depth_cost.py measures)")
    assert sorted(us) == ["census", "match_left", "match_right"] and all(v > 0.0 and np.isfinite(v) for v in us.values())
    assert np.array_equal(dst.frame(L.shape), want_d) and np.array_equal(sd.disparity(), want_q) and sd.stats() == want_s
    own = sd.time(left, right, reps=1)                      # and into the internal frame
    assert all(v > 0.0 for v in own.values()) and np.array_equal(sd.download(), want_d)
    sd.close()
    dst.free()
    for x in (left, right):
        ctx.free(x)


# ---- hand-over ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drive():
    """Three frames of the natural drive at 188 x 620 with the KITTI intrinsics halved, and the model's depth frame of each."""
    from odometry_amd import synth
    f, cx, cy = synth.KITTI_F / 2, synth.KITTI_CX / 2, synth.KITTI_CY / 2
    seq = synth.make_sequence(3, rows=188, cols=620, f=f, cx=cx, cy=cy, with_depth=True, drive="natural")
    p = sdc.rendered_params(2)
    model = [sdc.stereo_model(l, r, p)[0] for l, r in zip(seq["left"], seq["right"])]
    return dict(seq=seq, p=p, K=(f, cx, cy), model=model)


def test_matcher_feeds_the_volume_on_the_device(ctx, drive):
    """Each pair through StereoDepth.run straight into TsdfVolume.integrate on the device, with the true poses, nothing waited for in
    between: the same grid, bit for bit, as a second volume fed the model's frames from the host."""
    from odometry_amd import api
    seq, p = drive["seq"], drive["p"]
    make = lambda: api.TsdfVolume(ctx, (128, 64, 128), 0.2, (-12.8, -6.4, 0.0), 0.6, 20.0, 64, (188, 620), drive["K"], 1000.0)
    from_device, from_host = make(), make()
    sd = _matcher(ctx, (188, 620), p)
    bufs = []
    for l, r, pose, frame in zip(seq["left"], seq["right"], seq["poses"], drive["model"]):
        left, right = ctx.upload(np.asarray(l, np.float32)), ctx.upload(np.asarray(r, np.float32))
        bufs += [left, right]
        from_device.integrate(sd.run(left, right), pose)
        from_host.integrate(frame, pose)
    (qd, wd), (qh, wh) = from_device.grid(), from_host.grid()
    assert int((wh != 0).sum()) > 10000
    assert np.array_equal(wd, wh) and np.array_equal(qd, qh)
    assert np.array_equal(sd.download(), drive["model"][-1])
    for v in (from_device, from_host):
        v.close()
    sd.close()
    for b in bufs:
        ctx.free(b)


def test_matcher_feeds_the_rgbd_tracker_after_a_synchronize(drive):
    """RgbdTracker.init / track on the left image with the matcher's device frame (made on the tracker's context, which is then
    synchronized: the tracker reads its depth frame on a stream of its own) equals the tracker fed the model's frame, pose bits
    included."""
    from odometry_amd import _lib as L_, api
    seq, p = drive["seq"], drive["p"]
    args = dict(depth_scale=1000.0, max_depth_step=0.05, rows=188, cols=620, levels=3, lm_max_iters=(10, 20, 30), K=drive["K"], any_size=1)

    def matched_frame(trk, sd, left, right):
        """The pair's depth in a device buffer of the tracker's, complete: the tracker's context is synchronized."""
        frame = C.c_void_p()
        L_.check(trk.lib.odo_dev_alloc(trk._ctx, 2 * 188 * 620, C.byref(frame)), "odo_dev_alloc")
        trk._bufs.append(frame)
        sd.run(left, right, frame)
        L_.check(trk.lib.odo_ctx_synchronize(trk._ctx), "odo_ctx_synchronize")
        return frame

    def run(with_matcher):
        trk = api.RgbdTracker(0, **args)
        sd = _matcher(trk, (188, 620), p) if with_matcher else None
        out = []
        for k, (l, r) in enumerate(zip(seq["left"], seq["right"])):
            grey = trk.upload_frame(l)
            frame = matched_frame(trk, sd, grey, trk.upload_frame(r)) if with_matcher else trk.upload_depth(drive["model"][k])
            if k == 0:
                trk.init(grey, frame, seq["poses"][0])
            else:
                res = trk.track(grey, frame)
                out.append((res["abs_pose"].tobytes(), res["pose_to_keyframe"].tobytes(), res["new_keyframe"], res["solve_status"]))
        if sd is not None:
            assert np.array_equal(sd.download(frame), drive["model"][-1])
            sd.close()
        trk.close()
        return out

    a, b = run(True), run(False)
    print([(np.frombuffer(pose, np.float32)[3:12:4].round(3).tolist(), status) for pose, _, _, status in a])
    assert len(a) == 2 and a == b
