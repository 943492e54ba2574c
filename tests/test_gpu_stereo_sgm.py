"""The dense stereo matcher's semi-global mode on the GPU (odo_stereo_depth_enable_sgm, api.StereoDepth.enable_sgm) against the numpy
model of tests/stereo_sgm_cases.py: every row of the table bit for bit — the aggregate S through the debug read-out, the depth frame,
the q frame and all counters, no tolerance — into a buffer pre-filled with 0xAB with guarded margins, two runs; both path counts,
the caller's and the internal output frame, the box matcher's bytes after disable_sgm and other penalties after a second enable;
every refusal on a live context with frames, volume and statistics unchanged; the speckle filter behind the mode; two matchers on one
context, destroy with runs in flight, the timing call; and the hand-over: the mode's device frame straight into
TsdfVolume.integrate, equal to a volume fed the model's frame from the host."""
import ctypes as C

import numpy as np
import pytest

import speckle_cases as sc
import stereo_depth_cases as sdc
import stereo_sgm_cases as sgc
from test_gpu_depth_filter import Guarded
from test_gpu_stereo_depth import _matcher

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _sgm_matcher(ctx, size, p, sg):
    sd = _matcher(ctx, size, p)
    sd.enable_sgm(sg["p1"], sg["p2"], sg["paths"])
    return sd


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


@pytest.fixture(scope="module")
def natural():
    """The natural pair at 188 x 620 with rendered_params(2), and the model's result at the default penalties, 8 paths."""
    left, right = sdc.rendered_pair("natural")[:2]
    p = sdc.rendered_params(2)
    return dict(L=left, R=right, p=p, sg=sgc.sgm(), want=sgc.sgm_model(left, right, p, sgc.sgm()))


@pytest.mark.parametrize("index", range(len(sgc.rows())), ids=sgc.row_ids())
def test_every_row_bit_for_bit(ctx, index):
    name, L, R, p, sg, _ = sgc.rows()[index]
    want_d, want_q, want_s, want_S, _ = sgc.model_of(index)
    sd = _sgm_matcher(ctx, L.shape, p, sg)
    assert (sd.sgm_volume() == sgc.NONE).all() and not sd.disparity().any()                  # before the first run
    depth, q, stats = _run(ctx, sd, L, R)
    S = sd.sgm_volume()
    assert np.array_equal(S, want_S), (name, np.argwhere(S != want_S)[:4])
    assert np.array_equal(q, want_q), (name, np.argwhere(q != want_q)[:4])
    assert np.array_equal(depth, want_d), (name, np.argwhere(depth != want_d)[:4])
    assert stats == want_s, (name, stats, want_s)
    d2, q2, s2 = _run(ctx, sd, L, R)
    assert d2.tobytes() == depth.tobytes() and q2.tobytes() == q.tobytes() and s2 == stats and sd.sgm_volume().tobytes() == S.tobytes(), name
    sd.close()


def test_modes_paths_and_output_frames(ctx):
    """Both path counts into a caller's frame (at every alignment of it) and into the internal one; after disable_sgm the bytes are
    the box matcher's; enabling again with other penalties gives those penalties' frames."""
    from odometry_amd import _lib as L_
    L, R = sdc.occluding_step(31, (40, 120))
    p = sdc.params(dmin=1, dmax=24)
    box = sdc.stereo_model(L, R, p)
    sd = _matcher(ctx, L.shape, p)
    left, right = ctx.upload(L), ctx.upload(R)
    with pytest.raises(L_.OdoError):
        sd.sgm_volume()                                                                     # the mode is off
    with pytest.raises(L_.OdoError):
        sd.sgm_time(left, right)
    for sg in (sgc.sgm(paths=8), sgc.sgm(paths=4), sgc.sgm(p1=7, p2=900, paths=8)):
        want_d, want_q, want_s, want_S = sgc.sgm_model(L, R, p, sg)
        assert not np.array_equal(want_q, box[1])
        sd.enable_sgm(sg["p1"], sg["p2"], sg["paths"])
        for off in (0, 2, 4, 6):
            depth, q, stats = _run(ctx, sd, L, R, off)
            assert np.array_equal(depth, want_d) and np.array_equal(q, want_q) and stats == want_s, (sg, off)
        own = sd.run(left, right)
        assert own.value == sd.run(left, right).value
        assert np.array_equal(sd.download(), want_d) and np.array_equal(sd.sgm_volume(), want_S)
    sd.enable_sgm()                                                                         # the defaults: 100 / 600 at A = 2, 8 paths
    sd.run(left, right)
    assert np.array_equal(sd.disparity(), sgc.sgm_model(L, R, p, sgc.sgm())[1])
    sd.disable_sgm()
    depth, q, stats = _run(ctx, sd, L, R)
    assert np.array_equal(depth, box[0]) and np.array_equal(q, box[1]) and stats == box[2]
    assert all(v > 0.0 for v in sd.time(left, right, reps=1).values())                      # the old timing call is back
    with pytest.raises(L_.OdoError):
        sd.sgm_volume()
    sd.disable_sgm()                                                                        # twice is harmless
    sd.close()
    for b in (left, right):
        ctx.free(b)


def test_refusals_leave_frames_volume_and_statistics_unchanged(ctx):
    """Every bad bound on a live matcher (agg_radius 2), NULLs, bad frames and bad reps of the timing call, the old timing call
    while the mode is on: -1 with a message; the last run's frames, S and statistics are what they were, and so are the penalties."""
    from odometry_amd import _lib as L_
    from test_stereo_sgm_cpu import bad_sgm
    lib = L_.load()
    L, R = sdc.shifted_pair(32, (30, 80), 5)
    p, sg = sdc.params(), sgc.sgm(p1=50, p2=400, paths=4)
    want_d, want_q, want_s, want_S = sgc.sgm_model(L, R, p, sg)
    sd = _sgm_matcher(ctx, L.shape, p, sg)
    left, right = ctx.upload(L), ctx.upload(R)
    dst = Guarded(ctx, 2 * L.size)
    sd.run(left, right, dst.p)

    def unchanged(what):
        assert np.array_equal(dst.frame(L.shape), want_d) and np.array_equal(sd.disparity(), want_q) and sd.stats() == want_s, what
        assert np.array_equal(sd.sgm_volume(), want_S), what

    unchanged("the run itself")
    us5, us3 = (C.c_float * 5)(*[7.0] * 5), (C.c_float * 3)(*[7.0] * 3)
    calls = [(what, lambda p1=p1, p2=p2, n=n: lib.odo_stereo_depth_enable_sgm(sd.h, p1, p2, n)) for what, p1, p2, n, _ in bad_sgm(True)]
    calls += [("time: left NULL", lambda: lib.odo_stereo_depth_sgm_time_dev(sd.h, None, right, dst.p, 3, us5)),
              ("time: us NULL", lambda: lib.odo_stereo_depth_sgm_time_dev(sd.h, left, right, dst.p, 3, None)),
              ("time: reps 0", lambda: lib.odo_stereo_depth_sgm_time_dev(sd.h, left, right, dst.p, 0, us5)),
              ("time: reps 10001", lambda: lib.odo_stereo_depth_sgm_time_dev(sd.h, left, right, dst.p, 10001, us5)),
              ("time: output == right", lambda: lib.odo_stereo_depth_sgm_time_dev(sd.h, left, right, right, 3, us5)),
              ("the old timing call", lambda: lib.odo_stereo_depth_time_dev(sd.h, left, right, dst.p, 3, us3)),
              ("volume NULL", lambda: lib.odo_debug_sgm_volume(sd.h, None)),
              ("run: left NULL", lambda: lib.odo_stereo_depth_run_dev(sd.h, None, right, dst.p)),
              ("run: output == left", lambda: lib.odo_stereo_depth_run_dev(sd.h, left, right, left))]
    for what, call in calls:
        assert call() == -1 and L_.last_error(), what
        if what == "the old timing call":
            assert "odo_stereo_depth_sgm_time_dev" in L_.last_error()
        assert list(us5) == [7.0] * 5 and list(us3) == [7.0] * 3, what
        unchanged(what)
    sd.run(left, right, dst.p)                                                               # still 50 / 400, 4 paths
    unchanged("a run after the refusals")
    # the volume's bound needs a matcher of its own: 4096 x 8192 x 33 entries exceed 2^30
    big = _matcher(ctx, (4096, 8192), sdc.params(dmin=8, dmax=40))
    assert lib.odo_stereo_depth_enable_sgm(big.h, 100, 600, 8) == -1 and "2^30" in L_.last_error()
    big.close()
    unchanged("another matcher's refusal")
    sd.close()
    dst.free()
    for b in (left, right):
        ctx.free(b)


def test_speckle_filter_behind_the_mode(ctx):
    L, R = sc.wall_pair()
    p, sg = sc.wall_params(), sgc.sgm()
    depth, q, stats, _ = sgc.sgm_model(L, R, p, sg)
    M = sc.speckle_model(q, 16, 100)
    want_d, want_q = sc.apply_keep(depth, M), sc.apply_keep(q, M)
    assert M["stats"]["pixels"] == stats["matched"] and M["stats"]["removed_pixels"] > 0
    sd = _sgm_matcher(ctx, L.shape, p, sg)
    sd.enable_speckle(16, 100)
    left, right = ctx.upload(L), ctx.upload(R)
    dst = Guarded(ctx, 2 * L.size)
    for _ in range(2):
        sd.run(left, right, dst.p)
        assert np.array_equal(dst.frame(L.shape), want_d) and np.array_equal(sd.disparity(), want_q)
        assert sd.stats() == stats and sd.speckle_stats() == M["stats"]
    sd.run(left, right)
    assert np.array_equal(sd.download(), want_d)
    sd.close()
    dst.free()
    for b in (left, right):
        ctx.free(b)


def test_two_matchers_on_one_context(ctx):
    """The mode and the box matcher enqueued alternately, nothing waited for in between: each has its own planes, frames, statistics."""
    L, R = sdc.shifted_pair(33, (50, 140), 11)
    pa, pb, sg = sdc.params(A=1, dmax=30), sdc.params(A=3, dmin=4, dmax=60, uniq=25), sgc.sgm(A=1)
    a, b = _sgm_matcher(ctx, L.shape, pa, sg), _matcher(ctx, L.shape, pb)
    left, right = ctx.upload(L), ctx.upload(R)
    da, db = Guarded(ctx, 2 * L.size), Guarded(ctx, 2 * L.size)
    for _ in range(2):
        a.run(left, right, da.p)
        b.run(left, right, db.p)
    wa, wb = sgc.sgm_model(L, R, pa, sg), sdc.stereo_model(L, R, pb)
    assert np.array_equal(da.frame(L.shape), wa[0]) and np.array_equal(db.frame(L.shape), wb[0])
    assert np.array_equal(a.disparity(), wa[1]) and np.array_equal(b.disparity(), wb[1])
    assert a.stats() == wa[2] and b.stats() == wb[2] and np.array_equal(a.sgm_volume(), wa[3])
    for x in (a, b):
        x.close()
    for x in (da, db):
        x.free()
    for x in (left, right):
        ctx.free(x)


def test_destroy_with_ten_runs_in_flight(ctx, natural):
    L, R = natural["L"], natural["R"]
    sd = _sgm_matcher(ctx, L.shape, natural["p"], natural["sg"])
    left, right = ctx.upload(L), ctx.upload(R)
    dst = Guarded(ctx, 2 * L.size)
    for _ in range(10):
        sd.run(left, right, dst.p)
    sd.close()                                              # waits for the runs, then frees the volumes they read and write
    assert np.array_equal(dst.frame(L.shape), natural["want"][0])
    dst.free()
    for x in (left, right):
        ctx.free(x)


def test_timing_call_leaves_the_outputs_of_one_run(ctx, natural):
    L, R = natural["L"], natural["R"]
    want_d, want_q, want_s, want_S = natural["want"]
    sd = _sgm_matcher(ctx, L.shape, natural["p"], natural["sg"])
    left, right = ctx.upload(L), ctx.upload(R)
    dst = Guarded(ctx, 2 * L.size)
    us = sd.sgm_time(left, right, dst.p, reps=3)
    print("188 x 620, 63 candidates, A = 2, 8 paths:", ", ".join(f"{k} {v:.1f} us" for k, v in us.items()),
          "(3 repetitions each between two events; tools/stereo_sgm_cost.py measures)")
    assert tuple(us) == sd.SGM_GROUPS and all(v > 0.0 and np.isfinite(v) for v in us.values())
    assert np.array_equal(dst.frame(L.shape), want_d) and np.array_equal(sd.disparity(), want_q) and sd.stats() == want_s
    assert np.array_equal(sd.sgm_volume(), want_S)
    own = sd.sgm_time(left, right, reps=1)                  # and into the internal frame
    assert all(v > 0.0 for v in own.values()) and np.array_equal(sd.download(), want_d)
    sd.close()
    dst.free()
    for x in (left, right):
        ctx.free(x)


def test_mode_feeds_the_volume_on_the_device(ctx, natural):
    """The natural pair through the mode straight into TsdfVolume.integrate on the device, nothing waited for in between: the same
    grid, bit for bit, as a second volume fed the model's frame from the host."""
    from odometry_amd import api, synth
    K = (synth.KITTI_F / 2, synth.KITTI_CX / 2, synth.KITTI_CY / 2)
    pose = synth.drive_trajectory("natural", 1, 0)[0]
    make = lambda: api.TsdfVolume(ctx, (128, 64, 128), 0.2, (-12.8, -6.4, 0.0), 0.6, 20.0, 64, (188, 620), K, 1000.0)
    from_device, from_host = make(), make()
    sd = _sgm_matcher(ctx, (188, 620), natural["p"], natural["sg"])
    left, right = ctx.upload(natural["L"]), ctx.upload(natural["R"])
    from_device.integrate(sd.run(left, right), pose)
    from_host.integrate(natural["want"][0], pose)
    (qd, wd), (qh, wh) = from_device.grid(), from_host.grid()
    assert int((wh != 0).sum()) > 10000
    assert np.array_equal(wd, wh) and np.array_equal(qd, qh)
    assert np.array_equal(sd.download(), natural["want"][0])
    for v in (from_device, from_host):
        v.close()
    sd.close()
    for b in (left, right):
        ctx.free(b)
