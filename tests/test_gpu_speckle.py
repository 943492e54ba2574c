"""The speckle filter on the GPU (odo_speckle_*, api.SpeckleFilter, api.StereoDepth.enable_speckle) against the numpy model of
tests/speckle_cases.py: every row of the table bit for bit — both targets and all counters, no tolerance, guard == 0 — in buffers
pre-filled with 0xAB with guarded margins, with the key apart from the targets and as one of them, two runs, every refusal with the
frames and the statistics unchanged after it, two filters on one context, destroy with runs in flight, the timing call, the filter
behind the matcher (internal and caller's frame, and taken off again), and the hand-over: the filtered device frame straight into
TsdfVolume.integrate, equal to a volume fed the models' frame from the host."""
import ctypes as C

import numpy as np
import pytest

import speckle_cases as sc
import stereo_depth_cases as sdc
from test_gpu_depth_filter import MARGIN, Guarded

pytestmark = pytest.mark.gpu
ZERO = dict.fromkeys(sc.STATS, 0)
FILL = 0xABAB


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _held(ctx, frame=None, shape=None):
    """A guarded device buffer of one uint16 frame: 0xAB everywhere, or `frame` between the margins."""
    nbytes = 2 * (frame.size if frame is not None else shape[0] * shape[1])
    g = Guarded(ctx, nbytes)
    if frame is not None:
        blob = np.full(g.total, 0xAB, np.uint8)
        blob[MARGIN:MARGIN + nbytes] = np.ascontiguousarray(frame, np.uint16).reshape(-1).view(np.uint8)
        ctx.lib.odo_dev_upload(ctx.h, g.base, blob.ctypes.data_as(C.c_void_p), blob.nbytes)
    return g


@pytest.fixture(scope="module")
def big():
    """A 188 x 620 key frame and its model."""
    K = sc.blobs(7, (188, 620), 0.1)
    return K, sc.speckle_model(K, 3, 40)


@pytest.mark.parametrize("index", range(len(sc.rows())), ids=sc.row_ids())
def test_every_row_bit_for_bit(ctx, index):
    from odometry_amd import api
    name, K, max_diff, min_size, _ = sc.rows()[index]
    M = sc.model_of(index)
    want_fill, want_key = sc.apply_keep(np.full(K.shape, FILL), M), sc.apply_keep(K, M)
    flt = api.SpeckleFilter(ctx, K.shape, max_diff, min_size)
    assert flt.stats() == ZERO                                                      # before the first run
    key, a, b = _held(ctx, K), _held(ctx, shape=K.shape), _held(ctx, shape=K.shape)
    # the key apart from both targets, twice
    seen = []
    for _ in range(2):
        flt.run(key.p, a.p, b.p)
        seen.append((a.frame(K.shape).tobytes(), b.frame(K.shape).tobytes(), flt.stats()))
        assert np.array_equal(a.frame(K.shape), want_fill), (name, np.argwhere(a.frame(K.shape) != want_fill)[:4])
        assert np.array_equal(b.frame(K.shape), want_fill) and np.array_equal(key.frame(K.shape), K), name
        assert flt.stats() == M["stats"], (name, flt.stats(), M["stats"])
    assert seen[0] == seen[1], name
    # one target only
    a2 = _held(ctx, shape=K.shape)
    flt.run(key.p, a2.p)
    assert np.array_equal(a2.frame(K.shape), want_fill) and flt.stats() == M["stats"], name
    # the key as a target
    b2 = _held(ctx, shape=K.shape)
    flt.run(key.p, key.p, b2.p)
    assert np.array_equal(key.frame(K.shape), want_key), (name, np.argwhere(key.frame(K.shape) != want_key)[:4])
    assert np.array_equal(b2.frame(K.shape), want_fill) and flt.stats() == M["stats"], name
    flt.close()
    for g in (key, a, b, a2, b2):
        g.free()


def test_refusals_leave_the_frames_and_the_statistics_unchanged(ctx):
    """Every bound of create with a live context, NULL and misaligned frames, overlapping targets, a bad reps: -1 with a message, and
    the key, both targets and the statistics are what they were."""
    from odometry_amd import _lib as L_, api
    from test_speckle_cpu import bad_params, c_params
    lib = L_.load()
    index = sc.row_ids().index("blobs 33 x 128")
    _, K, max_diff, min_size, _ = sc.rows()[index]
    M = sc.model_of(index)
    want = sc.apply_keep(np.full(K.shape, FILL), M)
    flt = api.SpeckleFilter(ctx, K.shape, max_diff, min_size)
    key, a, b = _held(ctx, K), _held(ctx, shape=K.shape), _held(ctx, shape=K.shape)
    flt.run(key.p, a.p, b.p)

    def unchanged(what):
        assert np.array_equal(a.frame(K.shape), want) and np.array_equal(b.frame(K.shape), want) and np.array_equal(key.frame(K.shape), K), what
        assert flt.stats() == M["stats"], what

    unchanged("the run itself")
    for what, bad, _, word in bad_params():
        h = C.c_void_p(0x5A5A)
        assert lib.odo_speckle_create(ctx.h, C.byref(bad), C.byref(h)) == -1 and h.value == 0x5A5A, what
        assert "odo_speckle_create" in L_.last_error() and word in L_.last_error(), what
        unchanged(what)
    h = C.c_void_p(0x5A5A)
    assert lib.odo_speckle_create(None, C.byref(c_params()), C.byref(h)) == -1 and h.value == 0x5A5A
    us = (C.c_float * 5)(*[7.0] * 5)
    off = lambda ptr, n: C.c_void_p(ptr.value + n)
    calls = [("key NULL", lambda: lib.odo_speckle_run_dev(flt.h, None, a.p, b.p)),
             ("target a NULL", lambda: lib.odo_speckle_run_dev(flt.h, key.p, None, b.p)),
             ("filter NULL", lambda: lib.odo_speckle_run_dev(None, key.p, a.p, b.p)),
             ("odd key", lambda: lib.odo_speckle_run_dev(flt.h, off(key.p, 1), a.p, b.p)),
             ("odd target a", lambda: lib.odo_speckle_run_dev(flt.h, key.p, off(a.p, 1), b.p)),
             ("odd target b", lambda: lib.odo_speckle_run_dev(flt.h, key.p, a.p, off(b.p, 1))),
             ("target b two bytes into target a", lambda: lib.odo_speckle_run_dev(flt.h, key.p, a.p, off(a.p, 2))),
             ("target a ends inside target b", lambda: lib.odo_speckle_run_dev(flt.h, key.p, off(b.p, 2 - 2 * K.size), b.p)),
             ("time: key NULL", lambda: lib.odo_speckle_time_dev(flt.h, None, a.p, b.p, 3, us)),
             ("time: us NULL", lambda: lib.odo_speckle_time_dev(flt.h, key.p, a.p, b.p, 3, None)),
             ("time: reps 0", lambda: lib.odo_speckle_time_dev(flt.h, key.p, a.p, b.p, 0, us)),
             ("time: reps 10001", lambda: lib.odo_speckle_time_dev(flt.h, key.p, a.p, b.p, 10001, us)),
             ("time: overlapping targets", lambda: lib.odo_speckle_time_dev(flt.h, key.p, a.p, off(a.p, 2), 3, us)),
             ("stats NULL", lambda: lib.odo_speckle_stats(flt.h, None))]
    for what, call in calls:
        assert call() == -1 and L_.last_error(), what
        assert list(us) == [7.0] * 5, what
        unchanged(what)
    with pytest.raises(L_.OdoError):
        flt.run(key.p, a.p, off(a.p, 2))
    with pytest.raises(L_.OdoError):
        api.SpeckleFilter(ctx, K.shape, 8, 0)
    unchanged("api")
    flt.close()
    flt.close()                                                                     # twice is harmless
    for g in (key, a, b):
        g.free()


def test_two_filters_on_one_context(ctx):
    """Enqueued alternately, nothing waited for in between: each has its own planes and statistics."""
    from odometry_amd import api
    K = sc.blobs(8, (50, 140), 0.15)
    pa, pb = (1, 4), (3, 25)
    fa, fb = api.SpeckleFilter(ctx, K.shape, *pa), api.SpeckleFilter(ctx, K.shape, *pb)
    key, a, b = _held(ctx, K), _held(ctx, shape=K.shape), _held(ctx, shape=K.shape)
    for _ in range(2):
        fa.run(key.p, a.p)
        fb.run(key.p, b.p)
    ma, mb = sc.speckle_model(K, *pa), sc.speckle_model(K, *pb)
    fill = np.full(K.shape, FILL)
    assert np.array_equal(a.frame(K.shape), sc.apply_keep(fill, ma)) and np.array_equal(b.frame(K.shape), sc.apply_keep(fill, mb))
    assert fa.stats() == ma["stats"] and fb.stats() == mb["stats"] and ma["stats"] != mb["stats"]
    for x in (fa, fb):
        x.close()
    for x in (key, a, b):
        x.free()


def test_destroy_with_runs_in_flight(ctx, big):
    from odometry_amd import api
    K, M = big
    flt = api.SpeckleFilter(ctx, K.shape, 3, 40)
    key, a = _held(ctx, K), _held(ctx, shape=K.shape)
    for _ in range(10):
        flt.run(key.p, a.p)
    flt.close()                                             # waits for the runs, then frees the planes they read and write
    assert np.array_equal(a.frame(K.shape), sc.apply_keep(np.full(K.shape, FILL), M))
    for x in (key, a):
        x.free()


def test_timing_call_leaves_the_result_of_one_run(ctx, big):
    from odometry_amd import api
    K, M = big
    flt = api.SpeckleFilter(ctx, K.shape, 3, 40)
    key, a, b = _held(ctx, K), _held(ctx, shape=K.shape), _held(ctx, shape=K.shape)
    us = flt.time(key.p, a.p, b.p, reps=3)
    print("188 x 620:", ", ".join(f"{k} {v:.1f} us" for k, v in us.items()), "(3 launches each between two events; tools/speckle_cost.py measures)")
    assert tuple(us) == api.SpeckleFilter.KERNELS and all(np.isfinite(v) for v in us.values()) and us["run"] > 0.0
    fill = sc.apply_keep(np.full(K.shape, FILL), M)
    assert np.array_equal(a.frame(K.shape), fill) and np.array_equal(b.frame(K.shape), fill) and np.array_equal(key.frame(K.shape), K)
    assert flt.stats() == M["stats"] and M["stats"]["removed_pixels"] > 1000 and M["stats"]["largest"] > 1000
    own = flt.time(key.p, key.p, reps=2)                    # the key as its own target: the repeats run on copies
    assert own["run"] > 0.0 and np.array_equal(key.frame(K.shape), sc.apply_keep(K, M)) and flt.stats() == M["stats"]
    flt.close()
    for x in (key, a, b):
        x.free()


# ---- behind the matcher -------------------------------------------------------------------------------------------------------------------
def _matcher(owner, size, p):
    from odometry_amd import api
    return api.StereoDepth(owner, size, p["fx"], p["baseline"], p["depth_scale"], p["dmin"], p["dmax"], p["A"], p["uniq"], p["lr_max"],
                           None if p["max_raw"] == 65535 else p["max_raw"] / p["depth_scale"])


PAIRS = (("integer disparity pair 96 x 320", 8, 200), ("occluding step, lr_max 1", 8, 60), ("num of both signs", 4, 30),
         ("tile geometry 13 x 129", 8, 20), ("right image of period 17", 8, 250), ("wall", 16, 100))


def _pair(name):
    """(L, R, matcher parameters, the matcher model's (depth, q, stats)) of a row of stereo_depth_cases, or of the wall scene."""
    if name == "wall":
        return (*sc.wall_pair(), sc.wall_params(), sc.wall_match())
    index = sdc.row_ids().index(name)
    _, L, R, p, _ = sdc.rows()[index]
    return L, R, p, sdc.model_of(index)[:3]


@pytest.mark.parametrize("name,max_diff,min_size", PAIRS, ids=[p[0] for p in PAIRS])
def test_filter_behind_the_matcher(ctx, name, max_diff, min_size):
    """After enable_speckle the depth frame, the q frame and both sets of counters equal speckle_model applied to stereo_model's q, in
    the internal output frame and in a caller's; after enable_speckle(.., 0) the bytes are those of a matcher that never had it."""
    from odometry_amd import _lib as L_
    L, R, p, (depth, q, stats) = _pair(name)
    M = sc.speckle_model(q, max_diff, min_size)
    want_d, want_q = sc.apply_keep(depth, M), sc.apply_keep(q, M)
    assert M["stats"]["pixels"] == stats["matched"] and M["stats"]["removed_pixels"] > 0
    sd = _matcher(ctx, L.shape, p)
    left, right = ctx.upload(L), ctx.upload(R)
    with pytest.raises(L_.OdoError):
        sd.speckle_stats()                                                          # none enabled yet
    sd.run(left, right)
    assert np.array_equal(sd.download(), depth) and np.array_equal(sd.disparity(), q) and sd.stats() == stats
    sd.enable_speckle(max_diff, min_size)
    for _ in range(2):
        sd.run(left, right)
        assert np.array_equal(sd.download(), want_d), (name, np.argwhere(sd.download() != want_d)[:4])
        assert np.array_equal(sd.disparity(), want_q) and sd.stats() == stats and sd.speckle_stats() == M["stats"], (name, sd.speckle_stats())
    dst = Guarded(ctx, 2 * L.size)
    sd.run(left, right, dst.p)
    assert np.array_equal(dst.frame(L.shape), want_d) and np.array_equal(sd.disparity(), want_q) and sd.speckle_stats() == M["stats"]
    with pytest.raises(L_.OdoError):
        sd.enable_speckle(70000, 5)                                                 # a bad bound leaves the filter as it was
    sd.run(left, right, dst.p)
    assert np.array_equal(dst.frame(L.shape), want_d) and sd.speckle_stats() == M["stats"]
    sd.enable_speckle(max_diff, 0)
    sd.run(left, right, dst.p)
    assert np.array_equal(dst.frame(L.shape), depth) and np.array_equal(sd.disparity(), q) and sd.stats() == stats
    sd.run(left, right)
    assert np.array_equal(sd.download(), depth)
    sd.close()
    dst.free()
    for x in (left, right):
        ctx.free(x)


def test_filtered_frame_feeds_the_volume_on_the_device(ctx):
    """Two pairs of the natural drive through StereoDepth.run with the speckle filter enabled, straight into TsdfVolume.integrate on
    the device with the true poses, nothing waited for in between: the same grid, bit for bit, as a second volume fed the two models'
    filtered frame from the host."""
    from odometry_amd import api, synth
    f, cx, cy = synth.KITTI_F / 2, synth.KITTI_CX / 2, synth.KITTI_CY / 2
    seq = synth.make_sequence(2, rows=188, cols=620, f=f, cx=cx, cy=cy, with_depth=True, drive="natural")
    p = sdc.rendered_params(2)
    make = lambda: api.TsdfVolume(ctx, (128, 64, 128), 0.2, (-12.8, -6.4, 0.0), 0.6, 20.0, 64, (188, 620), (f, cx, cy), 1000.0)
    from_device, from_host = make(), make()
    sd = _matcher(ctx, (188, 620), p)
    sd.enable_speckle()                                                             # the defaults: max_diff 8, min_size 200
    bufs, removed = [], 0
    for l, r, pose in zip(seq["left"], seq["right"], seq["poses"]):
        depth, q, _ = sdc.stereo_model(l, r, p)
        M = sc.speckle_model(q, 8, 200)
        removed += M["stats"]["removed_pixels"]
        left, right = ctx.upload(np.asarray(l, np.float32)), ctx.upload(np.asarray(r, np.float32))
        bufs += [left, right]
        from_device.integrate(sd.run(left, right), pose)
        from_host.integrate(sc.apply_keep(depth, M), pose)
    (qd, wd), (qh, wh) = from_device.grid(), from_host.grid()
    assert removed > 100 and int((wh != 0).sum()) > 10000
    assert np.array_equal(wd, wh) and np.array_equal(qd, qh)
    assert sd.speckle_stats() == M["stats"] and np.array_equal(sd.download(), sc.apply_keep(depth, M))
    for v in (from_device, from_host):
        v.close()
    sd.close()
    for x in bufs:
        ctx.free(x)
