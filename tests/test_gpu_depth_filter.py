"""The bilateral depth filter on the GPU (odo_depth_filter_*, api.DepthFilter) against the numpy model of tests/depth_filter_cases.py:
every row of the table at every radius bit for bit, into a buffer pre-filled with 0xAB with guarded margins, the statistics, two runs,
both load paths on one frame, identity tables, every refusal with the frame and the statistics unchanged after it, two filters on one
context, destroy with a run in flight, the timing call, and the filter in front of the TSDF volume on the noisy ribbed corridor."""
import ctypes as C

import numpy as np
import pytest

import depth_filter_cases as dfc

pytestmark = pytest.mark.gpu
MARGIN = 64   # bytes in front of and behind every output frame, a multiple of 8: the frame keeps the buffer's alignment


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


class Guarded:
    """A device buffer of MARGIN + nbytes + MARGIN bytes filled with 0xAB; .p is the frame `offset` bytes behind the front margin."""

    def __init__(self, ctx, nbytes, offset=0):
        self.ctx, self.nbytes, self.offset = ctx, nbytes, offset
        self.total = 2 * MARGIN + nbytes + offset
        self.base = ctx.upload(np.full(self.total, 0xAB, np.uint8))
        self.p = C.c_void_p(self.base.value + MARGIN + offset)

    def frame(self, shape):
        """The frame, after checking that nothing round it was written (the download is ordered behind the run)."""
        b = self.ctx.download(self.base, (self.total,), np.uint8)
        lo = MARGIN + self.offset
        assert (b[:lo] == 0xAB).all() and (b[lo + self.nbytes:] == 0xAB).all(), "bytes outside the frame were written"
        return b[lo:lo + self.nbytes].view(np.uint16).reshape(shape)

    def free(self):
        self.ctx.free(self.base)


def _run(ctx, flt, raw, offset=0, in_offset=0):
    """One run of `raw` into a guarded buffer: (frame, statistics)."""
    src = Guarded(ctx, raw.nbytes, in_offset)
    blob = np.full(src.total, 0xAB, np.uint8)
    blob[MARGIN + in_offset:MARGIN + in_offset + raw.nbytes] = raw.reshape(-1).view(np.uint8)
    ctx.lib.odo_dev_upload(ctx.h, src.base, blob.ctypes.data_as(C.c_void_p), blob.nbytes)
    dst = Guarded(ctx, raw.nbytes, offset)
    assert flt.run(src.p, dst.p).value == dst.p.value
    out, stats = dst.frame(raw.shape).copy(), flt.stats()
    src.free()
    dst.free()
    return out, stats


@pytest.mark.parametrize("index", range(len(dfc.rows())), ids=dfc.row_ids())
def test_every_row_at_every_radius_bit_for_bit(ctx, index):
    from odometry_amd import api
    name, raw, tables_of, _, _ = dfc.rows()[index]
    for r in dfc.RADII:
        want, wstats = dfc.model_of(index, r)
        flt = api.DepthFilter(ctx, raw.shape, tables_of(r))
        assert flt.stats() == dict(n_valid=0, n_changed=0, sum_abs_change=0)          # before the first run
        got, stats = _run(ctx, flt, raw)
        assert np.array_equal(got, want), (name, r, np.argwhere(got != want)[:4])
        assert stats == wstats, (name, r, stats, wstats)
        again, stats2 = _run(ctx, flt, raw)
        assert again.tobytes() == got.tobytes() and stats2 == stats, (name, r)
        flt.close()


@pytest.mark.parametrize("size", [(16, 64), (17, 68), (120, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_load_paths_give_the_same_frame(ctx, size):
    """cols % 4 == 0 with 8-byte aligned frames takes the 8-byte loads and stores; the same frame 2, 4 and 6 bytes off that alignment
    (input, output, both) takes the guarded pixel path: all equal the model."""
    from odometry_amd import api
    raw = dfc.surface_frame(3, size)
    for r in (1, 4):
        tables = dfc.random_tables(5, r)
        want, wstats = dfc.filter_model(raw, *tables)
        flt = api.DepthFilter(ctx, size, tables)
        for off, in_off in ((0, 0), (2, 0), (0, 2), (4, 6), (6, 4)):
            got, stats = _run(ctx, flt, raw, off, in_off)
            assert np.array_equal(got, want) and stats == wstats, (size, r, off, in_off)
        flt.close()


def test_identity_tables_return_the_frame(ctx):
    from odometry_amd import api
    for size in ((1, 1), (17, 23), (48, 128)):
        raw = dfc.random_frame(9, size, 0.3)
        for r in dfc.RADII:
            flt = api.DepthFilter(ctx, size, dfc.identity_tables(r))
            got, stats = _run(ctx, flt, raw)
            assert np.array_equal(got, raw) and stats == dict(n_valid=int((raw != 0).sum()), n_changed=0, sum_abs_change=0)
            flt.close()


def test_default_tables_and_an_output_buffer_of_its_own(ctx):
    from odometry_amd import api
    raw = dfc.surface_frame(4, (60, 80))
    flt = api.DepthFilter(ctx, raw.shape, radius=3, sigma_s=2.0)
    want, wstats = dfc.filter_model(raw, *api.depth_filter_tables(radius=3, sigma_s=2.0))
    src = ctx.upload(raw)
    out = flt.run(src)
    assert out.value == flt.run(src).value                                       # the same buffer every time
    assert np.array_equal(flt.download(), want) and flt.stats() == wstats
    assert np.array_equal(ctx.download(out, raw.shape, np.uint16), want)
    with pytest.raises(TypeError):
        api.DepthFilter(ctx, raw.shape, dfc.default_tables(2), radius=3)
    flt.close()
    flt.close()                                                                  # twice is harmless
    ctx.free(src)


def test_refusals_leave_the_frame_and_the_statistics_unchanged(ctx):
    """Every bound of create with a live context, in == out, overlapping frames, NULL pointers, a bad reps: -1 with a message, and
    the last run's output and statistics are what they were."""
    from odometry_amd import _lib as L, api
    from test_depth_filter_cpu import _params, bad_params
    lib = L.load()
    raw = dfc.surface_frame(5, (40, 52))
    want, wstats = dfc.filter_model(raw, *dfc.default_tables(2))
    flt = api.DepthFilter(ctx, raw.shape)
    src = ctx.upload(raw)
    dst = Guarded(ctx, raw.nbytes)
    flt.run(src, dst.p)

    def unchanged(what):
        assert np.array_equal(dst.frame(raw.shape), want) and flt.stats() == wstats, what
        assert np.array_equal(ctx.download(src, raw.shape, np.uint16), raw), what

    unchanged("the run itself")
    for what, p in bad_params():
        h = C.c_void_p(0x5A5A)
        assert lib.odo_depth_filter_create(ctx.h, C.byref(p), C.byref(h)) == -1 and h.value == 0x5A5A, what
        assert "odo_depth_filter_create" in L.last_error(), what
        unchanged(what)
    good = _params(*raw.shape)
    h = C.c_void_p(0x5A5A)
    assert lib.odo_depth_filter_create(None, C.byref(good), C.byref(h)) == -1 and h.value == 0x5A5A
    us = C.c_float(7.0)
    calls = [("in == out", lambda: lib.odo_depth_filter_run_dev(flt.h, dst.p, dst.p)),
             ("in == out, the source", lambda: lib.odo_depth_filter_run_dev(flt.h, src, src)),
             ("out one row into in", lambda: lib.odo_depth_filter_run_dev(flt.h, dst.p, C.c_void_p(dst.p.value + 2 * raw.shape[1]))),
             ("in one pixel into out", lambda: lib.odo_depth_filter_run_dev(flt.h, C.c_void_p(dst.p.value + raw.nbytes - 2), dst.p)),
             ("in NULL", lambda: lib.odo_depth_filter_run_dev(flt.h, None, dst.p)),
             ("out NULL", lambda: lib.odo_depth_filter_run_dev(flt.h, src, None)),
             ("filter NULL", lambda: lib.odo_depth_filter_run_dev(None, src, dst.p)),
             ("odd pointer", lambda: lib.odo_depth_filter_run_dev(flt.h, src, C.c_void_p(dst.p.value + 1))),
             ("time: in == out", lambda: lib.odo_depth_filter_time_dev(flt.h, dst.p, dst.p, 3, C.byref(us))),
             ("time: NULL", lambda: lib.odo_depth_filter_time_dev(flt.h, src, None, 3, C.byref(us))),
             ("time: us NULL", lambda: lib.odo_depth_filter_time_dev(flt.h, src, dst.p, 3, None)),
             ("time: reps 0", lambda: lib.odo_depth_filter_time_dev(flt.h, src, dst.p, 0, C.byref(us))),
             ("time: reps 10001", lambda: lib.odo_depth_filter_time_dev(flt.h, src, dst.p, 10001, C.byref(us))),
             ("stats NULL", lambda: lib.odo_depth_filter_stats(flt.h, None))]
    for what, call in calls:
        assert call() == -1 and L.last_error(), what
        assert us.value == 7.0, what
        unchanged(what)
    with pytest.raises(L.OdoError):
        flt.run(src, src)
    unchanged("api")
    # frames that touch but do not overlap are fine
    both = Guarded(ctx, 2 * raw.nbytes)
    lib.odo_dev_upload(ctx.h, both.p, raw.ctypes.data_as(C.c_void_p), raw.nbytes)
    flt.run(both.p, C.c_void_p(both.p.value + raw.nbytes))
    assert np.array_equal(both.frame((2,) + raw.shape)[1], want) and flt.stats() == wstats
    both.free()
    flt.close()
    dst.free()
    ctx.free(src)


def test_two_filters_of_different_radius_on_one_context(ctx):
    """Enqueued alternately, nothing waited for in between: each has its own tables and its own statistics."""
    from odometry_amd import api
    raw = dfc.surface_frame(6, (70, 100))
    ta, tb = dfc.random_tables(1, 1), dfc.random_tables(2, 4)
    fa, fb = api.DepthFilter(ctx, raw.shape, ta), api.DepthFilter(ctx, raw.shape, tb)
    src = ctx.upload(raw)
    da, db, dc = (Guarded(ctx, raw.nbytes) for _ in range(3))
    fa.run(src, da.p)
    fb.run(src, db.p)
    fb.run(da.p, dc.p)                                      # the second filter of the first one's output, ordered by the stream
    wa, sa = dfc.filter_model(raw, *ta)
    wb, sb = dfc.filter_model(raw, *tb)
    wc, sc = dfc.filter_model(wa, *tb)
    assert np.array_equal(da.frame(raw.shape), wa) and np.array_equal(db.frame(raw.shape), wb) and np.array_equal(dc.frame(raw.shape), wc)
    assert fa.stats() == sa and fb.stats() == sc and sb != sc
    for x in (fa, fb):
        x.close()
    for x in (da, db, dc):
        x.free()
    ctx.free(src)


def test_destroy_with_a_run_in_flight(ctx):
    from odometry_amd import api
    raw = dfc.surface_frame(8, (480, 640), holes=0.05)
    tables = dfc.default_tables(4)
    flt = api.DepthFilter(ctx, raw.shape, tables)
    src = ctx.upload(raw)
    dst = Guarded(ctx, raw.nbytes)
    for _ in range(20):
        flt.run(src, dst.p)
    flt.close()                                             # waits for the runs, then frees the tables they read
    assert np.array_equal(dst.frame(raw.shape), dfc.filter_model(raw, *tables)[0])
    dst.free()
    ctx.free(src)


def test_timing_call_changes_nothing(ctx):
    from odometry_amd import api
    raw = dfc.surface_frame(2, (120, 160))
    flt = api.DepthFilter(ctx, raw.shape)
    want, wstats = dfc.filter_model(raw, *dfc.default_tables(2))
    src = ctx.upload(raw)
    dst = Guarded(ctx, raw.nbytes)
    us = flt.time(src, dst.p, reps=5)
    print(f"120 x 160, R = 2: {us:.2f} us per launch (5 launches between two events; tools/depth_filter_cost.py measures)")
    assert us > 0.0 and np.isfinite(us)
    assert np.array_equal(dst.frame(raw.shape), want) and flt.stats() == wstats
    flt.close()
    dst.free()
    ctx.free(src)


def test_filter_in_front_of_the_volume_on_the_noisy_ribbed_corridor(ctx):
    """DESIGN.md section 9.8's procedure at 120 x 160 with the Kinect noise model on every frame: frames 0 .. k - 1 fused at their
    true poses, frame k tracked from pose k - 1, once from the noisy frames and once from their filtered versions (the filter's
    output handed to the volume on the device, nothing waited for in between). There is no reference to derive a bound for the
    difference from: the test asserts that frame 6 is tracked (status 0) on both and prints both error series."""
    from odometry_amd import api
    from test_gpu_volume import _volume
    from test_volume_icp_cpu import SMALL, pose_error, ribbed_sequence
    seq = ribbed_sequence(7)
    noisy = [dfc.ribbed_frame(k, SMALL, dfc.NOISE_SEED)[1] for k in range(7)]
    flt = api.DepthFilter(ctx, SMALL)
    vols = dict(noisy=_volume(ctx, seq["p"]), filtered=_volume(ctx, seq["p"]))
    dev = [ctx.upload(f) for f in noisy]
    last = {}
    for k in range(1, 7):
        vols["noisy"].integrate(dev[k - 1], seq["poses"][k - 1])
        vols["filtered"].integrate(flt.run(dev[k - 1]), seq["poses"][k - 1])
        model = dfc.filter_model(noisy[k], *dfc.default_tables(2))[0]
        for name, frame in (("noisy", dev[k]), ("filtered", flt.run(dev[k]))):
            pose, res = vols[name].track(frame, seq["poses"][k - 1])
            et, er = pose_error(pose, seq["poses"][k]) if res["status"] == 0 else (np.nan, np.nan)
            print(f"frame {k} {name}: status {res['status']}, {et * 1e3:.2f} mm {er:.3f} deg, pairs {res['pairs']:.0f}, steps {res['iterations']}")
            last[name] = res["status"]
        assert np.array_equal(flt.download(), model), k
    assert last == dict(noisy=0, filtered=0)
    for v in vols.values():
        v.close()
    flt.close()
    for p in dev:
        ctx.free(p)
