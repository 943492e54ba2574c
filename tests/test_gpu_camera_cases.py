"""The camera model's kernels (undistort_map_kernel, remap_bilinear_kernel, odo_camera_*) on the GPU against the table of
tests/camera_cases.py, bit for bit: every row through ConfigureCamera + UndistortRectify, the geometry rows through the device-buffer
entry point with guarded margins, the camera's life cycle (reconfiguration, two cameras on one context, the staging buffers, the
accessors) and the refusals. tests/test_camera_cases_cpu.py proves on the CPU that each row reaches the case it is in the table for and
that the oracle, the plain loop and the models agree."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as CC
from camera_cases import f32

pytestmark = pytest.mark.gpu
FILL = 0xABABABAB
MARGIN = 96          # floats in front of and behind the destination of the device-buffer entry point


@pytest.fixture(scope="module")
def api():
    from odometry_amd import api
    api.default_context()
    return api


def make_cam(api, raw, dist, size=(94, 60), levels=3):
    return api.CameraPyramid(levels, raw[0], raw[1], raw[2], raw[3], raw[4], dist[0], dist[1], dist[2], dist[3], 6.0, 4.0, size[0], size[1])


def filled(shape):
    return np.full(shape, FILL, np.uint32).view(f32)


def rectify(cam, src, size, border):
    dst = filled((size[1], size[0]))
    assert cam.UndistortRectify(src, dst, borderValue=border, any_size=True) == 0
    return dst


def oracle(raw, dist, R, P, size, src, border):
    from oracle import oracle as O
    mx, my = O.camera_init_maps(np.array(raw), np.array(dist), R, P, size[1], size[0])
    return mx, my, O.camera_remap(src, mx, my, border)


@pytest.mark.parametrize("r", CC.TABLE, ids=lambda r: r["name"])
def test_every_row_bit_for_bit(api, r):
    cam = make_cam(api, r["raw"], r["dist"], r["size"])
    cam.ConfigureCamera(r["R"], r["P"], r["size"])
    mx, my = cam.maps()
    ox, oy = CC.oracle_maps(r)
    assert CC.same_floats(mx, ox) and CC.same_floats(my, oy)                 # NaNs by class
    src, want = CC.source(r), CC.oracle_output(r)
    got = rectify(cam, src, r["size"], r["border"])
    assert np.array_equal(CC.bits(got), CC.bits(want)), int((CC.bits(got) != CC.bits(want)).sum())
    if r["group"] != "real":
        model = CC.remap_model(src, ox, oy, r["border"])
        inexact = CC.border_weighted(src.shape, ox, oy) if r["group"] == "nonrep" else np.zeros(ox.shape, bool)
        assert np.array_equal(CC.bits(got)[~inexact], CC.bits(model)[~inexact])
        assert np.array_equal(CC.bits(got), CC.bits(CC.remap_model(src, ox, oy, r["border"], rounded=True)))
    if r["group"] == "nonrep":
        bad = ~(CC.fits(ox) & CC.fits(oy))
        assert bad.any() and (CC.bits(got)[bad] == CC.bits(f32(r["border"]))).all()     # the border value itself
    cam.close()


@pytest.mark.parametrize("r", [r for r in CC.TABLE if r["group"] == "geom"], ids=lambda r: r["name"])
def test_device_buffer_entry_writes_every_pixel_and_nothing_else(api, r):
    ctx = api.default_context()
    cam = make_cam(api, r["raw"], r["dist"], r["size"])
    cam.ConfigureCamera(r["R"], r["P"], r["size"])
    src, n = CC.source(r), CC.pixels(r)
    host = rectify(cam, src, r["size"], r["border"])
    assert not (CC.bits(host) == FILL).any()
    d_src, d_dst = ctx.upload(src), ctx.upload(filled(n + 2 * MARGIN))
    try:
        inner = C.c_void_p(d_dst.value + 4 * MARGIN)
        assert ctx.lib.odo_camera_undistort_rectify_dev(cam.h, d_src, src.shape[0], src.shape[1], inner, C.c_float(r["border"])) == 0
        ctx.synchronize()
        buf = ctx.download(d_dst, (n + 2 * MARGIN,), np.uint32)
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)
        cam.close()
    assert (buf[:MARGIN] == FILL).all() and (buf[MARGIN + n:] == FILL).all()
    assert np.array_equal(buf[MARGIN:MARGIN + n], CC.bits(host).ravel())
    assert np.array_equal(buf[MARGIN:MARGIN + n], CC.bits(CC.oracle_output(r)).ravel())


def test_reconfigure_larger_then_smaller_and_accessors(api):
    raw, dist = CC.EUROC_RAW, CC.EUROC_DIST
    cam = make_cam(api, raw, dist, levels=3)
    lib = cam.ctx.lib
    raw5, dist4, sensor2, res2 = (C.c_double * 5)(), (C.c_double * 4)(), (C.c_double * 2)(), (C.c_int * 2)()
    assert lib.odo_camera_raw(cam.h, raw5, dist4, sensor2, res2) == 0
    assert list(raw5) == list(raw) and list(dist4) == list(dist) and list(sensor2) == [6.0, 4.0] and list(res2) == [94, 60]
    assert lib.odo_camera_raw(cam.h, None, None, None, None) == 0 and lib.odo_camera_raw(None, raw5, None, None, None) == -1
    assert lib.odo_camera_levels(cam.h) == 3 and lib.odo_camera_levels(None) == -1
    rows, cols = C.c_int(-5), C.c_int(-5)
    assert lib.odo_camera_map_size(cam.h, C.byref(rows), C.byref(cols)) == -1 and (rows.value, cols.value) == (-5, -5)   # not configured
    src = CC.mantissa_source(60, 94, 70)
    for k, size in enumerate(((64, 48), (333, 95), (1, 1))):
        P = CC.shifted(CC.EUROC_P, 3.0 * k, -2.0 * k)
        cam.ConfigureCamera(CC.R_RECT, P, size)
        assert lib.odo_camera_map_size(cam.h, C.byref(rows), C.byref(cols)) == 0 and (cols.value, rows.value) == size
        assert lib.odo_camera_map_size(cam.h, None, None) == 0
        ox, oy, want = oracle(raw, dist, CC.R_RECT, P, size, src, 2.5)
        mx, my = cam.maps()
        assert mx.shape == (size[1], size[0]) and CC.same_floats(mx, ox) and CC.same_floats(my, oy)
        assert np.array_equal(CC.bits(rectify(cam, src, size, 2.5)), CC.bits(want)), size
        assert cam.fx_double(1) == P[0, 0] / 2.0 and cam.cx_double(0) == P[0, 2]
    cam.close()


def test_two_cameras_interleaved_and_staging_buffers_reused(api):
    a = make_cam(api, CC.EUROC_RAW, CC.EUROC_DIST)
    b = make_cam(api, CC.EUROC_RAW, CC.BARREL)
    size_a, size_b = (72, 52), (65, 5)
    a.ConfigureCamera(CC.R_RECT, CC.EUROC_P, size_a)
    b.ConfigureCamera(np.eye(3), CC.shifted(CC.EUROC_P, -4.0, -20.0), size_b)
    big, small = CC.mantissa_source(300, 400, 71), CC.mantissa_source(30, 40, 72)   # both views reach the small one
    mid = CC.mantissa_source(60, 94, 73)
    want = {}
    for tag, src in (("big", big), ("small", small), ("mid", mid)):
        want["a", tag] = oracle(CC.EUROC_RAW, CC.EUROC_DIST, CC.R_RECT, CC.EUROC_P, size_a, src, 1.5)[2]
        want["b", tag] = oracle(CC.EUROC_RAW, CC.BARREL, np.eye(3), CC.shifted(CC.EUROC_P, -4.0, -20.0), size_b, src, -3.0)[2]
    assert (want["a", "small"] != want["a", "big"]).any() and (want["a", "small"] != 1.5).sum() > 1000
    assert (want["b", "small"] != want["b", "big"]).any() and (want["b", "small"] != -3.0).sum() > 100
    # a large source first, then a small one through the same (grown) staging buffers, the two cameras taking turns
    for tag, src in (("big", big), ("small", small), ("mid", mid), ("small", small)):
        assert np.array_equal(CC.bits(rectify(a, src, size_a, 1.5)), CC.bits(want["a", tag])), ("a", tag)
        assert np.array_equal(CC.bits(rectify(b, src, size_b, -3.0)), CC.bits(want["b", tag])), ("b", tag)
    a.close()
    assert np.array_equal(CC.bits(rectify(b, mid, size_b, -3.0)), CC.bits(want["b", "mid"]))        # b outlives a
    b.close()


def test_refusals_leave_the_destination_and_the_camera_alone(api):
    from odometry_amd import _lib
    ctx = api.default_context()
    lib = ctx.lib
    r = CC.BY_NAME["half-top-left"]
    size, src, border = r["size"], CC.source(r), r["border"]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    cam = make_cam(api, r["raw"], r["dist"], size)
    dst = filled((size[1], size[0]))
    d_src, d_dst = ctx.upload(src), ctx.upload(dst)

    def refused_host(h, s, rows, cols, d):
        assert lib.odo_camera_undistort_rectify(h, s, rows, cols, d, C.c_float(border)) == -1
        assert (CC.bits(dst) == FILL).all()

    def refused_dev(h, s, rows, cols, d):
        assert lib.odo_camera_undistort_rectify_dev(h, s, rows, cols, d, C.c_float(border)) == -1
        ctx.synchronize()
        assert (ctx.download(d_dst, dst.shape, np.uint32) == FILL).all()

    try:
        # not configured yet
        refused_host(cam.h, fp(src), src.shape[0], src.shape[1], fp(dst))
        refused_dev(cam.h, d_src, src.shape[0], src.shape[1], d_dst)
        assert "ConfigureCamera has not run" in _lib.last_error()
        with pytest.raises(_lib.OdoError):
            cam.maps()
        # a singular P * R on a camera that has no maps, then on one that has
        with pytest.raises(_lib.OdoError):
            cam.ConfigureCamera(np.zeros((3, 3)), r["P"], size)
        refused_host(cam.h, fp(src), src.shape[0], src.shape[1], fp(dst))
        cam.ConfigureCamera(r["R"], r["P"], size)
        want = CC.oracle_output(r)
        assert np.array_equal(CC.bits(rectify(cam, src, size, border)), CC.bits(want))
        singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
        dp = C.POINTER(C.c_double)
        assert lib.odo_camera_configure(cam.h, singular.ctypes.data_as(dp), np.ascontiguousarray(r["P"]).ctypes.data_as(dp), size[0], size[1]) == -1
        assert "singular" in _lib.last_error()
        assert lib.odo_camera_configure(cam.h, None, np.ascontiguousarray(r["P"]).ctypes.data_as(dp), size[0], size[1]) == -1
        mx, my = cam.maps()                                                  # the maps of the last good configuration
        assert CC.same_floats(mx, CC.oracle_maps(r)[0]) and CC.same_floats(my, CC.oracle_maps(r)[1])
        # NULL buffers, a NULL camera, sizes of 0
        refused_host(cam.h, None, src.shape[0], src.shape[1], fp(dst))
        refused_host(cam.h, fp(src), src.shape[0], src.shape[1], None)
        refused_host(None, fp(src), src.shape[0], src.shape[1], fp(dst))
        refused_host(cam.h, fp(src), 0, src.shape[1], fp(dst))
        refused_host(cam.h, fp(src), src.shape[0], 0, fp(dst))
        assert "bad source size" in _lib.last_error()
        refused_dev(cam.h, None, src.shape[0], src.shape[1], d_dst)
        refused_dev(cam.h, d_src, src.shape[0], src.shape[1], None)
        refused_dev(cam.h, d_src, 0, src.shape[1], d_dst)
        refused_dev(cam.h, d_src, src.shape[0], 0, d_dst)
        # ... and the camera still works
        assert np.array_equal(CC.bits(rectify(cam, src, size, border)), CC.bits(want))
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)
        cam.close()
