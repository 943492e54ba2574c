"""Colour in the TSDF volume on the GPU (odo_volume_enable_colour, odo_volume_integrate_colour_dev, odo_volume_extract_colour /
_mesh_colour, odo_tracker_frame_colour, odo_rgbd_frontend_colour) against the numpy model of tests/test_volume_colour_cpu.py: both
grids and the counters after coloured integrations across the skip classes, the channel layouts and the launch geometries, the
colours of points and vertices on integrated and uploaded grids and at cut capacities, the read-out calls, the refusals, and a
coloured volume attached to an RgbdTracker, fed directly and through the front end. Every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest

import geometry_cases as G
from test_gpu_volume import _grid_equal, _points_equal, _row, _rows_equal, _run, _tracker, _volume, second_rig
from test_gpu_volume_mesh import _mesh_equal
from test_rgbd_cpu import N_FRAMES, drive
from test_volume_colour_cpu import (LAYOUTS, empty_colour, integrate_colour_model, mesh_colours_model, point_colours_model,
                                    random_colour, random_frame, read_ply_colour)
from test_volume_cpu import bits, empty_grid, extract_model, integrate_model, params, tiny_cases
from test_volume_mesh_cpu import grid_params, mesh_model, random_grid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seq():
    return drive()


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _colour_volume(owner, p, channels=3, bgr=False, max_weight=255):
    vol = _volume(owner, p)
    vol.enable_colour(channels, bgr, max_weight)
    return vol


def _colour_equal(vol, col, tag):
    got = vol.colour_grid()
    assert got.shape == col.shape and got.dtype == np.uint8
    assert np.array_equal(got[..., 3], col[..., 3]), f"{tag}: colour weights differ at {int((got[..., 3] != col[..., 3]).sum())} voxels"
    assert np.array_equal(got, col), f"{tag}: colours differ at {int((got != col).any(-1).sum())} voxels"


def _tinted(gray, channels=3, bgr=False):
    from odometry_amd import synth
    return synth.colour_from_gray(gray, channels, bgr, tint_seed=1)


# ---- coloured integration against the model ------------------------------------------------------------------------------------
def test_tiny_cases_reach_every_skip_class_in_the_four_layouts(ctx):
    n_col = 0
    for n, (p, frames) in enumerate(tiny_cases()):
        for channels, bgr in LAYOUTS:
            mw = (2, 255, 1, 3)[n]
            vol = _colour_volume(ctx, p, channels, bgr, mw)
            q, w = empty_grid(p)
            col = empty_colour(p)
            total = 0
            for f, (raw, pose) in enumerate(frames):
                frame = random_frame(p, channels, 100 * n + 10 * f + channels)
                vol.integrate(raw, pose, colour=frame)
                q, w, col, upd, band, nc = integrate_colour_model(q, w, col, raw, frame, pose, p, channels, bgr, mw)
                total += upd
                n_col += nc
                tag = f"tiny {n} layout {channels}/{bgr} frame {f}"
                assert vol.stats() == dict(frames=f + 1, updated=upd, in_band=band, cumulative=total), tag
                _grid_equal(vol, q, w, tag)
                _colour_equal(vol, col, tag)
            vol.close()
    assert n_col > 400


# row -> (channels, bgr). 300 x 420 frames with 3 channels put the pixels at every byte alignment; the last row has 241 x 423 frames,
# whose rows of 1 269 bytes are no multiple of 4 either.
GEOMETRY_ROWS = {"2x2x2": (4, True), "65x5x2": (3, True), "150x50x60": (3, False), "130x4x683": (4, False), "192x4x682": (3, True)}


@pytest.mark.parametrize("name", list(GEOMETRY_ROWS))
def test_launch_geometries(ctx, name):
    run = G.volume_run(name)
    p, frames = run["p"], run["frames"]
    channels, bgr = GEOMETRY_ROWS[name]
    vol = _colour_volume(ctx, p, channels, bgr, 2)
    plain = _volume(ctx, p)
    q, w = empty_grid(p)
    col = empty_colour(p)
    for f, (raw, pose) in enumerate(frames):
        frame = random_frame(p, channels, 7 * f + len(name))
        vol.integrate(raw, pose, colour=frame)
        plain.integrate(raw, pose)
        q, w, col, upd, band, _ = integrate_colour_model(q, w, col, raw, frame, pose, p, channels, bgr, 2)
        assert (upd, band) == run["counts"][f]
        assert vol.stats() == plain.stats() and vol.stats()["in_band"] == band
        if f in (0, len(frames) - 1):
            tag = f"{name} after {f + 1} integrations"
            assert np.array_equal(q, run["first" if f == 0 else "last"][0])
            _colour_equal(vol, col, tag)
            _grid_equal(vol, q, w, tag)
            _grid_equal(plain, q, w, tag + " (plain)")
    print(f"{name}: {int((col[..., 3] > 0).sum())} coloured voxels of {int((w > 0).sum())} observed")
    assert (col[..., 3] > 0).any()
    vol.close()
    plain.close()


@pytest.fixture(scope="module")
def pinned_model(seq):
    """The pinned case (true poses, tinted colour, weight 255) after 1 and 10 frames: {n: (q, w, col)} and the parameters."""
    p = params(seq)
    q, w = empty_grid(p)
    col = empty_colour(p)
    out = {}
    for k in range(10):
        q, w, col, _, _, _ = integrate_colour_model(q, w, col, seq["depth"][k], _tinted(seq["gray"][k]), seq["poses"][k], p)
        if k + 1 in (1, 10):
            out[k + 1] = (q, w, col)
    return p, out


def _check_read_out(vol, p, q, w, col, tag, mesh=True):
    """Coloured extraction (and mesh) against the model and against the uncoloured calls; neither grid, no counter changes."""
    before = vol.stats()
    want = extract_model(q, w, p)
    cap = len(want[0]) + 10
    got = vol.extract(cap, colour=True)
    _points_equal(got[:2], want, tag)
    assert got[2].dtype == np.uint8 and np.array_equal(got[2], point_colours_model(q, w, col)), f"{tag}: point colours differ"
    _points_equal(vol.extract(cap), want, tag + " (uncoloured)")
    if mesh:
        wm = mesh_model(q, w, p)
        gm = vol.mesh(colour=True)
        _mesh_equal(gm[:3], wm, tag)
        assert np.array_equal(gm[3], mesh_colours_model(q, w, col)), f"{tag}: vertex colours differ"
        _mesh_equal(vol.mesh(), wm, tag + " (uncoloured)")
    assert vol.stats() == before
    _grid_equal(vol, q, w, tag + " after the read-out")
    _colour_equal(vol, col, tag + " after the read-out")


def test_pinned_case_matches_the_model_bit_for_bit(ctx, seq, pinned_model):
    p, model = pinned_model
    vol = _colour_volume(ctx, p)
    for k in range(10):
        vol.integrate(seq["depth"][k], seq["poses"][k], colour=_tinted(seq["gray"][k]))
        if k + 1 in model:
            q, w, col = model[k + 1]
            _grid_equal(vol, q, w, f"pinned after {k + 1}")
            _colour_equal(vol, col, f"pinned after {k + 1}")
            _check_read_out(vol, p, q, w, col, f"pinned after {k + 1}")
    vol.close()


@pytest.mark.parametrize("cmax", [255, 3])
def test_second_rig_matches_the_model_bit_for_bit(ctx, cmax):
    p, frames = second_rig()
    vol = _colour_volume(ctx, p, 4, True, cmax)
    q, w = empty_grid(p)
    col = empty_colour(p)
    for f, (raw, A) in enumerate(frames):
        frame = random_frame(p, 4, 31 + f)
        vol.integrate(raw, A, colour=frame)
        q, w, col, _, _, _ = integrate_colour_model(q, w, col, raw, frame, A, p, 4, True, cmax)
    # six frames: without the cap a colour weight passes 3, with it the weight stops there
    assert col[..., 3].max() > 3 if cmax == 255 else (col[..., 3].max() == 3 and (col[..., 3] == 3).sum() > 100)
    _grid_equal(vol, q, w, "second rig")
    _colour_equal(vol, col, "second rig")
    _check_read_out(vol, p, q, w, col, f"second rig, colour weight {cmax}", mesh=cmax == 3)
    vol.close()


# ---- colours of points and vertices on uploaded grids -----------------------------------------------------------------------------
UPLOADED = {"9x8x7": ((9, 8, 7), 0.5), "65x5x2": ((65, 5, 2), 0.5), "1024x32x32": ((1024, 32, 32), 0.03), "1025x32x32": ((1025, 32, 32), 0.03)}


@pytest.mark.parametrize("name", list(UPLOADED))
def test_uploaded_random_grids(ctx, name):
    dims, negative = UPLOADED[name]
    p = grid_params(dims, vs=0.01)
    q, w = random_grid(dims, 7, holes=0.05, zeros=0.02, negative=negative)
    col = random_colour(q.shape, 17, holes=0.25)
    vol = _colour_volume(ctx, p)
    vol.upload(q, w)
    vol.upload_colour(col)
    _colour_equal(vol, col, name)
    X, N, T, vkeys, tkeys = mesh_model(q, w, p, detail=True)
    P = extract_model(q, w, p)
    pc, vc = point_colours_model(q, w, col), mesh_colours_model(q, w, col)
    nv, nt, npt = len(X), len(T), len(P[0])
    assert nv > 0 and npt > 0 and (pc[:, 3] == 0).any() and (pc[:, 3] == 255).any()
    # exact capacities, then 0, total - 1 and a cut inside a voxel with >= 2 vertices / points, then exact again
    first = np.unique(vkeys // 7, return_index=True)[1]
    many = np.nonzero(np.diff(np.append(first, nv)) >= 2)[0]
    v_cut = int(first[many[len(many) // 2]]) + 1
    p_cut = G.mid_voxel_capacity(G.edge_keys(q, w))
    assert 0 < v_cut < nv and p_cut is not None and 0 < p_cut < npt
    for cap in (npt, 0, npt - 1, p_cut, npt):
        got = vol.extract(cap, with_dropped=True, colour=True)
        tag = f"{name} extraction capacity {cap}"
        _points_equal(got[:2], (P[0][:cap], P[1][:cap]), tag)
        assert np.array_equal(got[2], pc[:cap]) and got[3] == npt - cap, tag
        _points_equal(vol.extract(cap), (P[0][:cap], P[1][:cap]), tag + " (uncoloured)")
    for cap in (nv, 0, nv - 1, v_cut, nv):
        got = vol.mesh(cap, nt, with_counts=True, colour=True)
        tag = f"{name} vertex capacity {cap}"
        assert got[4] == (cap, nv - cap, nt, 0), (tag, got[4])
        _mesh_equal(got[:3], (X[:cap], N[:cap], T), tag)
        assert np.array_equal(got[3], vc[:cap]), f"{tag}: vertex colours differ"
        _mesh_equal(vol.mesh(cap, nt), (X[:cap], N[:cap], T), tag + " (uncoloured)")
    got = vol.mesh(nv, 0, with_counts=True, colour=True)                   # no triangle asked for: the vertices and their colours all the same
    assert got[4] == (nv, 0, 0, nt) and np.array_equal(got[3], vc) and np.array_equal(bits(got[0]), bits(X))
    _grid_equal(vol, q, w, name + " after the read-outs")
    _colour_equal(vol, col, name + " after the read-outs")
    vol.close()


# ---- read-out calls ----------------------------------------------------------------------------------------------------------------
def test_download_upload_clear_and_the_plain_integration(ctx):
    dims = (37, 21, 13)
    p = grid_params(dims)
    q, w = random_grid(dims, 3, holes=0.1, zeros=0.05)
    col = random_colour(q.shape, 5)
    vol = _colour_volume(ctx, p, 4, False, 200)
    _colour_equal(vol, empty_colour(p), "enabled")
    vol.upload_colour(col)
    _colour_equal(vol, col, "uploaded")
    _grid_equal(vol, *empty_grid(p), "upload_colour leaves q / w alone")
    vol.upload(q, w)
    _colour_equal(vol, col, "upload(q, w) leaves the colour alone")
    raw = np.full(p["size"], 900, np.uint16)
    before = vol.stats()
    vol.integrate(raw, np.eye(4))                                          # the plain integration on a colour volume: legal, colour untouched
    q1, w1, upd, band = integrate_model(q, w, raw, np.eye(4), p)
    _grid_equal(vol, q1, w1, "plain integration")
    _colour_equal(vol, col, "plain integration leaves the colour alone")
    assert vol.stats()["frames"] == before["frames"] + 1 and band > 0
    frame = random_frame(p, 4, 9)
    vol.integrate(raw, np.eye(4), colour=frame)                            # a coloured one behind the uploads works on the uploaded grids
    q2, w2, col2, upd, band, _ = integrate_colour_model(q1, w1, col, raw, frame, np.eye(4), p, 4, False, 200)
    _grid_equal(vol, q2, w2, "upload + coloured integration")
    _colour_equal(vol, col2, "upload + coloured integration")
    _check_read_out(vol, p, q2, w2, col2, "upload + coloured integration")
    vol.clear()
    _colour_equal(vol, empty_colour(p), "cleared")
    _grid_equal(vol, *empty_grid(p), "cleared")
    assert vol.stats() == dict(frames=0, updated=0, in_band=0, cumulative=0)
    assert [len(a) for a in vol.extract(100, colour=True)] == [0, 0, 0]
    assert vol.mesh(with_counts=True, colour=True)[4] == (0, 0, 0, 0)
    vol.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(ctx, seq):
    from odometry_amd import _lib as L, api
    p = params(seq, dims=(32, 16, 24), vs=0.08, origin=(-1.28, 0.9, 3.6))
    lib = L.load()
    plain = _volume(ctx, p)
    plain.integrate(seq["depth"][0], seq["poses"][0])
    d = ctx.upload(seq["depth"][1])
    c = ctx.upload(_tinted(seq["gray"][1]))
    before = plain.stats(), plain.grid()
    pose = np.eye(4, dtype=np.float32).reshape(-1)
    fp = pose.ctypes.data_as(C.POINTER(C.c_float))
    buf = np.zeros((8, 4), np.float32)
    rgba = np.zeros((8, 4), np.uint8)
    n = C.c_long(0)
    counts = (C.c_long * 4)()
    # colour calls on a volume without colour
    assert lib.odo_volume_integrate_colour_dev(plain.h, d, c, fp) == -1 and "no colour grid" in L.last_error()
    assert lib.odo_volume_download_colour(plain.h, rgba.ctypes.data_as(L._u8p)) == -1 and "no colour grid" in L.last_error()
    assert lib.odo_volume_upload_colour(plain.h, rgba.ctypes.data_as(L._u8p)) == -1 and "no colour grid" in L.last_error()
    assert lib.odo_volume_extract_colour(plain.h, 8, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.ctypes.data_as(C.POINTER(C.c_float)),
                                         rgba.ctypes.data_as(L._u8p), C.byref(n), None) == -1 and "no colour grid" in L.last_error()
    assert lib.odo_volume_mesh_colour(plain.h, 0, 0, None, None, None, None, counts) == -1 and "no colour grid" in L.last_error()
    with pytest.raises(L.OdoError, match="no colour grid"):
        plain.integrate(d, np.eye(4), colour=c)
    after = plain.stats(), plain.grid()
    assert before[0] == after[0] and np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
    # a second enable_colour; a non-finite pose; a misaligned 4-channel frame
    vol = _colour_volume(ctx, p, 4, False, 255)
    with pytest.raises(L.OdoError, match="already"):
        vol.enable_colour(3, False, 255)
    assert vol.colour_params.channels == 4
    c4 = ctx.upload(_tinted(seq["gray"][1], 4))
    vol.integrate(d, seq["poses"][1], colour=c4)
    before = vol.stats(), vol.grid(), vol.colour_grid()
    assert before[0]["in_band"] > 0
    for bad in (np.nan, np.inf, -np.inf):
        A = np.array(seq["poses"][1], np.float32)
        A[2, 3] = bad
        with pytest.raises(L.OdoError, match="non-finite"):
            vol.integrate(d, A, colour=c4)
    assert lib.odo_volume_integrate_colour_dev(vol.h, d, C.c_void_p(c4.value + 1), fp) == -1 and "misaligned" in L.last_error()
    assert lib.odo_volume_integrate_colour_dev(vol.h, d, None, fp) == -1
    after = vol.stats(), vol.grid(), vol.colour_grid()
    assert before[0] == after[0] and all(np.array_equal(a, b) for a, b in zip(before[1] + (before[2],), after[1] + (after[2],)))
    vol.close()
    plain.close()
    for h in (d, c, c4):
        ctx.free(h)
    # with trackers: enable_colour and upload_colour while attached, frame_colour without a colour volume, on a stereo tracker
    trk = _tracker(seq)
    full = params(seq)
    v1 = _volume(trk, full)
    cdev = trk.upload_frame(np.zeros((480, 640), np.float32))              # any device buffer: every call below is refused
    assert lib.odo_tracker_frame_colour(trk.h, cdev) == -1 and "no volume with a colour grid" in L.last_error()   # no volume at all
    trk.attach_volume(v1)
    assert lib.odo_tracker_frame_colour(trk.h, cdev) == -1 and "no volume with a colour grid" in L.last_error()   # a plain volume
    with pytest.raises(L.OdoError, match="attached"):
        v1.enable_colour()
    assert not v1.has_colour
    trk.attach_volume(None)
    v1.enable_colour()
    trk.attach_volume(v1)
    with pytest.raises(L.OdoError, match="attached"):
        v1.upload_colour(np.zeros((200, 128, 240, 4), np.uint8))
    assert lib.odo_tracker_frame_colour(trk.h, None) == -1
    trk.frame_colour(cdev)                                                 # accepted now ...
    trk.attach_volume(None)                                                # ... and forgotten with the volume
    assert v1.stats() == dict(frames=0, updated=0, in_band=0, cumulative=0) and not v1.colour_grid().any()
    stereo = api.Tracker(0)
    assert lib.odo_tracker_frame_colour(stereo.h, cdev) == -1 and "RGB-D" in L.last_error()
    stereo.close()
    v1.close()
    trk.close()


# ---- attached to a tracker -----------------------------------------------------------------------------------------------------
PLAIN_FRAMES = (5, 17, 18)   # frames of the drive that are given no colour


def _run_coloured(trk, dev, cdev, hints, skip=PLAIN_FRAMES):
    """_run of tests/test_gpu_volume.py with every frame's colour named in front of its init / track, except the frames in `skip`."""
    if 0 not in skip:
        trk.frame_colour(cdev[0])
    trk.init(*dev[0])
    rows = [_row(trk, dict(abs_pose=np.eye(4, dtype=np.float32), solve_status=0))]
    for k in range(1, len(dev)):
        if k + 1 < len(dev) and hints:
            trk.hint_next(*dev[k + 1])
        if k not in skip:
            trk.frame_colour(cdev[k])
        rows.append(_row(trk, trk.track(*dev[k])))
    return rows


def _standalone_coloured(trk, p, dev, cdev, rows, skip=PLAIN_FRAMES):
    ref = _colour_volume(trk, p)
    for k, ((_, d), r) in enumerate(zip(dev, rows)):
        ref.integrate(d, r["abs_pose"], colour=None if k in skip else cdev[k])
    return ref


def _coloured_volumes_equal(a, b, tag):
    qa, wa = a.grid()
    _grid_equal(b, qa, wa, tag)
    _colour_equal(b, a.colour_grid(), tag)
    assert a.stats() == b.stats(), (tag, a.stats(), b.stats())


@pytest.fixture(scope="module")
def untouched(seq):
    """The drive's rows from a tracker without a volume, with and without announcements."""
    out = {}
    for hints in (False, True):
        t = _tracker(seq)
        out[hints] = _run(t, [(t.upload_frame(g), t.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])], hints)
        t.close()
    return out


@pytest.mark.parametrize("hints", [False, True])
def test_attached_coloured_volume_changes_nothing_and_equals_a_standalone_volume(seq, untouched, hints):
    p = params(seq)
    # a plain volume attached, no frame_colour
    a = _tracker(seq)
    va = _volume(a, p)
    a.attach_volume(va)
    rows_plain = _run(a, [(a.upload_frame(g), a.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])], hints)
    # a coloured volume attached, a colour frame named for all frames but three
    b = _tracker(seq)
    vb = _colour_volume(b, p)
    b.attach_volume(vb)
    dev = [(b.upload_frame(g), b.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])]
    cdev = [b.upload_colour(_tinted(g)) for g in seq["gray"]]
    got = _run_coloured(b, dev, cdev, hints)
    _rows_equal(got, rows_plain, f"hints {hints}: with against without frame_colour")
    _rows_equal(got, untouched[hints], f"hints {hints}: against a tracker without a volume")
    assert all(g["solve_status"] == 0 for g in got) and vb.stats()["frames"] == N_FRAMES
    _grid_equal(vb, *va.grid(), "the geometry of the coloured volume is the plain volume's")
    assert va.stats() == vb.stats()
    ref = _standalone_coloured(b, p, dev, cdev, got)
    _coloured_volumes_equal(ref, vb, f"hints {hints}: attached against standalone")
    col = vb.colour_grid()
    assert (col[..., 3] > 0).sum() > 100_000
    # the frames without a colour were integrated plain: with them coloured the grid differs
    allc = _standalone_coloured(b, p, dev, cdev, got, skip=())
    assert not np.array_equal(allc.colour_grid()[..., 3], col[..., 3])
    for v in (allc, ref, vb, va):
        v.close()
    b.close()
    a.close()


def test_a_frame_whose_depth_job_failed_is_still_coloured_and_a_colour_is_consumed_once(seq):
    from odometry_amd import _lib as L
    p = params(seq)
    trk = _tracker(seq)
    vol = _colour_volume(trk, p)
    trk.attach_volume(vol)
    g = [trk.upload_frame(x) for x in seq["gray"][:3]]
    d = [trk.upload_depth(x) for x in seq["depth"][:3]]
    c = [trk.upload_colour(_tinted(x)) for x in seq["gray"][:3]]
    sparse = np.zeros_like(seq["depth"][1])
    sparse[::40, ::40] = seq["depth"][1][::40, ::40]            # a few hundred readings: the depth job fails
    d_sparse = trk.upload_depth(sparse)
    trk.frame_colour(c[0])
    trk.init(g[0], d[0])
    T = np.zeros(16, np.float32)
    A = np.full(16, np.nan, np.float32)
    fp = C.POINTER(C.c_float)
    trk.frame_colour(c[1])
    rc = trk.lib.odo_tracker_track_rgbd(trk.h, g[1], d_sparse, T.ctypes.data_as(fp), A.ctypes.data_as(fp), None, None, None)
    assert rc == -1 and "depth failed" in L.last_error() and np.isfinite(A).all()
    assert vol.stats()["frames"] == 2
    ref = _colour_volume(trk, p)
    ref.integrate(d[0], np.eye(4), colour=c[0])
    ref.integrate(d_sparse, A.reshape(4, 4).T, colour=c[1])
    _coloured_volumes_equal(ref, vol, "after a failed depth job")
    assert vol.stats()["in_band"] > 0
    # the colour named for frame 1 was consumed by that call: frame 2, given none, is integrated plain
    trk.init(g[0], d[0])                                        # (a fresh sequence; no colour named: plain)
    r = trk.track(g[2], d[2])
    ref.integrate(d[0], np.eye(4))
    ref.integrate(d[2], r["abs_pose"])
    _coloured_volumes_equal(ref, vol, "frames without a colour")
    ref.close()
    vol.close()
    trk.close()


# ---- through the front end ---------------------------------------------------------------------------------------------------------
_raw_cache = []


def _tinted_raw_sequence():
    """The drive as the identity rig's sensor delivers it, the colour frames tinted; rendered once."""
    from test_rgbd_frontend_cpu import RIGS, raw_sequence
    if not _raw_cache:
        _raw_cache.append(raw_sequence(RIGS()["identity"], N_FRAMES, tint_seed=1))
    return _raw_cache[0]


@pytest.mark.parametrize("path", ["host", "device"])
def test_front_end_hands_the_colour_frame_on(seq, path):
    """The tinted colour frames go through RgbdFrontend.submit; RgbdFrontend.colour() of a slot is handed to frame_colour. The result
    equals that of a tracker given the front end's own outputs (the BT.601 grey of the tinted frames, the identity rig's depth) and
    the same colour frames as uploads of its own: rows and both grids."""
    from odometry_amd import api
    from test_rgbd_frontend_cpu import RIGS, grey_model
    n = N_FRAMES
    r = RIGS()["identity"]
    raw = _tinted_raw_sequence()
    p = params(seq)
    a = _tracker(seq)
    va = _colour_volume(a, p)
    a.attach_volume(va)
    dev = [(a.upload_frame(grey_model(c)), a.upload_depth(d)) for c, d in zip(raw["colour"], raw["raw_depth"])]
    cdev = [a.upload_colour(c) for c in raw["colour"]]
    want = _run_coloured(a, dev, cdev, True, skip=())
    assert all(g["solve_status"] == 0 for g in want)
    b = _tracker(seq)
    vb = _colour_volume(b, p)
    b.attach_volume(vb)
    fe = api.RgbdFrontend(b, r["depth_size"], r["depth_K"], 1000.0, r["size"], r["K"], 1000.0, r["E"], 3, False, 4)
    nothing = C.c_void_p()
    assert fe.lib.odo_rgbd_frontend_colour(fe.h, C.c_void_p(64), C.byref(nothing)) == -1      # no slot has that grey buffer
    if path == "host":
        frames = list(zip(raw["colour"], raw["raw_depth"]))
    else:
        frames = [(fe.upload(c), fe.upload(d)) for c, d in zip(raw["colour"], raw["raw_depth"])]
    slot = [fe.submit(*frames[k]) for k in range(3)]
    fe.wait(slot[0][0])
    if path == "device":
        assert fe.colour(slot[0][0]).value == frames[0][0].value           # the caller's own pointer
    b.frame_colour(fe.colour(slot[0][0]))
    b.init(*slot[0])
    got = [_row(b, dict(abs_pose=np.eye(4, dtype=np.float32), solve_status=0))]
    for k in range(1, n):
        if k + 2 < n:
            slot.append(fe.submit(*frames[k + 2]))
        fe.wait(slot[k][0])
        if k + 1 < n:
            fe.wait(slot[k + 1][0])
            b.hint_next(*slot[k + 1])
        b.frame_colour(fe.colour(slot[k][0]))
        got.append(_row(b, b.track(*slot[k])))
    _rows_equal(got, want, f"front end, {path} path")
    _coloured_volumes_equal(va, vb, f"front end, {path} path")
    assert (vb.colour_grid()[..., 3] > 0).sum() > 50_000
    fe.close()
    vb.close()
    b.close()
    va.close()
    a.close()


# ---- PLY -----------------------------------------------------------------------------------------------------------------------------
def test_save_ply_and_save_mesh_ply_carry_the_models_colours(ctx, tmp_path):
    from test_volume_mesh_cpu import read_ply_mesh
    dims = (24, 20, 16)
    p = grid_params(dims)
    q, w = random_grid(dims, 12, holes=0.05)
    col = random_colour(q.shape, 13)
    vol = _colour_volume(ctx, p)
    vol.upload(q, w)
    vol.upload_colour(col)
    path = str(tmp_path / "mesh.ply")
    vol.save_mesh_ply(path)
    vert, rgb, face = read_ply_colour(path, True)
    X, N, T = mesh_model(q, w, p)
    assert len(face) == len(T) > 0 and np.array_equal(bits(vert[:, :3]), bits(X[:, :3])) and np.array_equal(face, T)
    assert np.array_equal(rgb, mesh_colours_model(q, w, col)[:, :3])
    vol.save_ply(path)
    vert, rgb, _ = read_ply_colour(path, False)
    assert np.array_equal(bits(vert[:, :3]), bits(extract_model(q, w, p)[0][:, :3])) and np.array_equal(rgb, point_colours_model(q, w, col)[:, :3])
    vol.close()
    plain = _volume(ctx, p)                                                # a volume without colour writes what it wrote before
    plain.upload(q, w)
    plain.save_mesh_ply(path)
    vert, face = read_ply_mesh(path)
    assert np.array_equal(bits(vert[:, :3]), bits(X[:, :3])) and np.array_equal(face, T)
    plain.close()
