"""The moving TSDF volume on the GPU (odo_volume_shift, _follow, the spill store; api.TsdfVolume.shift / follow / spilled) against the
model of tests/test_volume_shift_cpu.py, bit for bit: every row of the CPU tests, the launch geometries of the shift and the spill,
the store's clamp at capacity, the existing operations in a moved window, the drive that leaves its box, and an attached tracker
that follows."""
import ctypes as C

import numpy as np
import pytest

import shape_cases as S
from test_volume_cpu import bits, extract_model, params, tiny_cases
from test_volume_colour_cpu import point_colours_model, random_colour
from test_volume_shift_cpu import (DRIVE, MAX_OFF, drive_case, edge_list, follow_model, grids, offset_model, origin_model, random_grid,
                                   shift_model, shifts_for, spill_mask, spill_model, window)

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _volume(owner, p, colour=False, spill=0, origin=None):
    from odometry_amd import api
    v = api.TsdfVolume(owner, p["dims"], p["vs"], p["origin"] if origin is None else origin, p["mu"], p["max_depth"], p["max_weight"],
                       p["size"], p["K"], p["depth_scale"])
    if colour:
        v.enable_colour()
    if spill:
        v.enable_spill(spill)
    return v


def _guard_intact(vol):
    """The library fills the store's buffers with 0xAB when it allocates them, 64 guard points behind the capacity included; the test
    hook counts the bytes behind the store's last point that no longer hold it. Zero: the spills so far wrote their own points and
    nothing else, neither between the last point and the capacity nor beyond it. Only for a store that was never emptied."""
    n = C.c_long(-1)
    assert vol.lib.odo_debug_volume_spill_guard(vol.h, C.byref(n)) == 0
    return n.value == 0


def _prefill(vol, q, colour):
    """Leaves 0xAB in every byte of the buffers the next shift writes: a grid of that pattern is shifted away, so it is the second
    pair of buffers that holds it."""
    vol.upload(np.full(q.shape, 0xABAB - 65536, np.int16), np.full(q.shape, 0xABAB, np.uint16))
    if colour:
        vol.upload_colour(np.full(q.shape + (4,), 0xAB, np.uint8))
    vol.shift((1, 0, 0))


def _window_equals(vol, p, off, tag):
    got_off, got_origin = vol.window()
    assert got_off == tuple(off), (tag, got_off, off)
    assert np.array_equal(bits(got_origin), bits(origin_model(p["origin"], off, p["vs"]))), (tag, got_origin)


def _store_equals(vol, P, N, rgba, tag, dropped=0):
    got = vol.spilled(colour=rgba is not None, with_dropped=True)
    assert len(got[0]) == len(P), f"{tag}: {len(got[0])} points in the store, the model has {len(P)}"
    assert np.array_equal(bits(got[0]), bits(P)), f"{tag}: positions differ"
    assert np.array_equal(bits(got[1]), bits(N)), f"{tag}: normals / weights differ"
    if rgba is not None:
        assert np.array_equal(got[2], rgba), f"{tag}: colours differ"
    assert got[-1] == dropped, (tag, got[-1], dropped)


def _cat(parts, width=4, dtype=np.float32):
    return np.concatenate(parts) if parts else np.zeros((0, width), dtype)


# ---- every CPU row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(grids()))
def test_every_cpu_row_matches_the_model_bit_for_bit(ctx, name):
    """Grid, colour grid, window and spill store after each shift of the CPU rows. Both destination grids and the store's three
    buffers hold 0xAB beforehand: the grids through a shifted-away grid of that pattern, the store since its allocation (a fresh
    store per shift), and behind the spilled points it still does afterwards."""
    p, q, w, col = grids()[name]
    for d in shifts_for(p["dims"]):
        vol = _volume(ctx, p, colour=True)
        _prefill(vol, q, True)
        off = (1, 0, 0)
        vol.enable_spill(1 << 14)
        vol.upload(q, w)
        vol.upload_colour(col)
        P, N, rgba = spill_model(q, w, col, window(p, off), d)
        vol.shift(d)
        off = offset_model(off, d)
        q2, w2, c2 = shift_model(q, w, col, d)
        gq, gw = vol.grid()
        assert np.array_equal(gw, w2) and np.array_equal(gq, q2), (name, d)
        assert np.array_equal(vol.colour_grid(), c2), (name, d)
        _window_equals(vol, p, off, (name, d))
        _store_equals(vol, P, N, rgba, (name, d))
        assert _guard_intact(vol), (name, d)
        assert vol.stats()["frames"] == 0
        vol.close()


# ---- launch geometries -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1024, 32, 33), (130, 7, 9)])
def test_launch_geometries_match_the_model(ctx, dims):
    """1024 x 32 x 33: 1 056 extraction blocks, two chunks of the scan, rows of whole 16-byte quads. 130 x 7 x 9: a partial last block
    and nx % 64 != 0, nx % 4 != 0 (the dword build of the shift). A quarter of the voxels observed, which keeps the model quick."""
    p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=dims, vs=0.05, origin=(-1.3, 0.1, 0.7))
    q, w = random_grid(dims, 41)
    rng = np.random.default_rng(42)
    w[rng.uniform(size=w.shape) < 0.7] = 0
    q[w == 0] = 0
    col = random_colour(q.shape, 43)
    Cb = point_colours_model(q, w, col)
    Pb, Nb = extract_model(q, w, window(p, (1, 0, 0)))
    for d in ((1, 0, 0), (-1, -1, -1)):
        vol = _volume(ctx, p, colour=True)
        _prefill(vol, q, True)
        off = (1, 0, 0)
        vol.enable_spill(1 << 17)      # (0xAB throughout, as the grids' second buffers are)
        vol.upload(q, w)
        vol.upload_colour(col)
        m = spill_mask(q, w, d)[0]
        assert 0 < m.sum() < len(m)
        vol.shift(d)
        off = offset_model(off, d)
        q2, w2, c2 = shift_model(q, w, col, d)
        gq, gw = vol.grid()
        assert np.array_equal(gw, w2) and np.array_equal(gq, q2), d
        assert np.array_equal(vol.colour_grid(), c2), d
        _window_equals(vol, p, off, d)
        _store_equals(vol, Pb[m], Nb[m], Cb[m], d)
        assert _guard_intact(vol), d
        vol.close()


# ---- the spill store -------------------------------------------------------------------------------------------------------------
def test_two_shifts_back_to_back_and_the_clamp_at_capacity(ctx):
    """Two shifts enqueued with nothing between them: the store is the models' concatenation. Then the same pair into stores of
    exactly the total, of one point less, and of a capacity that cuts between two edges of one voxel; a full store counts every
    later point as dropped, and nothing is ever written beyond the capacity (the guards behind the store's buffers)."""
    p, q, w, col = grids()["tiny 3"]
    d1, d2 = (2, -2, 2), (0, -2, 2)      # 12 and 27 points with this grid, 7 more with the third shift below
    P1, N1, C1 = spill_model(q, w, col, p, d1)
    q2, w2, c2 = shift_model(q, w, col, d1)
    P2, N2, C2 = spill_model(q2, w2, c2, window(p, d1), d2)
    P, N, Cc = np.concatenate([P1, P2]), np.concatenate([N1, N2]), np.concatenate([C1, C2])
    total = len(P)
    assert len(P1) > 4 and len(P2) > 4
    # a cut inside a voxel: two consecutive spilled edges of the first shift that share their voxel a
    e = edge_list(q, w)[spill_mask(q, w, d1)[0]]
    same = np.nonzero((e[1:, :3] == e[:-1, :3]).all(1))[0]
    assert len(same) > 0
    cut = int(same[0]) + 1
    for cap in (total + 5, total, total - 1, cut, len(P1), 1):
        vol = _volume(ctx, p, colour=True, spill=cap)
        vol.upload(q, w)
        vol.upload_colour(col)
        vol.shift(d1)
        vol.shift(d2)
        n = min(cap, total)
        _store_equals(vol, P[:n], N[:n], Cc[:n], f"capacity {cap}", dropped=total - n)
        assert _guard_intact(vol), cap
        if cap <= total:   # full: every later point is dropped
            q3, w3, c3 = shift_model(q2, w2, c2, d2)
            d3 = (-1, -1, 0)
            more = len(spill_model(q3, w3, c3, window(p, offset_model(d1, d2)), d3)[0])
            assert more > 0
            vol.shift(d3)
            _store_equals(vol, P[:n], N[:n], Cc[:n], f"capacity {cap}, full", dropped=total - n + more)
            assert _guard_intact(vol), cap
            # emptied, the store takes points again from its start
            vol.spilled(clear=True)
            _store_equals(vol, P[:0], N[:0], Cc[:0], f"capacity {cap}, cleared")
        vol.close()


def test_a_store_without_colour_and_a_volume_without_a_store(ctx):
    p, q, w, col = grids()["tiny 3"]
    d = (0, -1, 1)
    P, N, _ = spill_model(q, w, None, p, d)
    vol = _volume(ctx, p, spill=1 << 12)
    vol.upload(q, w)
    vol.shift(d)
    _store_equals(vol, P, N, None, "no colour")
    vol.close()
    vol = _volume(ctx, p)
    vol.upload(q, w)
    vol.shift(d)
    q2, w2, _ = shift_model(q, w, None, d)
    gq, gw = vol.grid()
    assert np.array_equal(gw, w2) and np.array_equal(gq, q2)
    vol.close()


# ---- the existing operations in a moved window -----------------------------------------------------------------------------------
def test_existing_operations_see_the_moved_window(ctx):
    """After a shift, extract, mesh, raycast and icp_eval equal the same calls on a FRESH volume created at window()'s origin and
    uploaded the shifted grid: nothing has kept the old origin or the old buffers."""
    case_p, frames = tiny_cases()[3]
    p, q, w, col = grids()["tiny 3"]
    d = (1, -1, 2)
    vol = _volume(ctx, p, colour=True)
    vol.upload(q, w)
    vol.upload_colour(col)
    vol.shift(d)
    off, origin = vol.window()
    assert off == d
    fresh = _volume(ctx, p, colour=True, origin=tuple(float(x) for x in origin))
    q2, w2, c2 = shift_model(q, w, col, d)
    fresh.upload(q2, w2)
    fresh.upload_colour(c2)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.05, -0.05, 0.1)
    for tag, call in (("extract", lambda v: v.extract(1 << 12, colour=True)), ("mesh", lambda v: v.mesh(colour=True)),
                      ("raycast", lambda v: v.raycast(pose, raw=True, colour=True))):
        a, b = call(vol), call(fresh)
        assert len(a) == len(b) and len(a[0]) > 0
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), tag
    depth, nrmw = vol.raycast(pose)[:2]
    assert (depth > 0).sum() > 20
    raw = frames[0][0]
    acc = [v.icp_eval(raw, depth, nrmw, pose, np.eye(4, dtype=np.float32)) for v in (vol, fresh)]
    assert acc[0].tobytes() == acc[1].tobytes() and acc[0].any()
    # and an integration lands where it lands in the fresh volume
    for v in (vol, fresh):
        v.integrate(raw, frames[0][1])
    assert all(np.array_equal(x, y) for x, y in zip(vol.grid(), fresh.grid()))
    assert np.array_equal(vol.colour_grid(), fresh.colour_grid())
    fresh.close()
    vol.close()


# ---- the drive ---------------------------------------------------------------------------------------------------------------------
def test_the_drive_that_leaves_its_box_matches_the_model(ctx):
    c = drive_case()
    p = c["p"]
    vol = _volume(ctx, p, spill=1 << 16)
    vol.set_follow(DRIVE["focus"], DRIVE["threshold"])
    shifts = []
    for raw, T in zip(c["depth"], c["poses"]):
        shifts.append(vol.follow(T))
        vol.integrate(raw, T)
    assert shifts == c["shifts"]
    _window_equals(vol, p, c["off"], "drive")
    gq, gw = vol.grid()
    assert np.array_equal(gw, c["w"]) and np.array_equal(gq, c["q"])
    _store_equals(vol, _cat([P for P, _ in c["spills"]]), _cat([N for _, N in c["spills"]]), None, "drive")
    assert vol.stats()["frames"] == len(c["depth"])
    vol.close()


# ---- attached to a tracker ---------------------------------------------------------------------------------------------------------
def _run(trk, dev, size):
    trk.init(*dev[0])
    rows = [dict(abs_pose=np.eye(4, dtype=np.float32), solve_status=0)]
    for k in range(1, len(dev)):
        rows.append(trk.track(*dev[k]))
    for r in rows[-1:]:
        r["val"], _, r["dep"] = trk.outputs(*size)
    return rows


def _rows_equal(a, b, tag):
    assert len(a) == len(b)
    for k, (g, c) in enumerate(zip(a, b)):
        for key in c:
            if isinstance(c[key], np.ndarray):
                assert g[key].tobytes() == c[key].tobytes(), f"{tag} frame {k}: {key} differs"
            else:
                assert g[key] == c[key], f"{tag} frame {k}: {key} differs"


def test_attached_tracker_follows_and_its_outputs_do_not_change():
    """The 120 x 160 RGB-D row of tests/shape_cases.py, 14 frames, in three configurations: no volume, a volume that stays, a volume
    that follows. Poses, keyframe flags, motion scores and the last frame's mask and inverse depth are the same bits in all three,
    and the following volume ends with the grid, window and store of a standalone volume fed the returned poses through follow and
    integrate."""
    from odometry_amd import api
    c = dict(S.find("rgbd", 120, 160, 3), frames=14)
    seq = S.render(c)
    size = (c["rows"], c["cols"])
    p = params(seq, size=size, dims=(112, 64, 56), vs=0.1, origin=(-5.6, -3.23, 3.0), mu=0.3, max_depth=8.0)
    focus, threshold = 5.8, 3

    def run(mode):
        trk = api.RgbdTracker(0, **S.tracker_args(c))
        vol = None
        if mode != "none":
            vol = _volume(trk, p, spill=1 << 15)
            if mode == "follow":
                vol.set_follow(focus, threshold)
            trk.attach_volume(vol)
        dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])]
        return trk, vol, dev, _run(trk, dev, size)

    trk0, _, _, want = run("none")
    trk0.close()
    assert all(r["solve_status"] == 0 for r in want)
    trk1, vol1, _, got1 = run("stay")
    _rows_equal(got1, want, "a volume that stays")
    assert vol1.window()[0] == (0, 0, 0) and vol1.stats()["frames"] == c["frames"]
    vol1.close()
    trk1.close()
    trk, vol, dev, got = run("follow")
    _rows_equal(got, want, "a volume that follows")
    ref = _volume(trk, p, spill=1 << 15)
    ref.set_follow(focus, threshold)
    off, n_shifts = (0, 0, 0), 0
    for (_, d), r in zip(dev, got):
        want_d = follow_model(r["abs_pose"], p, off, focus, threshold)
        assert ref.follow(r["abs_pose"]) == want_d
        off = offset_model(off, want_d)
        n_shifts += want_d != (0, 0, 0)
        ref.integrate(d, r["abs_pose"])
    print("the attached volume shifted", n_shifts, "times, to", off)
    assert n_shifts >= 3
    assert vol.window()[0] == off and vol.window()[1].tobytes() == ref.window()[1].tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(vol.grid(), ref.grid()))
    a, b = vol.spilled(with_dropped=True), ref.spilled(with_dropped=True)     # (legal while attached)
    assert len(a[0]) > 0 and a[2] == b[2] == 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert vol.stats() == ref.stats()
    ref.close()
    vol.close()
    trk.close()


def test_detach_drains_the_follow_step_of_the_last_frame():
    """odo_tracker_attach_volume(t, NULL) directly behind the last tracked frame, whose follow step (spill and shift) and integration
    are still enqueued: the detach waits for them. Without a wait of the test's own the volume then holds the grid, window and store
    of a standalone volume fed the returned poses through follow and integrate, and it is an ordinary volume again: upload, a shift
    and destroy work, and a volume without a store, detached the same way, accepts enable_spill."""
    from odometry_amd import _lib as L, api
    c = dict(S.find("rgbd", 120, 160, 3), frames=14)
    seq = S.render(c)
    p = params(seq, size=(c["rows"], c["cols"]), dims=(112, 64, 56), vs=0.1, origin=(-5.6, -3.23, 3.0), mu=0.3, max_depth=8.0)
    focus = 5.8
    trk = api.RgbdTracker(0, **S.tracker_args(c))
    dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])]
    vol = _volume(trk, p, spill=1 << 15)
    vol.set_follow(focus, 1)               # threshold 1: the window moves whenever the focus point is a voxel off centre
    trk.attach_volume(vol)
    trk.init(*dev[0])
    poses = [np.eye(4, dtype=np.float32)] + [trk.track(*dev[k])["abs_pose"] for k in range(1, 10)]
    trk.attach_volume(None)                # the last frame's spill, shift and integration are pending here
    off = (0, 0, 0)
    for A in poses:
        last = follow_model(A, p, off, focus, 1)
        off = offset_model(off, last)
    assert last != (0, 0, 0), "the last frame must shift, or nothing of the follow step is pending at the detach"
    assert vol.window()[0] == off
    got = (vol.grid(), vol.spilled(with_dropped=True), vol.stats())
    ref = _volume(trk, p, spill=1 << 15)
    ref.set_follow(focus, 1)
    for (_, d), A in zip(dev, poses):
        ref.follow(A)
        ref.integrate(d, A)
    assert ref.window()[0] == off and vol.window()[1].tobytes() == ref.window()[1].tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(got[0], ref.grid()))
    want = ref.spilled(with_dropped=True)
    assert len(want[0]) > 0 and got[1][2] == want[2] == 0
    assert got[1][0].tobytes() == want[0].tobytes() and got[1][1].tobytes() == want[1].tobytes()
    assert got[2] == ref.stats()
    ref.close()
    # an ordinary volume again
    q, w = random_grid(p["dims"], 5)
    vol.upload(q, w)
    vol.shift((1, 0, 0))
    q2, w2, _ = shift_model(q, w, None, (1, 0, 0))
    assert all(np.array_equal(x, y) for x, y in zip(vol.grid(), (q2, w2)))
    with pytest.raises(L.OdoError, match="already"):      # (no longer "attached")
        vol.enable_spill(64)
    vol.close()
    # a following volume without a store, detached the same way, takes one
    v2 = _volume(trk, p)
    v2.set_follow(focus, 1)
    trk.attach_volume(v2)
    for k in range(10, 14):
        trk.track(*dev[k])
    trk.attach_volume(None)
    v2.enable_spill(1 << 12)
    v2.shift((0, 0, 1))
    assert v2.stats()["frames"] == 4 and v2.spilled(with_dropped=True)[2] == 0
    v2.close()
    trk.close()


# ---- refusals and lifecycle --------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_volume(ctx):
    from odometry_amd import _lib as L, api
    p, q, w, col = grids()["tiny 3"]
    vol = _volume(ctx, p)
    vol.upload(q, w)
    n = C.c_long(0)
    buf = np.zeros((4, 4), np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert vol.lib.odo_volume_spill_points(vol.h, 4, fp, fp, None, C.byref(n), None, 0) == -1 and "no spill store" in L.last_error()
    assert vol.lib.odo_debug_volume_spill_guard(vol.h, C.byref(n)) == -1
    with pytest.raises(L.OdoError, match="no follow parameters"):
        vol.follow(np.eye(4))
    vol.enable_spill(64)
    with pytest.raises(L.OdoError, match="already"):
        vol.enable_spill(64)
    rgba = np.zeros((4, 4), np.uint8)
    assert vol.lib.odo_volume_spill_points(vol.h, 4, fp, fp, rgba.ctypes.data_as(L._u8p), C.byref(n), None, 0) == -1
    assert "no colours" in L.last_error()
    vol.set_follow(1.0, 2)
    bad = np.eye(4)
    bad[2, 3] = np.nan
    with pytest.raises(L.OdoError, match="non-finite"):
        vol.follow(bad)
    assert vol.window()[0] == (0, 0, 0)
    assert all(np.array_equal(x, y) for x, y in zip(vol.grid(), (q, w)))        # nothing was enqueued by any of them
    vol.set_follow()
    with pytest.raises(L.OdoError, match="no follow parameters"):
        vol.follow(np.eye(4))
    # the bound on the cumulative shift: 2^24 is reached, one more is refused, the window and the (now empty) grid stay
    vol.shift((0, 0, 0))
    vol.shift((MAX_OFF, -MAX_OFF, 0))
    _window_equals(vol, p, (MAX_OFF, -MAX_OFF, 0), "at the bound")
    assert not vol.grid()[1].any()
    for d in ((1, 0, 0), (0, -1, 0), (2 ** 31 - 1, 0, 0)):
        with pytest.raises(L.OdoError, match="2\\^24"):
            vol.shift(d)
    _window_equals(vol, p, (MAX_OFF, -MAX_OFF, 0), "after the refusals")
    vol.shift((-MAX_OFF, MAX_OFF, 0))
    _window_equals(vol, p, (0, 0, 0), "back")
    vol.close()
    # while attached: no new store
    c = S.find("rgbd", 120, 160, 3)
    trk = api.RgbdTracker(0, **S.tracker_args(c))
    v2 = _volume(trk, params((131.25, 79.5, 59.5), 1000.0, (120, 160), dims=(16, 16, 16), vs=0.2, origin=(-1.6, -1.6, 0.5)))
    trk.attach_volume(v2)
    with pytest.raises(L.OdoError, match="attached"):
        v2.enable_spill(64)
    v2.close()
    trk.close()


def test_clear_keeps_the_window_and_empties_the_store_and_destroy_waits(ctx):
    p, q, w, col = grids()["tiny 3"]
    d = (1, 0, -1)
    vol = _volume(ctx, p, colour=True, spill=1 << 12)
    vol.upload(q, w)
    vol.upload_colour(col)
    vol.shift(d)
    assert len(vol.spilled()[0]) > 0
    vol.clear()
    _window_equals(vol, p, d, "after clear")                                     # the window stays where it is
    assert not vol.grid()[1].any() and not vol.colour_grid().any()
    got = vol.spilled(with_dropped=True)
    assert len(got[0]) == 0 and got[2] == 0
    # and the store fills again from its start, in the window that stayed
    vol.upload(q, w)
    vol.upload_colour(col)
    P, N, rgba = spill_model(q, w, col, window(p, d), (0, 1, 0))
    vol.shift((0, 1, 0))
    _store_equals(vol, P, N, rgba, "after clear")
    # destroyed with a spill and a shift pending
    vol.upload(q, w)
    vol.shift((1, 1, 1))
    vol.shift((-2, 0, 1))
    vol.close()
    other = _volume(ctx, p)
    other.upload(q, w)
    assert all(np.array_equal(x, y) for x, y in zip(other.grid(), (q, w)))
    other.close()


def test_save_ply_refuses_a_store_without_colours_on_a_coloured_volume(ctx, tmp_path):
    p, q, w, col = grids()["tiny 3"]
    vol = _volume(ctx, p, spill=1 << 12)
    vol.enable_colour()
    vol.upload(q, w)
    vol.upload_colour(col)
    vol.shift((2, 0, 0))
    with pytest.raises(ValueError, match="enable_colour before enable_spill"):
        vol.save_ply(str(tmp_path / "whole.ply"), spill=True)
    vol.save_ply(str(tmp_path / "grid.ply"))          # the extraction alone is written as before
    vol.close()


def test_shift_time_leaves_the_volume_as_it_is(ctx):
    """The timing entry point of tools/volume_cost.py shift: six positive figures with a store, and the grid, the colour grid, the
    window and the store's points read the same afterwards."""
    p, q, w, col = grids()["tiny 3"]
    vol = _volume(ctx, p, colour=True, spill=1 << 12)
    vol.upload(q, w)
    vol.upload_colour(col)
    vol.shift((1, 0, 0))
    before = (vol.grid(), vol.colour_grid(), vol.window(), vol.spilled(colour=True, with_dropped=True))
    us = vol.shift_time((0, 1, -1), reps=3)
    assert len(us) == 6 and all(x > 0 for x in us), us
    after = (vol.grid(), vol.colour_grid(), vol.window(), vol.spilled(colour=True, with_dropped=True))
    flat = lambda t: list(t[0]) + [t[1], t[2][1]] + list(t[3][:3])
    assert before[2][0] == after[2][0] == (1, 0, 0) and before[3][3] == after[3][3] == 0 and len(before[3][0]) > 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flat(before), flat(after)))
    plain = _volume(ctx, p)
    us = plain.shift_time((1, 0, 0), reps=2)
    assert all(x > 0 for x in us[:3]) and us[3:] == (0.0, 0.0, 0.0)
    plain.close()
    vol.close()


def test_save_ply_with_the_store_in_front(ctx, tmp_path):
    p, q, w, col = grids()["tiny 3"]
    vol = _volume(ctx, p, colour=True, spill=1 << 12)
    vol.upload(q, w)
    vol.upload_colour(col)
    vol.save_ply(str(tmp_path / "before.ply"))
    vol.shift((2, 0, 0))
    vol.save_ply(str(tmp_path / "after.ply"))
    vol.save_ply(str(tmp_path / "whole.ply"), spill=True)
    sp, ex = vol.spilled(colour=True), vol.extract(1 << 12, colour=True)
    vol.close()

    def body(name):
        head, data = open(tmp_path / name, "rb").read().split(b"end_header\n", 1)
        n = int([ln for ln in head.decode().split("\n") if ln.startswith("element vertex")][0].split()[-1])
        return n, data

    n_before, _ = body("before.ply")
    n_after, after = body("after.ply")
    n_whole, whole = body("whole.ply")
    assert n_after == len(ex[0]) and n_whole == len(sp[0]) + len(ex[0]) == n_before and len(sp[0]) > 0
    assert whole.endswith(after) and len(whole) == len(after) // n_after * n_whole
