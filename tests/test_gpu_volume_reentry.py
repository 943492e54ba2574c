"""The re-entry store of the moving TSDF volume on the GPU (odo_volume_enable_reentry; api.TsdfVolume.enable_reentry / stored_voxels /
reentry_stats) against the model of tests/volume_reentry_cases.py, bit for bit: every row of the CPU tests, the launch paths of the
shift and of the store's passes, walks enqueued back to back, the existing readers over a round trip, a volume without the store,
an attached tracker on an out-and-back drive, and the lifecycle. No tolerance anywhere in this file."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import shape_cases as S
import volume_reentry_cases as R
from test_gpu_volume_shift import _prefill, _rows_equal, _run, _volume, _window_equals
from test_volume_cpu import params, tiny_cases
from test_volume_shift_cpu import follow_model, grids as surface_grids, offset_model, shift_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 16


def _constant(name, header="volume.hip.h"):
    src = open(os.path.join(ROOT, "odometry_amd", "csrc", header)).read()
    return int(re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", src).group(1))


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _guards(vol):
    a, b = C.c_long(-1), C.c_long(-1)
    assert vol.lib.odo_debug_volume_reentry_guard(vol.h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def _state_equals(vol, p, state, tag, behind=True):
    """Grid, colour grid, window, store in order and the four counters against one state of the model; the guards of both sets, and
    (behind: the live count has never gone down) every byte behind the live entries still 0xAB."""
    q, w, col, off, store = state
    gq, gw = vol.grid()
    assert np.array_equal(gw, w) and np.array_equal(gq, q), f"{tag}: grid differs"
    if col is not None:
        assert np.array_equal(vol.colour_grid(), col), f"{tag}: colour grid differs"
    _window_equals(vol, p, off, tag)
    got = vol.stored_voxels(colour=store["col"] is not None)
    assert len(got[0]) == store["live"], f"{tag}: {len(got[0])} entries in the store, the model has {store['live']}"
    assert np.array_equal(got[0], store["g"]), f"{tag}: keys differ"
    gq, gw = R.unwords(store["vox"], (-1,))
    assert np.array_equal(got[1], gq) and np.array_equal(got[2], gw), f"{tag}: voxel words differ"
    if store["col"] is not None:
        assert np.array_equal(got[3].reshape(-1).view("<u4"), store["col"]), f"{tag}: colour words differ"
    assert vol.reentry_stats() == {k: store[k] for k in ("live", "saved", "restored", "dropped")}, (tag, vol.reentry_stats())
    changed, guard = _guards(vol)
    assert guard == 0 and (changed == 0 or not behind), (tag, changed, guard)


def _walk(ctx, p, q, w, col, shifts, capacity, tag, store_before_colour=False, every=True, prefill=True):
    """The walk in a fresh volume whose destination grids hold 0xAB, checked against the model after every shift (every=False: the
    shifts are enqueued back to back and only the end is compared)."""
    colour = col is not None
    vol = _volume(ctx, p) if store_before_colour else _volume(ctx, p, colour=colour)
    off = (0, 0, 0)
    if prefill:
        if store_before_colour:
            vol.enable_colour()
        _prefill(vol, q, colour)
        off = (1, 0, 0)
        vol.enable_reentry(capacity)
    else:
        vol.enable_reentry(capacity)
        if store_before_colour:
            vol.enable_colour()
    vol.upload(q, w)
    if colour:
        vol.upload_colour(col)
    states = R.walk_model(q, w, col, shifts, capacity, store_colour=colour and not (store_before_colour and not prefill), off=off)
    behind = True
    for n, d in enumerate(shifts):
        vol.shift(d)
        behind = behind and states[n + 1][4]["live"] >= states[n][4]["live"]
        if every:
            _state_equals(vol, p, states[n + 1], (tag, n, d), behind)
    _state_equals(vol, p, states[-1], (tag, "end"), behind)
    assert vol.stats()["frames"] == 0
    vol.close()
    return states


# ---- every CPU row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.grids()))
def test_every_cpu_row_matches_the_model_bit_for_bit(ctx, name):
    """The 14 closed walks of the grid, with colour, and every other one without. Both destination grids are pre-filled with 0xAB."""
    p, q, w, col = R.grids()[name]
    for n in range(14):
        shifts = R.walk_for(p["dims"], n)
        end = _walk(ctx, p, q, w, col, shifts, BIG, (name, n))[-1]
        assert end[4]["live"] == 0 and np.array_equal(end[1], w) and np.array_equal(end[2], col)
        if n % 2:
            _walk(ctx, p, q, w, None, shifts, BIG, (name, n, "no colour"))


def test_round_trip_restores_the_slab_that_a_plain_shift_zeroes(ctx):
    """d then -d: with the store the grids come back bit for bit and the store is empty; without it the same calls leave zeros."""
    p, q, w, col = R.grids()["random 64x4x4"]
    d = (3, 0, 0)
    vol = _volume(ctx, p, colour=True)
    vol.enable_reentry(BIG)
    plain = _volume(ctx, p, colour=True)
    for v in (vol, plain):
        v.upload(q, w)
        v.upload_colour(col)
        v.shift(d)
        v.shift(R.neg(d))
    gq, gw = vol.grid()
    assert np.array_equal(gq, q) and np.array_equal(gw, w) and np.array_equal(vol.colour_grid(), col)
    assert vol.window()[0] == (0, 0, 0)
    s = vol.reentry_stats()
    assert s["live"] == 0 and s["saved"] == s["restored"] > 0 and s["dropped"] == 0
    q1, w1, c1 = shift_model(*shift_model(q, w, col, d), R.neg(d))
    gq, gw = plain.grid()
    assert np.array_equal(gq, q1) and np.array_equal(gw, w1) and np.array_equal(plain.colour_grid(), c1) and not gw[:, :, :3].any()
    vol.close()
    plain.close()


def test_capacity_cuts_and_a_shift_with_restore_keep_and_save(ctx):
    p, q, w, col = R.grids()["random 64x4x4"]
    shifts, n1, n2, caps = R.capacity_rows()
    for cap in caps:
        end = _walk(ctx, p, q, w, col, shifts, cap, ("capacity", cap))[-1]
        assert end[4]["live"] == min(cap, n1 + n2) and end[4]["dropped"] == max(0, n1 + n2 - cap)
    st = _walk(ctx, p, q, w, col, R.MIXED, BIG, "mixed")
    a, b = st[2][4], st[3][4]
    assert b["restored"] > a["restored"] and b["saved"] > a["saved"] and a["live"] > b["restored"] - a["restored"]


def test_a_store_made_before_the_colour_grid_gives_colour_word_zero_back(ctx):
    from odometry_amd import _lib as L
    p, q, w, col = R.grids()["random 65x5x4"]
    d = (4, 0, -1)
    st = _walk(ctx, p, q, w, col, [d, R.neg(d)], BIG, "store before colour", store_before_colour=True, prefill=False)
    assert st[1][4]["col"] is None and np.array_equal(st[-1][1], w) and not np.array_equal(st[-1][2], col)
    vol = _volume(ctx, p)
    vol.enable_reentry(16)
    vol.enable_colour()
    with pytest.raises(L.OdoError, match="no colours"):
        vol.stored_voxels(colour=True)
    vol.close()


# ---- launch paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,shifts", [
    ((130, 7, 9), [(3, -1, 2), (-3, 1, -2), (0, 0, 9), (0, 0, -9)]),                # the dword build with a partial last block
    ((256, 5, 2), [(4, 0, 0), (-4, 0, 0), (-4, 1, 0), (4, -1, 0)]),                 # the 16-byte load
    ((2, 3, 5), [(1, 0, 0), (0, -1, 2), (-1, 1, -2)]),                             # rows shorter than a quad
])
def test_launch_paths_of_the_shift_with_a_store(ctx, dims, shifts):
    block = _constant("kVolExtBlock")
    n = int(np.prod(dims))
    if dims == (130, 7, 9):
        assert dims[0] % 4 and n % block and n > block
    if dims == (256, 5, 2):
        assert dims[0] % 4 == 0 and all(d[0] % 4 == 0 and d[0] for d in shifts)
    p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=dims, vs=0.04, origin=(-1.3, 0.1, 0.7))
    q, w, col = R.random_content(dims, 71)
    end = _walk(ctx, p, q, w, col, shifts, BIG, dims)[-1]
    assert end[4]["live"] == 0 and np.array_equal(end[1], w)


def test_save_and_store_pass_both_span_two_scan_chunks(ctx):
    """1024 x 32 x 33: the save walks more extraction blocks than one chunk of the scan holds, and with d = (0, 0, nz) so many voxels
    are stored that the store pass of the way back does too."""
    block, chunk = _constant("kVolExtBlock"), _constant("kVolScanThreads")
    dims = (1024, 32, 33)
    n = int(np.prod(dims))
    assert -(-n // block) > chunk
    rng = np.random.default_rng(8)
    shape = dims[::-1]
    q = rng.integers(-32768, 32768, shape).astype(np.int16)
    w = rng.integers(1, 65536, shape).astype(np.uint16)
    zero = rng.uniform(size=shape) < 0.01
    q[zero], w[zero] = 0, 0
    p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=dims, vs=0.04, origin=(-1.3, 0.1, 0.7))
    d = (0, 0, dims[2])
    states = R.walk_model(q, w, None, [d, R.neg(d)], n)
    live = states[1][4]["live"]
    assert -(-live // block) > chunk and live < n, live                 # the store pass of the second shift spans two chunks
    vol = _volume(ctx, p)
    vol.enable_reentry(n)
    vol.upload(q, w)
    vol.shift(d)
    s = vol.reentry_stats()
    assert s == dict(live=live, saved=live, restored=0, dropped=0)
    g, sq, sw = vol.stored_voxels()
    assert np.array_equal(g, states[1][4]["g"]) and np.array_equal(R.unwords(states[1][4]["vox"], (-1,))[1], sw) and not vol.grid()[1].any()
    vol.shift(R.neg(d))
    gq, gw = vol.grid()
    assert np.array_equal(gq, q) and np.array_equal(gw, w)
    assert vol.reentry_stats() == dict(live=0, saved=live, restored=live, dropped=0) and _guards(vol)[1] == 0
    vol.close()


# ---- walks enqueued back to back -----------------------------------------------------------------------------------------------------
def test_closed_walk_and_chain_enqueued_back_to_back_equal_the_model(ctx):
    for name in ("random 64x4x4", "random 65x5x4"):
        p, q, w, col = R.grids()[name]
        for shifts in (R.CLOSED_WALK, R.CHAIN):
            end = _walk(ctx, p, q, w, col, shifts, BIG, (name, len(shifts)), every=False, prefill=False)[-1]
            assert end[4]["live"] == 0 and end[3] == (0, 0, 0) and np.array_equal(end[0], q) and np.array_equal(end[1], w) and \
                np.array_equal(end[2], col)


# ---- the readers over a round trip ---------------------------------------------------------------------------------------------------
def test_raycast_and_extract_are_the_same_bits_after_a_shift_away_and_back(ctx):
    p, q, w, col = surface_grids()["tiny 3"]
    vol = _volume(ctx, p, colour=True)
    vol.enable_reentry(BIG)
    vol.upload(q, w)
    vol.upload_colour(col)
    pose = np.asarray(tiny_cases()[3][1][0][1], np.float32)                # the pose of the frame that made the surface
    before = vol.raycast(pose, colour=True) + vol.extract(1 << 16, colour=True)
    assert before[0].any() and len(before[-3]) > 0
    d = (p["dims"][0] // 2, -1, p["dims"][2])
    vol.shift(d)
    assert not vol.grid()[1].any()                                       # |dz| = nz: the window is empty out there
    vol.shift(R.neg(d))
    after = vol.raycast(pose, colour=True) + vol.extract(1 << 16, colour=True)
    assert len(before) == len(after) and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    assert vol.reentry_stats()["live"] == 0
    vol.close()


# ---- without the store -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.grids()))
def test_a_volume_without_the_store_gives_the_plain_shift(ctx, name):
    from odometry_amd import _lib as L
    p, q, w, col = R.grids()[name]
    for n in range(14):
        vol = _volume(ctx, p, colour=True)
        vol.upload(q, w)
        vol.upload_colour(col)
        m, off = (q, w, col), (0, 0, 0)
        for d in R.walk_for(p["dims"], n):
            vol.shift(d)
            m, off = shift_model(*m, d), offset_model(off, d)
        gq, gw = vol.grid()
        assert np.array_equal(gq, m[0]) and np.array_equal(gw, m[1]) and np.array_equal(vol.colour_grid(), m[2]), (name, n)
        _window_equals(vol, p, off, (name, n))
        if n == 0:
            with pytest.raises(L.OdoError, match="no re-entry store"):
                vol.reentry_stats()
        vol.close()


# ---- attached to a tracker ---------------------------------------------------------------------------------------------------------
def _drive():
    c = dict(S.find("rgbd", 120, 160, 3), frames=14)
    seq = S.render(c)
    p = params(seq, size=(c["rows"], c["cols"]), dims=(112, 64, 56), vs=0.1, origin=(-5.6, -3.23, 3.0), mu=0.3, max_depth=8.0)
    order = list(range(c["frames"])) + list(range(c["frames"] - 2, -1, -1))     # out and back over the same frames
    return c, seq, p, order


def test_attached_tracker_on_an_out_and_back_drive(ctx):
    """Poses, keyframe flags, motion scores and the last frame's mask and inverse depth are the same bits with re-entry on and off,
    and the volume ends with the grid, window and store of a standalone volume fed the returned poses through follow + integrate."""
    from odometry_amd import api
    c, seq, p, order = _drive()
    size = (c["rows"], c["cols"])
    focus, threshold = 5.8, 3

    def run(reentry):
        trk = api.RgbdTracker(0, **S.tracker_args(c))
        vol = _volume(trk, p)
        if reentry:
            vol.enable_reentry(1 << 19)
        vol.set_follow(focus, threshold)
        trk.attach_volume(vol)
        dev = [(trk.upload_frame(seq["gray"][k]), trk.upload_depth(seq["depth"][k])) for k in order]
        return trk, vol, dev, _run(trk, dev, size)

    trk0, vol0, _, want = run(False)
    grid_off = vol0.grid()
    vol0.close()
    trk0.close()
    trk, vol, dev, got = run(True)
    _rows_equal(got, want, "re-entry on")
    ref = _volume(trk, p)
    ref.enable_reentry(1 << 19)
    ref.set_follow(focus, threshold)
    off, fwd, back = (0, 0, 0), 0, 0
    for (_, d), r in zip(dev, got):
        want_d = follow_model(r["abs_pose"], p, off, focus, threshold)
        assert ref.follow(r["abs_pose"]) == want_d
        off = offset_model(off, want_d)
        fwd += want_d[2] > 0
        back += want_d[2] < 0
        ref.integrate(d, r["abs_pose"])
    print("the attached volume shifted", fwd, "times out and", back, "times back, to", off)
    assert fwd >= 3 and back >= 3
    assert vol.window()[0] == off and vol.window()[1].tobytes() == ref.window()[1].tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(vol.grid(), ref.grid()))
    a, b = vol.stored_voxels(), ref.stored_voxels()                          # (legal while attached)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    sa = vol.reentry_stats()
    assert sa == ref.reentry_stats() and sa["restored"] > 0 and sa["dropped"] == 0
    assert vol.stats() == ref.stats()
    # what it is for: the voxels that came back kept the weight of the way out (restored > 0, and every fused voxel has w > 0)
    w_on, w_off = vol.grid()[1].astype(np.int64), grid_off[1].astype(np.int64)
    print("final window: observed voxels", int((w_on > 0).sum()), "with re-entry,", int((w_off > 0).sum()), "without; total weight",
          int(w_on.sum()), "against", int(w_off.sum()))
    assert w_on.sum() > w_off.sum()
    ref.close()
    vol.close()
    trk.close()


def test_detach_clear_and_destroy_with_a_shift_pending(ctx):
    """Detach directly behind a frame whose follow step is still enqueued; clear empties the store; destroy with a shift pending."""
    from odometry_amd import _lib as L, api
    c, seq, p, order = _drive()
    focus = 5.8
    trk = api.RgbdTracker(0, **S.tracker_args(c))
    dev = [(trk.upload_frame(seq["gray"][k]), trk.upload_depth(seq["depth"][k])) for k in order[:10]]
    vol = _volume(trk, p)
    vol.set_follow(focus, 1)               # threshold 1: the window moves whenever the focus point is a voxel off centre
    trk.attach_volume(vol)
    with pytest.raises(L.OdoError, match="attached"):
        vol.enable_reentry(16)
    trk.attach_volume(None)
    vol.enable_reentry(1 << 19)
    trk.attach_volume(vol)
    with pytest.raises(L.OdoError, match="attached"):
        vol.reentry_time((1, 0, 0), 1)
    trk.init(*dev[0])
    poses = [np.eye(4, dtype=np.float32)] + [trk.track(*dev[k])["abs_pose"] for k in range(1, 10)]
    trk.attach_volume(None)                # the last frame's passes, shift and integration are pending here
    off = (0, 0, 0)
    for A in poses:
        last = follow_model(A, p, off, focus, 1)
        off = offset_model(off, last)
    assert last != (0, 0, 0), "the last frame must shift, or nothing of the follow step is pending at the detach"
    assert vol.window()[0] == off
    got = (vol.grid(), vol.stored_voxels(), vol.reentry_stats())
    ref = _volume(trk, p)
    ref.enable_reentry(1 << 19)
    ref.set_follow(focus, 1)
    for (_, d), A in zip(dev, poses):
        ref.follow(A)
        ref.integrate(d, A)
    assert all(np.array_equal(x, y) for x, y in zip(got[0], ref.grid()))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[1], ref.stored_voxels())) and got[2] == ref.reentry_stats()
    assert got[2]["live"] > 1
    # a buffer below the live count is refused: the count comes back, nothing is copied or cleared
    n, g1, v1 = C.c_long(0), np.full((1, 3), -7, np.int32), np.full(1, 7, np.uint32)
    assert vol.lib.odo_volume_reentry_voxels(vol.h, 1, g1.ctypes.data_as(C.POINTER(C.c_int32)), v1.ctypes.data_as(C.POINTER(C.c_uint32)), None,
                                             C.byref(n), 1) == -1 and "holds" in L.last_error()
    assert n.value == got[2]["live"] and (g1 == -7).all() and v1[0] == 7 and vol.reentry_stats() == got[2]
    # clear=True hands the entries out and empties the store
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[1], ref.stored_voxels(clear=True)))
    assert ref.reentry_stats() == dict(live=0, saved=0, restored=0, dropped=0) and len(ref.stored_voxels()[0]) == 0
    ref.close()
    with pytest.raises(L.OdoError, match="already"):      # (no longer "attached")
        vol.enable_reentry(64)
    # the timing leaves the volume and the store as they are
    us = vol.reentry_time((0, 0, -2), 3)
    assert len(us) == 5 and all(u > 0 for u in us)
    assert all(np.array_equal(x, y) for x, y in zip(got[0], vol.grid())) and vol.reentry_stats() == got[2]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[1], vol.stored_voxels()))
    # clear empties the store; the window stays; the next shift saves from the store's start
    vol.clear()
    assert vol.reentry_stats() == dict(live=0, saved=0, restored=0, dropped=0) and vol.window()[0] == off
    q, w, _ = R.random_content(p["dims"], 5)
    vol.upload(q, w)
    d = (0, 0, 1)
    vol.shift(d)
    st = R.reentry_model(q, w, None, off, R.empty_store(False), d, 1 << 19)
    assert np.array_equal(vol.stored_voxels()[0], st[4]["g"]) and vol.reentry_stats()["saved"] == st[4]["live"]
    # a refused shift touches nothing
    with pytest.raises(L.OdoError, match="2\\^24"):
        vol.shift((1 << 25, 0, 0))
    assert vol.window()[0] == st[3] and vol.reentry_stats()["saved"] == st[4]["live"]
    vol.shift((2, 1, 0))                   # pending at the destroy
    vol.close()
    trk.close()
