"""The mesh of the leaving slab on the GPU (odo_volume_enable_spill_mesh, odo_volume_spill_mesh; api.TsdfVolume.enable_spill_mesh /
spilled_mesh / save_mesh_ply(spill=True)) against the model of tests/volume_spill_mesh_cases.py, bit for bit: every row of the CPU
tests, the launch geometries, the all-or-nothing rule, a chain of 27 shifts enqueued back to back, the point store beside the mesh
store, the existing operations after a mesh spill, the drive that leaves its box and an attached tracker that follows. No
tolerance anywhere in this file."""
import ctypes as C
import functools

import numpy as np
import pytest

import shape_cases as S
import volume_spill_mesh_cases as M
from test_gpu_volume_shift import _prefill, _rows_equal, _run, _volume, _window_equals
from test_volume_cpu import bits, params, tiny_cases
from test_volume_colour_cpu import mesh_colours_model, random_colour
from test_volume_mesh_cpu import mesh_model, read_ply_mesh
from test_volume_shift_cpu import DRIVE, drive_case, grids, offset_model, shift_model, window

pytestmark = pytest.mark.gpu
BIG = (1 << 14, 1 << 14)


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _guard_intact(vol):
    """The library fills the mesh store's buffers with 0xAB when it allocates them, 64 guard items behind each capacity included; the
    test hook counts the bytes behind the store's last vertex and last triangle that no longer hold it. Zero: the spills so far
    wrote their own items and nothing else. Only for a store that was never emptied or timed."""
    n = C.c_long(-1)
    assert vol.lib.odo_debug_volume_spill_mesh_guard(vol.h, C.byref(n)) == 0
    return n.value == 0


def _store_equals(vol, want, tag):
    colour = want["rgba"] is not None
    got = vol.spilled_mesh(colour=colour, with_dropped=True)
    assert (len(got[0]), len(got[2])) == (len(want["xyz0"]), len(want["tri"])), \
        f"{tag}: {len(got[0])} vertices and {len(got[2])} triangles in the store, the model has {len(want['xyz0'])} and {len(want['tri'])}"
    assert np.array_equal(bits(got[0]), bits(want["xyz0"])), f"{tag}: positions differ"
    assert np.array_equal(bits(got[1]), bits(want["nrmw"])), f"{tag}: normals / weights differ"
    assert np.array_equal(got[2], want["tri"]), f"{tag}: triangles differ"
    if colour:
        assert np.array_equal(got[3], want["rgba"]), f"{tag}: colours differ"
    assert tuple(got[-1]) == tuple(want["dropped"]), (tag, got[-1], want["dropped"])


def _loaded(ctx, p, q, w, col, capacities, points=0):
    """A volume whose second buffers hold 0xAB, with the grids uploaded and a fresh 0xAB-filled mesh store (and point store)."""
    vol = _volume(ctx, p, colour=col is not None)
    _prefill(vol, q, col is not None)
    vol.enable_spill_mesh(*capacities)
    if points:
        vol.enable_spill(points)
    vol.upload(q, w)
    if col is not None:
        vol.upload_colour(col)
    return vol


def _after(vol, p, r, tag, off0=(1, 0, 0)):
    """The grids and the window after the row's shifts (the volume was prefilled: its window started at off0)."""
    gq, gw = vol.grid()
    assert np.array_equal(gw, r["w"]) and np.array_equal(gq, r["q"]), tag
    if r["col"] is not None:
        assert np.array_equal(vol.colour_grid(), r["col"]), tag
    _window_equals(vol, p, offset_model(off0, r["off"]), tag)


# ---- every CPU row -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour,points", [(True, True), (False, False)])
@pytest.mark.parametrize("name", [r[0] for r in M.ROWS])
def test_every_cpu_row_matches_the_model_bit_for_bit(ctx, name, colour, points):
    """Vertices, normals and weights, colours, triangles, counts and dropped after the row's shifts; the buffers started at 0xAB and
    behind the store's items they still hold it. With the point store beside the mesh store its bytes are those of a volume that has
    the point store alone."""
    _, grid, shifts, _, _ = M.row(name)
    p, q, w, col = M.all_grids()[grid]
    col = col if colour else None
    # (the model's window starts at off (1, 0, 0) here, as _prefill leaves it: positions are taken in that window)
    r = M.run_shifts(p, q, w, col, shifts, BIG, off=(1, 0, 0))
    r["off"] = tuple(a - b for a, b in zip(r["off"], (1, 0, 0)))
    vol = _loaded(ctx, p, q, w, col, BIG, points=1 << 12 if points else 0)
    for d in shifts:
        vol.shift(d)
    _store_equals(vol, r["store"], name)
    assert _guard_intact(vol), name
    _after(vol, p, r, name)
    if points:
        ref = _volume(ctx, p, colour=colour)
        _prefill(ref, q, colour)
        ref.enable_spill(1 << 12)
        ref.upload(q, w)
        ref.upload_colour(col)
        for d in shifts:
            ref.shift(d)
        a, b = vol.spilled(colour=colour, with_dropped=True), ref.spilled(colour=colour, with_dropped=True)
        assert a[-1] == b[-1] and all(x.tobytes() == y.tobytes() for x, y in zip(a[:-1], b[:-1])), name
        ref.close()
    vol.close()


# ---- launch geometries ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sheets(dims):
    """A grid of slanted sheets (a sine of a plane wave, 3 % of the voxels never observed, random weights and colours): surface in every
    slab and every block's neighbourhood, and few enough vertices for the model. Its mesh and colours, computed once."""
    nx, ny, nz = dims
    p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=dims, vs=0.05, origin=(-1.3, 0.1, 0.7))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    rng = np.random.default_rng(sum(dims))
    a, b, c = (0.02, 0.15, 0.2) if nx >= 1024 else (0.35, 0.9, 0.7)      # (the small grid needs sheets inside a slab two voxels thick)
    q = np.rint(20000.0 * np.sin(a * i + b * j + c * k + 0.3) + rng.integers(-50, 51, i.shape)).astype(np.int16)
    w = rng.integers(1, 300, i.shape).astype(np.uint16)
    w[rng.uniform(size=w.shape) < 0.03] = 0
    q[w == 0] = 0
    col = random_colour(q.shape, 5)
    return p, q, w, col, mesh_model(q, w, window(p, (1, 0, 0)), detail=True), mesh_colours_model(q, w, col)


@pytest.mark.parametrize("dims,d", [((130, 7, 9), (1, 0, 0)), ((130, 7, 9), (-1, -1, -1)), ((1024, 32, 33), (0, 0, 1)),
                                    ((1024, 32, 33), (-1, -1, -1))])
def test_launch_geometries_match_the_model(ctx, dims, d):
    """130 x 7 x 9: a partial last block and rows that are no multiple of 64. 1024 x 32 x 33: 1 056 blocks, past one chunk of the scan;
    under (0, 0, 1) only the blocks of the two lowest planes have a voxel near the slab and every other block returns early, under
    (-1, -1, -1) every block has one and most of its threads skip."""
    p, q, w, col, mesh, colours = _sheets(dims)
    P, N, T, Cc = M.spill_of_mesh(mesh, colours, d, dims)
    assert 0 < len(P) < len(mesh[0]) and 0 < len(T) < len(mesh[2])
    vol = _loaded(ctx, p, q, w, col, (len(P) + 3, len(T) + 5))
    vol.shift(d)
    _store_equals(vol, dict(xyz0=P, nrmw=N, tri=T, rgba=Cc, dropped=(0, 0)), (dims, d))
    assert _guard_intact(vol), (dims, d)
    q2, w2, c2 = shift_model(q, w, col, d)
    _after(vol, p, dict(q=q2, w=w2, col=c2, off=d), (dims, d))
    vol.close()


# ---- the store -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.one_short()))
def test_a_spill_is_appended_whole_or_not_at_all(ctx, name):
    caps, taken = M.one_short()[name]
    p, q, w, col = M.all_grids()[M.TWO_SHIFTS[0]]
    r = M.run_shifts(p, q, w, col, M.TWO_SHIFTS[1], caps, off=(1, 0, 0))
    assert r["taken"] == taken
    vol = _loaded(ctx, p, q, w, col, caps)
    for d in M.TWO_SHIFTS[1]:
        vol.shift(d)
    _store_equals(vol, r["store"], name)
    assert _guard_intact(vol), name
    vol.close()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_chain_of_27_shifts_into_stores_that_fit_fill_exactly_and_refuse_in_the_middle(ctx, which):
    """24 shifts by (1, 0, 0) and 3 by (0, 1, 0) with nothing between them. The store holds exactly the spills the model appends: all
    of them; the first 12, which fill it to the last item; all but those that do not fit after the 5th is refused by one triangle,
    the later, smaller ones included. Emptied, it takes the next spill from its start."""
    c = M.chain()
    p, q, w, col = c["p"], c["q"], c["w"], c["col"]
    caps = c["capacities"][which]
    r = M.run_shifts(p, q, w, col, M.CHAIN, caps, off=(1, 0, 0))
    assert all(r["taken"]) == (which == 0)
    vol = _loaded(ctx, p, q, w, col, caps)
    for d in M.CHAIN:
        vol.shift(d)
    _store_equals(vol, r["store"], f"capacities {caps}")
    assert _guard_intact(vol), caps
    off = tuple(a - b for a, b in zip(r["off"], (1, 0, 0)))
    _after(vol, p, dict(r, off=off), caps)
    got = vol.spilled_mesh(clear=True, with_dropped=True)
    assert len(got[0]) == len(r["store"]["xyz0"])
    d = (0, 0, 1)
    nxt = M.run_shifts(p, r["q"], r["w"], r["col"], [d], caps, off=r["off"])
    assert nxt["taken"] == [True] and len(nxt["store"]["xyz0"]) > 0
    vol.shift(d)
    _store_equals(vol, nxt["store"], f"capacities {caps}, after clear")
    vol.close()


def test_a_store_made_before_the_colour_grid_and_copies_that_would_cut(ctx):
    from odometry_amd import _lib as L
    p, q, w, col = M.all_grids()["dyadic 6x5x4 20%"]
    vol = _volume(ctx, p)
    vol.enable_spill_mesh(*BIG)
    vol.enable_colour()
    vol.upload(q, w)
    vol.upload_colour(col)
    d = (1, 0, -1)
    vol.shift(d)
    want = M.run_shifts(p, q, w, None, [d], BIG)["store"]
    _store_equals(vol, want, "no colours")
    with pytest.raises(L.OdoError, match="no colours"):
        vol.spilled_mesh(colour=True)
    # the C entry with buffers one item short of the store on either side: refused, the counts returned, nothing copied or cleared
    nv, nt = len(want["xyz0"]), len(want["tri"])
    n, m = C.c_long(0), C.c_long(0)
    for vc, tc in ((nv - 1, nt), (nv, nt - 1)):
        xyz0, nrmw, tri = np.full((nv, 4), 7, np.float32), np.full((nv, 4), 7, np.float32), np.full((nt, 3), 7, np.int32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        assert vol.lib.odo_volume_spill_mesh(vol.h, vc, tc, fp(xyz0), fp(nrmw), None, tri.ctypes.data_as(C.POINTER(C.c_int32)),
                                             C.byref(n), C.byref(m), None, 1) == -1
        assert (n.value, m.value) == (nv, nt) and (xyz0 == 7).all() and (tri == 7).all()
    _store_equals(vol, want, "after the refusals")
    vol.close()


# ---- the rest of the volume does not notice --------------------------------------------------------------------------------------------
def test_existing_operations_after_a_mesh_spill_equal_those_without_a_store(ctx):
    """mesh (which shares the spill's scratch), extract, ray-cast, icp_eval and an integration after a mesh spill equal the same calls
    on a volume without a mesh store; a mesh taken between two spills does not disturb the second."""
    case_p, frames = tiny_cases()[3]
    p, q, w, col = grids()["tiny 3"]
    d1, d2 = (1, -1, 2), (0, 1, -1)
    vols = []
    for store in (True, False):
        v = _volume(ctx, p, colour=True)
        if store:
            v.enable_spill_mesh(*BIG)
        v.upload(q, w)
        v.upload_colour(col)
        v.shift(d1)
        vols.append(v)
    vol, ref = vols
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.05, -0.05, 0.1)
    for tag, call in (("mesh", lambda v: v.mesh(colour=True)), ("extract", lambda v: v.extract(1 << 12, colour=True)),
                      ("raycast", lambda v: v.raycast(pose, raw=True, colour=True))):
        a, b = call(vol), call(ref)
        assert len(a) == len(b) and len(a[0]) > 0
        for x, y in zip(a, b):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), tag
    depth, nrmw = vol.raycast(pose)[:2]
    raw = frames[0][0]
    acc = [v.icp_eval(raw, depth, nrmw, pose, np.eye(4, dtype=np.float32)) for v in (vol, ref)]
    assert acc[0].tobytes() == acc[1].tobytes() and acc[0].any()
    for v in (vol, ref):
        v.shift(d2)
        v.integrate(raw, frames[0][1])
    assert all(np.array_equal(x, y) for x, y in zip(vol.grid(), ref.grid())) and np.array_equal(vol.colour_grid(), ref.colour_grid())
    _store_equals(vol, M.run_shifts(p, q, w, col, [d1, d2], BIG)["store"], "a mesh between two spills")
    assert len(vol.spilled_mesh()[2]) > 0
    for v in vols:
        v.close()


def test_the_drive_that_leaves_its_box_matches_the_model(ctx, tmp_path):
    """DESIGN.md section 9.9's drive with both stores: the mesh store is the model's, spill by spill, and save_mesh_ply(spill=True)
    writes it in front of the window's mesh with the window's indices offset; the default writes what it wrote before."""
    c = drive_case()
    p = c["p"]
    vol = _volume(ctx, p, spill=1 << 16)
    vol.enable_spill_mesh(1 << 18, 1 << 18)
    vol.set_follow(DRIVE["focus"], DRIVE["threshold"])
    from test_volume_cpu import empty_grid, integrate_model
    q, w = empty_grid(p)
    off, store = (0, 0, 0), M.empty_store(False)
    for raw, T, d in zip(c["depth"], c["poses"], c["shifts"]):
        assert vol.follow(T) == d
        if d != (0, 0, 0):
            mesh = mesh_model(q, w, window(p, off), detail=True)
            store, ok = M.store_append(store, lambda f: M.spill_of_mesh(mesh, None, d, p["dims"], f), (1 << 18, 1 << 18))
            assert ok
            q, w, _ = shift_model(q, w, None, d)
            off = offset_model(off, d)
        vol.integrate(raw, T)
        q, w, _, _ = integrate_model(q, w, raw, T, window(p, off))
    _store_equals(vol, store, "drive")
    a = vol.spilled(with_dropped=True)
    assert a[2] == 0 and a[0].tobytes() == np.concatenate([P for P, _ in c["spills"]]).tobytes()
    final = mesh_model(q, w, window(p, off))
    both, alone = str(tmp_path / "both.ply"), str(tmp_path / "window.ply")
    vol.save_mesh_ply(both, spill=True)
    vol.save_mesh_ply(alone)
    V, T = read_ply_mesh(both)
    ns = len(store["xyz0"])
    assert np.array_equal(bits(V[:, :3]), bits(np.concatenate([store["xyz0"], final[0]])[:, :3]))
    assert np.array_equal(bits(V[:, 3:]), bits(np.concatenate([store["nrmw"], final[1]])[:, :3]))
    assert np.array_equal(T, np.concatenate([store["tri"], final[2] + ns]))
    V1, T1 = read_ply_mesh(alone)
    assert np.array_equal(bits(V1[:, :3]), bits(final[0][:, :3])) and np.array_equal(T1, final[2])
    vol.close()


def test_attached_tracker_follows_and_fills_the_mesh_store():
    """The 120 x 160 RGB-D row of tests/shape_cases.py, 14 frames: with a mesh store on the attached, following volume the tracker's
    rows are the bits of a run without a store, and the store equals that of a standalone volume fed the returned poses."""
    from odometry_amd import _lib as L, api
    c = dict(S.find("rgbd", 120, 160, 3), frames=14)
    seq = S.render(c)
    size = (c["rows"], c["cols"])
    p = params(seq, size=size, dims=(112, 64, 56), vs=0.1, origin=(-5.6, -3.23, 3.0), mu=0.3, max_depth=8.0)
    focus, threshold = 5.8, 3

    def run(store):
        trk = api.RgbdTracker(0, **S.tracker_args(c))
        vol = _volume(trk, p)
        if store:
            vol.enable_spill_mesh(1 << 17, 1 << 18)
        vol.set_follow(focus, threshold)
        trk.attach_volume(vol)
        dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])]
        return trk, vol, dev, _run(trk, dev, size)

    trk0, vol0, _, want = run(False)
    grid0 = vol0.grid()
    vol0.close()
    trk0.close()
    trk, vol, dev, got = run(True)
    _rows_equal(got, want, "a following volume with a mesh store")
    assert all(np.array_equal(x, y) for x, y in zip(vol.grid(), grid0))
    ref = _volume(trk, p)
    ref.enable_spill_mesh(1 << 17, 1 << 18)
    ref.set_follow(focus, threshold)
    n_shifts = 0
    for (_, d), r in zip(dev, got):
        n_shifts += ref.follow(r["abs_pose"]) != (0, 0, 0)
        ref.integrate(d, r["abs_pose"])
    assert n_shifts >= 3
    with pytest.raises(L.OdoError, match="attached"):
        vol.spill_mesh_time((1, 0, 0), 2)
    fresh = _volume(trk, p)
    trk.attach_volume(None)
    trk.attach_volume(fresh)
    with pytest.raises(L.OdoError, match="attached"):
        fresh.enable_spill_mesh(8, 8)
    trk.attach_volume(None)
    fresh.close()
    a, b = vol.spilled_mesh(with_dropped=True), ref.spilled_mesh(with_dropped=True)
    assert len(a[0]) > 0 and len(a[2]) > 0 and a[3] == b[3] == (0, 0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))
    assert a[2].max() < len(a[0])
    ref.close()
    vol.close()
    trk.close()


# ---- clear, destroy, refusals, timing --------------------------------------------------------------------------------------------------
def test_clear_refusals_on_a_live_volume_timing_and_destroy_with_a_spill_pending(ctx):
    from odometry_amd import _lib as L
    p, q, w, col = M.all_grids()["dyadic 9x8x7 20%"]
    vol = _volume(ctx, p, colour=True)
    with pytest.raises(L.OdoError, match="no mesh store"):
        vol.spilled_mesh()
    with pytest.raises(L.OdoError, match="no mesh store"):
        vol.spill_mesh_time((1, 0, 0), 2)
    n = C.c_long(0)
    assert vol.lib.odo_debug_volume_spill_mesh_guard(vol.h, C.byref(n)) == -1
    vol.enable_spill_mesh(*BIG)
    with pytest.raises(L.OdoError, match="already"):
        vol.enable_spill_mesh(*BIG)
    vol.upload(q, w)
    vol.upload_colour(col)
    d = (1, -1, 1)
    vol.shift(d)
    want = M.run_shifts(p, q, w, col, [d], BIG)
    _store_equals(vol, want["store"], "before timing")
    # the timing call changes neither the store nor the grids nor the window
    us = vol.spill_mesh_time((0, 2, 0), 3)
    assert len(us) == 5 and all(np.isfinite(x) and x > 0 for x in us)
    _store_equals(vol, want["store"], "after timing")
    _after(vol, p, want, "after timing", off0=(0, 0, 0))
    # without a colour grid the colour stage is not launched: its figure is exactly 0, and the grid and the store stay as they are
    plain = _volume(ctx, p)
    plain.enable_spill_mesh(*BIG)
    plain.upload(q, w)
    plain.shift(d)
    before = (plain.grid(), plain.window(), plain.spilled_mesh(with_dropped=True))
    us = plain.spill_mesh_time((0, 2, 0), 2)
    assert len(us) == 5 and all(np.isfinite(x) and x > 0 for x in us[:4]) and us[4] == 0.0, us
    after = (plain.grid(), plain.window(), plain.spilled_mesh(with_dropped=True))
    assert before[1][0] == after[1][0] == d and before[2][3] == after[2][3] and len(before[2][0]) > 0
    flat = lambda t: list(t[0]) + [np.asarray(t[1][1])] + list(t[2][:3])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(flat(before), flat(after)))
    plain.close()
    # and the next spill lands behind the store's items as if the timing had not run
    vol.shift((0, 2, 0))
    _store_equals(vol, M.run_shifts(p, q, w, col, [d, (0, 2, 0)], BIG)["store"], "a spill after timing")
    # clear empties the store and keeps the window
    vol.clear()
    got = vol.spilled_mesh(with_dropped=True)
    assert len(got[0]) == 0 and len(got[2]) == 0 and got[3] == (0, 0)
    assert vol.window()[0] == (1, 1, 1)
    vol.upload(q, w)
    vol.upload_colour(col)
    vol.shift((0, 0, -1))          # destroyed with this spill pending
    vol.close()
