"""The moving TSDF volume with its three stores together on the GPU (the point store of odo_volume_enable_spill, the mesh store of
odo_volume_enable_spill_mesh, the re-entry store of odo_volume_enable_reentry; DESIGN.md sections 9.9, 9.13, 9.14) against the
composed model of tests/volume_stores_cases.py, bit for bit: every row of the CPU tests after every shift and back to back, the
orders in which the stores and the colour grid can be made, the readers between shifts, the three timing calls, the launch
geometries, clearing, and an attached tracker on an out-and-back drive. No tolerance anywhere in this file."""
import ctypes as C
import itertools

import numpy as np
import pytest

import shape_cases as S
import test_gpu_volume_spill_mesh as GM
import volume_reentry_cases as R
import volume_spill_mesh_cases as M
import volume_stores_cases as V
from test_gpu_volume_reentry import _constant, _drive, _guards, _state_equals
from test_gpu_volume_shift import _guard_intact, _prefill, _rows_equal, _run, _store_equals, _volume, _window_equals
from test_volume_colour_cpu import mesh_colours_model
from test_volume_mesh_cpu import mesh_model
from test_volume_shift_cpu import follow_model, offset_model, spill_model, window

pytestmark = pytest.mark.gpu
OFF1 = (1, 0, 0)           # where _prefill leaves the window


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _enable(vol, store, caps):
    if store == "points":
        vol.enable_spill(caps["points"])
    elif store == "mesh":
        vol.enable_spill_mesh(*caps["mesh"])
    else:
        vol.enable_reentry(caps["reentry"])


def _make(ctx, p, q, w, col, caps, flags, order=V.STORES, readers_first=False):
    """A fresh volume in the window OFF1 whose second voxel buffer holds 0xAB (and the second colour buffer, when every store is
    made after the colour grid), with the stores `caps` names made in `order`: those whose flag is False in front of
    enable_colour, the others behind it. readers_first: extract() and mesh() run before any store exists, so that they allocate
    the scratch the spills share."""
    have = [s for s in order if caps.get(s)]
    early = [s for s in have if not flags[s]]
    vol = _volume(ctx, p)
    if col is not None and not early:
        vol.enable_colour()
    _prefill(vol, q, vol.has_colour)
    if readers_first:
        vol.upload(q, w)
        assert len(vol.extract(1 << 14)[0]) > 0 and len(vol.mesh()[2]) > 0
    for s in early:
        _enable(vol, s, caps)
    if col is not None and early:
        vol.enable_colour()
    for s in have:
        if s not in early:
            _enable(vol, s, caps)
    vol.upload(q, w)
    if col is not None:
        vol.upload_colour(col)
    return vol


def _check(vol, p, st, tag, behind=True, intact=True):
    """One state of the model: the grids, the colour grid, the window, the point store with its dropped count, the mesh store with
    both dropped counts, the re-entry store in order with its four counters; the three guard hooks (intact: neither log has been
    emptied or timed; behind: the re-entry store's live count has never gone down)."""
    if st["reentry"] is not None:
        _state_equals(vol, p, (st["q"], st["w"], st["col"], st["off"], st["reentry"]), tag, behind)
    else:
        gq, gw = vol.grid()
        assert np.array_equal(gw, st["w"]) and np.array_equal(gq, st["q"]), f"{tag}: grid differs"
        if st["col"] is not None:
            assert np.array_equal(vol.colour_grid(), st["col"]), f"{tag}: colour grid differs"
        _window_equals(vol, p, st["off"], tag)
    if st["points"] is not None:
        s = st["points"]
        _store_equals(vol, s["xyz0"], s["nrmw"], s["rgba"], (tag, "points"), dropped=s["dropped"])
        assert not intact or _guard_intact(vol), (tag, "the point store's guard")
    if st["mesh"] is not None:
        GM._store_equals(vol, st["mesh"], (tag, "mesh"))
        assert not intact or GM._guard_intact(vol), (tag, "the mesh store's guard")


def _walk(ctx, p, q, w, col, shifts, caps, flags, tag, every=True, **how):
    vol = _make(ctx, p, q, w, col, caps, flags, **how)
    states = V.stores_walk_model(p, q, w, col, shifts, caps, flags, off=OFF1)
    behind = True
    for n, d in enumerate(shifts):
        vol.shift(d)
        if caps.get("reentry"):
            behind = behind and states[n + 1]["reentry"]["live"] >= states[n]["reentry"]["live"]
        if every:
            _check(vol, p, states[n + 1], (tag, n, d), behind)
    _check(vol, p, states[-1], (tag, "end"), behind)
    assert vol.stats()["frames"] == 0
    vol.close()
    return states


# ---- every CPU row ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r["name"] for r in V.rows()])
def test_every_cpu_row_matches_the_model_after_every_shift_and_back_to_back(ctx, name):
    """9 x 8 x 7 voxels. A fresh volume per run; the second run enqueues the shifts with nothing between them and compares the end."""
    r = V.row(name)
    p, q, w, col = V.grid(r["grid"])
    st = _walk(ctx, p, q, w, col, r["shifts"], r["capacities"], r["colour_flags"], name)
    c = V.counts(st)
    print(name, c)
    assert all(c[k] > 0 for s, k in (("points", "points"), ("mesh", "triangles"), ("reentry", "restored")) if s in r["stores"]), c
    _walk(ctx, p, q, w, col, r["shifts"], r["capacities"], r["colour_flags"], (name, "back to back"), every=False)


# ---- the order of the enable calls -------------------------------------------------------------------------------------------------
ORDERS = [(o, True, False) for o in itertools.permutations(V.STORES)] + [(("mesh", "reentry", "points"), False, False),
                                                                         (("reentry", "points", "mesh"), True, True)]


@pytest.mark.parametrize("order,colour_first,readers_first", ORDERS)
def test_every_order_of_the_enable_calls_gives_the_same_stores(ctx, order, colour_first, readers_first):
    """The "twice" walk with the three stores made in each of the six orders behind enable_colour, in one order in front of it (all
    three stores are then without colours, and restored voxels come back with colour word 0), and in one order behind an extract()
    and a mesh() that allocated the scratch the spills share. Whichever call comes first allocates; the bits do not depend on it."""
    p, q, w, col = V.grid()
    flags = {s: colour_first for s in V.STORES}
    st = _walk(ctx, p, q, w, col, V.TWICE, V.AMPLE, flags, (order, colour_first, readers_first), order=order, readers_first=readers_first)
    assert st[-1]["reentry"]["restored"] > 0 and len(st[-1]["mesh"]["tri"]) > 0 and (st[-1]["points"]["rgba"] is not None) == colour_first


# ---- the readers between shifts ------------------------------------------------------------------------------------------------------
def test_readers_between_shifts_see_the_models_grid_and_do_not_disturb_the_stores(ctx):
    """"Back in two pieces": behind every shift extract, mesh and raycast, all with colour, equal the same calls on a fresh volume
    without stores that was created at the model's window and uploaded the model's grid; extract and mesh write the scratch that the
    next shift's spills use, and the stores still equal the model after every later shift."""
    p, q, w, col = V.grid()
    vol = _make(ctx, p, q, w, col, V.AMPLE, V.ALL_COLOUR)
    states = V.stores_walk_model(p, q, w, col, V.TWO_PIECES, V.AMPLE, V.ALL_COLOUR, off=OFF1)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.0, 1.5, -0.4)
    behind = True
    for n, d in enumerate(V.TWO_PIECES):
        vol.shift(d)
        st = states[n + 1]
        fresh = _volume(ctx, window(p, st["off"]), colour=True)
        fresh.upload(st["q"], st["w"])
        fresh.upload_colour(st["col"])
        for tag, call in (("extract", lambda v: v.extract(1 << 12, colour=True)), ("mesh", lambda v: v.mesh(colour=True)),
                          ("raycast", lambda v: v.raycast(pose, colour=True))):
            a, b = call(vol), call(fresh)
            assert len(a) == len(b) and a[0].any(), (tag, n)
            for x, y in zip(a, b):
                assert x.shape == y.shape and x.tobytes() == y.tobytes(), (tag, n, d)
        fresh.close()
        behind = behind and st["reentry"]["live"] >= states[n]["reentry"]["live"]
        _check(vol, p, st, ("readers", n, d), behind)
    vol.close()


# ---- the timing calls ----------------------------------------------------------------------------------------------------------------
def _not_ab(*arrays):
    return sum(int((np.ascontiguousarray(a).view(np.uint8) != 0xAB).sum()) for a in arrays if a is not None)


def test_timing_calls_leave_the_volume_and_all_three_stores_as_they_are(ctx):
    """shift_time, spill_mesh_time and reentry_time behind the first shift of the "twice" walk, for a shift that is not applied. They
    write the grids' second buffers, the re-entry store's second set and the two logs behind their counted items: the grids, the
    window, every store's contents and counters read the same afterwards; the re-entry store's guards are untouched; behind the logs'
    counted items exactly the bytes of the timed spill, as the model has it, differ from the 0xAB fill (nothing further back, nothing
    in the guards); and the rest of the walk still matches the model."""
    p, q, w, col = V.grid()
    vol = _make(ctx, p, q, w, col, V.AMPLE, V.ALL_COLOUR)
    states = V.stores_walk_model(p, q, w, col, V.TWICE, V.AMPLE, V.ALL_COLOUR, off=OFF1)
    vol.shift(V.TWICE[0])
    st = states[1]
    _check(vol, p, st, "before timing")
    dt = (1, -1, 1)           # (it would push out the three faces that the first shift did not empty)
    assert all(len(us) == n and all(u > 0 for u in us) for us, n in ((vol.shift_time(dt, reps=2), 6), (vol.spill_mesh_time(dt, reps=2), 5),
                                                                      (vol.reentry_time(dt, reps=2), 5)))
    _check(vol, p, st, "after timing", intact=False)
    pw = window(p, st["off"])
    timed = spill_model(st["q"], st["w"], st["col"], pw, dt)
    n = C.c_long(-1)
    assert vol.lib.odo_debug_volume_spill_guard(vol.h, C.byref(n)) == 0
    assert len(timed[0]) > 0 and n.value == _not_ab(*timed), (n.value, _not_ab(*timed))
    fill = (len(st["mesh"]["xyz0"]), len(st["mesh"]["tri"]))
    timed = M.spill_of_mesh(mesh_model(st["q"], st["w"], pw, detail=True), mesh_colours_model(st["q"], st["w"], st["col"]), dt, p["dims"], fill)
    assert vol.lib.odo_debug_volume_spill_mesh_guard(vol.h, C.byref(n)) == 0
    assert len(timed[2]) > 0 and n.value == _not_ab(*timed), (n.value, _not_ab(*timed))
    for k in (1, 2):
        vol.shift(V.TWICE[k])
        _check(vol, p, states[k + 1], ("after timing", k), behind=False, intact=False)
    vol.close()


# ---- launch geometries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,shifts,counts", [
    ((130, 7, 9), [(3, -1, 2), (-3, 1, -2), (3, -1, 2)], dict(points=3124, vertices=14892, triangles=18824, saved=5676, restored=2838)),
    ((1024, 32, 33), [(0, 0, 1), (0, 0, -1), (0, 0, 1)], dict(points=7068, vertices=37692, triangles=46576, saved=65142, restored=32571)),
])
def test_launch_geometries_with_all_three_stores(ctx, dims, shifts, counts):
    """130 x 7 x 9: the dword build of the shift, a partial last block in every pass. 1024 x 32 x 33: the point spill, the mesh spill
    and the re-entry save all walk 1 056 blocks, more than one chunk of their scans holds. The slanted sheets of
    test_gpu_volume_spill_mesh.py give surface in every slab: the walk's three shifts append the counts stated above, the first
    and the third the same items."""
    block, chunk = _constant("kVolExtBlock"), _constant("kVolScanThreads")
    mblock, mchunk = _constant("kMeshBlock", "volume_mesh.hip.h"), _constant("kMeshScanThreads", "volume_mesh.hip.h")
    n = int(np.prod(dims))
    if dims[0] == 130:
        assert dims[0] % 4 and n % block and n % mblock and n > block
    else:
        assert -(-n // block) > chunk and -(-n // mblock) > mchunk
    p, q, w, col = GM._sheets(dims)[:4]
    caps = dict(points=1 << 14, mesh=(1 << 16, 1 << 17), reentry=1 << 16)
    st = _walk(ctx, p, q, w, col, shifts, caps, V.ALL_COLOUR, dims)
    assert V.counts(st) == counts, V.counts(st)
    assert st[-1]["points"]["dropped"] == 0 and st[-1]["mesh"]["dropped"] == (0, 0) and st[-1]["reentry"]["dropped"] == 0
    assert st[3]["spill"] == st[1]["spill"] and st[1]["spill"]["mesh"][1] > 0 and st[2]["reentry"]["live"] == 0


# ---- clearing ------------------------------------------------------------------------------------------------------------------------
def _behind(mesh, v0, t0):
    """What a mesh store emptied at (v0, t0) of the model's holds: the later items, their indices counted from the new start."""
    return dict(xyz0=mesh["xyz0"][v0:], nrmw=mesh["nrmw"][v0:], tri=mesh["tri"][t0:] - v0, rgba=mesh["rgba"][v0:], dropped=(0, 0))


def _joined(a, b):
    """The mesh store a with the store b, which began empty, appended behind it."""
    return dict(xyz0=np.concatenate([a["xyz0"], b["xyz0"]]), nrmw=np.concatenate([a["nrmw"], b["nrmw"]]),
                tri=np.concatenate([a["tri"], b["tri"] + len(a["xyz0"])]), rgba=np.concatenate([a["rgba"], b["rgba"]]), dropped=(0, 0))


def test_each_clear_empties_its_own_store_and_clear_empties_all_three(ctx):
    """"Back in two pieces" with a store emptied behind each of the first three shifts: the points behind the first, the re-entry store
    behind the second (its entries are not restored by the third, as the model continued with an empty store has it), the mesh
    behind the third. The other two stores read the same before and after each, and the next shift appends at the emptied store's
    start. clear() then empties all three and keeps the window, and the next shift appends at the start of every store."""
    p, q, w, col = V.grid()
    vol = _make(ctx, p, q, w, col, V.AMPLE, V.ALL_COLOUR)
    a = V.stores_walk_model(p, q, w, col, V.TWO_PIECES, V.AMPLE, V.ALL_COLOUR, off=OFF1)
    # the model behind the second shift, continued with an empty re-entry store (the logs' parts are joined below)
    b = V.stores_walk_model(p, a[2]["q"], a[2]["w"], a[2]["col"], V.TWO_PIECES[2:], V.AMPLE, V.ALL_COLOUR, off=a[2]["off"])
    assert a[2]["reentry"]["live"] > 0 and b[1]["reentry"]["restored"] == 0 and not V.grids_equal(a[3], b[1])
    n1 = len(a[1]["points"]["xyz0"])
    cut = lambda s, n: dict(s, xyz0=s["xyz0"][n:], nrmw=s["nrmw"][n:], rgba=s["rgba"][n:])
    cat = lambda s, t: dict(s, xyz0=np.concatenate([s["xyz0"], t["xyz0"]]), nrmw=np.concatenate([s["nrmw"], t["nrmw"]]),
                            rgba=np.concatenate([s["rgba"], t["rgba"]]))
    empty_p, empty_m, empty_r = V.empty_points(True), M.empty_store(True), R.empty_store(True)
    vol.shift(V.TWO_PIECES[0])
    _check(vol, p, a[1], "shift 1")
    got = vol.spilled(clear=True, colour=True)
    assert len(got[0]) == n1 > 0 and got[0].tobytes() == a[1]["points"]["xyz0"].tobytes()
    _check(vol, p, dict(a[1], points=empty_p), "the points emptied", intact=False)
    vol.shift(V.TWO_PIECES[1])
    assert len(a[2]["points"]["xyz0"]) > n1
    _check(vol, p, dict(a[2], points=cut(a[2]["points"], n1)), "shift 2", intact=False)
    got = vol.stored_voxels(clear=True, colour=True)
    assert len(got[0]) == a[2]["reentry"]["live"] and np.array_equal(got[0], a[2]["reentry"]["g"])
    _check(vol, p, dict(a[2], points=cut(a[2]["points"], n1), reentry=empty_r), "the re-entry store emptied", behind=False, intact=False)
    vol.shift(V.TWO_PIECES[2])
    points = cat(cut(a[2]["points"], n1), b[1]["points"])
    mesh = _joined(a[2]["mesh"], b[1]["mesh"])
    _check(vol, p, dict(b[1], points=points, mesh=mesh), "shift 3", behind=False, intact=False)
    got = vol.spilled_mesh(clear=True, colour=True)
    assert len(got[0]) == len(mesh["xyz0"]) and np.array_equal(got[2], mesh["tri"])
    _check(vol, p, dict(b[1], points=points, mesh=empty_m), "the mesh emptied", behind=False, intact=False)
    vol.shift(V.TWO_PIECES[3])
    assert len(b[1]["mesh"]["xyz0"]) > 0 and len(b[2]["mesh"]["tri"]) > len(b[1]["mesh"]["tri"])
    _check(vol, p, dict(b[2], points=cat(cut(a[2]["points"], n1), b[2]["points"]),
                        mesh=_behind(b[2]["mesh"], len(b[1]["mesh"]["xyz0"]), len(b[1]["mesh"]["tri"]))), "shift 4", behind=False, intact=False)
    # clear(): all three empty, the grids zero, the window where it was
    vol.clear()
    zero = dict(q=np.zeros_like(q), w=np.zeros_like(w), col=np.zeros_like(col), off=b[2]["off"], points=empty_p, mesh=empty_m, reentry=empty_r)
    _check(vol, p, zero, "clear()", behind=False, intact=False)
    vol.upload(q, w)
    vol.upload_colour(col)
    c = V.stores_walk_model(p, q, w, col, [V.D], V.AMPLE, V.ALL_COLOUR, off=b[2]["off"])
    vol.shift(V.D)
    assert min(V.counts(c)[k] for k in ("points", "triangles", "saved")) > 0
    _check(vol, p, c[1], "the shift after clear()", behind=False, intact=False)
    vol.close()


# ---- attached to a tracker -----------------------------------------------------------------------------------------------------------
def test_attached_tracker_on_an_out_and_back_drive_with_all_three_stores(ctx):
    """The out-and-back drive of test_gpu_volume_reentry.py with the three stores on the attached volume. The tracker's rows are the
    bits of a run without a store; the stores, the grid, the window and the stats are those of a standalone volume with the same
    three stores fed the returned poses through follow + integrate; and each store is that of a standalone volume with that store
    and the re-entry store only, the paths the single-store tests hold to the model on this drive."""
    from odometry_amd import api
    c, seq, p, order = _drive()
    size = (c["rows"], c["cols"])
    focus, threshold = 5.8, 3
    caps = dict(points=1 << 18, mesh=(1 << 20, 1 << 21), reentry=1 << 19)

    def stores(vol, which):
        for s in which:
            _enable(vol, s, caps)
        vol.set_follow(focus, threshold)
        return vol

    def run(which):
        trk = api.RgbdTracker(0, **S.tracker_args(c))
        vol = stores(_volume(trk, p), which)
        trk.attach_volume(vol)
        dev = [(trk.upload_frame(seq["gray"][k]), trk.upload_depth(seq["depth"][k])) for k in order]
        return trk, vol, dev, _run(trk, dev, size)

    def read(vol, which):
        out = {}
        if "points" in which:
            out["points"] = vol.spilled(with_dropped=True)
        if "mesh" in which:
            out["mesh"] = vol.spilled_mesh(with_dropped=True)
        if "reentry" in which:
            out["reentry"] = vol.stored_voxels() + (vol.reentry_stats(),)
        return out

    def same(a, b):
        return len(a) == len(b) and all(x.tobytes() == y.tobytes() if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))

    trk0, vol0, _, want = run(())
    vol0.close()
    trk0.close()
    trk, vol, dev, got = run(V.STORES)
    _rows_equal(got, want, "three stores")
    refs = {which: stores(_volume(trk, p), which) for which in (V.STORES, ("points", "reentry"), ("mesh", "reentry"), ("reentry",))}
    off, fwd, back = (0, 0, 0), 0, 0
    for (_, d), r in zip(dev, got):
        want_d = follow_model(r["abs_pose"], p, off, focus, threshold)
        for ref in refs.values():
            assert ref.follow(r["abs_pose"]) == want_d
            ref.integrate(d, r["abs_pose"])
        off = offset_model(off, want_d)
        fwd += want_d[2] > 0
        back += want_d[2] < 0
    assert fwd >= 3 and back >= 3
    mine = read(vol, V.STORES)
    print("points", len(mine["points"][0]), "vertices", len(mine["mesh"][0]), "triangles", len(mine["mesh"][2]), mine["reentry"][-1])
    assert len(mine["points"][0]) > 0 and len(mine["mesh"][2]) > 0 and mine["mesh"][2].max() < len(mine["mesh"][0])
    assert mine["points"][-1] == 0 and mine["mesh"][-1] == (0, 0) and mine["reentry"][-1]["dropped"] == 0 and mine["reentry"][-1]["restored"] > 0
    for which, ref in refs.items():
        assert vol.window()[0] == off == ref.window()[0] and vol.window()[1].tobytes() == ref.window()[1].tobytes(), which
        assert all(np.array_equal(x, y) for x, y in zip(vol.grid(), ref.grid())), which
        assert vol.stats() == ref.stats(), which
        theirs = read(ref, which)
        for s in which:
            assert same(mine[s], theirs[s]), (which, s)
        ref.close()
    assert _guard_intact(vol) and GM._guard_intact(vol) and _guards(vol)[1] == 0
    vol.close()
    trk.close()
