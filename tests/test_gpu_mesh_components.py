"""The mesh component filter on the GPU (odo_mesh_components_*, api.MeshComponents, api.TsdfVolume.cleaned_mesh /
save_cleaned_mesh_ply) against the numpy model of tests/mesh_components_cases.py: every row of the table bit for bit — vertices,
attributes, triangles, labels and all counters, no tolerance, guard == 0 — from inputs held between 64 guarded items of 0xAB either
side, which are unchanged afterwards, into the filter's own result buffers, which were filled with 0xAB and stay so beyond the input's
counts; two runs the same bytes; one filter reused across all rows forwards and backwards; the drive's welded mesh at both grid
counts; every refusal on a live filter with the result and the statistics unchanged after it; two filters on one context, destroy
with runs in flight, the timing call; and the volume's convenience against the model on the volume's own store and mesh, through the
PLY reader."""
import ctypes as C

import numpy as np
import pytest

import mesh_components_cases as mc
import mesh_weld_cases as wc
from test_gpu_mesh_weld import DTYPE, GUARD, ITEM, Held, read_ply_mesh_rgb

pytestmark = pytest.mark.gpu
ZERO = dict.fromkeys(mc.STATS, 0)


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _run_dev(f, held, rule):
    f.run_dev(held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], held.p["tri"], held.p["rgba"], min_triangles=rule["min_triangles"],
              keep_largest=rule["keep_largest"], drop_unreferenced=rule["drop"])


def _result_bytes(ctx, f, capacity, colour):
    """The whole of the filter's result arrays (capacity items each, not the result's counts alone), and the counts."""
    x, n, c, t, nv, nt = f.result_dev()
    out = dict(xyz0=ctx.download(x, (capacity[0] * 16,), np.uint8), nrmw=ctx.download(n, (capacity[0] * 16,), np.uint8),
               tri=ctx.download(t, (capacity[1] * 12,), np.uint8))
    if colour:
        assert c is not None
        out["rgba"] = ctx.download(c, (capacity[0] * 4,), np.uint8)
    else:
        assert c is None
    return out, nv, nt


def _fill_result(ctx, f, capacity, colour):
    x, n, c, t, _, _ = f.result_dev()
    for p, nbytes in ((x, capacity[0] * 16), (n, capacity[0] * 16), (c if colour else None, capacity[0] * 4), (t, capacity[1] * 12)):
        if p is not None:
            blob = np.full(nbytes, 0xAB, np.uint8)
            ctx.lib.odo_dev_upload(ctx.h, p, blob.ctypes.data_as(C.c_void_p), blob.nbytes)


def _equals_model(got, M, what):
    assert (len(got["xyz0"]), len(got["tri"])) == (len(M["xyz0"]), len(M["tri"])), (what, len(got["xyz0"]), len(got["tri"]), M["stats"])
    assert np.array_equal(wc.bits(got["xyz0"]), wc.bits(M["xyz0"])), f"{what}: positions differ"
    assert np.array_equal(wc.bits(got["nrmw"]), wc.bits(M["nrmw"])), f"{what}: normals / weights differ"
    assert np.array_equal(got["tri"], M["tri"]), (what, np.argwhere(got["tri"] != M["tri"])[:4])
    if M["rgba"] is not None:
        assert np.array_equal(got["rgba"], M["rgba"]), f"{what}: colours differ"
    if "labels" in got:
        assert np.array_equal(got["labels"], M["labels"]), (what, np.argwhere(got["labels"] != M["labels"])[:4])


def _capacity(r):
    if r["name"].startswith("256 edges homed"):
        return r["capacity"]                                                       # (the table the edges were designed for)
    return len(r["mesh"]["xyz0"]) + GUARD, len(r["mesh"]["tri"]) + GUARD


@pytest.mark.parametrize("index", range(len(mc.rows())), ids=mc.row_ids())
def test_every_row_bit_for_bit(ctx, index):
    from odometry_amd import api
    r = mc.rows()[index]
    m, rule, M = r["mesh"], r["rule"], mc.model_of(index)
    colour = m["rgba"] is not None
    cap = _capacity(r)
    f = api.MeshComponents(ctx, cap[0], cap[1], colour=colour)
    assert f.stats() == ZERO and f.result_dev()[4:] == (0, 0) and len(f.labels()) == 0         # before the first run
    held = Held(ctx, m)
    _run_dev(f, held, rule)                                                         # (the first run: where the result lies)
    _fill_result(ctx, f, cap, colour)
    seen = []
    for _ in range(2):
        _run_dev(f, held, rule)
        raw, nv, nt = _result_bytes(ctx, f, cap, colour)
        assert (nv, nt) == (len(M["xyz0"]), len(M["tri"])), (r["name"], nv, nt, f.stats())
        for k in raw:
            n, n_in = (nt, held.n_t) if k == "tri" else (nv, held.n_v)
            want = np.ascontiguousarray(M[k], DTYPE[k]).reshape(-1).view(np.uint8)
            assert np.array_equal(raw[k][:n * ITEM[k]], want), (r["name"], k)
            assert (raw[k][n_in * ITEM[k]:] == 0xAB).all(), f"{r['name']}: {k} written beyond the input's count"
        assert f.stats() == M["stats"], (r["name"], f.stats(), M["stats"])
        labels = f.labels()
        assert np.array_equal(labels, M["labels"]), (r["name"], np.argwhere(labels != M["labels"])[:4])
        p, n = f.labels_dev()
        assert n == held.n_t and (n == 0 or np.array_equal(ctx.download(p, (n,), np.int32), M["labels"]))
        assert held.unchanged(), r["name"]
        seen.append(dict({k: v.tobytes() for k, v in raw.items()}, labels=labels.tobytes()))
    assert seen[0] == seen[1], r["name"]
    _equals_model(f.download(colour=colour), M, r["name"])
    f.close()
    held.free()


def test_one_filter_reused_across_all_rows(ctx):
    """Rows of different sizes through one filter, host arrays in and out, forwards and backwards: nothing is carried in the parent
    array, the sizes, the edge table or the counters. The same through a filter without edge statistics: its six edge counters are
    0, everything else is the same."""
    from odometry_amd import api
    f = api.MeshComponents(ctx, 4352, 4352, colour=True)
    bare = api.MeshComponents(ctx, 4352, 4352, colour=True, edge_stats=False)
    assert f.stats() == ZERO and bare.stats() == ZERO
    order = list(range(len(mc.rows())))
    for index in order + order[::-1]:
        r, M = mc.rows()[index], mc.model_of(index)
        rule = r["rule"]
        for filt, edges in ((f, True), (bare, False)):
            got = filt.run(r["mesh"]["xyz0"], r["mesh"]["nrmw"], r["mesh"]["tri"], rgba=r["mesh"]["rgba"], min_triangles=rule["min_triangles"],
                           keep_largest=rule["keep_largest"], drop_unreferenced=rule["drop"])
            _equals_model(got, M, r["name"])
            want = {k: (v if edges or k not in mc.EDGE_STATS else 0) for k, v in M["stats"].items()}
            assert got["stats"] == want and ("rgba" in got) == (M["rgba"] is not None), (r["name"], got["stats"], want)
    f.close()
    bare.close()


@pytest.fixture(scope="module")
def drive(ctx):
    held = {g: Held(ctx, mc.drive_welded(g)) for g in (8, 1)}
    yield held
    for h in held.values():
        h.free()


@pytest.mark.parametrize("grids", [8, 1])
def test_the_drives_welded_mesh_is_the_models_bytes(ctx, drive, grids):
    from odometry_amd import api
    held = drive[grids]
    f = api.MeshComponents(ctx, held.n_v, held.n_t)
    for min_triangles in (0, 128):
        M = mc.drive_components(grids, min_triangles)
        _run_dev(f, held, dict(min_triangles=min_triangles, keep_largest=False, drop=True))
        _equals_model(dict(f.download(), labels=f.labels()), M, f"drive, grids {grids}, min_triangles {min_triangles}")
        assert f.stats() == M["stats"], (f.stats(), M["stats"])
        print(f"grids {grids}, min_triangles {min_triangles}: {f.stats()}")
    largest = mc.components_model(mc.drive_welded(grids), 0, keep_largest=True)
    _run_dev(f, held, dict(min_triangles=0, keep_largest=True, drop=True))
    _equals_model(dict(f.download(), labels=f.labels()), largest, f"drive, grids {grids}, the largest alone")
    assert f.stats() == largest["stats"] and f.stats()["triangles_out"] == mc.DRIVE[grids]["sizes"][-1]
    assert held.unchanged()
    f.close()


def test_refusals_leave_the_result_and_the_statistics_unchanged(ctx):
    """Every refusal on a live filter: the bounds of create with a live context, every bad rule, counts beyond the capacities,
    colours on a filter without colour, misaligned and NULL pointers, an input inside the filter's own buffers, bad reps, a download
    into capacities below the counts: -1 with a message, and the result, the labels and the statistics are what they were."""
    from odometry_amd import _lib as L_, api
    from test_mesh_components_cpu import bad_sets, c_rule
    lib = L_.load()
    index = mc.row_ids().index("257 triangles")
    r, M = mc.rows()[index], mc.model_of(index)
    held = Held(ctx, r["mesh"])
    coloured = Held(ctx, mc.rows()[mc.row_ids().index("a coloured mesh")]["mesh"])
    f = api.MeshComponents(ctx, 300, 700)
    _run_dev(f, held, r["rule"])

    def unchanged(what):
        _equals_model(dict(f.download(), labels=f.labels()), M, what)
        assert f.stats() == M["stats"] and held.unchanged(), what

    unchanged("the run itself")
    for what, s, check, _, word in bad_sets():
        if check == 0:
            h, p = C.c_void_p(0x5A5A), L_.MeshComponentsParams(s["vcap"], s["tcap"], s["colour"], s["edges"])
            assert lib.odo_mesh_components_create(ctx.h, C.byref(p), C.byref(h)) == -1 and h.value == 0x5A5A, what
        else:
            n_v = 301 if what == "n_v beyond the capacity" else s["n_v"]
            n_t = 701 if what == "n_t beyond the capacity" else s["n_t"]
            rule = c_rule(s["min_triangles"], s["keep"], s["drop"])
            assert lib.odo_mesh_components_run_dev(f.h, C.byref(rule), n_v, n_t, held.p["xyz0"], held.p["nrmw"], None, held.p["tri"]) == -1, what
        assert word in L_.last_error(), (what, L_.last_error())
        unchanged(what)
    good = c_rule(r["rule"]["min_triangles"], int(r["rule"]["keep_largest"]), int(r["rule"]["drop"]))
    x, n, _, t, nv, nt = f.result_dev()
    lab, n_lab = f.labels_dev()
    off = lambda ptr, k: C.c_void_p(ptr.value + k)
    us = (C.c_float * 7)(*[7.0] * 7)
    cnt = (C.c_long(7), C.c_long(7))
    small = np.zeros((nv, 4), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    run = lambda *a: lib.odo_mesh_components_run_dev(f.h, C.byref(good), held.n_v, held.n_t, *a)
    time = lambda reps, us_, x_=None: lib.odo_mesh_components_time_dev(f.h, C.byref(good), held.n_v, held.n_t, x_ or held.p["xyz0"], held.p["nrmw"],
                                                                       None, held.p["tri"], reps, us_)
    calls = [("filter NULL", lambda: lib.odo_mesh_components_run_dev(None, C.byref(good), held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], None, held.p["tri"])),
             ("rule NULL", lambda: lib.odo_mesh_components_run_dev(f.h, None, held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], None, held.p["tri"])),
             ("xyz0 NULL", lambda: run(None, held.p["nrmw"], None, held.p["tri"])),
             ("nrmw NULL", lambda: run(held.p["xyz0"], None, None, held.p["tri"])),
             ("tri NULL", lambda: run(held.p["xyz0"], held.p["nrmw"], None, None)),
             ("xyz0 misaligned", lambda: run(off(held.p["xyz0"], 4), held.p["nrmw"], None, held.p["tri"])),
             ("nrmw misaligned", lambda: run(held.p["xyz0"], off(held.p["nrmw"], 8), None, held.p["tri"])),
             ("tri misaligned", lambda: run(held.p["xyz0"], held.p["nrmw"], None, off(held.p["tri"], 2))),
             ("rgba misaligned", lambda: run(held.p["xyz0"], held.p["nrmw"], off(coloured.p["rgba"], 1), held.p["tri"])),
             ("colours on a filter without colour", lambda: run(held.p["xyz0"], held.p["nrmw"], coloured.p["rgba"], held.p["tri"])),
             ("xyz0 is the filter's own result", lambda: run(x, held.p["nrmw"], None, held.p["tri"])),
             ("nrmw ends inside the filter's block", lambda: run(held.p["xyz0"], off(x, 16 - 16 * held.n_v), None, held.p["tri"])),
             ("tri is the filter's own result", lambda: run(held.p["xyz0"], held.p["nrmw"], None, t)),
             ("tri is the filter's own labels", lambda: run(held.p["xyz0"], held.p["nrmw"], None, lab)),
             ("time: reps 0", lambda: time(0, us)), ("time: reps 10001", lambda: time(10001, us)), ("time: us NULL", lambda: time(3, None)),
             ("time: an input of the filter's own", lambda: time(3, us, x)),
             ("stats NULL", lambda: lib.odo_mesh_components_stats(f.h, None)),
             ("labels: one short", lambda: lib.odo_mesh_components_labels(f.h, n_lab - 1, vp(small), C.byref(cnt[0]))),
             ("download: a vertex short", lambda: lib.odo_mesh_components_download(f.h, nv - 1, nt, vp(small), vp(small), None, vp(small), C.byref(cnt[0]), C.byref(cnt[1]))),
             ("download: a triangle short", lambda: lib.odo_mesh_components_download(f.h, nv, nt - 1, vp(small), vp(small), None, vp(small), C.byref(cnt[0]), C.byref(cnt[1]))),
             ("download: colours of a run without", lambda: lib.odo_mesh_components_download(f.h, nv, nt, vp(small), vp(small), vp(small), vp(small), C.byref(cnt[0]), C.byref(cnt[1])))]
    for what, call in calls:
        assert call() == -1 and L_.last_error(), what
        assert list(us) == [7.0] * 7, what
        unchanged(what)
    assert not small.any() and n_lab == held.n_t                                    # a refused download copies nothing
    with pytest.raises(L_.OdoError):
        f.run_dev(301, held.n_t, held.p["xyz0"], held.p["nrmw"], held.p["tri"], min_triangles=1)
    with pytest.raises(L_.OdoError):
        api.MeshComponents(ctx, 0, 8)
    with pytest.raises(ValueError):
        f.run(r["mesh"]["xyz0"], r["mesh"]["nrmw"], r["mesh"]["tri"])               # no min_triangles
    unchanged("api")
    f.close()
    f.close()                                                                       # twice is harmless
    held.free()
    coloured.free()


def test_two_filters_on_one_context(ctx):
    """Enqueued alternately, nothing waited for in between: each has its own arrays, table, buffers and statistics."""
    from odometry_amd import api
    ia, ib = mc.row_ids().index("255 triangles"), mc.row_ids().index("a coloured mesh")
    ra, rb = mc.rows()[ia], mc.rows()[ib]
    ha, hb = Held(ctx, ra["mesh"]), Held(ctx, rb["mesh"])
    fa, fb = api.MeshComponents(ctx, 400, 800), api.MeshComponents(ctx, 300, 700, colour=True)
    for _ in range(4):
        _run_dev(fa, ha, ra["rule"])
        _run_dev(fb, hb, rb["rule"])
    _equals_model(dict(fb.download(colour=True), labels=fb.labels()), mc.model_of(ib), "b")
    _equals_model(dict(fa.download(), labels=fa.labels()), mc.model_of(ia), "a")
    assert fa.stats() == mc.model_of(ia)["stats"] and fb.stats() == mc.model_of(ib)["stats"]
    fa.close()
    fb.close()
    ha.free()
    hb.free()


def test_destroy_with_ten_runs_in_flight_and_the_timing_call(ctx, drive):
    """Ten runs of the drive's welded mesh enqueued and the filter destroyed at once: destroy waits, and the context goes on. The
    timing call leaves exactly one run's result, labels and statistics."""
    from odometry_amd import api
    held = drive[8]
    rule = dict(min_triangles=128, keep_largest=False, drop=True)
    f = api.MeshComponents(ctx, held.n_v, held.n_t)
    for _ in range(10):
        _run_dev(f, held, rule)
    f.close()
    assert held.unchanged()
    f = api.MeshComponents(ctx, held.n_v, held.n_t)
    us = f.time(held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], held.p["tri"], min_triangles=128, reps=3)
    print({k: round(v, 1) for k, v in us.items()})
    assert list(us) == list(api.MeshComponents.GROUPS) and all(v > 0.0 for v in us.values())
    assert abs(us["run"] - sum(v for k, v in us.items() if k != "run")) <= 1e-3 * us["run"]
    M = mc.drive_components(8, 128)
    _equals_model(dict(f.download(), labels=f.labels()), M, "after the timing call")
    assert f.stats() == M["stats"] and held.unchanged()
    f.close()


def test_the_volumes_cleaned_mesh_and_its_ply(ctx, tmp_path):
    """A volume with a mesh store, a re-entry store and colours after the d, -d, d walk of tests/volume_stores_cases.py:
    cleaned_mesh equals components_model(weld_model(spilled_mesh() + mesh())), coloured and plain, at a min_triangles taken from the
    model's sizes so that at least one component leaves and one stays; save_cleaned_mesh_ply round-trips through the PLY reader;
    welded_mesh returns what it returned."""
    import volume_stores_cases as VS
    from test_gpu_volume_shift import _volume
    p, q, w, col = VS.grid()
    vol = _volume(ctx, p, colour=True)
    vol.enable_spill_mesh(1 << 14, 1 << 14)
    vol.enable_reentry(1 << 16)
    vol.upload(q, w)
    vol.upload_colour(col)
    for d in VS.TWICE:
        vol.shift(d)
    store, win = vol.spilled_mesh(colour=True), vol.mesh(colour=True)
    both = dict(xyz0=np.concatenate([store[0], win[0]]), nrmw=np.concatenate([store[1], win[1]]),
                tri=np.concatenate([store[2], win[2] + len(store[0])]).astype(np.int32), rgba=np.concatenate([store[3], win[3]]))
    eps = np.float32(p["vs"]) / np.float32(64.0)
    W = wc.weld_model(both, eps, p["origin"], 8)
    sizes = sorted(mc.components_model(W, 0)["sizes"].tolist())
    assert len(sizes) >= 2 and sizes[0] < sizes[-1], sizes
    bound = sizes[-1]                                                              # the largest stays, at equality; the smallest leaves
    M = mc.components_model(W, bound)
    assert 0 < M["stats"]["removed_components"] < M["stats"]["components"] and 0 < M["stats"]["triangles_out"] < M["stats"]["triangles_in"]
    got = vol.cleaned_mesh(colour=True, min_triangles=bound)
    _equals_model(got, M, "store + window, coloured")
    assert got["stats"] == M["stats"] and got["weld_stats"] == W["stats"]
    W1 = wc.weld_model(dict(both, rgba=None), eps, p["origin"], 1)
    M1 = mc.components_model(W1, 0, keep_largest=True)
    plain = vol.cleaned_mesh(grids=1, min_triangles=0, keep_largest=True)
    _equals_model(plain, M1, "store + window, one grid, the largest alone")
    assert "rgba" not in plain and plain["stats"] == M1["stats"] and plain["weld_stats"] == W1["stats"]
    default = vol.cleaned_mesh()                                                   # min_triangles = 128
    _equals_model(default, mc.components_model(dict(W, rgba=None), 128), "the default bound")
    welded = vol.welded_mesh(colour=True)                                          # as it was
    assert welded["stats"] == W["stats"] and np.array_equal(welded["tri"], W["tri"]) and np.array_equal(wc.bits(welded["xyz0"]), wc.bits(W["xyz0"]))
    assert np.array_equal(welded["rgba"], W["rgba"]) and sorted(welded) == ["nrmw", "rgba", "stats", "tri", "xyz0"]
    path = str(tmp_path / "cleaned.ply")
    stats = vol.save_cleaned_mesh_ply(path, min_triangles=bound)
    V, T = read_ply_mesh_rgb(path)
    assert stats == M["stats"] and np.array_equal(T, M["tri"])
    assert np.array_equal(wc.bits(V[0]), wc.bits(M["xyz0"][:, :3])) and np.array_equal(wc.bits(V[1]), wc.bits(M["nrmw"][:, :3]))
    assert np.array_equal(V[2], M["rgba"][:, :3])
    vol.close()
