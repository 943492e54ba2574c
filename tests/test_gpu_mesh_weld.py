"""The mesh welder on the GPU (odo_mesh_weld_*, api.MeshWeld, api.TsdfVolume.welded_mesh / save_welded_mesh_ply) against the numpy
model of tests/mesh_weld_cases.py: every row of the table bit for bit — vertices, attributes, triangles and all counters, no
tolerance, guard == 0 — from inputs held between 64 guarded items of 0xAB either side, which are unchanged afterwards, into the
welder's own result buffers, whose 64 items beyond the input's counts were filled with 0xAB and stay so; two runs the same bytes; one
welder reused across all rows; the drive's mesh at one and eight grids; every refusal on a live welder with the result and the
statistics unchanged after it; two welders on one context, destroy with runs in flight, the timing call; and the volume's
convenience against the model on the volume's own store and mesh, through the PLY reader."""
import ctypes as C

import numpy as np
import pytest

import mesh_weld_cases as wc

pytestmark = pytest.mark.gpu
ZERO = dict.fromkeys(wc.STATS, 0)
GUARD = 64                                        # items either side of an input, and behind a result
ITEM = dict(xyz0=16, nrmw=16, rgba=4, tri=12)
DTYPE = dict(xyz0=np.float32, nrmw=np.float32, rgba=np.uint8, tri=np.int32)


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


class Held:
    """A mesh's arrays on the device, each between GUARD items of 0xAB either side."""

    def __init__(self, ctx, mesh):
        self.ctx, self.mesh, self.blobs, self.base, self.p = ctx, mesh, {}, {}, {}
        for k in ("xyz0", "nrmw", "rgba", "tri"):
            if mesh[k] is None:
                self.p[k] = None
                continue
            body = np.ascontiguousarray(mesh[k], DTYPE[k]).reshape(-1).view(np.uint8)
            margin = np.full(GUARD * ITEM[k] + (4 if k == "tri" else 0), 0xAB, np.uint8)   # (768 + 4: the triangles 4-byte aligned only)
            blob = np.concatenate([margin, body, margin])
            self.blobs[k], self.base[k] = blob, ctx.upload(blob)
            self.p[k] = C.c_void_p(self.base[k].value + len(margin))
        self.n_v, self.n_t = len(mesh["xyz0"]), len(mesh["tri"])

    def unchanged(self):
        return all(np.array_equal(self.ctx.download(self.base[k], (len(b),), np.uint8), b) for k, b in self.blobs.items())

    def free(self):
        for b in self.base.values():
            self.ctx.free(b)


def _run_dev(w, held, rule):
    w.run_dev(held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], held.p["tri"], held.p["rgba"], eps=rule["eps"], origin=rule["origin"],
              grids=rule["grids"], drop_unreferenced=rule["drop"])


def _result_bytes(ctx, w, capacity, colour):
    """The whole of the welder's result arrays (capacity items each, not the result's counts alone), and the counts."""
    x, n, c, t, nv, nt = w.result_dev()
    out = dict(xyz0=ctx.download(x, (capacity[0] * 16,), np.uint8), nrmw=ctx.download(n, (capacity[0] * 16,), np.uint8),
               tri=ctx.download(t, (capacity[1] * 12,), np.uint8))
    if colour:
        assert c is not None
        out["rgba"] = ctx.download(c, (capacity[0] * 4,), np.uint8)
    else:
        assert c is None
    return out, nv, nt


def _fill_result(ctx, w, capacity, colour):
    x, n, c, t, _, _ = w.result_dev()
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


def _capacity(r):
    if r["name"].startswith("256 keys homed"):
        return r["capacity"]                                                       # (the table the keys were designed for)
    return len(r["mesh"]["xyz0"]) + GUARD, len(r["mesh"]["tri"]) + GUARD


@pytest.mark.parametrize("index", range(len(wc.rows())), ids=wc.row_ids())
def test_every_row_bit_for_bit(ctx, index):
    from odometry_amd import api
    r = wc.rows()[index]
    m, rule, M = r["mesh"], r["rule"], wc.model_of(index)
    colour = m["rgba"] is not None
    cap = _capacity(r)
    w = api.MeshWeld(ctx, cap[0], cap[1], colour=colour)
    assert w.stats() == ZERO and w.result_dev()[4:] == (0, 0)                       # before the first run
    held = Held(ctx, m)
    _run_dev(w, held, rule)                                                         # (the first run: where the result lies)
    _fill_result(ctx, w, cap, colour)
    seen = []
    for _ in range(2):
        _run_dev(w, held, rule)
        raw, nv, nt = _result_bytes(ctx, w, cap, colour)
        assert (nv, nt) == (len(M["xyz0"]), len(M["tri"])), (r["name"], nv, nt, w.stats())
        for k in raw:
            n, n_in = (nt, held.n_t) if k == "tri" else (nv, held.n_v)
            want = np.ascontiguousarray(M[k], DTYPE[k]).reshape(-1).view(np.uint8)
            assert np.array_equal(raw[k][:n * ITEM[k]], want), (r["name"], k)
            assert (raw[k][n_in * ITEM[k]:] == 0xAB).all(), f"{r['name']}: {k} written beyond the input's count"
        assert w.stats() == M["stats"], (r["name"], w.stats(), M["stats"])
        assert held.unchanged(), r["name"]
        seen.append({k: v.tobytes() for k, v in raw.items()})
    assert seen[0] == seen[1], r["name"]
    _equals_model(w.download(colour=colour), M, r["name"])
    w.close()
    held.free()


def test_one_welder_reused_across_all_rows(ctx):
    """Rows of different sizes through one welder, host arrays in and out, forwards and backwards: nothing is carried in the tables, the
    scratch or the counters."""
    from odometry_amd import api
    w = api.MeshWeld(ctx, 2048, 2048, colour=True)
    order = list(range(len(wc.rows())))
    for index in order + order[::-1]:
        r, M = wc.rows()[index], wc.model_of(index)
        rule = r["rule"]
        got = w.run(r["mesh"]["xyz0"], r["mesh"]["nrmw"], r["mesh"]["tri"], rgba=r["mesh"]["rgba"], eps=rule["eps"], origin=rule["origin"],
                    grids=rule["grids"], drop_unreferenced=rule["drop"])
        _equals_model(got, M, r["name"])
        assert got["stats"] == M["stats"] and ("rgba" in got) == (M["rgba"] is not None), (r["name"], got["stats"])
    w.close()


@pytest.fixture(scope="module")
def drive(ctx):
    m, p, _ = wc.drive_mesh()
    held = Held(ctx, m)
    yield m, p, held
    held.free()


@pytest.mark.parametrize("grids", [1, 8])
def test_the_drive_mesh_is_the_models_bytes(ctx, drive, grids):
    from odometry_amd import api
    m, p, held = drive
    M = wc.drive_model(grids)
    w = api.MeshWeld(ctx, held.n_v, held.n_t)
    _run_dev(w, held, dict(eps=np.float32(p["vs"]) / np.float32(64.0), origin=p["origin"], grids=grids, drop=True))
    _equals_model(w.download(), M, f"drive, grids {grids}")
    assert w.stats() == M["stats"], (w.stats(), M["stats"])
    assert held.unchanged()
    print(f"grids {grids}: {w.stats()}")
    w.close()


def test_refusals_leave_the_result_and_the_statistics_unchanged(ctx):
    """Every refusal on a live welder: the bounds of create with a live context, every bad rule, counts beyond the capacities,
    colours on a welder without colour, misaligned and NULL pointers, an input inside the welder's own buffers, bad reps, a download
    into capacities below the counts: -1 with a message, and the result and the statistics are what they were."""
    from odometry_amd import _lib as L_, api
    from test_mesh_weld_cpu import bad_sets, c_rule
    lib = L_.load()
    index = wc.row_ids().index("257 vertices, 600 triangles")
    r, M = wc.rows()[index], wc.model_of(index)
    held = Held(ctx, r["mesh"])
    coloured = Held(ctx, wc.rows()[wc.row_ids().index("a coloured mesh")]["mesh"])
    w = api.MeshWeld(ctx, 300, 700)
    _run_dev(w, held, r["rule"])

    def unchanged(what):
        _equals_model(w.download(), M, what)
        assert w.stats() == M["stats"] and held.unchanged(), what

    unchanged("the run itself")
    for what, s, check, _, word in bad_sets():
        if check == 0:
            h, p = C.c_void_p(0x5A5A), L_.MeshWeldParams(s["vcap"], s["tcap"], s["colour"])
            assert lib.odo_mesh_weld_create(ctx.h, C.byref(p), C.byref(h)) == -1 and h.value == 0x5A5A, what
        else:
            n_v = 301 if what == "n_v beyond the capacity" else s["n_v"]
            n_t = 701 if what == "n_t beyond the capacity" else s["n_t"]
            rule = c_rule(s["eps"], s["origin"], s["grids"], s["drop"])
            assert lib.odo_mesh_weld_run_dev(w.h, C.byref(rule), n_v, n_t, held.p["xyz0"], held.p["nrmw"], None, held.p["tri"]) == -1, what
        assert word in L_.last_error(), (what, L_.last_error())
        unchanged(what)
    good = c_rule(r["rule"]["eps"], r["rule"]["origin"], r["rule"]["grids"], int(r["rule"]["drop"]))
    x, n, _, t, nv, nt = w.result_dev()
    off = lambda ptr, k: C.c_void_p(ptr.value + k)
    us = (C.c_float * 7)(*[7.0] * 7)
    cnt = (C.c_long(7), C.c_long(7))
    small = np.zeros((nv, 4), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    run = lambda *a: lib.odo_mesh_weld_run_dev(w.h, C.byref(good), held.n_v, held.n_t, *a)
    calls = [("welder NULL", lambda: lib.odo_mesh_weld_run_dev(None, C.byref(good), held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], None, held.p["tri"])),
             ("rule NULL", lambda: lib.odo_mesh_weld_run_dev(w.h, None, held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], None, held.p["tri"])),
             ("xyz0 NULL", lambda: run(None, held.p["nrmw"], None, held.p["tri"])),
             ("nrmw NULL", lambda: run(held.p["xyz0"], None, None, held.p["tri"])),
             ("tri NULL", lambda: run(held.p["xyz0"], held.p["nrmw"], None, None)),
             ("xyz0 misaligned", lambda: run(off(held.p["xyz0"], 4), held.p["nrmw"], None, held.p["tri"])),
             ("nrmw misaligned", lambda: run(held.p["xyz0"], off(held.p["nrmw"], 8), None, held.p["tri"])),
             ("tri misaligned", lambda: run(held.p["xyz0"], held.p["nrmw"], None, off(held.p["tri"], 2))),
             ("rgba misaligned", lambda: run(held.p["xyz0"], held.p["nrmw"], off(coloured.p["rgba"], 1), held.p["tri"])),
             ("colours on a welder without colour", lambda: run(held.p["xyz0"], held.p["nrmw"], coloured.p["rgba"], held.p["tri"])),
             ("xyz0 is the welder's own result", lambda: run(x, held.p["nrmw"], None, held.p["tri"])),
             ("nrmw ends inside the welder's block", lambda: run(held.p["xyz0"], off(x, 16 - 16 * held.n_v), None, held.p["tri"])),
             ("tri is the welder's own result", lambda: run(held.p["xyz0"], held.p["nrmw"], None, t)),
             ("time: reps 0", lambda: lib.odo_mesh_weld_time_dev(w.h, C.byref(good), held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], None, held.p["tri"], 0, us)),
             ("time: reps 10001", lambda: lib.odo_mesh_weld_time_dev(w.h, C.byref(good), held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], None, held.p["tri"], 10001, us)),
             ("time: us NULL", lambda: lib.odo_mesh_weld_time_dev(w.h, C.byref(good), held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], None, held.p["tri"], 3, None)),
             ("time: an input of the welder's own", lambda: lib.odo_mesh_weld_time_dev(w.h, C.byref(good), held.n_v, held.n_t, x, held.p["nrmw"], None, held.p["tri"], 3, us)),
             ("stats NULL", lambda: lib.odo_mesh_weld_stats(w.h, None)),
             ("download: a vertex short", lambda: lib.odo_mesh_weld_download(w.h, nv - 1, nt, vp(small), vp(small), None, vp(small), C.byref(cnt[0]), C.byref(cnt[1]))),
             ("download: a triangle short", lambda: lib.odo_mesh_weld_download(w.h, nv, nt - 1, vp(small), vp(small), None, vp(small), C.byref(cnt[0]), C.byref(cnt[1]))),
             ("download: colours of a run without", lambda: lib.odo_mesh_weld_download(w.h, nv, nt, vp(small), vp(small), vp(small), vp(small), C.byref(cnt[0]), C.byref(cnt[1])))]
    for what, call in calls:
        assert call() == -1 and L_.last_error(), what
        assert list(us) == [7.0] * 7, what
        unchanged(what)
    assert not small.any()                                                          # a refused download copies nothing
    with pytest.raises(L_.OdoError):
        w.run_dev(301, held.n_t, held.p["xyz0"], held.p["nrmw"], held.p["tri"], eps=1.0)
    with pytest.raises(L_.OdoError):
        api.MeshWeld(ctx, 0, 8)
    with pytest.raises(ValueError):
        w.run(r["mesh"]["xyz0"], r["mesh"]["nrmw"], r["mesh"]["tri"])               # no eps
    unchanged("api")
    w.close()
    w.close()                                                                       # twice is harmless
    held.free()
    coloured.free()


def test_two_welders_on_one_context(ctx):
    """Enqueued alternately, nothing waited for in between: each has its own tables, buffers and statistics."""
    from odometry_amd import api
    ia, ib = wc.row_ids().index("255 vertices, 511 triangles"), wc.row_ids().index("a coloured mesh")
    ra, rb = wc.rows()[ia], wc.rows()[ib]
    ha, hb = Held(ctx, ra["mesh"]), Held(ctx, rb["mesh"])
    wa, wb = api.MeshWeld(ctx, 400, 800), api.MeshWeld(ctx, 300, 700, colour=True)
    for _ in range(4):
        _run_dev(wa, ha, ra["rule"])
        _run_dev(wb, hb, rb["rule"])
    _equals_model(wb.download(colour=True), wc.model_of(ib), "b")
    _equals_model(wa.download(), wc.model_of(ia), "a")
    assert wa.stats() == wc.model_of(ia)["stats"] and wb.stats() == wc.model_of(ib)["stats"]
    wa.close()
    wb.close()
    ha.free()
    hb.free()


def test_destroy_with_ten_runs_in_flight_and_the_timing_call(ctx, drive):
    """Ten runs of the drive's mesh enqueued and the welder destroyed at once: destroy waits, and the context goes on. The timing call
    leaves exactly one run's result and statistics."""
    from odometry_amd import api
    m, p, held = drive
    rule = dict(eps=np.float32(p["vs"]) / np.float32(64.0), origin=p["origin"], grids=8, drop=True)
    w = api.MeshWeld(ctx, held.n_v, held.n_t)
    for _ in range(10):
        _run_dev(w, held, rule)
    w.close()
    assert held.unchanged()
    w = api.MeshWeld(ctx, held.n_v, held.n_t)
    us = w.time(held.n_v, held.n_t, held.p["xyz0"], held.p["nrmw"], held.p["tri"], eps=rule["eps"], origin=rule["origin"], grids=8, reps=3)
    print({k: round(v, 1) for k, v in us.items()})
    assert list(us) == list(api.MeshWeld.GROUPS) and all(v > 0.0 for v in us.values())
    assert abs(us["run"] - sum(v for k, v in us.items() if k != "run")) <= 1e-3 * us["run"]
    M = wc.drive_model(8)
    _equals_model(w.download(), M, "after the timing call")
    assert w.stats() == M["stats"] and held.unchanged()
    w.close()


def test_the_volumes_welded_mesh_and_its_ply(ctx, tmp_path):
    """A volume with a mesh store, a re-entry store and colours after the d, -d, d walk of tests/volume_stores_cases.py (what left
    comes back and leaves again, so the store holds it twice): welded_mesh equals the model on
    the volume's own spilled_mesh() + mesh(), with and without the store, with and without colour; save_welded_mesh_ply round-trips
    through the PLY reader; save_mesh_ply writes what it always did."""
    import volume_stores_cases as VS
    from test_gpu_volume_shift import _volume
    from test_volume_mesh_cpu import read_ply_mesh
    p, q, w, col = VS.grid()
    vol = _volume(ctx, p, colour=True)
    vol.enable_spill_mesh(1 << 14, 1 << 14)
    vol.enable_reentry(1 << 16)                                                     # (what leaves comes back, and leaves again: duplicates)
    vol.upload(q, w)
    vol.upload_colour(col)
    for d in VS.TWICE:
        vol.shift(d)
    store, win = vol.spilled_mesh(colour=True), vol.mesh(colour=True)
    both = dict(xyz0=np.concatenate([store[0], win[0]]), nrmw=np.concatenate([store[1], win[1]]),
                tri=np.concatenate([store[2], win[2] + len(store[0])]).astype(np.int32), rgba=np.concatenate([store[3], win[3]]))
    eps = np.float32(p["vs"]) / np.float32(64.0)
    M = wc.weld_model(both, eps, p["origin"], 8)
    assert M["stats"]["duplicate"] > 0 and M["stats"]["merged"] > 0 and len(store[0]) > 0 and len(win[0]) > 0
    got = vol.welded_mesh(colour=True)
    _equals_model(got, M, "store + window, coloured")
    assert got["stats"] == M["stats"]
    plain = vol.welded_mesh(grids=1)
    M1 = wc.weld_model(dict(both, rgba=None), eps, p["origin"], 1)
    _equals_model(plain, M1, "store + window, one grid")
    assert "rgba" not in plain and plain["stats"] == M1["stats"]
    alone = vol.welded_mesh(spill=False, eps=0.01)
    Mw = wc.weld_model(dict(xyz0=win[0], nrmw=win[1], tri=win[2], rgba=None), 0.01, p["origin"], 8)
    _equals_model(alone, Mw, "the window alone, a coarser cell")
    path = str(tmp_path / "welded.ply")
    stats = vol.save_welded_mesh_ply(path)
    V, T = read_ply_mesh_rgb(path)
    assert stats == M["stats"] and np.array_equal(T, M["tri"])
    assert np.array_equal(wc.bits(V[0]), wc.bits(M["xyz0"][:, :3])) and np.array_equal(wc.bits(V[1]), wc.bits(M["nrmw"][:, :3]))
    assert np.array_equal(V[2], M["rgba"][:, :3])
    # a volume without colour or store: the plain reader, and save_mesh_ply's bytes are the concatenation still
    bare = _volume(ctx, p)
    bare.upload(q, w)
    path2 = str(tmp_path / "bare.ply")
    bare.save_welded_mesh_ply(path2, grids=1)
    V2, T2 = read_ply_mesh(path2)
    bm = bare.mesh()
    Mb = wc.weld_model(dict(xyz0=bm[0], nrmw=bm[1], tri=bm[2], rgba=None), eps, p["origin"], 1)
    assert np.array_equal(T2, Mb["tri"]) and np.array_equal(wc.bits(V2[:, :3]), wc.bits(Mb["xyz0"][:, :3]))
    assert np.array_equal(wc.bits(V2[:, 3:]), wc.bits(Mb["nrmw"][:, :3]))
    path3 = str(tmp_path / "unwelded.ply")
    bare.save_mesh_ply(path3)
    V3, T3 = read_ply_mesh(path3)
    assert np.array_equal(T3, bm[2]) and np.array_equal(wc.bits(V3[:, :3]), wc.bits(bm[0][:, :3]))
    bare.close()
    vol.close()


def read_ply_mesh_rgb(path):
    """tests/test_volume_mesh_cpu.py's reader for a mesh with colours: ((xyz, normals, rgb), faces)."""
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    assert [ln.split()[-1] for ln in lines if ln.startswith("property float")] == ["x", "y", "z", "nx", "ny", "nz"]
    assert [ln.split()[-1] for ln in lines if ln.startswith("property uchar")] == ["red", "green", "blue"]
    assert len(body) == 27 * nv + 13 * nf
    vert = np.frombuffer(body[:27 * nv], np.dtype([("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (3,))]))
    face = np.frombuffer(body[27 * nv:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert (face["n"] == 3).all()
    return (vert["p"], vert["n"], vert["c"]), face["v"]
