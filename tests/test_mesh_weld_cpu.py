"""The mesh welder (odo_mesh_weld_*, api.MeshWeld, api.TsdfVolume.welded_mesh / save_welded_mesh_ply) without a GPU: the numpy model of
the specification (include/odometry_hip.h) pinned to the prose by plain loops on every row of
tests/mesh_weld_cases.py small enough for them, every row held to the situation it is in the table for, five switches of the model
each caught by exactly its rows, the host + device header odometry_amd/csrc/mesh_weld_math.h as a stand-alone g++ program under
sanitizers, the refusals that the arguments alone decide, the ABI, the kernels' code-object metadata, and what the method is for: the
mesh of the drive that leaves its box, whose seams it closes.

The model is the yardstick of tests/test_gpu_mesh_weld.py, which asks the GPU for the same bits."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import mesh_weld_cases as wc

ROOT = wc.ROOT
HARNESS = os.path.join(ROOT, "tests", "mesh_weld_math_harness.cpp")
NEW_SYMBOLS = ["odo_mesh_weld_create", "odo_mesh_weld_run_dev", "odo_mesh_weld_result_dev", "odo_mesh_weld_download", "odo_mesh_weld_run",
               "odo_mesh_weld_stats", "odo_mesh_weld_time_dev", "odo_mesh_weld_destroy"]
NEW_KERNELS = ["weld_begin_kernel", "weld_key_kernel", "weld_rep_kernel", "weld_remap_kernel", "weld_tri_table_kernel", "weld_tri_keep_kernel",
               "weld_vertex_keep_kernel", "weld_scan_kernel", "weld_vertex_scatter_kernel", "weld_tri_scatter_kernel"]

# The model's own counts on the drive's mesh at voxel_size / 64 (the tests below print them). `open` = edges
# used by one triangle.
DRIVE_IN = dict(vertices=159944, triangles=300970, open=13020, store_vertices=114143, store_triangles=213926)
DRIVE = {1: dict(vertices_out=152266, merged=4843, unreferenced=2835, triangles_out=299579, degenerate=1391, duplicate=0, open=5295),
         8: dict(vertices_out=151506, merged=5602, unreferenced=2836, triangles_out=299223, degenerate=1747, duplicate=0, open=3853)}


def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", header) and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert C.sizeof(_lib.MeshWeldParams) == 3 * 4 and C.sizeof(_lib.MeshWeldRule) == 6 * 4
    assert api.MeshWeld.STATS == wc.STATS and len(api.MeshWeld.GROUPS) == wc.constants()["kWeldGroups"] + 1
    assert wc.constants()["kWeldStatWords"] == len(wc.STATS) == 12
    for name in ("run", "run_dev", "result_dev", "download", "stats", "time", "close"):
        assert callable(getattr(api.MeshWeld, name)), name
    assert list(inspect.signature(api.MeshWeld.__init__).parameters) == ["self", "ctx_or_tracker", "vertex_capacity", "triangle_capacity", "colour"]
    run = inspect.signature(api.MeshWeld.run).parameters
    assert list(run) == ["self", "xyz0", "nrmw", "tri", "rgba", "eps", "origin", "grids", "drop_unreferenced"]
    assert run["grids"].default == 8 and run["drop_unreferenced"].default is True and run["rgba"].default is None
    welded = inspect.signature(api.TsdfVolume.welded_mesh).parameters
    assert list(welded) == ["self", "eps", "grids", "spill", "colour"]
    assert (welded["eps"].default, welded["grids"].default, welded["spill"].default, welded["colour"].default) == (None, 8, True, False)
    assert callable(api.TsdfVolume.save_welded_mesh_ply)
    sig = inspect.signature(api.TsdfVolume.save_mesh_ply)
    assert list(sig.parameters) == ["self", "path", "spill"] and sig.parameters["spill"].default is False   # as it was


def c_rule(eps=0.01, origin=(0.0, 0.0, 0.0), grids=8, drop=1):
    from odometry_amd import _lib
    r = _lib.MeshWeldRule()
    r.eps, r.grids, r.drop_unreferenced = eps, grids, drop
    for i in range(3):
        r.origin[i] = origin[i]
    return r


def bad_sets():
    """(what, record, index of the check that refuses it, number of the bound, a word of the message): every bound of
    odo_mesh_weld_create, of a rule and of a run's counts. A record is what the harness reads: n_v, n_t, grids, drop, colour,
    vertex_capacity, triangle_capacity, eps, origin."""
    good = dict(n_v=3, n_t=1, grids=8, drop=1, colour=0, vcap=8, tcap=8, eps=0.01, origin=(0.0, 0.0, 0.0))
    nan, inf = float("nan"), float("inf")
    return [(what, dict(good, **kw), check, bound, word) for what, kw, check, bound, word in (
        ("vertex_capacity 0", dict(vcap=0), 0, 1, "vertex_capacity"), ("vertex_capacity -1", dict(vcap=-1), 0, 1, "vertex_capacity"),
        ("vertex_capacity 2^28 + 1", dict(vcap=(1 << 28) + 1), 0, 1, "vertex_capacity"),
        ("triangle_capacity 0", dict(tcap=0), 0, 2, "triangle_capacity"),
        ("triangle_capacity 2^28 + 1", dict(tcap=(1 << 28) + 1), 0, 2, "triangle_capacity"),
        ("colour 2", dict(colour=2), 0, 3, "colour"), ("colour -1", dict(colour=-1), 0, 3, "colour"),
        ("eps 0", dict(eps=0.0), 1, 1, "eps"), ("eps -1", dict(eps=-1.0), 1, 1, "eps"), ("eps nan", dict(eps=nan), 1, 1, "eps"),
        ("eps inf", dict(eps=inf), 1, 1, "eps"), ("origin nan", dict(origin=(0.0, nan, 0.0)), 1, 2, "origin"),
        ("origin inf", dict(origin=(inf, 0.0, 0.0)), 1, 2, "origin"), ("origin -inf", dict(origin=(0.0, 0.0, -inf)), 1, 2, "origin"),
        ("grids 0", dict(grids=0), 1, 3, "grids"), ("grids 2", dict(grids=2), 1, 3, "grids"), ("grids 7", dict(grids=7), 1, 3, "grids"),
        ("grids 9", dict(grids=9), 1, 3, "grids"), ("grids -8", dict(grids=-8), 1, 3, "grids"),
        ("drop 2", dict(drop=2), 1, 4, "drop_unreferenced"), ("drop -1", dict(drop=-1), 1, 4, "drop_unreferenced"),
        ("n_v -1", dict(n_v=-1), 2, 1, "n_vertices"), ("n_v beyond the capacity", dict(n_v=9), 2, 1, "vertices"),
        ("n_t -1", dict(n_t=-1), 2, 2, "n_triangles"), ("n_t beyond the capacity", dict(n_t=9), 2, 2, "triangles"))]


def test_bad_arguments_are_refused_before_touching_a_device():
    """Every refusal that the arguments alone decide, on handles that are never dereferenced; *out stays as it was and the message
    names the bound. NULLs everywhere."""
    from odometry_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)
    for what, s, check, _, word in bad_sets():
        if check != 0:
            continue
        p = _lib.MeshWeldParams(s["vcap"], s["tcap"], s["colour"])
        h = C.c_void_p(0x5A5A)
        assert lib.odo_mesh_weld_create(fake, C.byref(p), C.byref(h)) == -1, what
        assert h.value == 0x5A5A and "odo_mesh_weld_create" in _lib.last_error() and word in _lib.last_error(), (what, _lib.last_error())
    h, good = C.c_void_p(0x5A5A), _lib.MeshWeldParams(8, 8, 0)
    assert lib.odo_mesh_weld_create(None, C.byref(good), C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_mesh_weld_create(fake, None, C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_mesh_weld_create(fake, C.byref(good), None) == -1
    # a run: the rule, the signs and the range of the counts, NULL meshes and misaligned pointers come before the welder is read
    a16, a4 = C.c_void_p(0x10000), C.c_void_p(0x20004)
    us = (C.c_float * 7)(*[7.0] * 7)
    for what, s, check, _, word in bad_sets():
        if check == 0 or "capacity" in what:
            continue
        r = c_rule(s["eps"], s["origin"], s["grids"], s["drop"])
        assert lib.odo_mesh_weld_run_dev(fake, C.byref(r), s["n_v"], s["n_t"], a16, a16, None, a4) == -1, what
        assert "odo_mesh_weld_run_dev" in _lib.last_error() and word in _lib.last_error(), (what, _lib.last_error())
        assert lib.odo_mesh_weld_time_dev(fake, C.byref(r), s["n_v"], s["n_t"], a16, a16, None, a4, 1, us) == -1, what
        assert "odo_mesh_weld_time_dev" in _lib.last_error() and list(us) == [7.0] * 7
    r = c_rule()
    for what, args in (("NULL welder", (None, C.byref(r), 3, 1, a16, a16, None, a4)), ("NULL rule", (fake, None, 3, 1, a16, a16, None, a4)),
                       ("n_v 2^28 + 1", (fake, C.byref(r), (1 << 28) + 1, 1, a16, a16, None, a4)),
                       ("n_t 2^28 + 1", (fake, C.byref(r), 3, (1 << 28) + 1, a16, a16, None, a4)),
                       ("NULL xyz0", (fake, C.byref(r), 3, 1, None, a16, None, a4)), ("NULL nrmw", (fake, C.byref(r), 3, 1, a16, None, None, a4)),
                       ("NULL tri", (fake, C.byref(r), 3, 1, a16, a16, None, None)),
                       ("xyz0 off 16", (fake, C.byref(r), 3, 1, C.c_void_p(0x10008), a16, None, a4)),
                       ("nrmw off 16", (fake, C.byref(r), 3, 1, a16, C.c_void_p(0x10004), None, a4)),
                       ("rgba off 4", (fake, C.byref(r), 3, 1, a16, a16, C.c_void_p(0x30002), a4)),
                       ("tri off 4", (fake, C.byref(r), 3, 1, a16, a16, None, C.c_void_p(0x20001)))):
        assert lib.odo_mesh_weld_run_dev(*args) == -1 and "odo_mesh_weld_run_dev" in _lib.last_error(), what
    for reps in (0, -1, 10001):
        assert lib.odo_mesh_weld_time_dev(fake, C.byref(r), 3, 1, a16, a16, None, a4, reps, us) == -1 and "reps" in _lib.last_error()
    assert lib.odo_mesh_weld_time_dev(fake, C.byref(r), 3, 1, a16, a16, None, a4, 1, None) == -1 and list(us) == [7.0] * 7
    n, m = C.c_long(7), C.c_long(7)
    out12 = (C.c_long * 12)(*[7] * 12)
    assert lib.odo_mesh_weld_stats(None, out12) == -1 and lib.odo_mesh_weld_stats(fake, None) == -1 and list(out12) == [7] * 12
    assert lib.odo_mesh_weld_result_dev(None, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_result_dev(fake, None, None, None, None, None, C.byref(m)) == -1
    assert lib.odo_mesh_weld_result_dev(fake, None, None, None, None, C.byref(n), None) == -1
    buf = np.zeros(64, np.float32).ctypes.data_as(C.c_void_p)
    assert lib.odo_mesh_weld_download(None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_download(fake, -1, 0, buf, buf, None, buf, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_download(fake, 0, -1, buf, buf, None, buf, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_download(fake, 1, 0, None, buf, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_download(fake, 0, 1, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_download(fake, 0, 0, None, None, None, None, None, C.byref(m)) == -1
    assert lib.odo_mesh_weld_run(None, C.byref(r), 0, 0, None, None, None, None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_run(fake, None, 0, 0, None, None, None, None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_run(fake, C.byref(r), -1, 0, None, None, None, None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_run(fake, C.byref(r), 1, 0, None, None, None, None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_weld_run(fake, C.byref(r), 0, 0, None, None, None, None, 0, 0, None, None, None, None, None, C.byref(m)) == -1
    assert (n.value, m.value) == (7, 7)
    assert lib.odo_mesh_weld_destroy(None) == 0


# ---- model, loops, rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(wc.rows())), ids=wc.row_ids())
def test_model_equals_the_loops_and_the_row_reaches_its_situation(index):
    r = wc.rows()[index]
    M = wc.model_of(index)
    s = M["stats"]
    assert r["holds"](M), (r["name"], s)
    assert s["guard"] == 0 and s["passes"] == r["rule"]["grids"]
    assert s["vertices_out"] == s["vertices_in"] - s["merged"] - s["unreferenced"] == len(M["xyz0"]) == len(M["nrmw"])
    assert s["triangles_out"] == s["triangles_in"] - s["degenerate"] - s["duplicate"] - s["bad_index"] == len(M["tri"])
    assert r["rule"]["drop"] or s["unreferenced"] == 0
    if len(M["tri"]):
        t = M["tri"]
        assert 0 <= t.min() and t.max() < len(M["xyz0"]) and (t[:, 0] < t[:, 1]).all() and (t[:, 0] < t[:, 2]).all()   # rotated
    # every kept vertex is an input vertex, whole: position, normal, weight and colour bit for bit, in ascending input order
    src = np.concatenate([wc.bits(r["mesh"]["xyz0"]).reshape(-1, 4), wc.bits(r["mesh"]["nrmw"]).reshape(-1, 4)], 1)
    got = np.concatenate([wc.bits(M["xyz0"]).reshape(-1, 4), wc.bits(M["nrmw"]).reshape(-1, 4)], 1)
    at = 0
    for row in got:
        while at < len(src) and not np.array_equal(src[at], row):
            at += 1
        assert at < len(src), r["name"]
        at += 1
    assert len(r["mesh"]["xyz0"]) + len(r["mesh"]["tri"]) <= wc.LOOP_ITEMS
    rule = r["rule"]
    assert wc.same_as_loop(M, wc.weld_loop(r["mesh"], rule["eps"], rule["origin"], rule["grids"], rule["drop"])), r["name"]


def test_rows_cover_the_launch_geometry():
    """Vertex and triangle counts of 0, 1 and 2, either side of a wave and of a workgroup, more than one workgroup, both settings of
    grids and of drop_unreferenced, meshes with and without colour; a table row whose probes wrap."""
    k = wc.constants()
    assert k["kWeldBlock"] == 256 and k["kWeldMaxPasses"] == 8 and k["kWeldMaxCapacity"] == 1 << 28 and k["kWeldCellLimit"] == wc.LIMIT
    nv = {len(r["mesh"]["xyz0"]) for r in wc.rows()}
    nt = {len(r["mesh"]["tri"]) for r in wc.rows()}
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257} <= nv and {0, 1} <= nt and max(nv) > 4 * k["kWeldBlock"] and max(nt) > 2 * k["kWeldBlock"]
    assert any(k["kWeldBlock"] - 1 <= n <= k["kWeldBlock"] + 1 for n in nt)
    assert {r["rule"]["grids"] for r in wc.rows()} == {1, 8} and {r["rule"]["drop"] for r in wc.rows()} == {True, False}
    assert any(r["mesh"]["rgba"] is not None for r in wc.rows()) and any(r["mesh"]["rgba"] is None for r in wc.rows())
    assert wc.n_slots(1) == 2 and wc.n_slots(256) == 512 and wc.n_slots(257) == 1024 and wc.n_slots(1 << 28) == 1 << 29


@pytest.mark.parametrize("switch", wc.SWITCHES)
def test_each_switch_is_caught_by_exactly_its_rows(switch):
    placed = wc.CAUGHT_BY[switch]
    caught = [name for index, name in enumerate(wc.row_ids()) if wc.differs(index, switch)]
    want = [n for i, n in enumerate(wc.row_ids()) if placed(i)] if callable(placed) else [n for n in wc.row_ids() if n in placed]
    assert caught == want and len(caught) >= 1, (switch, set(caught) ^ set(want))
    if not callable(placed):
        assert len(want) == len(placed)


def test_the_rows_placed_for_a_switch_are_among_those_that_catch_it():
    caught = {sw: {n for i, n in enumerate(wc.row_ids()) if wc.differs(i, sw)} for sw in wc.SWITCHES}
    assert "one ulp either side of a face below the origin" in caught["trunc"] and "a coordinate exactly on a face" not in caught["trunc"]
    assert "256 vertices in one cell" in caught["largest_rep"] and "a coloured mesh" in caught["largest_rep"]
    assert "three rotations and the mirror image" in caught["no_rotation"] & caught["mirror_duplicate"]
    assert "pairs joined by grid 1, 2, 4 and 7 only" in caught["whole_cell"] and "the same pairs on one grid" not in caught["whole_cell"]


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------------
def _record(s, mesh=None):
    head = np.array([s["n_v"], s["n_t"], s["grids"], s["drop"], s["colour"], s["vcap"], s["tcap"], 0], np.int32).tobytes()
    head += np.array([s["eps"], *s["origin"]], np.float32).tobytes()
    if mesh is not None:
        head += np.ascontiguousarray(mesh["xyz0"], np.float32).tobytes() + np.ascontiguousarray(mesh["nrmw"], np.float32).tobytes()
        if mesh["rgba"] is not None:
            head += np.ascontiguousarray(mesh["rgba"], np.uint8).tobytes()
        head += np.ascontiguousarray(mesh["tri"], np.int32).tobytes()
    return head


def test_shared_header_under_sanitizers(tmp_path):
    """mesh_weld_math.h as a g++ program of its own (ASan + UBSan; both tables, the scratch and every pass's outputs heap blocks of
    exactly their sizes): the reference pass over the kernels' own tables equals the model byte for byte on every row — vertices,
    attributes, triangles, counters — and the three checks name the bound of every bad parameter set and pass the outermost good
    ones."""
    exe = str(tmp_path / "mesh_weld_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", HARNESS, "-o", exe])
    outer = dict(n_v=0, n_t=0, grids=1, drop=0, colour=1, vcap=1, tcap=1, eps=1e-30, origin=(-3e38, 3e38, 0.0))
    with open(tmp_path / "in.bin", "wb") as f:
        for r in wc.rows():
            m, rule = r["mesh"], r["rule"]
            f.write(_record(dict(n_v=len(m["xyz0"]), n_t=len(m["tri"]), grids=rule["grids"], drop=int(rule["drop"]),
                                 colour=int(m["rgba"] is not None), vcap=r["capacity"][0], tcap=r["capacity"][1], eps=rule["eps"],
                                 origin=rule["origin"]), m))
        for _, s, _, _, _ in bad_sets():
            f.write(_record(s))
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert done.stdout.strip() == f"{len(wc.rows()) + len(bad_sets())} records"
    blob = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(blob, dtype, n, at)
        at += a.nbytes
        return a

    for index, r in enumerate(wc.rows()):
        M = wc.model_of(index)
        assert take(np.int32, 3).tolist() == [0, 0, 0], r["name"]
        nv, nt = take(np.int32, 2).tolist()
        assert (nv, nt) == (len(M["xyz0"]), len(M["tri"])), r["name"]
        assert np.array_equal(take(np.uint32, 4 * nv), wc.bits(M["xyz0"]).ravel()), r["name"]
        assert np.array_equal(take(np.uint32, 4 * nv), wc.bits(M["nrmw"]).ravel()), r["name"]
        if M["rgba"] is not None:
            assert np.array_equal(take(np.uint8, 4 * nv), M["rgba"].ravel()), r["name"]
        assert np.array_equal(take(np.int32, 3 * nt), M["tri"].ravel()), r["name"]
        assert dict(zip(wc.STATS, take(np.int64, 12).tolist())) == M["stats"], r["name"]
    for what, _, check, bound, _ in bad_sets():
        got = take(np.int32, 3).tolist()
        assert got[check] == bound and not any(got[:check]) and not any(got[check + 1:2]), (what, got)   # (a bad capacity also fails the counts)
    assert at == len(blob)
    # an outermost good set passes all three checks: the smallest welder, an empty coloured mesh, a tiny cell about a far origin
    with open(tmp_path / "in2.bin", "wb") as f:
        f.write(_record(outer, dict(xyz0=np.zeros((0, 4)), nrmw=np.zeros((0, 4)), rgba=np.zeros((0, 4)), tri=np.zeros((0, 3)))))
    done = subprocess.run([exe, str(tmp_path / "in2.bin"), str(tmp_path / "out2.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "1 records", done.stderr[-2000:]
    blob = open(tmp_path / "out2.bin", "rb").read()
    assert np.frombuffer(blob, np.int32, 5).tolist() == [0, 0, 0, 0, 0]
    assert np.frombuffer(blob, np.int64, 12, 20).tolist() == [0] * 11 + [1] and len(blob) == 20 + 96


# ---- what the method gives: the drive that leaves its box ------------------------------------------------------------------------------------
def test_the_drive_mesh_is_the_unwelded_stack_of_sheets():
    m, p, store = wc.drive_mesh()
    opened, many = wc.edge_use(m["tri"])
    print(f"as written today: {len(m['xyz0'])} vertices, {len(m['tri'])} triangles, {opened} edges used by one triangle, {many} by more "
          f"than two; the store holds {store[0]} vertices and {store[1]} triangles")
    assert dict(vertices=len(m["xyz0"]), triangles=len(m["tri"]), open=opened, store_vertices=store[0], store_triangles=store[1]) == DRIVE_IN
    assert many == 0


@pytest.mark.parametrize("grids", [1, 8])
def test_the_drive_mesh_welded_closes_its_seams(grids):
    """The drive's mesh at eps = voxel_size / 64: the model's own counts, no edge used by more than two triangles, every kept vertex
    an input vertex bit for bit, and at eight grids fewer than a third of the unwelded mesh's open edges."""
    m, p, _ = wc.drive_mesh()
    M = wc.drive_model(grids)
    s = M["stats"]
    opened, many = wc.edge_use(M["tri"])
    print(f"grids {grids}: {s}; {opened} edges used by one triangle, {many} by more than two")
    assert {k: s[k] for k in DRIVE[grids] if k != "open"} == {k: v for k, v in DRIVE[grids].items() if k != "open"}
    assert opened == DRIVE[grids]["open"] and many == 0 and s["guard"] == 0 and s["keyless"] == 0 and s["bad_index"] == 0
    assert s["vertices_out"] == s["vertices_in"] - s["merged"] - s["unreferenced"]
    if grids == 8:
        assert 3 * opened < DRIVE_IN["open"]
    # kept vertices: rows of the input, whole, in ascending order
    src = np.concatenate([wc.bits(m["xyz0"]), wc.bits(m["nrmw"])], 1)
    got = np.concatenate([wc.bits(M["xyz0"]), wc.bits(M["nrmw"])], 1)
    keep = np.ones(len(src), bool)
    for p_ in M["passes"]:
        k = np.nonzero(keep)[0]
        keep[k[~p_["vkeep"]]] = False
    assert np.array_equal(src[keep], got)


def test_the_drive_mesh_by_the_loops():
    """The loops on the drive's mesh at one grid: the model's bytes (eight grids are eight times the same code)."""
    m, p, _ = wc.drive_mesh()
    assert wc.same_as_loop(wc.drive_model(1), wc.weld_loop(m, np.float32(p["vs"]) / np.float32(64.0), p["origin"], 1))


# ---- code object ---------------------------------------------------------------------------------------------------------------------------
def test_weld_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
    from odometry_amd import _lib
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools here")
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "lib.so")
        shutil.copy(_lib.LIB_PATH, so)
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], cwd=td, check=True, capture_output=True)
        notes = ""
        for f in sorted(os.listdir(td)):
            if "gfx950" in f:
                notes += subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(td, f)], check=True,
                                        capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        for k in NEW_KERNELS:
            if k in name:
                found[k] = tuple(int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1)) for key in (
                    "vgpr_count", "sgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"))
    print(found)
    assert sorted(found) == sorted(NEW_KERNELS), found
    for key, (vgprs, _, lds, vspill, sspill, scratch) in found.items():
        assert (vspill, sspill, scratch) == (0, 0, 0), key
        assert vgprs <= 64 and lds <= 128, key                               # eight waves per SIMD, a word per wave of LDS
