"""The mesh component filter (odo_mesh_components_*, api.MeshComponents, api.TsdfVolume.cleaned_mesh / save_cleaned_mesh_ply) without
a GPU: the numpy model of the specification (include/odometry_hip.h) pinned to the prose by plain loops on
every row of tests/mesh_components_cases.py, every row held to the situation it is in the table for, six switches of the model each
caught by exactly its rows, the host + device header odometry_amd/csrc/mesh_components_math.h as a stand-alone g++ program under
sanitizers, the refusals that the arguments alone decide, the ABI, the kernels' code-object metadata, and what the method is for: the
welded mesh of the drive that leaves its box, whose debris it removes.

The model is the yardstick of tests/test_gpu_mesh_components.py, which asks the GPU for the same bits."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import mesh_components_cases as mc
from mesh_weld_cases import edge_use

ROOT = mc.ROOT
HARNESS = os.path.join(ROOT, "tests", "mesh_components_math_harness.cpp")
NEW_SYMBOLS = ["odo_mesh_components_" + n for n in ("create", "run_dev", "result_dev", "download", "run", "labels_dev", "labels", "stats",
                                                    "time_dev", "destroy")]
NEW_KERNELS = ["mc_begin_kernel", "mc_init_kernel", "mc_union_kernel", "mc_flatten_kernel", "mc_label_kernel", "mc_roots_kernel",
               "mc_edge_kernel", "mc_census_kernel", "mc_tri_keep_kernel", "mc_vertex_keep_kernel", "mc_scan_kernel",
               "mc_vertex_scatter_kernel", "mc_tri_scatter_kernel"]


def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", header) and hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert C.sizeof(_lib.MeshComponentsParams) == 4 * 4 and C.sizeof(_lib.MeshComponentsRule) == 3 * 4
    k = mc.constants()
    assert api.MeshComponents.STATS == mc.STATS and len(api.MeshComponents.GROUPS) == k["kMcGroups"] + 1
    assert k["kMcStatWords"] == len(mc.STATS) == 19 and "removed_vertices" in mc.STATS
    for name in ("run", "run_dev", "result_dev", "download", "labels", "labels_dev", "stats", "time", "close"):
        assert callable(getattr(api.MeshComponents, name)), name
    init = inspect.signature(api.MeshComponents.__init__).parameters
    assert list(init) == ["self", "ctx_or_tracker", "vertex_capacity", "triangle_capacity", "colour", "edge_stats"]
    assert init["colour"].default is False and init["edge_stats"].default is True
    run = inspect.signature(api.MeshComponents.run).parameters
    assert list(run) == ["self", "xyz0", "nrmw", "tri", "rgba", "min_triangles", "keep_largest", "drop_unreferenced"]
    assert run["keep_largest"].default is False and run["drop_unreferenced"].default is True and run["rgba"].default is None
    cleaned = inspect.signature(api.TsdfVolume.cleaned_mesh).parameters
    assert list(cleaned) == ["self", "eps", "grids", "spill", "colour", "min_triangles", "keep_largest"]
    assert [cleaned[n].default for n in list(cleaned)[1:]] == [None, 8, True, False, 128, False]
    assert callable(api.TsdfVolume.save_cleaned_mesh_ply)
    # what was there keeps its signatures
    assert list(inspect.signature(api.TsdfVolume.welded_mesh).parameters) == ["self", "eps", "grids", "spill", "colour"]
    assert list(inspect.signature(api.TsdfVolume.save_welded_mesh_ply).parameters) == ["self", "path", "eps", "grids", "spill"]
    assert list(inspect.signature(api.TsdfVolume.save_mesh_ply).parameters) == ["self", "path", "spill"]


def c_rule(min_triangles=3, keep_largest=0, drop=1):
    from odometry_amd import _lib
    return _lib.MeshComponentsRule(min_triangles, keep_largest, drop)


def bad_sets():
    """(what, record, index of the check that refuses it, number of the bound, a word of the message): every bound of
    odo_mesh_components_create, of a rule and of a run's counts. A record is what the harness reads."""
    good = dict(n_v=3, n_t=1, min_triangles=3, keep=0, drop=1, colour=0, edges=1, vcap=8, tcap=8)
    return [(what, dict(good, **kw), check, bound, word) for what, kw, check, bound, word in (
        ("vertex_capacity 0", dict(vcap=0), 0, 1, "vertex_capacity"), ("vertex_capacity -1", dict(vcap=-1), 0, 1, "vertex_capacity"),
        ("vertex_capacity 2^28 + 1", dict(vcap=(1 << 28) + 1), 0, 1, "vertex_capacity"),
        ("triangle_capacity 0", dict(tcap=0), 0, 2, "triangle_capacity"),
        ("triangle_capacity 2^28 + 1", dict(tcap=(1 << 28) + 1), 0, 2, "triangle_capacity"),
        ("colour 2", dict(colour=2), 0, 3, "colour"), ("colour -1", dict(colour=-1), 0, 3, "colour"),
        ("edge_stats 2", dict(edges=2), 0, 4, "edge_stats"), ("edge_stats -1", dict(edges=-1), 0, 4, "edge_stats"),
        ("min_triangles -1", dict(min_triangles=-1), 1, 1, "min_triangles"),
        ("min_triangles INT32_MIN", dict(min_triangles=-(1 << 31)), 1, 1, "min_triangles"),
        ("keep_largest 2", dict(keep=2), 1, 2, "keep_largest"), ("keep_largest -1", dict(keep=-1), 1, 2, "keep_largest"),
        ("drop 2", dict(drop=2), 1, 3, "drop_unreferenced"), ("drop -1", dict(drop=-1), 1, 3, "drop_unreferenced"),
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
        p = _lib.MeshComponentsParams(s["vcap"], s["tcap"], s["colour"], s["edges"])
        h = C.c_void_p(0x5A5A)
        assert lib.odo_mesh_components_create(fake, C.byref(p), C.byref(h)) == -1, what
        assert h.value == 0x5A5A and "odo_mesh_components_create" in _lib.last_error() and word in _lib.last_error(), (what, _lib.last_error())
    h, good = C.c_void_p(0x5A5A), _lib.MeshComponentsParams(8, 8, 0, 1)
    assert lib.odo_mesh_components_create(None, C.byref(good), C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_mesh_components_create(fake, None, C.byref(h)) == -1 and h.value == 0x5A5A
    assert lib.odo_mesh_components_create(fake, C.byref(good), None) == -1
    # a run: the rule, the signs and the range of the counts, NULL meshes and misaligned pointers come before the filter is read
    a16, a4 = C.c_void_p(0x10000), C.c_void_p(0x20004)
    us = (C.c_float * 7)(*[7.0] * 7)
    for what, s, check, _, word in bad_sets():
        if check == 0 or "capacity" in what:
            continue
        r = c_rule(s["min_triangles"], s["keep"], s["drop"])
        assert lib.odo_mesh_components_run_dev(fake, C.byref(r), s["n_v"], s["n_t"], a16, a16, None, a4) == -1, what
        assert "odo_mesh_components_run_dev" in _lib.last_error() and word in _lib.last_error(), (what, _lib.last_error())
        assert lib.odo_mesh_components_time_dev(fake, C.byref(r), s["n_v"], s["n_t"], a16, a16, None, a4, 1, us) == -1, what
        assert "odo_mesh_components_time_dev" in _lib.last_error() and list(us) == [7.0] * 7
    r = c_rule()
    for what, args in (("NULL filter", (None, C.byref(r), 3, 1, a16, a16, None, a4)), ("NULL rule", (fake, None, 3, 1, a16, a16, None, a4)),
                       ("n_v 2^28 + 1", (fake, C.byref(r), (1 << 28) + 1, 1, a16, a16, None, a4)),
                       ("n_t 2^28 + 1", (fake, C.byref(r), 3, (1 << 28) + 1, a16, a16, None, a4)),
                       ("NULL xyz0", (fake, C.byref(r), 3, 1, None, a16, None, a4)), ("NULL nrmw", (fake, C.byref(r), 3, 1, a16, None, None, a4)),
                       ("NULL tri", (fake, C.byref(r), 3, 1, a16, a16, None, None)),
                       ("xyz0 off 16", (fake, C.byref(r), 3, 1, C.c_void_p(0x10008), a16, None, a4)),
                       ("nrmw off 16", (fake, C.byref(r), 3, 1, a16, C.c_void_p(0x10004), None, a4)),
                       ("rgba off 4", (fake, C.byref(r), 3, 1, a16, a16, C.c_void_p(0x30002), a4)),
                       ("tri off 4", (fake, C.byref(r), 3, 1, a16, a16, None, C.c_void_p(0x20001)))):
        assert lib.odo_mesh_components_run_dev(*args) == -1 and "odo_mesh_components_run_dev" in _lib.last_error(), what
    for reps in (0, -1, 10001):
        assert lib.odo_mesh_components_time_dev(fake, C.byref(r), 3, 1, a16, a16, None, a4, reps, us) == -1 and "reps" in _lib.last_error()
    assert lib.odo_mesh_components_time_dev(fake, C.byref(r), 3, 1, a16, a16, None, a4, 1, None) == -1 and list(us) == [7.0] * 7
    n, m = C.c_long(7), C.c_long(7)
    out19 = (C.c_long * 19)(*[7] * 19)
    assert lib.odo_mesh_components_stats(None, out19) == -1 and lib.odo_mesh_components_stats(fake, None) == -1 and list(out19) == [7] * 19
    assert lib.odo_mesh_components_result_dev(None, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_components_result_dev(fake, None, None, None, None, None, C.byref(m)) == -1
    assert lib.odo_mesh_components_result_dev(fake, None, None, None, None, C.byref(n), None) == -1
    buf = np.zeros(64, np.float32).ctypes.data_as(C.c_void_p)
    assert lib.odo_mesh_components_download(None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_components_download(fake, -1, 0, buf, buf, None, buf, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_components_download(fake, 0, -1, buf, buf, None, buf, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_components_download(fake, 1, 0, None, buf, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_components_download(fake, 0, 1, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert lib.odo_mesh_components_download(fake, 0, 0, None, None, None, None, None, C.byref(m)) == -1
    p = C.c_void_p(0x5A5A)
    assert lib.odo_mesh_components_labels_dev(None, C.byref(p), C.byref(n)) == -1 and lib.odo_mesh_components_labels_dev(fake, None, C.byref(n)) == -1
    assert lib.odo_mesh_components_labels_dev(fake, C.byref(p), None) == -1 and p.value == 0x5A5A
    assert lib.odo_mesh_components_labels(None, 0, None, C.byref(n)) == -1 and lib.odo_mesh_components_labels(fake, 0, None, None) == -1
    assert lib.odo_mesh_components_labels(fake, -1, buf, C.byref(n)) == -1 and lib.odo_mesh_components_labels(fake, 1, None, C.byref(n)) == -1
    run = lib.odo_mesh_components_run
    assert run(None, C.byref(r), 0, 0, None, None, None, None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert run(fake, None, 0, 0, None, None, None, None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert run(fake, C.byref(r), -1, 0, None, None, None, None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert run(fake, C.byref(r), 1, 0, None, None, None, None, 0, 0, None, None, None, None, C.byref(n), C.byref(m)) == -1
    assert run(fake, C.byref(r), 0, 0, None, None, None, None, 0, 0, None, None, None, None, None, C.byref(m)) == -1
    assert (n.value, m.value) == (7, 7)
    assert lib.odo_mesh_components_destroy(None) == 0


# ---- model, loops, rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(mc.rows())), ids=mc.row_ids())
def test_model_equals_the_loops_and_the_row_reaches_its_situation(index):
    r = mc.rows()[index]
    M = mc.model_of(index)
    s = M["stats"]
    assert r["holds"](M), (r["name"], s, M["sizes"].tolist()[:16])
    assert s["guard"] == 0
    assert s["triangles_out"] == s["triangles_in"] - s["removed_triangles"] - s["bad_index"] == len(M["tri"])
    assert s["vertices_out"] == s["vertices_in"] - s["removed_vertices"] - s["unreferenced"] == len(M["xyz0"]) == len(M["nrmw"])
    assert r["rule"]["drop"] or s["unreferenced"] == 0
    assert s["components"] == len(M["comps"]) and s["removed_components"] == int((~M["survives"]).sum())
    assert s["largest"] == (int(M["sizes"].max()) if len(M["sizes"]) else 0) and int(M["sizes"].sum()) == s["triangles_in"] - s["bad_index"]
    # a label is its component's smallest vertex index; the surviving triangles are the input's, in order, renumbered
    tri_in, lab = M["tri_in"], M["labels"]
    assert (lab[~M["valid"]] == -1).all() and (lab[M["valid"]] == M["root"][tri_in[M["valid"]][:, 0]]).all()
    kept = np.nonzero(M["vkeep"])[0]
    assert np.array_equal(kept[M["tri"]], tri_in[M["tkeep"]]) if len(M["tri"]) else not M["tkeep"].any()
    # every kept vertex is an input vertex, whole, in ascending order
    assert np.array_equal(mc.bits(M["xyz0"]), mc.bits(r["mesh"]["xyz0"])[kept]) and np.array_equal(mc.bits(M["nrmw"]), mc.bits(r["mesh"]["nrmw"])[kept])
    # the census is edge_use's, before and after (without self-edges there is nothing else to count)
    if not (tri_in[M["valid"]][:, [0, 1, 2]] == tri_in[M["valid"]][:, [1, 2, 0]]).any():
        assert edge_use(tri_in[M["valid"]]) == (s["open_edges"], s["nonmanifold_edges"])
        assert edge_use(M["tri"]) == (s["open_edges_out"], s["nonmanifold_edges_out"])
    assert len(r["mesh"]["xyz0"]) + len(r["mesh"]["tri"]) <= mc.LOOP_ITEMS
    rule = r["rule"]
    assert mc.same_as_loop(M, mc.components_loop(r["mesh"], rule["min_triangles"], rule["keep_largest"], rule["drop"])), r["name"]
    off = mc.components_model(r["mesh"], rule["min_triangles"], rule["keep_largest"], rule["drop"], edge_stats=False)
    assert all(off["stats"][k] == 0 for k in mc.EDGE_STATS) and {k: v for k, v in off["stats"].items() if k not in mc.EDGE_STATS} == \
        {k: v for k, v in s.items() if k not in mc.EDGE_STATS}


def test_rows_cover_the_launch_geometry():
    """Vertex and triangle counts of 0 and 1, either side of a wave and of a workgroup, a component one past eight workgroups, chains
    as deep as the mesh, both settings of keep_largest and of drop_unreferenced, meshes with and without colour; a table row whose
    probes wrap."""
    k = mc.constants()
    assert k["kMcBlock"] == 256 and k["kMcMaxCapacity"] == 1 << 28 and k["kMcGroups"] == 6
    nv = {len(r["mesh"]["xyz0"]) for r in mc.rows()}
    nt = {len(r["mesh"]["tri"]) for r in mc.rows()}
    assert {0, 1, 63, 64, 65, 255, 256, 257} <= nv and {0, 1, 63, 64, 65, 255, 256, 257} <= nt
    assert max(nv) > 4 * k["kMcBlock"] and max(nt) > 4 * k["kMcBlock"]
    assert any(2049 in mc.model_of(i)["sizes"].tolist() for i in range(len(mc.rows())))
    assert {r["rule"]["keep_largest"] for r in mc.rows()} == {True, False} and {r["rule"]["drop"] for r in mc.rows()} == {True, False}
    assert any(r["mesh"]["rgba"] is not None for r in mc.rows()) and any(r["mesh"]["rgba"] is None for r in mc.rows())
    assert mc.edge_slots(1) == 8 and mc.edge_slots(256) == 2048 and mc.edge_slots(341) == 2048 and mc.edge_slots(342) == 4096
    assert mc.edge_slots(1 << 28) == 1 << 31


@pytest.mark.parametrize("switch", mc.SWITCHES)
def test_each_switch_is_caught_by_exactly_its_rows(switch):
    placed = mc.CAUGHT_BY[switch]
    caught = [name for index, name in enumerate(mc.row_ids()) if mc.differs(index, switch)]
    want = [n for i, n in enumerate(mc.row_ids()) if placed(i)] if callable(placed) else [n for n in mc.row_ids() if n in placed]
    assert caught == want and len(caught) >= 1, (switch, set(caught) ^ set(want))
    if not callable(placed):
        assert len(want) == len(placed)


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------------
def _record(s, mesh=None):
    head = np.array([s["n_v"], s["n_t"], s["min_triangles"], s["keep"], s["drop"], s["colour"], s["edges"], s["vcap"], s["tcap"], 0],
                    np.int64).astype(np.int32).tobytes()
    if mesh is not None:
        head += np.ascontiguousarray(mesh["xyz0"], np.float32).tobytes() + np.ascontiguousarray(mesh["nrmw"], np.float32).tobytes()
        if mesh["rgba"] is not None:
            head += np.ascontiguousarray(mesh["rgba"], np.uint8).tobytes()
        head += np.ascontiguousarray(mesh["tri"], np.int32).tobytes()
    return head


def _row_record(r, edges=1):
    m, rule = r["mesh"], r["rule"]
    return _record(dict(n_v=len(m["xyz0"]), n_t=len(m["tri"]), min_triangles=rule["min_triangles"], keep=int(rule["keep_largest"]),
                        drop=int(rule["drop"]), colour=int(m["rgba"] is not None), edges=edges, vcap=r["capacity"][0], tcap=r["capacity"][1]), m)


def test_shared_header_under_sanitizers(tmp_path):
    """mesh_components_math.h as a g++ program of its own (ASan + UBSan; the parent, size and label arrays, the edge table and the
    outputs heap blocks of exactly their sizes): the reference pass over the kernels' own arrays equals the model byte for byte on
    every row — vertices, attributes, triangles, labels, counters — with the edge table and, for two rows, without; and the three
    checks name the bound of every bad parameter set and pass the outermost good one."""
    exe = str(tmp_path / "mesh_components_math_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", HARNESS, "-o", exe])
    plain = [mc.row_ids().index("a coloured mesh"), mc.row_ids().index("three triangles on one edge")]
    with open(tmp_path / "in.bin", "wb") as f:
        for r in mc.rows():
            f.write(_row_record(r))
        for i in plain:
            f.write(_row_record(mc.rows()[i], edges=0))
        for _, s, _, _, _ in bad_sets():
            f.write(_record(s))
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    assert done.stdout.strip() == f"{len(mc.rows()) + len(plain) + len(bad_sets())} records"
    blob = open(tmp_path / "out.bin", "rb").read()
    at = 0

    def take(dtype, n):
        nonlocal at
        a = np.frombuffer(blob, dtype, n, at)
        at += a.nbytes
        return a

    for index, edges in [(i, 1) for i in range(len(mc.rows()))] + [(i, 0) for i in plain]:
        r, M = mc.rows()[index], mc.model_of(index)
        assert take(np.int32, 3).tolist() == [0, 0, 0], r["name"]
        nv, nt = take(np.int32, 2).tolist()
        assert (nv, nt) == (len(M["xyz0"]), len(M["tri"])), r["name"]
        assert np.array_equal(take(np.uint32, 4 * nv), mc.bits(M["xyz0"]).ravel()), r["name"]
        assert np.array_equal(take(np.uint32, 4 * nv), mc.bits(M["nrmw"]).ravel()), r["name"]
        if M["rgba"] is not None:
            assert np.array_equal(take(np.uint8, 4 * nv), M["rgba"].ravel()), r["name"]
        assert np.array_equal(take(np.int32, 3 * nt), M["tri"].ravel()), r["name"]
        assert np.array_equal(take(np.int32, len(M["labels"])), M["labels"]), r["name"]
        got = dict(zip(mc.STATS, take(np.int64, 19).tolist()))
        want = {k: (v if edges or k not in mc.EDGE_STATS else 0) for k, v in M["stats"].items()}
        assert got == want and (edges or M["stats"]["edges"] > 0), (r["name"], got, want)
    for what, _, check, bound, _ in bad_sets():
        got = take(np.int32, 3).tolist()
        assert got[check] == bound and not any(got[:check]) and not any(got[check + 1:2]), (what, got)   # (a bad capacity also fails the counts)
    assert at == len(blob)
    # the outermost good set passes all three checks: the smallest filter, an empty coloured mesh, the largest bound
    outer = dict(n_v=0, n_t=0, min_triangles=(1 << 31) - 1, keep=1, drop=0, colour=1, edges=1, vcap=1, tcap=1)
    with open(tmp_path / "in2.bin", "wb") as f:
        f.write(_record(outer, dict(xyz0=np.zeros((0, 4)), nrmw=np.zeros((0, 4)), rgba=np.zeros((0, 4)), tri=np.zeros((0, 3)))))
    done = subprocess.run([exe, str(tmp_path / "in2.bin"), str(tmp_path / "out2.bin")], capture_output=True, text=True)
    assert done.returncode == 0 and done.stdout.strip() == "1 records", done.stderr[-2000:]
    blob = open(tmp_path / "out2.bin", "rb").read()
    assert np.frombuffer(blob, np.int32, 5).tolist() == [0, 0, 0, 0, 0]
    assert np.frombuffer(blob, np.int64, 19, 20).tolist() == [0] * 19 and len(blob) == 20 + 19 * 8


# ---- what the method gives: the drive that leaves its box ------------------------------------------------------------------------------------
@pytest.mark.parametrize("grids", [8, 1])
def test_the_drive_mesh_loses_its_debris(grids):
    """The drive's welded mesh: the model's component sizes are the prototype's, min_triangles = 128 removes the six small ones
    and their 208 triangles, the surface sheets stay, and the census agrees with edge_use before and after."""
    want = mc.DRIVE[grids]
    all_in, M = mc.drive_components(grids, 0), mc.drive_components(grids, 128)
    s0, s = all_in["stats"], M["stats"]
    print(f"grids {grids}: min_triangles 0 {s0}; min_triangles 128 {s}")
    assert (s["vertices_in"], s["triangles_in"]) == (want["vertices"], want["triangles"])
    assert sorted(M["sizes"].tolist()) == want["sizes"] == sorted(all_in["sizes"].tolist()) and s["components"] == len(want["sizes"])
    assert s0["removed_components"] == 0 and s0["triangles_out"] == s0["triangles_in"] and s0["vertices_out"] == s0["vertices_in"]
    assert np.array_equal(all_in["tri"], all_in["tri_in"])
    assert s["removed_components"] == 6 and s["removed_triangles"] == 208 and s["bad_index"] == 0 and s["unreferenced"] == 0
    assert s["largest"] == want["sizes"][-1] and s["guard"] == 0
    assert (s["open_edges"], s["open_edges_out"]) == (want["open"], want["open_out"]) and s["nonmanifold_edges"] == 0
    assert edge_use(M["tri_in"]) == (s["open_edges"], s["nonmanifold_edges"]) and edge_use(M["tri"]) == (s["open_edges_out"], s["nonmanifold_edges_out"])
    assert s["triangles_out"] == s["triangles_in"] - 208 and s["vertices_out"] == s["vertices_in"] - s["removed_vertices"]


def test_the_drive_mesh_by_the_loops():
    assert mc.same_as_loop(mc.drive_components(8, 128), mc.components_loop(mc.drive_welded(8), 128))


# ---- code object ---------------------------------------------------------------------------------------------------------------------------
def test_component_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        assert vgprs <= 64 and lds <= 256, key                               # eight waves per SIMD, a few words per wave of LDS
