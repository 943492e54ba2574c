"""The mesh of the leaving slab (odo_volume_enable_spill_mesh, odo_volume_spill_mesh; api.TsdfVolume.enable_spill_mesh / spilled_mesh /
save_mesh_ply(spill=True)) without a GPU: the ABI and the refusals, the model of tests/volume_spill_mesh_cases.py pinned by a plain-
loop version, the partition of the mesh into what is spilled and what stays, the rows' predicates, the all-or-nothing rule, three
mutants of the model, the shared header as a stand-alone program under sanitizers, the new kernels' code-object metadata, and the
drive that leaves its box (DESIGN.md sections 9.9 and 9.13)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import volume_spill_mesh_cases as M
from test_volume_cpu import bits, plane_errors
from test_volume_mesh_cpu import DIRS, mesh_model
from test_volume_shift_cpu import _leaves, drive_case, leaves_model, offset_model, shift_model, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["odo_volume_enable_spill_mesh", "odo_volume_spill_mesh", "odo_volume_spill_mesh_time", "odo_debug_volume_spill_mesh_guard"]
NEW_KERNELS = ["volume_spill_mesh_count_kernel", "volume_spill_mesh_scan_kernel", "volume_spill_mesh_vertex_kernel",
               "volume_spill_mesh_triangle_kernel", "volume_spill_mesh_colour_kernel", "volume_spill_mesh_advance_kernel"]


# ---- ABI and refusals ----------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    for name in ("enable_spill_mesh", "spilled_mesh", "save_mesh_ply", "spill_mesh_time"):
        assert callable(getattr(api.TsdfVolume, name))
    import inspect
    sig = inspect.signature(api.TsdfVolume.save_mesh_ply)
    assert list(sig.parameters) == ["self", "path", "spill"] and sig.parameters["spill"].default is False   # additive


def test_bad_arguments_are_refused_before_touching_a_device():
    """Every case below is refused by the validation alone: the volume's handle is a fake that is never dereferenced."""
    from odometry_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(8)
    d = (C.c_int * 3)(1, 0, 0)
    n, m = C.c_long(0), C.c_long(0)
    buf = np.zeros(8, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    tri = np.zeros(3, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.odo_volume_enable_spill_mesh(None, 1, 1) == -1
    for vc, tc in ((0, 1), (1, 0), (-1, 1), ((1 << 28) + 1, 1), (1, (1 << 28) + 1)):
        assert lib.odo_volume_enable_spill_mesh(fake, vc, tc) == -1, (vc, tc)
        assert "out of range" in L.last_error()
    assert lib.odo_volume_spill_mesh(None, 0, 0, None, None, None, None, C.byref(n), C.byref(m), None, 0) == -1
    assert lib.odo_volume_spill_mesh(fake, 0, 0, None, None, None, None, None, C.byref(m), None, 0) == -1
    assert lib.odo_volume_spill_mesh(fake, 0, 0, None, None, None, None, C.byref(n), None, None, 0) == -1
    assert lib.odo_volume_spill_mesh(fake, -1, 0, fp, fp, None, tri, C.byref(n), C.byref(m), None, 0) == -1
    assert lib.odo_volume_spill_mesh(fake, 1, (1 << 28) + 1, fp, fp, None, tri, C.byref(n), C.byref(m), None, 0) == -1
    assert lib.odo_volume_spill_mesh(fake, 1, 1, None, fp, None, tri, C.byref(n), C.byref(m), None, 0) == -1
    assert lib.odo_volume_spill_mesh(fake, 1, 1, fp, fp, None, None, C.byref(n), C.byref(m), None, 0) == -1
    assert "odo_volume_spill_mesh" in L.last_error()
    assert lib.odo_volume_spill_mesh_time(None, d, 1, fp) == -1 and lib.odo_volume_spill_mesh_time(fake, None, 1, fp) == -1
    assert lib.odo_volume_spill_mesh_time(fake, d, 1, None) == -1
    assert lib.odo_volume_spill_mesh_time(fake, d, 0, fp) == -1 and lib.odo_volume_spill_mesh_time(fake, d, 10001, fp) == -1
    assert lib.odo_debug_volume_spill_mesh_guard(None, C.byref(n)) == -1 and lib.odo_debug_volume_spill_mesh_guard(fake, None) == -1


# ---- the predicates ------------------------------------------------------------------------------------------------------------------
def _rows_of_predicates():
    out = [(dims, d) for dims in M.DYADIC_DIMS for d in M.shifts_for(dims)]
    return out + [((3, 2, 2), (2 ** 31 - 1, 0, 0)), ((3, 2, 2), (0, -2 ** 31, 0)), ((4, 3, 2), (-2, 1, 0))]


def _closed_form(dims, d):
    """near[n], edge[n][7] (2: the far end is outside) and cell[...] from the vectorised closed forms of the cases file."""
    nx, ny, nz = dims
    k, j, i = [a.ravel() for a in np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")]
    edge = np.full((len(i), 7), 2, np.uint8)
    for e, de in enumerate(DIRS):
        inside = (i + de[0] < nx) & (j + de[1] < ny) & (k + de[2] < nz)
        edge[inside, e] = M.edge_spilled(i[inside], j[inside], k[inside], np.full(inside.sum(), e), d, dims)
    kc, jc, ic = [a.ravel() for a in np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")]
    return edge, M.cell_spilled(ic, jc, kc, d, dims).astype(np.uint8)


def _from_the_definition(dims, d):
    nx, ny, nz = dims
    small = tuple(int(np.clip(x, -max(dims), max(dims))) for x in d)   # (beyond +-n a shift is the same shift)
    cells, edges = M.spilled_sets_loop(small, dims)
    near = np.zeros((nz, ny, nx), np.uint8)
    edge = np.full((nz, ny, nx, 7), 2, np.uint8)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                near[k, j, i] = any(_leaves((i + a, j + b, k + c), small, dims) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
                                    if 0 <= i + a < nx and 0 <= j + b < ny and 0 <= k + c < nz)
                for e, de in enumerate(DIRS):
                    if i + de[0] < nx and j + de[1] < ny and k + de[2] < nz:
                        edge[k, j, i, e] = ((i, j, k), e) in edges
    cell = np.array([[[(i, j, k) in cells for i in range(nx - 1)] for j in range(ny - 1)] for k in range(nz - 1)], np.uint8)
    return near.ravel(), edge.reshape(-1, 7), cell.ravel()


def test_closed_forms_equal_the_definition_and_near_covers_every_spilled_edge_and_cell():
    for dims, d in _rows_of_predicates():
        if max(abs(x) for x in d) > 2 ** 20:
            continue
        near, edge, cell = _from_the_definition(dims, d)
        e2, c2 = _closed_form(dims, d)
        assert np.array_equal(edge, e2) and np.array_equal(cell, c2), (dims, d)
        owns = (edge == 1).any(1)
        nx, ny, nz = dims
        low = np.zeros((nz, ny, nx), bool)
        low[:nz - 1, :ny - 1, :nx - 1] = cell.reshape(nz - 1, ny - 1, nx - 1) > 0
        assert not ((owns | low.ravel()) & (near == 0)).any(), (dims, d)      # a thread that is not near may load nothing
        # a cell's leaving corners number 0, 4, 6, 7 or 8: never the +x+y+z corner alone (see the row "far corner")
        lv = leaves_model((nz, ny, nx), tuple(int(np.clip(x, -max(dims), max(dims))) for x in d))
        count = sum(lv[c >> 2 & 1:nz - 1 + (c >> 2 & 1), c >> 1 & 1:ny - 1 + (c >> 1 & 1), (c & 1):nx - 1 + (c & 1)].astype(int) for c in range(8))
        assert set(np.unique(count)) <= {0, 4, 6, 7, 8} and np.array_equal(count.ravel() > 0, cell > 0), (dims, d)


def test_shared_header_as_a_standalone_program_under_sanitizers(tmp_path):
    """volume_shift_math.h's new functions compiled by g++ with AddressSanitizer and UBSan: byte for byte the definition's answers,
    for every grid and shift of the table and for shifts at the ends of int."""
    if shutil.which("g++") is None:
        pytest.skip("no g++ here")
    exe = str(tmp_path / "volume_spill_mesh_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "volume_spill_mesh_harness.cpp"), "-o", exe])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for dims, d in _rows_of_predicates():
        open(src, "wb").write(np.array([*dims, *d], "<i4").tobytes())
        out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
        near, edge, cell = _from_the_definition(dims, d)
        assert open(dst, "rb").read() == near.tobytes() + edge.tobytes() + cell.tobytes(), (dims, d)


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2]) and
            a[2].dtype == b[2].dtype and np.array_equal(a[3], b[3]))


def test_model_equals_the_plain_loops_bit_for_bit():
    n = 0
    for name, (p, q, w, col) in M.dyadic_grids().items():
        for d in M.shifts_for(p["dims"]):
            for fill in ((0, 0), (37, 5)):
                a, b = M.spill_mesh_model(q, w, col, p, d, fill), M.spill_mesh_loop(q, w, col, p, d, fill)
                assert _same(a, b), (name, d, fill)
                n += len(a[0])
    assert n > 10000


def test_spill_and_what_stays_partition_the_mesh():
    """Triangles before = spilled + after as multisets of world positions and weights; vertices before = spilled | after as sets, the
    seam's in both; no spilled triangle names an unspilled vertex (asserted inside the model)."""
    for name, (p, q, w, col) in M.dyadic_grids().items():
        before = mesh_model(q, w, p)
        tb, vb = M.triangle_multiset(*before), M.vertex_set(before[0], before[1])
        for d in M.shifts_for(p["dims"]):
            sp = M.spill_mesh_model(q, w, None, p, d)
            q2, w2, _ = shift_model(q, w, None, d)
            after = mesh_model(q2, w2, window(p, d))
            assert M.triangle_multiset(*sp[:3]) + M.triangle_multiset(*after) == tb, (name, d)
            vs_, va = M.vertex_set(sp[0], sp[1]), M.vertex_set(after[0], after[1])
            assert vs_ | va == vb, (name, d)
            if name == "dyadic 9x8x7 20%" and d == (1, -1, 1):
                print(name, d, f"{len(sp[2])} of {len(before[2])} triangles and {len(sp[0])} of {len(before[0])} vertices spill, "
                      f"{len(sp[0]) + len(after[0]) - len(before[0])} vertices are on the seam")
                assert 0 < len(sp[2]) < len(before[2]) and len(sp[0]) + len(after[0]) > len(before[0])


def test_every_row_holds_what_it_is_there_for():
    for name, grid, shifts, holds, why in M.ROWS:
        assert holds(grid, shifts[0]), (name, why)
    r = M.row_result("nothing")
    assert r["taken"] == [] and len(r["store"]["xyz0"]) == 0 and r["off"] == (0, 0, 0)
    r = M.row_result("no triangle")
    assert len(r["store"]["xyz0"]) > 0 and len(r["store"]["tri"]) == 0
    r = M.row_result("second spill")
    assert r["taken"] == [True, True] and r["store"]["tri"].max() < len(r["store"]["xyz0"])


@pytest.mark.parametrize("variant", sorted(M.MUTANT_ROWS))
def test_each_mutant_is_caught_by_the_row_placed_for_it(variant):
    name = M.MUTANT_ROWS[variant]
    assert not M.store_equal(M.row_result(name)["store"], M.row_result(name, variant)["store"]), (variant, name)


def test_a_spill_is_appended_whole_or_not_at_all():
    """Two shifts into stores that are one item short, on either capacity, of the first spill and of the second."""
    p, q, w, col = M.all_grids()[M.TWO_SHIFTS[0]]
    full = M.run_shifts(p, q, w, col, M.TWO_SHIFTS[1], (1 << 14, 1 << 14))["store"]
    first = M.run_shifts(p, q, w, col, M.TWO_SHIFTS[1][:1], (1 << 14, 1 << 14))["store"]
    for name, (caps, taken) in M.one_short().items():
        r = M.run_shifts(p, q, w, col, M.TWO_SHIFTS[1], caps)
        s = r["store"]
        assert r["taken"] == taken, name
        v2, t2 = len(full["xyz0"]) - len(first["xyz0"]), len(full["tri"]) - len(first["tri"])
        if taken == [True, True]:
            assert M.store_equal(s, full), name
        elif taken == [True, False]:
            assert M.store_equal(s, dict(first, dropped=(v2, t2))), name
        else:   # the first refused, the second appended from the store's start: its indices start at 0
            assert s["dropped"] == (len(first["xyz0"]), len(first["tri"])) and len(s["xyz0"]) == v2 and len(s["tri"]) == t2, name
            assert np.array_equal(s["tri"], full["tri"][len(first["tri"]):] - len(first["xyz0"])), name
            assert np.array_equal(bits(s["xyz0"]), bits(full["xyz0"][len(first["xyz0"]):])), name
        assert s["tri"].size == 0 or (0 <= s["tri"].min() and s["tri"].max() < len(s["xyz0"])), name   # a complete mesh at any time


def test_the_chain_spills_at_every_shift_and_its_capacities_cut_where_they_should():
    c = M.chain()
    assert len(c["counts"]) == 27 and all(v > 0 for v, t in c["counts"]) and c["counts"][4][1] > 0, c["counts"]
    assert sum(t > 0 for v, t in c["counts"]) >= 14 and any(t == 0 for v, t in c["counts"]), c["counts"]   # (spills without a triangle too)
    p, q, w, col = c["p"], c["q"], c["w"], c["col"]
    fits, at12, middle = [M.run_shifts(p, q, w, col, M.CHAIN, caps) for caps in c["capacities"]]
    assert all(fits["taken"]) and fits["store"]["dropped"] == (0, 0)
    assert at12["taken"] == [True] * 12 + [False] * 15
    assert (len(at12["store"]["xyz0"]), len(at12["store"]["tri"])) == c["capacities"][1]
    t = middle["taken"]
    assert t[:5] == [True] * 4 + [False] and any(t[5:]), t          # refused in the middle, later smaller spills still appended
    print("chain counts", c["counts"], "middle taken", t)


# ---- the code object -----------------------------------------------------------------------------------------------------------------
def test_spill_mesh_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)), int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
                print(name, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
    assert sorted(found) == sorted(NEW_KERNELS), found
    assert all(v == (0, 0, 0) for v in found.values()), found


# ---- the drive that leaves its box ---------------------------------------------------------------------------------------------------
def test_the_drive_keeps_its_surface_as_one_mesh():
    """DESIGN.md section 9.9's drive with a mesh store: the store and the final window's mesh, every vertex within half a voxel of its
    nearest plane (the bound test_pinned_case_against_the_corridors_planes asserts for mesh vertices), and the store's axis-edge
    vertices whose edge loses a voxel equal the point store's points bit for bit, spill by spill."""
    c = drive_case()
    p = c["p"]
    from test_volume_cpu import empty_grid, integrate_model
    q, w = empty_grid(p)
    off, n, store = (0, 0, 0), 0, M.empty_store(False)
    for raw, T, d in zip(c["depth"], c["poses"], c["shifts"]):
        if d != (0, 0, 0):
            mesh = mesh_model(q, w, window(p, off), detail=True)
            fill = len(store["xyz0"])
            store, ok = M.store_append(store, lambda f: M.spill_of_mesh(mesh, None, d, p["dims"], f), (1 << 20, 1 << 20))
            assert ok
            # the point spill's points are the axis-edge vertices with a or b leaving, in the same order
            vm, _ = M.spill_masks(mesh[3], mesh[4], d, p["dims"])
            pm, _ = M.spill_masks(mesh[3], mesh[4], d, p["dims"], "a-or-b")
            assert not (pm & ~vm).any()
            axis = (mesh[3] % 7 < 3) & pm
            Ps, Ns = c["spills"][n]
            assert np.array_equal(bits(mesh[0][axis][:, :3]), bits(Ps[:, :3])) and np.array_equal(bits(mesh[1][axis]), bits(Ns)), n
            assert np.array_equal(bits(store["xyz0"][fill:][(mesh[3][vm] % 7 < 3) & pm[vm]]), bits(mesh[0][axis]))
            q, w, _ = shift_model(q, w, None, d)
            off = offset_model(off, d)
            n += 1
        q, w, _, _ = integrate_model(q, w, raw, T, window(p, off))
    assert n == 13 and off == c["off"] and np.array_equal(w, c["w"]) and np.array_equal(q, c["q"])
    final = mesh_model(q, w, window(p, off))
    P = np.concatenate([store["xyz0"], final[0]])
    N = np.concatenate([store["nrmw"], final[1]])
    dist = plane_errors(P, N, p["vs"])[0]
    print(f"{n} shifts; the store holds {len(store['xyz0'])} vertices and {len(store['tri'])} triangles, the window's mesh "
          f"{len(final[0])} and {len(final[2])}; distance / voxel median {np.median(dist):.3f} max {dist.max():.3f}")
    assert len(store["xyz0"]) > len(final[0]) and len(store["tri"]) > len(final[2])      # most of the surface is in the store
    assert 0 <= store["tri"].min() and store["tri"].max() < len(store["xyz0"])
    assert dist.max() <= 0.5, dist.max()
