"""The mesh of the leaving slab (odo_volume_enable_spill_mesh, odo_volume_spill_mesh): the model, the same as
plain loops, the store's all-or-nothing rule, the table of rows with what each is there for, and three mutants of the model.

The model is the existing one plus two masks: spill_mesh_model is test_volume_mesh_cpu.mesh_model(detail=True) (and
test_volume_colour_cpu.mesh_colours_model) on the pre-shift grid, filtered by "edge spilled" and "cell spilled" and renumbered into
the store. It is the yardstick of tests/test_gpu_volume_spill_mesh.py, which asks the GPU for the same bits."""
import collections
import functools

import numpy as np

from test_volume_cpu import bits, params
from test_volume_colour_cpu import mesh_colours_model, random_colour
from test_volume_mesh_cpu import DIRS, mesh_model
from test_volume_shift_cpu import _leaves, grids, leaves_model, random_grid, shift_model, window

f32 = np.float32


# ---- the predicates (closed form, vectorised) ----------------------------------------------------------------------------------------
def stay_box(d, n):
    """[lo, hi] of the old voxels that stay on an axis of n voxels under d; lo > hi: none."""
    return max(0, d), min(n - 1, n - 1 + d)


def _cell_axis(c, d, n):
    lo, hi = stay_box(d, n)
    return (c < lo) | (c + 1 > hi)


def cell_spilled(i, j, k, d, dims, variant=None):
    """The cells with low corners (i, j, k) (arrays), all eight corners inside the grid: at least one corner leaves."""
    if variant == "low-corner":   # MUTANT: a cell is spilled only when its low corner leaves
        lv = leaves_model((dims[2], dims[1], dims[0]), d)
        return lv[k, j, i]
    return _cell_axis(i, d[0], dims[0]) | _cell_axis(j, d[1], dims[1]) | _cell_axis(k, d[2], dims[2])


def _edge_axis(a, step, d, n):
    if step:
        return _cell_axis(a, d, n)
    return ((a >= 1) & _cell_axis(a - 1, d, n)) | ((a <= n - 2) & _cell_axis(a, d, n))


def edge_spilled(i, j, k, e, d, dims, variant=None):
    """The edges (voxel (i, j, k), direction e) (arrays), far end inside the grid: an edge of at least one spilled cell."""
    e = np.asarray(e)
    out = np.zeros(len(e), bool)
    for x, de in enumerate(DIRS):
        m = e == x
        if variant == "a-or-b":   # MUTANT: the point spill's predicate
            lv = leaves_model((dims[2], dims[1], dims[0]), d)
            out[m] = lv[k[m], j[m], i[m]] | lv[k[m] + de[2], j[m] + de[1], i[m] + de[0]]
        else:
            out[m] = (_edge_axis(i[m], de[0], d[0], dims[0]) | _edge_axis(j[m], de[1], d[1], dims[1]) |
                      _edge_axis(k[m], de[2], d[2], dims[2]))
    return out


def _ijk(word, dims):
    return word % dims[0], (word // dims[0]) % dims[1], word // (dims[0] * dims[1])


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def spill_masks(vkeys, tkeys, d, dims, variant=None):
    vm = edge_spilled(*_ijk(vkeys // 7, dims), vkeys % 7, d, dims, variant)
    tm = cell_spilled(*_ijk(tkeys // 12, dims), d, dims, variant)
    return vm, tm


def spill_of_mesh(mesh, colours, d, dims, fill=(0, 0), variant=None):
    """What a shift by d appends to a store that holds fill[0] vertices, from the pre-shift mesh (mesh_model(detail=True)) and its
    colours (or None): xyz0, nrmw, tri (the store's indices), rgba."""
    xyz0, nrmw, tri, vkeys, tkeys = mesh
    vm, tm = spill_masks(vkeys, tkeys, d, dims, variant)
    rank = np.cumsum(vm) - 1
    t = tri[tm]
    if variant not in ("low-corner", "a-or-b"):
        assert vm[t].all()                                   # no spilled triangle names an unspilled vertex
    base = 0 if variant == "no-offset" else fill[0]          # MUTANT: indices not offset by the store's fill
    return xyz0[vm], nrmw[vm], (rank[t] + base).astype(np.int32), (colours[vm] if colours is not None else None)


def spill_mesh_model(q, w, col, p, d, fill=(0, 0), variant=None):
    """What a shift by d of the grid (q, w, col) in the window p appends to the mesh store: xyz0, nrmw, tri and rgba (None without
    colour)."""
    return spill_of_mesh(mesh_model(q, w, p, detail=True), mesh_colours_model(q, w, col) if col is not None else None, d, p["dims"],
                         fill, variant)


# ---- the same as plain loops ---------------------------------------------------------------------------------------------------------
def spilled_sets_loop(d, dims):
    """From the definition alone: the set of spilled cells (some corner leaves, decided corner by corner) and the set of spilled edges
    (voxel, e): the edges of those cells, cell by cell."""
    nx, ny, nz = dims
    cells, edges = set(), set()
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                corners = [(i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)) for c in range(8)]
                if not any(_leaves(v, d, dims) for v in corners):
                    continue
                cells.add((i, j, k))
                for a in corners:
                    for e, de in enumerate(DIRS):
                        if tuple(a[c] + de[c] for c in range(3)) in corners:
                            edges.add((a, e))
    return cells, edges


def spill_mesh_loop(q, w, col, p, d, fill=(0, 0)):
    """spill_mesh_model with the two predicates from spilled_sets_loop and the renumbering as a loop."""
    dims = p["dims"]
    xyz0, nrmw, tri, vkeys, tkeys = mesh_model(q, w, p, detail=True)
    rgba = mesh_colours_model(q, w, col) if col is not None else None
    cells, edges = spilled_sets_loop(d, dims)
    new, keep = {}, []
    for n, key in enumerate(vkeys):
        word, e = int(key) // 7, int(key) % 7
        a = (word % dims[0], (word // dims[0]) % dims[1], word // (dims[0] * dims[1]))
        if (a, e) in edges:
            new[n] = fill[0] + len(keep)
            keep.append(n)
    out = []
    for n, key in enumerate(tkeys):
        word = int(key) // 12
        if (word % dims[0], (word // dims[0]) % dims[1], word // (dims[0] * dims[1])) in cells:
            out.append([new[int(x)] for x in tri[n]])
    keep = np.array(keep, np.int64)
    return xyz0[keep], nrmw[keep], np.array(out, np.int32).reshape(-1, 3), (rgba[keep] if rgba is not None else None)


# ---- the store -------------------------------------------------------------------------------------------------------------------------
def empty_store(colour):
    return dict(xyz0=np.zeros((0, 4), f32), nrmw=np.zeros((0, 4), f32), tri=np.zeros((0, 3), np.int32),
                rgba=np.zeros((0, 4), np.uint8) if colour else None, dropped=(0, 0))


def store_append(store, spill_fn, capacities):
    """The all-or-nothing rule: spill_fn(fill) -> (xyz0, nrmw, tri, rgba) for a store that holds `fill`; appended whole when both
    counts fit what is left of both capacities, else both counts go to the dropped totals. Returns (store, appended)."""
    fill = (len(store["xyz0"]), len(store["tri"]))
    P, N, T, Cc = spill_fn(fill)
    if fill[0] + len(P) > capacities[0] or fill[1] + len(T) > capacities[1]:
        return dict(store, dropped=(store["dropped"][0] + len(P), store["dropped"][1] + len(T))), False
    return dict(xyz0=np.concatenate([store["xyz0"], P]), nrmw=np.concatenate([store["nrmw"], N]), tri=np.concatenate([store["tri"], T]),
                rgba=np.concatenate([store["rgba"], Cc]) if store["rgba"] is not None else None, dropped=store["dropped"]), True


def run_shifts(p, q, w, col, shifts, capacities, off=(0, 0, 0), variant=None):
    """The store, the grids and the window after `shifts` enqueued in turn, from the model; also which spills were appended."""
    store, taken = empty_store(col is not None), []
    for d in shifts:
        if tuple(d) != (0, 0, 0):
            mesh = mesh_model(q, w, window(p, off), detail=True)
            colours = mesh_colours_model(q, w, col) if col is not None else None
            store, ok = store_append(store, lambda fill: spill_of_mesh(mesh, colours, d, p["dims"], fill, variant), capacities)
            taken.append(ok)
            q, w, col = shift_model(q, w, col, d)
            off = tuple(a + b for a, b in zip(off, d))
    return dict(store=store, taken=taken, q=q, w=w, col=col, off=off)


def store_equal(a, b):
    return (len(a["xyz0"]) == len(b["xyz0"]) and len(a["tri"]) == len(b["tri"]) and np.array_equal(bits(a["xyz0"]), bits(b["xyz0"])) and
            np.array_equal(bits(a["nrmw"]), bits(b["nrmw"])) and np.array_equal(a["tri"], b["tri"]) and
            (a["rgba"] is None or np.array_equal(a["rgba"], b["rgba"])) and tuple(a["dropped"]) == tuple(b["dropped"]))


# ---- the partition -------------------------------------------------------------------------------------------------------------------
def triangle_multiset(xyz0, nrmw, tri, base=0):
    """Counter of triangles as three (x, y, z, weight) bit patterns, rotated to the smallest triple first (the cyclic order kept)."""
    out = collections.Counter()
    V = np.concatenate([bits(xyz0)[:, :3], bits(nrmw)[:, 3:]], 1)
    for t in tri:
        c = [tuple(int(x) for x in V[int(i) - base]) for i in t]
        r = min(range(3), key=lambda s: c[s])
        out[(c[r], c[(r + 1) % 3], c[(r + 2) % 3])] += 1
    return out


def vertex_set(xyz0, nrmw):
    return {tuple(int(x) for x in row) for row in np.concatenate([bits(xyz0), bits(nrmw)[:, 3:]], 1)}


# ---- the grids and the shifts --------------------------------------------------------------------------------------------------------
DYADIC_DIMS = [(2, 2, 2), (3, 2, 2), (6, 5, 4), (9, 8, 7)]


@functools.lru_cache(maxsize=None)
def dyadic_grids():
    """name -> (p, q, w, col): random grids on a dyadic lattice (voxel size 0.25, origin in quarters), so that a voxel centre is the
    same fp32 number in every window and positions can be compared bit for bit across a shift; 0 % and 20 % never observed."""
    out = {}
    for n, dims in enumerate(DYADIC_DIMS):
        for holes in (0, 20):
            p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=dims, vs=0.25, origin=(-1.25, 0.5, 0.75))
            q, w = random_grid(dims, 500 + n)
            if not holes:
                w = np.where(w == 0, np.uint16(7), w)
                q = np.where(q == 0, np.int16(-5), q)
            out["dyadic %dx%dx%d %d%%" % (dims + (holes,))] = (p, q, w, random_colour(q.shape, 600 + n))
    return out


def shifts_for(dims):
    """One voxel either way on each axis, two on one, mixed ones, all but one layer, everything, nothing."""
    nx, ny, nz = dims
    return [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 2, 0), (1, -1, 1), (3, -2, 1), (nx - 1, 0, 0),
            (0, -(ny - 1), 0), (0, 0, nz - 1), (nx, 0, 0), (0, -ny, 0), (0, 0, nz), (0, 0, 0)]


def vertices_without_triangles():
    """A 2 x 2 x 2 grid with one corner never observed: its one cell is not live, and every edge between observed voxels of opposite
    sign carries a vertex."""
    p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=(2, 2, 2), vs=0.25, origin=(-1.25, 0.5, 0.75))
    q = np.array([[[900, -700], [-300, 1200]], [[-1500, 400], [250, 0]]], np.int16)
    w = np.array([[[3, 9], [4, 1]], [[2, 6], [8, 0]]], np.uint16)
    return p, q, w, random_colour(q.shape, 77, holes=0.0)


# ---- the rows: (grid, shifts) and what each is there for -------------------------------------------------------------------------------
def _first(name, d):
    p, q, w, col = all_grids()[name]
    mesh = mesh_model(q, w, p, detail=True)
    return p, mesh, spill_masks(mesh[3], mesh[4], d, p["dims"])


def _holds_far_corner(name, d):
    """A spilled cell with triangles whose low corner stays: it is spilled by its far corners alone, the +x+y+z one among them. (A
    cell whose ONLY leaving corner is +x+y+z cannot exist: a voxel leaves by one axis, and the cell's corner that differs from +x+y+z
    on the other two axes alone shares that coordinate and leaves with it; the leaving corners of a cell number 4, 6, 7 or 8.)"""
    p, mesh, (vm, tm) = _first(name, d)
    i, j, k = _ijk(mesh[4] // 12, p["dims"])
    lv = leaves_model(mesh_shape(p), d)
    return bool((tm & ~lv[k, j, i] & lv[k + 1, j + 1, i + 1]).any())


def _holds_both_ends_stay(name, d):
    p, mesh, (vm, tm) = _first(name, d)
    i, j, k = _ijk(mesh[3] // 7, p["dims"])
    de = np.array(DIRS)[mesh[3] % 7]
    lv = leaves_model(mesh_shape(p), d)
    return bool((vm & ~lv[k, j, i] & ~lv[k + de[:, 2], j + de[:, 1], i + de[:, 0]]).any())


def _holds_no_triangle(name, d):
    p, mesh, (vm, tm) = _first(name, d)
    return bool(vm.any() and not tm.any())


def _holds_everything(name, d):
    p, mesh, (vm, tm) = _first(name, d)
    return bool(any(abs(x) >= n for x, n in zip(d, p["dims"])) and vm.all() and tm.all() and len(vm) > 0 and len(tm) > 0)


def _holds_nothing(name, d):
    return tuple(d) == (0, 0, 0)


def mesh_shape(p):
    return (p["dims"][2], p["dims"][1], p["dims"][0])


@functools.lru_cache(maxsize=None)
def all_grids():
    g = dict(dyadic_grids())
    g["no live cell 2x2x2"] = vertices_without_triangles()
    for name in ("random 64x4x4", "random 65x5x4"):
        g[name] = grids()[name]
    return g


# (row name, grid, shifts enqueued in turn, predicate on the first shift, what it is there for)
ROWS = [
    ("far corner", "dyadic 9x8x7 20%", [(-1, -1, -1)], _holds_far_corner, "a spilled cell whose low corner stays (mutant: low-corner)"),
    ("both ends stay", "dyadic 6x5x4 0%", [(1, 0, 0)], _holds_both_ends_stay, "a spilled vertex on an edge with both ends staying (mutant: a-or-b)"),
    ("no triangle", "no live cell 2x2x2", [(0, 1, 0)], _holds_no_triangle, "a spill with vertices and no triangle"),
    ("everything", "dyadic 6x5x4 20%", [(0, -5, 0)], _holds_everything, "|d| >= n: everything spills"),
    ("nothing", "dyadic 3x2x2 0%", [(0, 0, 0)], _holds_nothing, "d = 0: nothing enqueued"),
    ("second spill", "dyadic 9x8x7 20%", [(1, -1, 1), (0, 2, 0)], lambda name, d: True, "indices offset by the store's fill (mutant: no-offset)"),
    ("mixed", "dyadic 9x8x7 0%", [(3, -2, 1)], lambda name, d: True, "a slab on all three axes"),
    ("one block", "random 64x4x4", [(1, 0, 0), (0, 0, -1)], lambda name, d: True, "64 x 4 x 4: one block"),
    ("partial block", "random 65x5x4", [(-1, 0, 0), (0, 1, 0)], lambda name, d: True, "65 x 5 x 4: a partial last block, nx % 64 != 0"),
    ("2x2x2", "dyadic 2x2x2 0%", [(1, 0, 0)], lambda name, d: True, "the smallest grid: one cell"),
    ("3x2x2", "dyadic 3x2x2 20%", [(-1, 0, 0), (1, 0, 0)], lambda name, d: True, "two cells, one of them spilled"),
]
MUTANT_ROWS = {"low-corner": "far corner", "a-or-b": "both ends stay", "no-offset": "second spill"}


def row(name):
    return next(r for r in ROWS if r[0] == name)


@functools.lru_cache(maxsize=None)
def row_result(name, variant=None, colour=True):
    _, grid, shifts, _, _ = row(name)
    p, q, w, col = all_grids()[grid]
    return run_shifts(p, q, w, col if colour else None, shifts, (1 << 14, 1 << 14), variant=variant)


# ---- the all-or-nothing rule: two shifts into stores one item short ------------------------------------------------------------------
TWO_SHIFTS = ("dyadic 9x8x7 20%", [(1, -1, 1), (0, 2, 0)])


@functools.lru_cache(maxsize=None)
def one_short():
    """name -> (capacities, expected `taken`): the two spills of TWO_SHIFTS into stores that are one item short, on either capacity,
    of the first spill and of both; and one that fits both exactly."""
    p, q, w, col = all_grids()[TWO_SHIFTS[0]]
    full = run_shifts(p, q, w, col, TWO_SHIFTS[1], (1 << 14, 1 << 14))
    s1 = run_shifts(p, q, w, col, TWO_SHIFTS[1][:1], (1 << 14, 1 << 14))["store"]
    v1, t1 = len(s1["xyz0"]), len(s1["tri"])
    v12, t12 = len(full["store"]["xyz0"]), len(full["store"]["tri"])
    v2, t2 = v12 - v1, t12 - t1
    assert 0 < v2 < v1 and 0 < t2 < t1      # the second spill is the smaller one: it fits a store that refused the first
    return {"exact": ((v12, t12), [True, True]),
            "first, a vertex short": ((v1 - 1, 1 << 14), [False, True]), "first, a triangle short": ((1 << 14, t1 - 1), [False, True]),
            "second, a vertex short": ((v12 - 1, 1 << 14), [True, False]), "second, a triangle short": ((1 << 14, t12 - 1), [True, False])}


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
CHAIN = [(1, 0, 0)] * 24 + [(0, 1, 0)] * 3


@functools.lru_cache(maxsize=None)
def chain():
    """The random 64 x 4 x 4 grid under CHAIN, from the model: every spill's counts, and three pairs of capacities: one that fits, one
    that fills exactly at the 12th spill's end (so every later spill with a vertex is refused), and one that refuses the 5th spill, in
    the middle, by one triangle, and so still takes the first later spill that is smaller."""
    p, q, w, col = grids()["random 64x4x4"]
    big = run_shifts(p, q, w, col, CHAIN, (1 << 16, 1 << 16))
    counts, off, q1, w1, c1 = [], (0, 0, 0), q, w, col
    for d in CHAIN:
        mesh = mesh_model(q1, w1, window(p, off), detail=True)
        vm, tm = spill_masks(mesh[3], mesh[4], d, p["dims"])
        counts.append((int(vm.sum()), int(tm.sum())))
        q1, w1, c1 = shift_model(q1, w1, c1, d)
        off = tuple(a + b for a, b in zip(off, d))
    v = [c[0] for c in counts]
    t = [c[1] for c in counts]
    at12 = (sum(v[:12]), sum(t[:12]))
    middle = (1 << 16, sum(t[:4]) + t[4] - 1)
    return dict(p=p, q=q, w=w, col=col, counts=counts, final=big, capacities=[(1 << 16, 1 << 16), at12, middle])
