"""Launch paths the moving volume's shift is held to (tests/test_volume_shift_cases_cpu.py, tests/test_gpu_volume_shift_cases.py): the
launch constants read out of volume_shift.hip.h and launch_volume_shift, the path every quad of a row takes through shift_quad, a
replay of volume_shift_kernel's walk with switches that each leave out one thing, the table of rows — each with the branch it is in
the table for, as a predicate on those paths and on the launch geometry —, the chain of 27 back-to-back shifts, and the inputs and
model results of every row. Nothing here imports the GPU library.

The models are the ones of tests/test_volume_shift_cpu.py, imported unchanged. A row's inputs and the points of its pre-shift grid are
computed once per process (the tall grids and the 1 M-voxel grids take the longest) and shared by the shifts of the row."""
import functools
import os
import re

import numpy as np

import geometry_cases as G
from test_volume_cpu import extract_model, params, words
from test_volume_colour_cpu import point_colours_model, random_colour
from test_volume_shift_cpu import edge_list, grids, leaves_model, random_grid, shift_model, spill_model, window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "odometry_amd", "csrc")
FILL = 0xABABABAB           # what every destination word holds before a shift (test_gpu_volume_shift._prefill)
OFF0 = (1, 0, 0)            # where _prefill leaves the window


# ---- launch constants -----------------------------------------------------------------------------------------------------------
def plane_cap_matches():
    """Every `a.nz < N ? a.nz : M` inside launch_volume_shift's body, as (N, M) strings: the cap on gridDim.y."""
    src = open(os.path.join(CSRC, "volume_shift_kernels.hip")).read()
    body = re.search(r"void\s+launch_volume_shift\s*\([^)]*\)\s*\{(.*?)\n\}", src, re.S).group(1)
    return re.findall(r"a\.nz\s*<\s*(\d+)\s*\?\s*a\.nz\s*:\s*(\d+)", body)


@functools.lru_cache(maxsize=None)
def constants():
    """kVolShiftLanes and kVolShiftRows of volume_shift.hip.h, plane_cap of launch_volume_shift, and the extraction's block and scan
    sizes (geometry_cases.constants: the spill's count and scan walk the grid as the extraction does)."""
    out = {}
    for m in re.finditer(r"^constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, "volume_shift.hip.h")).read(), re.M):
        out[m.group(1)] = int(m.group(2))
    caps = plane_cap_matches()
    assert len(caps) == 1 and caps[0][0] == caps[0][1], caps
    out["plane_cap"] = int(caps[0][0])
    vol = G.constants()
    out["kVolExtBlock"], out["kVolScanThreads"] = vol["kVolExtBlock"], vol["kVolScanThreads"]
    return out


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- the paths of shift_quad -----------------------------------------------------------------------------------------------------
def _lanes(nx, dx):
    """Per quad of a row (qpr, 4): the destination x of lane t, whether it lies in the row, and whether its source x + dx lies in the
    old row; and per quad whether shift_quad<Vec> takes the 16-byte load."""
    i = 4 * np.arange((nx + 3) >> 2, dtype=np.int64)[:, None] + np.arange(4, dtype=np.int64)[None, :]
    s = i + dx
    valid, inside = i < nx, (s >= 0) & (s < nx)
    vload = inside[:, 0] & inside[:, 3] if (nx % 4 == 0 and dx % 4 == 0) else np.zeros(len(i), bool)
    return i, valid, inside, vload


def quad_paths(nx, dx, k=None):
    """Which path of shift_quad the quads of one row take under an x shift of dx, as counts per row: `vload` (one 16-byte load),
    `dword_all` (four dword loads, all inside the old row), `partly` (one to three inside), `none`; per trip of the quad loop in
    `per_trip`. build: "vector" (16-byte stores, nx % 4 == 0) or "dword" (dword stores, the row's end guarded); trips of the loop;
    tail: the last quad's trip, how many of its lanes lie in the row (valid), how many of those have their source inside the old
    row (valid_inside), and how many lanes BEHIND the row's end would have one (guarded_inside: what `i0 + t < nx` keeps from
    being read)."""
    k = k or constants()
    lanes = k["kVolShiftLanes"]
    i, valid, inside, vload = _lanes(nx, dx)
    n_in = (valid & inside).sum(1)
    kinds = dict(vload=vload, dword_all=~vload & (n_in == 4), partly=~vload & (n_in > 0) & (n_in < 4), none=~vload & (n_in == 0))
    qpr = len(i)
    trip = np.arange(qpr) // lanes
    trips = _cdiv(qpr, lanes)
    out = {name: int(m.sum()) for name, m in kinds.items()}
    out.update(build="vector" if nx % 4 == 0 else "dword", qpr=qpr, trips=trips, tail_guarded=nx % 4 != 0,
               per_trip=[{name: int(m[trip == t].sum()) for name, m in kinds.items()} for t in range(trips)],
               tail=dict(trip=int(trip[-1]), valid=int(valid[-1].sum()), valid_inside=int((valid & inside)[-1].sum()),
                         guarded_inside=int((~valid & inside)[-1].sum())))
    return out


def paths_line(nx, dx):
    p = quad_paths(nx, dx)
    return (f"dx {dx:5d}: {p['build']} build, {p['trips']} trip(s), vload {p['vload']} dword_all {p['dword_all']} partly {p['partly']} "
            f"none {p['none']}, tail trip {p['tail']['trip']} valid {p['tail']['valid']} inside {p['tail']['valid_inside']} "
            f"guarded-inside {p['tail']['guarded_inside']}")


# ---- volume_shift_kernel's walk, replayed ------------------------------------------------------------------------------------------
def shift_replay(q, w, col, d, info=None, vload_ignores_dx=False, one_quad_trip=False, one_plane_trip=False,
                 tail_unguarded_read=False):
    """The grids after launch_volume_shift as the kernel walks them: blockIdx.x and threadIdx.y give the row j, blockIdx.y the plane k
    in strides of gridDim.y = min(nz, cap) (vectorised here: one trip of that loop is a run of consecutive planes), threadIdx.x the
    quad in strides of kVolShiftLanes; a quad takes the 16-byte load or the four guarded dword loads as shift_quad decides, and the
    16-byte store or the guarded dword stores by the build. Destination words nobody writes keep 0xAB. Returns what shift_model
    returns. info (a dict) receives `loaded`: the number of source words read (a 16-byte load counts four).

    Each switch leaves out one thing: vload_ignores_dx reads the 16 bytes at i0 instead of i0 + dx; one_quad_trip and one_plane_trip
    stop the two loops after their first trip; tail_unguarded_read leaves `i0 + t < nx` out of the load's condition, so lanes behind
    the row's end read the old row's word at i0 + t + dx when that lies inside it. The dword build's store keeps its own guard, so
    the last switch changes what is read and not what is written: it shows in `loaded` alone."""
    k = constants()
    lanes, rows, cap = k["kVolShiftLanes"], k["kVolShiftRows"], k["plane_cap"]
    nz, ny, nx = q.shape
    dx, dy, dz = (int(x) for x in d)
    srcs = [words(q, w)] + ([np.ascontiguousarray(col).view(np.uint32).reshape(-1)] if col is not None else [])
    dsts = [np.full(nz * ny * nx, FILL, np.uint32) for _ in srcs]
    vec = nx % 4 == 0
    i, valid, inside, vload = _lanes(nx, dx)
    qpr = len(i)
    load = (inside & (valid | tail_unguarded_read)) & ~vload[:, None]            # the dword path's loads
    load |= vload[:, None]
    at = np.where(vload[:, None] & vload_ignores_dx, i, i + dx)                  # source x of every lane that loads
    store = np.ones_like(valid) if vec else valid
    grid_y = min(nz, cap)
    loaded = 0
    for bx in range(_cdiv(ny, rows)):
        for ty in range(rows):
            j = bx * rows + ty
            if j >= ny:
                continue
            sj = j + dy
            j_in = 0 <= sj < ny
            for k0 in range(0, grid_y if one_plane_trip else nz, grid_y):        # blockIdx.y = 0 .. grid_y - 1, the k0 // grid_y-th trip
                ks = np.arange(k0, min(k0 + grid_y, nz), dtype=np.int64)
                sk = ks + dz
                row_in = j_in & (sk >= 0) & (sk < nz)
                drow = (ks * ny + j) * nx
                srow = np.where(row_in, (sk * ny + sj) * nx, 0)
                for q0 in range(0, lanes if one_quad_trip else qpr, lanes):      # threadIdx.x = 0 .. lanes - 1
                    sl = slice(q0, min(q0 + lanes, qpr))
                    m_load = row_in[:, None, None] & load[sl][None]
                    m_store = np.broadcast_to(store[sl][None], m_load.shape)
                    s_at = (srow[:, None, None] + at[sl][None])[m_load]
                    d_at = (drow[:, None, None] + i[sl][None])[m_store]
                    loaded += int(m_load.sum())
                    for src, dst in zip(srcs, dsts):
                        wv = np.zeros(m_load.shape, np.uint32)
                        wv[m_load] = src[s_at]
                        dst[d_at] = wv[m_store]
    if info is not None:
        info["loaded"] = loaded
    q2 = (dsts[0] & 0xFFFF).astype(np.uint16).view(np.int16).reshape(q.shape)
    w2 = (dsts[0] >> 16).astype(np.uint16).reshape(w.shape)
    c2 = dsts[1].view(np.uint8).reshape(col.shape) if col is not None else None
    return q2, w2, c2


def stays(dims, d):
    """How many voxels of the new grid take an old voxel's value: what a shift has to read, per grid."""
    return int(np.prod([max(0, n - abs(int(dc))) for n, dc in zip(dims, d)]))


def second_trip_planes(nz, dz, k=None):
    """(inside, outside): how many planes of the second and later trips of the plane loop have their source plane inside / outside
    the old grid."""
    cap = (k or constants())["plane_cap"]
    ks = np.arange(cap, nz, dtype=np.int64)
    ok = (ks + dz >= 0) & (ks + dz < nz)
    return int(ok.sum()), int((~ok).sum())


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _uniq(shifts):
    out = []
    for d in shifts:
        d = tuple(int(x) for x in d)
        if d not in out and d != (0, 0, 0):
            out.append(d)
    return out


def _dx(*dxs):
    return [(x, 0, 0) for x in dxs]


def _dy(ny):
    """The y shifts every short-row grid is put through as well (ny against kVolShiftRows)."""
    return [(0, 1, 0), (0, -1, 0), (0, ny - 1, 0), (0, ny, 0)]


def _paths(row):
    return [quad_paths(row["dims"][0], d[0]) for d in row["shifts"]]


def _vload_one_trip(row):
    ps = _paths(row)
    return all(p["build"] == "vector" and p["trips"] == 1 for p in ps) and \
        sum(1 for p, d in zip(ps, row["shifts"]) if p["vload"] > 0 and d[0] != 0) >= 3 and \
        any(p["vload"] > 0 and d[0] > 0 for p, d in zip(ps, row["shifts"])) and \
        any(p["vload"] > 0 and d[0] < 0 for p, d in zip(ps, row["shifts"])) and \
        any(p["vload"] > 0 and d[0] != 0 and d[1] != 0 and d[2] != 0 for p, d in zip(ps, row["shifts"]))


def _dword_loads_vector_store(row):
    ps = [p for p, d in zip(_paths(row), row["shifts"]) if d[0] != 0]
    return all(p["build"] == "vector" and p["vload"] == 0 for p in ps) and any(p["partly"] > 0 for p in ps) and \
        any(p["partly"] > 0 and p["none"] > 0 for p in ps) and any(p["dword_all"] > 0 for p in ps)


def _later(p, kind):
    return sum(t[kind] for t in p["per_trip"][1:])


def _vector_trips(row):
    """(A quad partly inside on a later trip is asserted over the class: the second trip of 260 words is a single quad.)"""
    ps = [p for p, d in zip(_paths(row), row["shifts"]) if d[0] != 0]
    return all(p["build"] == "vector" and p["trips"] >= 2 for p in ps) and any(_later(p, "vload") > 0 for p in ps) and \
        any(_later(p, "dword_all") > 0 for p in ps) and any(_later(p, "none") > 0 for p in ps)


def _dword_trips(row):
    """Two or more trips in the dword build, the guarded tail quad on a later trip; over the shifts its lanes inside the row have
    their sources all inside the old row, and all outside it (partly: asserted over the class, a tail of one lane cannot)."""
    ps = [p for p, d in zip(_paths(row), row["shifts"]) if d[0] != 0]
    return all(p["build"] == "dword" and p["trips"] >= 2 and p["tail_guarded"] and p["tail"]["trip"] >= 1 for p in ps) and \
        any(p["tail"]["valid_inside"] == p["tail"]["valid"] for p in ps) and any(p["tail"]["valid_inside"] == 0 for p in ps) and \
        any(p["tail"]["guarded_inside"] > 0 for p in ps)


def _short_rows(row):
    ps = [p for p, d in zip(_paths(row), row["shifts"]) if d[0] != 0]
    return row["dims"][0] < 4 and all(p["qpr"] == 1 and p["build"] == "dword" for p in ps) and \
        any(p["partly"] > 0 for p in ps) and any(p["tail"]["guarded_inside"] > 0 for p in ps)


def _tall(row):
    """More planes than the cap, and over the shifts the planes of the second trip have rows both inside and outside the old grid
    (with j inside: dy = 0 or a row that stays)."""
    nz = row["dims"][2]
    got = [second_trip_planes(nz, d[2]) for d in row["shifts"] if abs(d[1]) < row["dims"][1]]
    return nz > constants()["plane_cap"] and any(a > 0 for a, _ in got) and any(b > 0 for _, b in got)


def _scan_chunk(over):
    def holds(row):
        k = constants()
        blocks = _cdiv(int(np.prod(row["dims"])), k["kVolExtBlock"])
        return blocks == k["kVolScanThreads"] + over
    return holds


def _row(cls, dims, shifts, why, holds, unobserved=0.2, dy=True):
    shifts = _uniq(list(shifts) + (_dy(dims[1]) if dy else []))
    return dict(name="%s %dx%dx%d" % ((cls,) + tuple(dims)), cls=cls, dims=tuple(dims), shifts=shifts, colour=True, why=why, holds=holds,
                unobserved=unobserved, dy=dy)


def _tall_shifts(extra=()):
    return [(0, 0, 1), (0, 0, -1), (0, 0, 65535), (0, 0, -65535), (0, 0, 65536), (1, -1, -65535)] + list(extra)


SHIFT = (
    [_row("vload", (nx, ny, nz), _dx(4, -4, 8, -8, nx - 4, -(nx - 4)) + [(4, 1, -1)],
          "the 16-byte load with dx != 0, one trip of the quad loop", _vload_one_trip) for nx, ny, nz in ((8, 4, 3), (256, 5, 2))] +
    [_row("dword-loads", (nx, ny, nz), _dx(1, 2, -3, nx - 1, -(nx - 1)),
          "16-byte stores fed by four dword loads, quads partly inside the old row", _dword_loads_vector_store)
     for nx, ny, nz in ((8, 4, 3), (256, 5, 2))] +
    [_row("trips-vector", dims, _dx(4, -4, 256, -256, 260, -3, 5),
          "the vector build's quad loop runs two or three times, every path on a later trip", _vector_trips)
     for dims in ((260, 3, 3), (512, 4, 2), (516, 3, 3))] +
    [_row("trips-dword", dims, _dx(1, -1, 3, 4, -4, 256, -257, 257),
          "the dword build's quad loop runs two or three times and ends in a guarded tail quad, inside and outside the old row",
          _dword_trips) for dims in ((257, 6, 2), (259, 3, 3), (261, 6, 2), (513, 2, 3))] +
    [_row("short", dims, _dx(1, -1, -2), "rows shorter than a quad", _short_rows) for dims in ((2, 3, 5), (3, 2, 2))] +
    [_row("tall", (2, 2, 65537), _tall_shifts(), "more planes than gridDim.y may hold: the plane loop runs twice", _tall, dy=False),
     _row("tall", (4, 2, 65536), _tall_shifts([(4, 0, 0)]), "the same in the vector build, one plane on the second trip", _tall, dy=False),
     _row("tall", (3, 5, 65539), _tall_shifts(), "the same with two blocks in x and four planes on the second trip", _tall, dy=False)] +
    [_row("scan", (1024, 32, 32), [(4, 0, 0), (0, -1, 1)], "the spill's scan: the blocks end exactly with a chunk", _scan_chunk(0),
          unobserved=0.7, dy=False),
     _row("scan", (1025, 32, 32), [(4, 0, 0), (0, -1, 1)], "the spill's scan: one block over a chunk", _scan_chunk(1),
          unobserved=0.7, dy=False)])

CLASSES = ("vload", "dword-loads", "trips-vector", "trips-dword", "short", "tall", "scan")

# One row of each build runs additionally without a colour grid (src_col == nullptr) and with a store made before enable_colour.
NO_COLOUR = ("trips-vector 260x3x3", "trips-dword 259x3x3")


def names():
    return [r["name"] for r in SHIFT]


def find(name):
    return next(r for r in SHIFT if r["name"] == name)


def class_holds():
    """What the table has to hold as a whole: every class is there; the multi-trip classes have rows of two and of three trips; a
    guarded tail quad is met partly inside the old row; ny lies below, at and above kVolShiftRows among the rows given y shifts."""
    k = constants()
    trips = {c: {p["trips"] for r in SHIFT if r["cls"] == c for p in _paths(r)} for c in ("trips-vector", "trips-dword")}
    partly = any(0 < p["tail"]["valid_inside"] < p["tail"]["valid"] for r in SHIFT if r["cls"] == "trips-dword" for p in _paths(r))
    later_partly = any(_later(p, "partly") > 0 for r in SHIFT if r["cls"] == "trips-vector" for p in _paths(r))
    nys = {r["dims"][1] for r in SHIFT if r["dy"]}
    emptied = any(stays(r["dims"], d) == 0 for r in SHIFT if r["cls"] == "tall" for d in r["shifts"])
    return dict(classes={r["cls"] for r in SHIFT} == set(CLASSES), trips=all(t >= {2, 3} for t in trips.values()), tail_partly=partly,
                later_partly=later_partly, tall_emptied=emptied,
                ny={k["kVolShiftRows"] - 2, k["kVolShiftRows"] - 1, k["kVolShiftRows"], k["kVolShiftRows"] + 1} <= nys,
                no_colour={find(n)["cls"] for n in NO_COLOUR} == {"trips-vector", "trips-dword"})


# The rows the suite held the shift to before this table: every grid of test_volume_shift_cpu.rows() under shifts_for, and the two
# grids of test_gpu_volume_shift.test_launch_geometries_match_the_model under their two shifts.
EARLIER_GEOMETRY_ROWS = [((1024, 32, 33), (1, 0, 0)), ((1024, 32, 33), (-1, -1, -1)), ((130, 7, 9), (1, 0, 0)), ((130, 7, 9), (-1, -1, -1))]


# ---- inputs and model results ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def inputs(name):
    """(p, q, w, col) of a row: a random grid with the row's share of voxels never observed, random colours."""
    row = find(name)
    n = names().index(name)
    p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=row["dims"], vs=0.05, origin=(-1.3, 0.1, 0.7))
    q, w = random_grid(row["dims"], 100 + n)
    if row["unobserved"] > 0.2:
        rng = np.random.default_rng(200 + n)
        w[rng.uniform(size=w.shape) < row["unobserved"]] = 0
        q[w == 0] = 0
    return p, q, w, random_colour(q.shape, 300 + n)


@functools.lru_cache(maxsize=2)
def _points(name, off):
    """extract_model's and point_colours_model's points of the row's grid in the window `off`, with their edges: what spill_model
    computes anew for every shift, once."""
    p, q, w, col = inputs(name)
    P, N = extract_model(q, w, window(p, off))
    return P, N, point_colours_model(q, w, col), edge_list(q, w)


def spill(name, d, off=OFF0, colour=True):
    """spill_model(q, w, col, window(p, off), d) of the row, from the points computed once (held equal to spill_model on the small
    rows by tests/test_volume_shift_cases_cpu.py)."""
    p, q, w, col = inputs(name)
    P, N, Cc, e = _points(name, off)
    lv = leaves_model(q.shape, d)
    b = e[:, :3].copy()
    b[np.arange(len(e)), e[:, 3]] += 1
    m = lv[e[:, 2], e[:, 1], e[:, 0]] | lv[b[:, 2], b[:, 1], b[:, 0]]
    return P[m], N[m], (Cc[m] if colour else None)


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
CHAIN = [(1, 0, 0)] * 24 + [(0, 1, 0)] * 3


@functools.lru_cache(maxsize=None)
def chain():
    """The random 64 x 4 x 4 grid of test_volume_shift_cpu.grids() under CHAIN, from the model: the spill of every shift, the final
    grids and window, and the three capacities — more than the total, the sum of the first 12 spills (the store fills at a spill's
    end), and that sum plus one point more than half of the 13th (the store fills inside a spill)."""
    p, q, w, col = grids()["random 64x4x4"]
    off, spills = (0, 0, 0), []
    for d in CHAIN:
        spills.append(spill_model(q, w, col, window(p, off), d))
        q, w, col = shift_model(q, w, col, d)
        off = tuple(a + b for a, b in zip(off, d))
    counts = [len(s[0]) for s in spills]
    at12 = sum(counts[:12])
    return dict(p=p, spills=spills, counts=counts, q=q, w=w, col=col, off=off,
                capacities=(sum(counts) + 7, at12, at12 + counts[12] // 2 + 1))
