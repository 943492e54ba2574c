"""The mesh welder's specification as code (include/odometry_hip.h, odo_mesh_weld_create), shared by
tests/test_mesh_weld_cpu.py and tests/test_gpu_mesh_weld.py: the constants read out of the kernels' headers, the numpy model
(np.unique on the keys, a lexicographic sort on the rotated triples), the same rule as plain loops over Python integers and
dictionaries written independently of it, and the rows — each with the situation it is in the table for as a predicate on the
model's intermediates. Nothing here loads the GPU library.

A row is dict(name, mesh, rule, capacity, holds). mesh = dict(xyz0 (n, 4) float32, nrmw (n, 4) float32, tri (m, 3) int32, rgba (n, 4)
uint8 or None); rule = dict(eps, origin, grids, drop). The model can be told to get one of five things wrong (SWITCHES); CAUGHT_BY
names, for each, the rows that are in the table to notice. Meshes and model results are computed once per process and shared."""
import functools
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "odometry_amd", "csrc")
STATS = ("vertices_in", "vertices_out", "merged", "keyless", "unreferenced", "triangles_in", "triangles_out", "degenerate", "duplicate",
         "bad_index", "guard", "passes")
SWITCHES = ("trunc", "largest_rep", "no_rotation", "mirror_duplicate", "whole_cell")
LOOP_ITEMS = 20000            # rows with no more vertices + triangles than this go through the loops
f32, u64 = np.float32, np.uint64
LIMIT = 1 << 20
M64 = (1 << 64) - 1
INT32_MAX = (1 << 31) - 1


def constants():
    """{kName: value} of every `constexpr int kName = <integer or 1 << n>;` line of mesh_weld_math.h and mesh_weld.hip.h."""
    out = {}
    for name in ("mesh_weld_math.h", "mesh_weld.hip.h"):
        for m in re.finditer(r"^constexpr\s+int\s+(k\w+)\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*;", open(os.path.join(CSRC, name)).read(), re.M):
            out[m.group(1)] = int(m.group(2)) << int(m.group(3) or 0)
    return out


def n_slots(capacity):
    """weld_slots: 2^ceil(log2(2 capacity))."""
    s = 2
    while s < 2 * capacity:
        s <<= 1
    return s


def mix(k):
    """weld_hash: the splitmix64 finaliser on uint64 (products modulo 2^64)."""
    k = np.array(k, u64)
    with np.errstate(over="ignore"):
        k ^= k >> u64(30)
        k *= u64(0xbf58476d1ce4e5b9)
        k ^= k >> u64(27)
        k *= u64(0x94d049bb133111eb)
        return k ^ (k >> u64(31))


def mix_int(k):
    k ^= k >> 30
    k = (k * 0xbf58476d1ce4e5b9) & M64
    k ^= k >> 27
    k = (k * 0x94d049bb133111eb) & M64
    return k ^ (k >> 31)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def mesh(xyz, tri, seed=0, colour=False):
    """A mesh from (n, 3) positions and (m, 3) indices: e = the vertex's index, a random normal and weight, random colours."""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    n = len(xyz)
    xyz0 = np.concatenate([xyz, np.arange(n, dtype=f32)[:, None]], 1)
    nrmw = rng.standard_normal((n, 4)).astype(f32)
    return dict(xyz0=xyz0, nrmw=nrmw, tri=np.asarray(tri, np.int32).reshape(-1, 3),
                rgba=rng.integers(0, 256, (n, 4)).astype(np.uint8) if colour else None)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def cells_of(xyz0, eps, origin, grid, trunc=False, whole_cell=False):
    """(cells (n, 3) int64, keyless (n,) bool): three fp32 operations and a floor per coordinate. The switches: truncation towards
    zero for the floor; an offset of a whole cell for the half."""
    inv = f32(1.0) / f32(eps)
    x = np.asarray(xyz0, f32)[:, :3]
    o = np.asarray(origin, f32)
    off = np.array([(f32(1.0) if whole_cell else f32(0.5)) if (grid >> a) & 1 else f32(0.0) for a in range(3)], f32)
    with np.errstate(all="ignore"):
        d = x - o
        s = d * inv
        t = s + off
        f = np.trunc(t) if trunc else np.floor(t)
        keyless = (~np.isfinite(x) | ~np.isfinite(f) | ~(np.abs(f) < f32(LIMIT))).any(1)
        c = np.where(keyless[:, None], 0, f).astype(np.int64)
    return c, keyless


def pack(c):
    """weld_key's packing: the cells + 2^20 as three 21-bit fields."""
    f = (np.asarray(c, np.int64) + LIMIT).astype(u64)
    return f[:, 0] | (f[:, 1] << u64(21)) | (f[:, 2] << u64(42))


def weld_pass(m, eps, origin, grid, drop, trunc=False, largest_rep=False, no_rotation=False, mirror_duplicate=False, whole_cell=False):
    """One pass: dict(mesh, counts, cells, keyless, key, rep, rot, bad, degenerate, duplicate, tkeep, vkeep). The switches beyond
    cells_of's: the largest index of a key as its representative; the duplicate test on the triple as it came, not rotated; the
    duplicate test blind to the winding."""
    xyz0, nrmw, tri, rgba = m["xyz0"], m["nrmw"], m["tri"], m["rgba"]
    n_v, n_t = len(xyz0), len(tri)
    idx = np.arange(n_v, dtype=np.int64)
    c, keyless = cells_of(xyz0, eps, origin, grid, trunc, whole_cell)
    key = np.where(keyless, (u64(1) << u64(63)) | idx.astype(u64), pack(c))          # (a keyless vertex: a key of its own)
    if n_v:
        if largest_rep:
            _, first, inverse = np.unique(key[::-1], return_index=True, return_inverse=True)
            rep = (n_v - 1 - first)[inverse][::-1]
        else:
            _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
            rep = first[inverse]
    else:
        rep = idx
    t = tri.astype(np.int64)
    bad = ((t < 0) | (t >= n_v)).any(1) if n_t else np.zeros(0, bool)
    r = rep[np.where(bad[:, None], 0, t)] if n_v else np.zeros((n_t, 3), np.int64)
    deg = ~bad & ((r[:, 0] == r[:, 1]) | (r[:, 1] == r[:, 2]) | (r[:, 0] == r[:, 2]))
    valid = ~bad & ~deg
    shift = np.argmin(r, 1) if n_t else np.zeros(0, np.int64)
    rot = np.take_along_axis(r, (shift[:, None] + np.arange(3)[None, :]) % 3, 1) if n_t else r
    probe = np.sort(r, 1) if mirror_duplicate else (r if no_rotation else rot)
    dup = np.zeros(n_t, bool)
    v = np.nonzero(valid)[0]
    if len(v):
        order = v[np.lexsort((v, probe[v, 2], probe[v, 1], probe[v, 0]))]           # equal triples together, in input order
        same = (probe[order[1:]] == probe[order[:-1]]).all(1)
        dup[order[1:][same]] = True
    tkeep = valid & ~dup
    ref = np.zeros(n_v, bool)
    ref[rot[tkeep].ravel()] = True
    own = rep == idx
    vkeep = own & (ref | (not drop))
    new = np.cumsum(vkeep) - 1
    out = dict(xyz0=xyz0[vkeep], nrmw=nrmw[vkeep], tri=new[rot[tkeep]].astype(np.int32).reshape(-1, 3),
               rgba=rgba[vkeep] if rgba is not None else None)
    counts = dict(merged=int((~own).sum()), keyless=int(keyless.sum()), unreferenced=int((own & ~vkeep).sum()), degenerate=int(deg.sum()),
                  duplicate=int(dup.sum()), bad_index=int(bad.sum()))
    return dict(mesh=out, counts=counts, cells=c, keyless=keyless, key=key, rep=rep, rot=rot, bad=bad, degenerate=deg, duplicate=dup,
                tkeep=tkeep, vkeep=vkeep)


def weld_model(m, eps, origin=(0.0, 0.0, 0.0), grids=8, drop=True, **switches):
    """dict(xyz0, nrmw, tri, rgba, stats, passes): grids = 1 is pass 0, grids = 8 passes 0 .. 7 chained. stats as odo_mesh_weld_stats:
    the first pass's inputs, the last pass's outputs, the passes' counts summed."""
    assert grids in (1, 8)
    stats = dict.fromkeys(STATS, 0)
    stats["vertices_in"], stats["triangles_in"] = len(m["xyz0"]), len(m["tri"])
    cur = dict(xyz0=np.ascontiguousarray(m["xyz0"], f32).reshape(-1, 4), nrmw=np.ascontiguousarray(m["nrmw"], f32).reshape(-1, 4),
               tri=np.ascontiguousarray(m["tri"], np.int32).reshape(-1, 3), rgba=m.get("rgba"))
    passes = []
    for k in range(grids):
        p = weld_pass(cur, eps, origin, k, drop, **switches)
        passes.append(p)
        cur = p["mesh"]
        for name, n in p["counts"].items():
            stats[name] += n
        stats["passes"] += 1
    stats["vertices_out"], stats["triangles_out"] = len(cur["xyz0"]), len(cur["tri"])
    return dict(cur, stats=stats, passes=passes)


# ---- the same as plain loops ---------------------------------------------------------------------------------------------------------
def weld_loop(m, eps, origin=(0.0, 0.0, 0.0), grids=8, drop=True):
    """The rule read off the prose, a vertex and a triangle at a time: a dictionary from a cell to the first vertex in it, a set of
    the rotated triples seen. (xyz0, nrmw, tri, rgba, stats) with the arrays as lists of rows of bit patterns / integers."""
    inv = f32(1.0) / f32(eps)
    V = [[int(b) for b in row] for row in np.concatenate([bits(m["xyz0"]).reshape(-1, 4), bits(m["nrmw"]).reshape(-1, 4)], 1)]
    C = [[int(b) for b in row] for row in m["rgba"]] if m.get("rgba") is not None else None
    X = [[f32(c) for c in row[:3]] for row in np.asarray(m["xyz0"], f32).reshape(-1, 4)]
    T = [[int(i) for i in row] for row in np.asarray(m["tri"]).reshape(-1, 3)]
    stats = dict.fromkeys(STATS, 0)
    stats["vertices_in"], stats["triangles_in"] = len(V), len(T)
    for k in range(grids):
        first, rep = {}, []
        for i, x in enumerate(X):
            cell = []
            for a in range(3):
                with np.errstate(all="ignore"):
                    t = (x[a] - f32(origin[a])) * inv + (f32(0.5) if (k >> a) & 1 else f32(0.0))
                if not math.isfinite(float(x[a])) or not math.isfinite(float(t)) or abs(math.floor(float(t))) >= LIMIT:
                    cell = None
                    break
                cell.append(math.floor(float(t)))
            if cell is None:
                stats["keyless"] += 1
                rep.append(i)
                continue
            rep.append(first.setdefault(tuple(cell), i))
            stats["merged"] += rep[i] != i
        seen, kept, named = set(), [], set()
        for t in T:
            if any(i < 0 or i >= len(V) for i in t):
                stats["bad_index"] += 1
                continue
            r = [rep[i] for i in t]
            if len(set(r)) < 3:
                stats["degenerate"] += 1
                continue
            while r[0] != min(r):
                r = r[1:] + r[:1]
            if tuple(r) in seen:
                stats["duplicate"] += 1
                continue
            seen.add(tuple(r))
            kept.append(r)
            named.update(r)
        new, keep = {}, []
        for i in range(len(V)):
            if rep[i] != i:
                continue
            if drop and i not in named:
                stats["unreferenced"] += 1
                continue
            new[i] = len(keep)
            keep.append(i)
        V, X, T = [V[i] for i in keep], [X[i] for i in keep], [[new[i] for i in r] for r in kept]
        C = [C[i] for i in keep] if C is not None else None
        stats["passes"] += 1
    stats["vertices_out"], stats["triangles_out"] = len(V), len(T)
    return [v[:4] for v in V], [v[4:] for v in V], T, C, stats


def same_as_loop(M, loop):
    """The model's result against weld_loop's, bit for bit."""
    xyz0, nrmw, tri, rgba, stats = loop
    return (bits(M["xyz0"]).tolist() == xyz0 and bits(M["nrmw"]).tolist() == nrmw and M["tri"].tolist() == tri and
            (M["rgba"] is None) == (rgba is None) and (rgba is None or M["rgba"].tolist() == rgba) and M["stats"] == stats)


def same_result(a, b):
    return (np.array_equal(bits(a["xyz0"]), bits(b["xyz0"])) and np.array_equal(bits(a["nrmw"]), bits(b["nrmw"])) and
            np.array_equal(a["tri"], b["tri"]) and (a["rgba"] is None) == (b["rgba"] is None) and
            (a["rgba"] is None or np.array_equal(a["rgba"], b["rgba"])) and a["stats"] == b["stats"])


# ---- what a mesh is worth: its edges -------------------------------------------------------------------------------------------------
def edge_use(tri):
    """(edges used by exactly one triangle, edges used by more than two), edges undirected."""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e.sort(1)
    _, n = np.unique(e[:, 0] << 32 | e[:, 1], return_counts=True)
    return int((n == 1).sum()), int((n > 2).sum())


# ---- the rows: generic meshes -----------------------------------------------------------------------------------------------------------
def lattice(n_v, n_t, seed, colour=False, span=6, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """n_v vertices in the cells of a span^3 block that starts at cell (1, 1, 1), each between 0.1 and 0.4 of the cell's edge from the
    cell's low faces: the half-cell grids put them into the same cells, and truncation is floor on them. n_t random triangles, of
    which no two name the same three cells: a lattice mesh has degenerate triangles and no duplicates, rotated or mirrored."""
    rng = np.random.default_rng(seed)
    cell = rng.integers(1, 1 + span, (n_v, 3))
    xyz = ((cell + rng.uniform(0.1, 0.4, (n_v, 3))) * scale + np.asarray(shift)).astype(f32)
    tri, seen = [], set()
    while len(tri) < n_t:
        t = rng.integers(0, n_v, 3).tolist()
        c = tuple(sorted(tuple(cell[i]) for i in t))
        if len(set(c)) == 3 and c in seen:
            continue
        seen.add(c)
        tri.append(t)
    return mesh(xyz, tri, seed + 1, colour)


def homed(n, capacity, predicate, y=3, z=5, n_cand=1 << 19):
    """n positions (k + 0.25, y + 0.25, z + 0.25), eps 1, origin 0, whose keys are all different and have homes in a table for
    `capacity` vertices that satisfy the predicate: the design of tests/map_hash_cases.py."""
    slots = n_slots(capacity)
    k = np.arange(1, 1 + n_cand)
    cells = np.stack([k, np.full_like(k, y), np.full_like(k, z)], 1)
    home = (mix(pack(cells)) & u64(slots - 1)).astype(np.int64)
    pick = k[predicate(home, slots)][:n]
    assert len(pick) == n, "not enough candidates"
    xyz = np.stack([pick + 0.25, np.full(n, y + 0.25), np.full(n, z + 0.25)], 1).astype(f32)
    assert np.array_equal(np.floor(xyz[:, 0]).astype(np.int64), pick)
    return xyz


def probe_replay(keys, slots):
    """The table after the keys are inserted in order (any order gives the same set of occupied slots): slot -> key, and the
    longest probe."""
    table, longest = {}, 0
    for key in keys:
        s, trips = mix_int(int(key)) & (slots - 1), 0
        while s in table and table[s] != int(key):
            s = (s + 1) & (slots - 1)
            trips += 1
        table[s] = int(key)
        longest = max(longest, trips)
    return table, longest


def _rule(eps=1.0, origin=(0.0, 0.0, 0.0), grids=8, drop=True):
    return dict(eps=eps, origin=tuple(origin), grids=grids, drop=drop)


def _row(name, m, rule, holds, capacity=None):
    return dict(name=name, mesh=m, rule=rule, holds=holds, capacity=capacity or (max(len(m["xyz0"]), 1), max(len(m["tri"]), 1)))


def _p0(M):
    return M["passes"][0]


ULP_FACE = f32(-2.0)


def _ulp_row():
    lo, hi = np.nextafter(ULP_FACE, f32(-np.inf)), np.nextafter(ULP_FACE, f32(0.0))
    xyz = [[lo, 1.25, 1.25], [hi, 1.25, 1.25], [ULP_FACE, 1.25, 1.25], [5.25, 1.25, 1.25], [6.25, 2.25, 1.25], [7.25, 1.25, 1.25]]
    return mesh(xyz, [[0, 3, 4], [1, 3, 4], [2, 3, 5]], 70)   # (the face itself goes with the vertex above it: triangle (1, 3, 5))


def _offset_pairs():
    """Four pairs, eps 1. On an axis a pair either straddles an integer face (0.9 | 1.1: one cell only with the half offset) or a
    half face (1.4 | 1.6: one cell only without it). Pair g straddles integer faces on the axes of g's bits and half faces on the
    others: grid g alone puts it into one cell."""
    xyz, tri = [], []
    for n, g in enumerate((1, 2, 4, 7)):
        base = 10.0 * (n + 1)
        a = [base + (0.9 if (g >> c) & 1 else 0.4) for c in range(3)]
        b = [base + (1.1 if (g >> c) & 1 else 0.6) for c in range(3)]
        far = [[base + 3.25 + c, base + 3.25, base + 3.25] for c in range(3)]
        i = len(xyz)
        xyz += [a, b] + far
        tri += [[i, i + 2, i + 3], [i + 1, i + 2, i + 4]]
    return mesh(xyz, tri, 71)


def _limits():
    big = float(LIMIT)
    xs = [np.nan, np.inf, -np.inf, big - 0.75, big + 0.25, -big + 0.25, -big + 1.25, 3.0e38, -3.0e38]
    xyz = [[x, 1.25, 1.25] for x in xs for _ in range(2)] + [[1.25, np.nan, 1.25], [1.25, 1.25, np.inf], [2.25, 1.25, 1.25], [3.25, 1.25, 1.25]]
    n = len(xyz)
    tri = [[i, n - 2, n - 1] for i in range(n - 2)]
    return mesh(xyz, tri, 72)


def _bad_indices():
    m = lattice(9, 0, 73, span=3)
    m["tri"] = np.array([[0, 1, 2], [-1, 1, 2], [0, 9, 2], [0, 1, INT32_MAX], [-(1 << 31), 1, 2], [3, 4, 5], [9, 9, 9], [-1, -1, -1]], np.int32)
    m["xyz0"][:, :3] = np.array([[c + 1.25, 1.25, 1.25] for c in range(9)], f32)
    return m


def _late_degenerate():
    xyz = [[1.25, 1.25, 1.25], [1.3, 1.3, 1.3], [2.25, 1.25, 1.25], [3.25, 1.25, 1.25]]
    return mesh(xyz, [[0, 1, 2], [0, 2, 3], [1, 2, 3]], 74)


def _rotations():
    xyz = [[c + 1.25, 1.25, 1.25] for c in range(7)]
    return mesh(xyz, [[5, 3, 4], [3, 4, 5], [4, 5, 3], [5, 4, 3], [4, 3, 5], [0, 1, 2], [6, 1, 2]], 75)


def _only_a_dropped_triangle_names_it():
    xyz = [[c + 1.25, 1.25, 1.25] for c in range(6)] + [[1.3, 1.3, 1.3]]
    return mesh(xyz, [[0, 1, 2], [3, 0, 6], [1, 2, 0], [4, 4, 5]], 76)


def _one_cell(n=256):
    rng = np.random.default_rng(77)
    xyz = np.concatenate([4.0 + rng.uniform(0.1, 0.4, (n, 3)), [[1.25, 1.25, 1.25], [2.25, 1.25, 1.25]]]).astype(f32)
    tri = np.concatenate([rng.integers(0, n, (n, 3)), [[i, n, n + 1] for i in range(n)]])
    return mesh(xyz, tri, 78)


@functools.lru_cache(maxsize=None)
def split_grid():
    """A small dyadic grid's mesh, unsplit, and the same surface as save_mesh_ply(spill=True) writes it after one shift: the store's
    mesh in front of the shifted window's. (unsplit, split, p)."""
    import volume_spill_mesh_cases as SM
    from test_volume_mesh_cpu import mesh_model
    from test_volume_shift_cpu import window
    p, q, w, col = SM.all_grids()["dyadic 6x5x4 0%"]
    d = (1, 0, 0)
    whole = mesh_model(q, w, p)
    r = SM.run_shifts(p, q, w, None, [d], (1 << 14, 1 << 14))
    rest = mesh_model(r["q"], r["w"], window(p, r["off"]))
    s = r["store"]
    split = dict(xyz0=np.concatenate([s["xyz0"], rest[0]]), nrmw=np.concatenate([s["nrmw"], rest[1]]),
                 tri=np.concatenate([s["tri"], rest[2] + len(s["xyz0"])]).astype(np.int32), rgba=None)
    return dict(xyz0=whole[0], nrmw=whole[1], tri=whole[2].astype(np.int32), rgba=None), split, p


def cell_triangles(m, eps, origin):
    """The sorted list of triangles as three cells of grid 0, rotated to the smallest first, and the set of cells with a vertex: what
    a welded mesh is, whichever vertex of a cell came first and stands for it."""
    P = [tuple(row) for row in cells_of(m["xyz0"], eps, origin, 0)[0].tolist()]
    out = []
    for t in m["tri"].tolist():
        c = [P[i] for i in t]
        r = min(range(3), key=lambda s: c[s])
        out.append((c[r], c[(r + 1) % 3], c[(r + 2) % 3]))
    return sorted(out), set(P)


@functools.lru_cache(maxsize=None)
def twice_store():
    """The mesh store of tests/volume_stores_cases.py's d, -d, d walk: what left, returned and left again is in it twice."""
    import volume_stores_cases as VS
    s = VS.row_states("twice")[-1]["mesh"]
    p = VS.grid()[0]
    return dict(xyz0=s["xyz0"], nrmw=s["nrmw"], tri=s["tri"].astype(np.int32), rgba=s["rgba"]), p


def _holds_split(M):
    whole, split, p = split_grid()
    W = weld_model(whole, p["vs"] / 64, p["origin"], 1)
    a, b = cell_triangles(M, p["vs"] / 64, p["origin"]), cell_triangles(W, p["vs"] / 64, p["origin"])
    return (M["stats"]["merged"] > W["stats"]["merged"] and a == b and len(a[1]) == len(M["xyz0"]) == len(W["xyz0"]) and
            len(split["xyz0"]) > len(whole["xyz0"]) and len(split["tri"]) == len(whole["tri"]))


def _holds_twice(M):
    t = M["tri"].tolist()
    return M["stats"]["duplicate"] > 0 and M["stats"]["merged"] > 0 and len({tuple(x) for x in t}) == len(t)


def _holds_homes(M):
    slots = n_slots(256)
    keys = _p0(M)["key"].tolist()
    table, longest = probe_replay(keys, slots)
    homes = [mix_int(k) & (slots - 1) for k in keys]
    return (len(set(keys)) == 256 and min(homes) >= slots - 4 and len(set(homes)) == 4 and min(table) == 0 and max(table) == slots - 1 and
            len(table) == 256 and longest >= 250)


@functools.lru_cache(maxsize=None)
def rows():
    out = [
        _row("no vertex, no triangle", lattice(0, 0, 1), _rule(), lambda M: M["stats"]["vertices_out"] == 0 and M["stats"]["passes"] == 8),
        _row("one vertex, no triangle", lattice(1, 0, 2), _rule(drop=False), lambda M: len(M["xyz0"]) == 1 and len(M["tri"]) == 0),
        _row("one vertex, no triangle, dropped", lattice(1, 0, 2), _rule(), lambda M: M["stats"]["unreferenced"] == 1 and len(M["xyz0"]) == 0),
        _row("two vertices, one triangle", mesh([[1.25, 1.25, 1.25], [1.3, 1.3, 1.3]], [[0, 1, 0]], 3), _rule(grids=1, drop=False),
             lambda M: M["stats"]["merged"] == 1 and M["stats"]["degenerate"] == 1 and len(M["xyz0"]) == 1),
        _row("no vertex, one triangle", mesh(np.zeros((0, 3)), [[0, 0, 0]], 4), _rule(grids=1),
             lambda M: M["stats"]["bad_index"] == 1 and M["stats"]["triangles_out"] == 0),
    ]
    for n_v, n_t in ((63, 130), (64, 128), (65, 257), (255, 511), (256, 512), (257, 600)):
        out.append(_row(f"{n_v} vertices, {n_t} triangles", lattice(n_v, n_t, 10 + n_v, span=4 if n_v < 100 else 6),
                        _rule(grids=8 if n_v % 2 else 1),
                        lambda M: M["stats"]["merged"] > 0 and M["stats"]["degenerate"] > 0 and M["stats"]["triangles_out"] > 0 and
                        M["stats"]["duplicate"] == 0))
    out += [
        _row("256 vertices in one cell", _one_cell(), _rule(grids=1),
             lambda M: _p0(M)["counts"]["merged"] == 255 and (_p0(M)["rep"][:256] == 0).all() and M["stats"]["degenerate"] == 256 and
             M["stats"]["duplicate"] == 255 and len(M["tri"]) == 1),
        _row("256 keys homed in the table's last four slots", mesh(homed(256, 256, lambda h, s: h >= s - 4), [[0, 1, 2], [255, 0, 128]], 20),
             _rule(grids=1, drop=False), _holds_homes, capacity=(256, 2)),
        _row("one ulp either side of a face below the origin", _ulp_row(), _rule(grids=1),
             lambda M: _p0(M)["cells"][:3, 0].tolist() == [-3, -2, -2] and _p0(M)["rep"][:3].tolist() == [0, 1, 1]),
        _row("a coordinate exactly on a face", mesh([[3.0, 1.25, 1.25], [3.5, 1.25, 1.25], [np.nextafter(f32(3.0), f32(0.0)), 1.25, 1.25],
                                                     [5.25, 1.25, 1.25], [6.25, 2.25, 1.25]], [[0, 3, 4], [1, 3, 4], [2, 3, 4]], 21),
             _rule(grids=1), lambda M: _p0(M)["cells"][:3, 0].tolist() == [3, 3, 2] and M["stats"]["duplicate"] == 1),
        _row("pairs joined by grid 1, 2, 4 and 7 only", _offset_pairs(), _rule(),
             lambda M: [p["counts"]["merged"] for p in M["passes"]] == [0, 1, 1, 0, 1, 0, 0, 1] and len(M["xyz0"]) == 16),
        _row("the same pairs on one grid", _offset_pairs(), _rule(grids=1), lambda M: M["stats"]["merged"] == 0 and len(M["xyz0"]) == 20),
        _row("not a number, infinities and the ends of a field", _limits(), _rule(grids=1),
             lambda M: _p0(M)["keyless"].tolist() == [True] * 6 + [False] * 2 + [True] * 4 + [False] * 2 + [True] * 6 + [False] * 2 and
             _p0(M)["cells"][[6, 12], 0].tolist() == [LIMIT - 1, -(LIMIT - 1)] and M["stats"]["merged"] == 2),
        _row("the same on eight grids", _limits(), _rule(), lambda M: M["stats"]["keyless"] == 8 * 16 and M["stats"]["merged"] == 2),
        _row("triangles naming -1, n_v and INT32_MAX", _bad_indices(), _rule(grids=1),
             lambda M: _p0(M)["bad"].tolist() == [False, True, True, True, True, False, True, True] and len(M["tri"]) == 2),
        _row("degenerate only after the weld", _late_degenerate(), _rule(grids=1),
             lambda M: _p0(M)["degenerate"].tolist() == [True, False, False] and M["stats"]["duplicate"] == 1 and len(M["tri"]) == 1),
        _row("three rotations and the mirror image", _rotations(), _rule(grids=1),
             lambda M: _p0(M)["duplicate"].tolist() == [False, True, True, False, True, False, False] and
             M["tri"].tolist() == [[3, 4, 5], [3, 5, 4], [0, 1, 2], [1, 2, 6]]),
        _row("a vertex only a dropped triangle names, kept", _only_a_dropped_triangle_names_it(), _rule(grids=1, drop=False),
             lambda M: M["stats"]["unreferenced"] == 0 and len(M["xyz0"]) == 6 and M["stats"]["degenerate"] == 2),
        _row("a vertex only a dropped triangle names, dropped", _only_a_dropped_triangle_names_it(), _rule(grids=1),
             lambda M: M["stats"]["unreferenced"] == 3 and len(M["xyz0"]) == 3 and M["stats"]["duplicate"] == 1),
        _row("a coloured mesh", lattice(300, 700, 30, colour=True), _rule(),
             lambda M: M["rgba"] is not None and len(M["rgba"]) == len(M["xyz0"]) and M["stats"]["merged"] > 0),
        _row("a fine cell about an origin", lattice(200, 500, 31, scale=0.1 / 64, shift=(-5.6, -3.2, 0.5)),
             _rule(eps=0.1 / 64, origin=(-5.6, -3.2, 0.5), grids=1), lambda M: M["stats"]["merged"] > 0 and M["stats"]["triangles_out"] > 0),
    ]
    whole, split, p = split_grid()
    out.append(_row("a dyadic grid split by a spill and put back together", split, _rule(p["vs"] / 64, p["origin"], 1), _holds_split))
    store, p = twice_store()
    out.append(_row("the store of the d, -d, d walk", store, _rule(p["vs"] / 64, p["origin"], 1), _holds_twice))
    return out


def row_ids():
    return [r["name"] for r in rows()]


@functools.lru_cache(maxsize=None)
def model_of(index, switch=None):
    r = rows()[index]
    return weld_model(r["mesh"], r["rule"]["eps"], r["rule"]["origin"], r["rule"]["grids"], r["rule"]["drop"], **({switch: True} if switch else {}))


def differs(index, switch):
    return not same_result(model_of(index), model_of(index, switch))


# Which rows each switch must change; it changes no other.
CAUGHT_BY = {
    "trunc": ("one ulp either side of a face below the origin", "not a number, infinities and the ends of a field",
              "the same on eight grids"),
    # (every row with a merge but the d, -d, d store, whose merged vertices are bit-identical copies at mirrored ranks)
    "largest_rep": lambda i: model_of(i)["stats"]["merged"] > 0 and rows()[i]["name"] != "the store of the d, -d, d walk",
    "no_rotation": ("three rotations and the mirror image", "a vertex only a dropped triangle names, kept",
                    "a vertex only a dropped triangle names, dropped"),
    "mirror_duplicate": ("three rotations and the mirror image",),
    # (a whole cell's offset also pushes the field's last cell over its end)
    "whole_cell": ("pairs joined by grid 1, 2, 4 and 7 only", "the same on eight grids"),
}


# ---- the drive that leaves its box -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def drive_mesh():
    """DESIGN.md section 9.9's drive with a mesh store, as tests/test_volume_spill_mesh_cpu.py's
    test_the_drive_keeps_its_surface_as_one_mesh builds it: the store in front of the final window's mesh, indices offset, as
    save_mesh_ply(spill=True) writes them. (mesh, p)."""
    import volume_spill_mesh_cases as SM
    from test_volume_cpu import empty_grid, integrate_model
    from test_volume_mesh_cpu import mesh_model
    from test_volume_shift_cpu import drive_case, offset_model, shift_model, window
    c = drive_case()
    p = c["p"]
    q, w = empty_grid(p)
    off, store = (0, 0, 0), SM.empty_store(False)
    for raw, T, d in zip(c["depth"], c["poses"], c["shifts"]):
        if d != (0, 0, 0):
            pre = mesh_model(q, w, window(p, off), detail=True)
            store, ok = SM.store_append(store, lambda f: SM.spill_of_mesh(pre, None, d, p["dims"], f), (1 << 20, 1 << 20))
            assert ok
            q, w, _ = shift_model(q, w, None, d)
            off = offset_model(off, d)
        q, w, _, _ = integrate_model(q, w, raw, T, window(p, off))
    final = mesh_model(q, w, window(p, off))
    n = len(store["xyz0"])
    m = dict(xyz0=np.concatenate([store["xyz0"], final[0]]), nrmw=np.concatenate([store["nrmw"], final[1]]),
             tri=np.concatenate([store["tri"], final[2] + n]).astype(np.int32), rgba=None)
    return m, p, (n, len(store["tri"]))


@functools.lru_cache(maxsize=None)
def drive_model(grids):
    m, p, _ = drive_mesh()
    return weld_model(m, f32(p["vs"]) / f32(64.0), p["origin"], grids)
