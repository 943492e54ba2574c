"""The mesh component filter's specification as code (include/odometry_hip.h, odo_mesh_components_create),
shared by tests/test_mesh_components_cpu.py and tests/test_gpu_mesh_components.py: the constants read out of the kernels' headers,
the numpy model (label propagation by minimum over sorted incidences, np.unique on the edge keys), the same rule as plain loops over
Python integers and dictionaries written independently of it (a dictionary union-find, a dict of edge uses), and the rows — each with
the situation it is in the table for as a predicate on the model's intermediates. Nothing here loads the GPU library.

A row is dict(name, mesh, rule, capacity, holds). mesh = dict(xyz0 (n, 4) float32, nrmw (n, 4) float32, tri (m, 3) int32, rgba (n, 4)
uint8 or None); rule = dict(min_triangles, keep_largest, drop). The model can be told to get one of six things wrong (SWITCHES);
CAUGHT_BY names, for each, the rows that are in the table to notice. Meshes and model results are computed once per process and
shared."""
import functools
import os
import re

import numpy as np

import mesh_weld_cases as wc

ROOT = wc.ROOT
CSRC = wc.CSRC
STATS = ("vertices_in", "triangles_in", "vertices_out", "triangles_out", "components", "removed_components", "removed_triangles",
         "removed_vertices", "largest", "bad_index", "degenerate", "unreferenced", "edges", "open_edges", "nonmanifold_edges", "edges_out",
         "open_edges_out", "nonmanifold_edges_out", "guard")
EDGE_STATS = STATS[12:18]
SWITCHES = ("greater_than", "largest_label", "tie_to_larger", "edge_connectivity", "degenerate_not_counted", "self_edges")
LOOP_ITEMS = 20000            # rows with no more vertices + triangles than this go through the loops
f32, u64 = np.float32, np.uint64
INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)
bits, mix, mix_int = wc.bits, wc.mix, wc.mix_int


def constants():
    """{kName: value} of every `constexpr int kName = <integer or 1 << n>;` line of mesh_components_math.h and mesh_components.hip.h."""
    out = {}
    for name in ("mesh_components_math.h", "mesh_components.hip.h"):
        for m in re.finditer(r"^constexpr\s+int\s+(k\w+)\s*=\s*(\d+)(?:\s*<<\s*(\d+))?\s*;", open(os.path.join(CSRC, name)).read(), re.M):
            out[m.group(1)] = int(m.group(2)) << int(m.group(3) or 0)
    return out


def edge_slots(triangle_capacity):
    """mc_edge_slots: 2^ceil(log2(6 triangle_capacity))."""
    s = 2
    while s < 6 * triangle_capacity:
        s <<= 1
    return s


# ---- the model --------------------------------------------------------------------------------------------------------------------
def _group_min(values, groups, n_groups, start):
    """out[g] = min(start[g], the values whose group is g)."""
    out = start.copy()
    if len(values):
        order = np.argsort(groups, kind="stable")
        g = groups[order]
        first = np.nonzero(np.r_[True, g[1:] != g[:-1]])[0]
        out[g[first]] = np.minimum(out[g[first]], np.minimum.reduceat(values[order], first))
    return out


def vertex_roots(tv, n_v):
    """root[i] = the smallest vertex index of vertex i's component under vertex connectivity: every triangle hands the minimum of
    its three labels to its vertices, then every label is replaced by its label's label, until nothing moves."""
    lab = np.arange(n_v, dtype=np.int64)
    flat = tv.ravel()
    while True:
        m = np.repeat(lab[tv].min(1), 3) if len(tv) else np.zeros(0, np.int64)
        new = _group_min(m, flat, n_v, lab)
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, lab):
            return lab
        lab = new


def edge_components(tv):
    """The switch: per valid triangle an id of its component when only a shared EDGE connects (the smallest triangle number)."""
    n = len(tv)
    lab = np.arange(n, dtype=np.int64)
    e = np.sort(np.concatenate([tv[:, [0, 1]], tv[:, [1, 2]], tv[:, [2, 0]]]), 1)
    _, eid = np.unique(e[:, 0] << 32 | e[:, 1], return_inverse=True)
    owner = np.tile(np.arange(n), 3)
    while True:
        emin = _group_min(lab[owner], eid, eid.max() + 1 if n else 0, np.full(eid.max() + 1 if n else 0, n, np.int64))
        new = _group_min(emin[eid], owner, n, lab)
        new = new[new]
        if np.array_equal(new, lab):
            return lab
        lab = new


def components_model(m, min_triangles, keep_largest=False, drop=True, edge_stats=True, greater_than=False, largest_label=False,
                     tie_to_larger=False, edge_connectivity=False, degenerate_not_counted=False, self_edges=False):
    """dict(xyz0, nrmw, tri, rgba, labels, stats) and the intermediates: valid (n_t,), root (n_v,) under vertex connectivity, comps
    (the labels, ascending), sizes and survives (per entry of comps), tkeep, vkeep, edge_keys / edge_uses / edge_out. The switches:
    size > min for >=; the largest vertex index as a component's label; a tie for the largest to the larger label; edges in place of
    vertices as what connects; degenerate triangles left out of the sizes; the edges (a, a) of degenerate triangles counted."""
    xyz0, nrmw, rgba = np.ascontiguousarray(m["xyz0"], f32).reshape(-1, 4), np.ascontiguousarray(m["nrmw"], f32).reshape(-1, 4), m.get("rgba")
    tri = np.ascontiguousarray(m["tri"], np.int32).reshape(-1, 3)
    n_v, n_t = len(xyz0), len(tri)
    t = tri.astype(np.int64)
    valid = ((t >= 0) & (t < n_v)).all(1) if n_t else np.zeros(0, bool)
    tv = t[valid]
    deg = (tv[:, 0] == tv[:, 1]) | (tv[:, 1] == tv[:, 2]) | (tv[:, 0] == tv[:, 2])
    root = vertex_roots(tv, n_v)
    tc = edge_components(tv) if edge_connectivity else root[tv[:, 0]]
    ids, inv = np.unique(tc, return_inverse=True)
    n_c = len(ids)
    # a component's label: its smallest vertex index
    if largest_label:
        lab = -_group_min(-tv.max(1), inv, n_c, np.full(n_c, 0, np.int64))
    else:
        lab = _group_min(tv.min(1), inv, n_c, np.full(n_c, n_v, np.int64))
    size = np.bincount(inv[~deg] if degenerate_not_counted else inv, minlength=n_c).astype(np.int64)
    survives = (size > min_triangles) if greater_than else (size >= min_triangles)
    largest = int(size.max()) if n_c else 0
    if keep_largest and n_c:
        top = np.nonzero(size == largest)[0]
        pick = top[np.argmax(lab[top])] if tie_to_larger else top[np.argmin(lab[top])]
        only = np.zeros(n_c, bool)
        only[pick] = True
        survives &= only
    labels = np.full(n_t, -1, np.int32)
    labels[valid] = lab[inv]
    tkeep = np.zeros(n_t, bool)
    tkeep[valid] = survives[inv]
    named = np.zeros(n_v, bool)
    named[tv.ravel()] = True
    ref = np.zeros(n_v, bool)
    ref[t[tkeep].ravel()] = True
    vkeep = ref | (~named & (not drop))
    new = np.cumsum(vkeep) - 1
    out = dict(xyz0=xyz0[vkeep], nrmw=nrmw[vkeep], tri=new[t[tkeep]].astype(np.int32).reshape(-1, 3),
               rgba=np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)[vkeep] if rgba is not None else None)
    stats = dict.fromkeys(STATS, 0)
    stats.update(vertices_in=n_v, triangles_in=n_t, vertices_out=int(vkeep.sum()), triangles_out=int(tkeep.sum()), components=n_c,
                 removed_components=int((~survives).sum()), removed_triangles=int((valid & ~tkeep).sum()),
                 removed_vertices=int((named & ~ref).sum()), largest=largest, bad_index=int((~valid).sum()), degenerate=int(deg.sum()),
                 unreferenced=int((~named & ~vkeep).sum()))
    # the edges of the valid triangles, each in the component of the first triangle that has it
    e = np.concatenate([tv[:, [0, 1]], tv[:, [1, 2]], tv[:, [2, 0]]])
    ec = np.tile(inv, 3)
    if not self_edges:
        ec, e = ec[e[:, 0] != e[:, 1]], e[e[:, 0] != e[:, 1]]
    e = np.sort(e, 1)
    keys, first, uses = np.unique((e[:, 0] << 32 | e[:, 1]).astype(u64), return_index=True, return_counts=True)
    edge_out = survives[ec[first]] if len(keys) else np.zeros(0, bool)
    if edge_stats:
        stats.update(edges=len(keys), open_edges=int((uses == 1).sum()), nonmanifold_edges=int((uses > 2).sum()), edges_out=int(edge_out.sum()),
                     open_edges_out=int((edge_out & (uses == 1)).sum()), nonmanifold_edges_out=int((edge_out & (uses > 2)).sum()))
    order = np.argsort(lab, kind="stable")
    return dict(out, labels=labels, stats=stats, tri_in=tri, valid=valid, root=root, comps=lab[order], sizes=size[order], survives=survives[order],
                tkeep=tkeep, vkeep=vkeep, edge_keys=keys, edge_uses=uses, edge_out=edge_out)


# ---- the same as plain loops ---------------------------------------------------------------------------------------------------------
def components_loop(m, min_triangles, keep_largest=False, drop=True, edge_stats=True):
    """The rule read off the prose, a triangle at a time: a dictionary union-find over the vertices valid triangles name, a dict of
    edge uses. (xyz0, nrmw, tri, rgba, labels, stats) with the arrays as lists of rows of bit patterns / integers."""
    V = [[int(b) for b in row] for row in np.concatenate([bits(m["xyz0"]).reshape(-1, 4), bits(m["nrmw"]).reshape(-1, 4)], 1)]
    C = [[int(b) for b in row] for row in m["rgba"]] if m.get("rgba") is not None else None
    T = [[int(i) for i in row] for row in np.asarray(m["tri"]).reshape(-1, 3)]
    up = {}

    def find(i):
        up.setdefault(i, i)
        while up[i] != i:
            up[i] = up[up[i]]
            i = up[i]
        return i

    stats = dict.fromkeys(STATS, 0)
    stats["vertices_in"], stats["triangles_in"] = len(V), len(T)
    ok = [all(0 <= i < len(V) for i in t) for t in T]
    for t, good in zip(T, ok):
        if not good:
            stats["bad_index"] += 1
            continue
        stats["degenerate"] += len(set(t)) < 3
        for i in t[1:]:
            a, b = find(t[0]), find(i)
            if a != b:
                up[max(a, b)] = min(a, b)
    size, use = {}, {}
    for t, good in zip(T, ok):
        if good:
            size[find(t[0])] = size.get(find(t[0]), 0) + 1
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                if a != b:
                    use[(min(a, b), max(a, b))] = use.get((min(a, b), max(a, b)), 0) + 1
    alive = {c for c, n in size.items() if n >= min_triangles}
    stats["components"] = len(size)
    stats["largest"] = max(size.values(), default=0)
    if keep_largest and size:
        alive &= {min(c for c, n in size.items() if n == stats["largest"])}
    stats["removed_components"] = len(size) - len(alive)
    labels, kept, named = [], [], set()
    for t, good in zip(T, ok):
        labels.append(find(t[0]) if good else -1)
        if good and labels[-1] in alive:
            kept.append(t)
            named.update(t)
        elif good:
            stats["removed_triangles"] += 1
    new, keep = {}, []
    for i in range(len(V)):
        if i in up:                                   # a valid triangle names it: it goes where its component goes
            if find(i) not in alive:
                stats["removed_vertices"] += 1
                continue
        elif drop:
            stats["unreferenced"] += 1
            continue
        new[i] = len(keep)
        keep.append(i)
    assert all(i in new for i in named)
    if edge_stats:
        for (a, b), n in use.items():
            out = find(a) in alive
            assert find(a) == find(b)
            stats["edges"] += 1
            stats["edges_out"] += out
            stats["open_edges"] += n == 1
            stats["open_edges_out"] += n == 1 and out
            stats["nonmanifold_edges"] += n > 2
            stats["nonmanifold_edges_out"] += n > 2 and out
    stats["vertices_out"], stats["triangles_out"] = len(keep), len(kept)
    return ([V[i][:4] for i in keep], [V[i][4:] for i in keep], [[new[i] for i in t] for t in kept],
            [C[i] for i in keep] if C is not None else None, labels, stats)


def same_as_loop(M, loop):
    """The model's result against components_loop's, bit for bit."""
    xyz0, nrmw, tri, rgba, labels, stats = loop
    return (bits(M["xyz0"]).tolist() == xyz0 and bits(M["nrmw"]).tolist() == nrmw and M["tri"].tolist() == tri and
            (M["rgba"] is None) == (rgba is None) and (rgba is None or M["rgba"].tolist() == rgba) and M["labels"].tolist() == labels and
            M["stats"] == stats)


def same_result(a, b):
    return (np.array_equal(bits(a["xyz0"]), bits(b["xyz0"])) and np.array_equal(bits(a["nrmw"]), bits(b["nrmw"])) and
            np.array_equal(a["tri"], b["tri"]) and (a["rgba"] is None) == (b["rgba"] is None) and
            (a["rgba"] is None or np.array_equal(a["rgba"], b["rgba"])) and np.array_equal(a["labels"], b["labels"]) and
            a["stats"] == b["stats"])


# ---- the rows: meshes -----------------------------------------------------------------------------------------------------------------
TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])


def strip(k, base=0):
    """k triangles (i, i + 1, i + 2) over k + 2 vertices from `base` on, every other one turned so that the winding is consistent."""
    i = np.arange(k)[:, None] + base
    t = np.concatenate([i, i + 1, i + 2], 1)
    t[1::2] = t[1::2][:, [1, 0, 2]]
    return t


def pieces(sizes, seed, shuffle=True, colour=False, extra=0):
    """Strips of the given numbers of triangles on vertices of their own, plus `extra` vertices nobody names. With shuffle the vertex
    indices are permuted across the whole mesh and the triangles come in a random order."""
    rng = np.random.default_rng(seed)
    tri, n = [], 0
    for k in sizes:
        tri.append(strip(k, n))
        n += k + 2
    n += extra
    tri = np.concatenate(tri) if tri else np.zeros((0, 3), np.int64)
    if shuffle:
        tri = rng.permutation(n)[tri][rng.permutation(len(tri))]
    return wc.mesh(rng.uniform(0.0, 4.0, (n, 3)), tri, seed + 1, colour)


# Strip sizes for the rows either side of a wave and of a workgroup: none is 4, the rows' min_triangles, some lie on either side.
SIZES_T = {63: [29, 17, 9, 5, 2, 1], 64: [29, 17, 9, 5, 3, 1], 65: [29, 17, 9, 5, 3, 2], 255: [61, 61, 61, 29, 17, 13, 7, 3, 2, 1],
           256: [61, 61, 61, 29, 17, 13, 7, 3, 3, 1], 257: [61, 61, 61, 29, 17, 13, 7, 3, 3, 2]}
SIZES_V = {63: [29, 17, 5, 1], 64: [29, 17, 5, 2], 65: [29, 17, 5, 3], 255: [61, 61, 61, 29, 17, 3, 1, 3], 256: [61, 61, 61, 29, 17, 3, 2, 3],
           257: [61, 61, 61, 29, 17, 3, 3, 3]}              # (three more vertices that nobody names)


def _fan(k):
    return wc.mesh(np.random.default_rng(40).uniform(0.0, 4.0, (k + 2, 3)), [[0, i, i + 1] for i in range(1, k + 1)], 41)


def _two_tetrahedra(pinched):
    b = TETRA + (3 if pinched else 4)
    return wc.mesh(np.random.default_rng(42).uniform(0.0, 4.0, (7 if pinched else 8, 3)), np.concatenate([TETRA, b]), 43)


def _bad_indices():
    m = pieces([2, 4], 44, shuffle=False)
    n = len(m["xyz0"])
    m["tri"] = np.concatenate([m["tri"][:2], [[-1, 1, 2], [0, n, 2], [0, 1, INT32_MAX], [INT32_MIN, 1, 2], [n, n, n], [-1, -1, -1]],
                               m["tri"][2:]]).astype(np.int32)
    return m


def _degenerates():
    """Vertices 0 .. 3: two real triangles and the degenerate (0, 0, 3) and (2, 2, 1): a component of 4 with 2 that have an area.
    Vertex 4: (4, 4, 4) alone. Vertices 5 .. 11: a strip of 5."""
    return wc.mesh(np.random.default_rng(45).uniform(0.0, 4.0, (12, 3)),
                   [[0, 1, 2], [0, 0, 3], [4, 4, 4], [2, 1, 3], [2, 2, 1], [5, 6, 7], [6, 8, 7], [7, 8, 9], [8, 10, 9], [9, 10, 11]], 46)


def _three_on_an_edge():
    return wc.mesh(np.random.default_rng(47).uniform(0.0, 4.0, (5, 3)), [[0, 1, 2], [1, 0, 3], [0, 1, 4]], 48)


HOMED_CAPACITY = (601, 256)


def _homed():
    """256 triangles (a, b, 600) whose edges a | b are all different and home in the last four slots of the table for 256 triangles:
    their probe runs wrap to the table's start."""
    slots = edge_slots(HOMED_CAPACITY[1])
    a, b = np.triu_indices(600, 1)
    home = (mix((a.astype(u64) << u64(32)) | b.astype(u64)) & u64(slots - 1)).astype(np.int64)
    pick = np.nonzero(home >= slots - 4)[0][:256]
    assert len(pick) == 256
    tri = np.stack([a[pick], b[pick], np.full(256, 600)], 1)
    return wc.mesh(np.random.default_rng(49).uniform(0.0, 4.0, (601, 3)), tri, 50)


def probe_replay(keys, slots):
    """The table after the keys are inserted in order (any order gives the same set of occupied slots): slot -> key, and the
    longest probe."""
    return wc.probe_replay(keys, slots)


def _holds_homed(M):
    slots = edge_slots(HOMED_CAPACITY[1])
    keys = [int(k) for k in M["edge_keys"]]
    table, longest = probe_replay(keys, slots)
    last = [k for k in keys if mix_int(k) & (slots - 1) >= slots - 4]
    return len(last) >= 256 and min(table) == 0 and max(table) == slots - 1 and longest >= 250 and 2 * len(keys) <= slots


def _rule(min_triangles=0, keep_largest=False, drop=True):
    return dict(min_triangles=min_triangles, keep_largest=keep_largest, drop=drop)


def _row(name, m, rule, holds, capacity=None):
    return dict(name=name, mesh=m, rule=rule, holds=holds, capacity=capacity or (max(len(m["xyz0"]), 1), max(len(m["tri"]), 1)))


def _euler(M, label):
    """V - E + F of the component with this label."""
    t = M["tri_in"][M["labels"] == label].astype(np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    return len(np.unique(t)) - len(np.unique(e, axis=0)) + len(t)


@functools.lru_cache(maxsize=None)
def welded(which):
    """tests/mesh_weld_cases.py's split grid and the store of the d, -d, d walk after a weld on one grid."""
    if which == "split":
        _, m, p = wc.split_grid()
    else:
        m, p = wc.twice_store()
    W = wc.weld_model(m, p["vs"] / 64, p["origin"], 1)
    return dict(xyz0=W["xyz0"], nrmw=W["nrmw"], tri=W["tri"], rgba=W["rgba"])


def _sizes(M):
    return M["sizes"].tolist()


@functools.lru_cache(maxsize=None)
def rows():
    S = lambda M: M["stats"]
    out = [
        _row("no vertex, no triangle", pieces([], 1), _rule(3), lambda M: S(M)["components"] == 0 and S(M)["vertices_out"] == 0),
        _row("one vertex, no triangle, kept", pieces([], 2, extra=1), _rule(3, drop=False),
             lambda M: len(M["xyz0"]) == 1 and S(M)["unreferenced"] == 0 and S(M)["components"] == 0),
        _row("one vertex, no triangle, dropped", pieces([], 2, extra=1), _rule(3), lambda M: len(M["xyz0"]) == 0 and S(M)["unreferenced"] == 1),
        _row("no vertex, one triangle", wc.mesh(np.zeros((0, 3)), [[0, 0, 0]], 3), _rule(), lambda M: S(M)["bad_index"] == 1 and M["labels"].tolist() == [-1]),
        _row("one vertex, one triangle", wc.mesh(np.ones((1, 3)), [[0, 0, 0]], 4), _rule(0),
             lambda M: S(M)["degenerate"] == 1 and S(M)["components"] == 1 and len(M["tri"]) == 1 and S(M)["edges"] == 0),
        _row("two disjoint tetrahedra", _two_tetrahedra(False), _rule(3),
             lambda M: S(M)["components"] == 2 and S(M)["open_edges"] == 0 and S(M)["edges"] == 12 and
             [_euler(M, c) for c in M["comps"]] == [2, 2] and S(M)["triangles_out"] == 8),
        _row("two tetrahedra that share one vertex", _two_tetrahedra(True), _rule(5),
             lambda M: S(M)["components"] == 1 and _sizes(M) == [8] and S(M)["triangles_out"] == 8 and S(M)["edges"] == 12),
        _row("components of 1 to 5 triangles, three stay", pieces([1, 2, 3, 4, 5], 5), _rule(3),
             lambda M: sorted(_sizes(M)) == [1, 2, 3, 4, 5] and S(M)["removed_components"] == 2 and S(M)["removed_triangles"] == 3 and
             S(M)["removed_vertices"] == 7),
    ]
    for n in (63, 64, 65, 255, 256, 257):
        out.append(_row(f"{n} triangles", pieces(SIZES_T[n], 10 + n), _rule(4),
                        lambda M, n=n: S(M)["triangles_in"] == n and 0 < S(M)["removed_components"] < S(M)["components"] and 4 not in _sizes(M)))
        out.append(_row(f"{n} vertices", pieces(SIZES_V[n], 20 + n, extra=3), _rule(4, drop=n % 2 == 1),
                        lambda M, n=n: S(M)["vertices_in"] == n and 0 < S(M)["removed_components"] < S(M)["components"] and 4 not in _sizes(M) and
                        S(M)["unreferenced"] == (3 if n % 2 else 0)))
    asc = pieces([4096], 30, shuffle=False)
    desc = dict(asc, tri=(4097 - asc["tri"]).astype(np.int32))
    out += [
        _row("a strip of 4096 triangles, ascending", asc, _rule(100), lambda M: _sizes(M) == [4096] and (M["root"] == 0).all()),
        _row("a strip of 4096 triangles, descending", desc, _rule(100), lambda M: _sizes(M) == [4096] and M["tri"][0].max() == 4097),
        _row("a strip of 4096 triangles, shuffled", pieces([4096], 31), _rule(100), lambda M: _sizes(M) == [4096] and S(M)["open_edges"] == 4098),
        _row("a fan of 1024 triangles round one vertex", _fan(1024), _rule(100),
             lambda M: _sizes(M) == [1024] and S(M)["edges"] == 2049 and S(M)["open_edges"] == 1026),
        _row("one component of 2049 triangles and debris", pieces([2049, 2, 1], 32), _rule(100),
             lambda M: sorted(_sizes(M)) == [1, 2, 2049] and S(M)["triangles_out"] == 2049 and S(M)["largest"] == 2049),
        _row("triangles naming -1, n_v, INT32_MAX and INT32_MIN", _bad_indices(), _rule(3),
             lambda M: M["valid"].tolist() == [True, True] + [False] * 6 + [True] * 4 and S(M)["bad_index"] == 6 and
             M["labels"].tolist() == [0, 0, -1, -1, -1, -1, -1, -1, 4, 4, 4, 4] and S(M)["triangles_out"] == 4),
        _row("(a, a, b) and (a, a, a)", _degenerates(), _rule(3),
             lambda M: _sizes(M) == [4, 1, 5] and S(M)["degenerate"] == 3 and S(M)["removed_triangles"] == 1 and S(M)["edges"] == 6 + 11 and
             S(M)["nonmanifold_edges"] == 1 and
             M["tri"].tolist()[1] == [0, 0, 3]),
        _row("a triangle given twice", wc.mesh(np.random.default_rng(51).uniform(0, 4, (6, 3)), [[0, 1, 2], [3, 4, 5], [0, 1, 2]], 52),
             _rule(0, keep_largest=True),
             lambda M: _sizes(M) == [2, 1] and S(M)["open_edges"] == 3 and S(M)["open_edges_out"] == 0 and S(M)["edges_out"] == 3 and
             M["tri"].tolist() == [[0, 1, 2], [0, 1, 2]]),
        _row("three triangles on one edge", _three_on_an_edge(), _rule(), lambda M: S(M)["nonmanifold_edges"] == 1 == S(M)["nonmanifold_edges_out"] and
             S(M)["edges"] == 7 and S(M)["open_edges"] == 6),
        _row("a vertex nobody names, kept", pieces([3, 1], 53, extra=2), _rule(2, drop=False),
             lambda M: S(M)["unreferenced"] == 0 and S(M)["vertices_out"] == 5 + 2 and S(M)["removed_vertices"] == 3),
        _row("a vertex nobody names, dropped", pieces([3, 1], 53, extra=2), _rule(2),
             lambda M: S(M)["unreferenced"] == 2 and S(M)["vertices_out"] == 5 and S(M)["removed_vertices"] == 3),
        _row("the largest of two that tie", pieces([5, 3, 5], 54), _rule(2, keep_largest=True),
             lambda M: sorted(_sizes(M)) == [3, 5, 5] and M["survives"].sum() == 1 and
             M["comps"][M["survives"]][0] == min(c for c, s in zip(M["comps"], M["sizes"]) if s == 5) and S(M)["removed_components"] == 2),
        _row("the largest below min_triangles", pieces([5, 3, 6], 55), _rule(7, keep_largest=True),
             lambda M: S(M)["largest"] == 6 and len(M["tri"]) == 0 and len(M["xyz0"]) == 0 and S(M)["removed_triangles"] == 14),
        _row("the largest alone", pieces([5, 3, 9, 7], 56), _rule(0, keep_largest=True),
             lambda M: S(M)["triangles_out"] == 9 and S(M)["removed_components"] == 3),
        _row("a coloured mesh", pieces([40, 3, 17, 2, 1, 150, 9], 57, colour=True, extra=5), _rule(10),
             lambda M: M["rgba"] is not None and len(M["rgba"]) == len(M["xyz0"]) and S(M)["removed_components"] == 4),
        _row("256 edges homed in the table's last four slots", _homed(), _rule(), _holds_homed, capacity=HOMED_CAPACITY),
        _row("a dyadic grid split by a spill, welded", welded("split"), _rule(8), lambda M: _sizes(M) == [369] and S(M)["triangles_out"] == 369),
        _row("the store of the d, -d, d walk, welded", welded("twice"), _rule(8),
             lambda M: sorted(_sizes(M)) == [2, 2, 2, 14, 14, 36, 36, 74, 104] and S(M)["removed_components"] == 3 and S(M)["open_edges_out"] == 200),
    ]
    return out


def row_ids():
    return [r["name"] for r in rows()]


@functools.lru_cache(maxsize=None)
def model_of(index, switch=None):
    r = rows()[index]
    return components_model(r["mesh"], r["rule"]["min_triangles"], r["rule"]["keep_largest"], r["rule"]["drop"], **({switch: True} if switch else {}))


def differs(index, switch):
    return not same_result(model_of(index), model_of(index, switch))


# Which rows each switch must change; it changes no other.
CAUGHT_BY = {
    "greater_than": ("components of 1 to 5 triangles, three stay",),
    # (every row with a component of more than one vertex: the labels are part of the result)
    "largest_label": lambda i: bool((model_of(i)["root"] != np.arange(len(model_of(i)["root"]))).any()),
    "tie_to_larger": ("the largest of two that tie",),
    # (the pinch; a degenerate triangle shares no edge with its neighbours; fans about vertex 600 whose rims do not meet; the store's
    #  sheets that touch in single vertices)
    "edge_connectivity": ("two tetrahedra that share one vertex", "(a, a, b) and (a, a, a)", "256 edges homed in the table's last four slots",
                          "the store of the d, -d, d walk, welded"),
    "degenerate_not_counted": ("one vertex, one triangle", "(a, a, b) and (a, a, a)"),
    "self_edges": ("one vertex, one triangle", "(a, a, b) and (a, a, a)"),
}


# ---- the drive that leaves its box, welded -------------------------------------------------------------------------------------------
DRIVE = {8: dict(vertices=151506, triangles=299223, sizes=[8, 16, 16, 40, 48, 80, 299015], open=3853, open_out=3733),
         1: dict(vertices=152266, triangles=299579, sizes=[8, 16, 16, 40, 48, 80, 104012, 195359], open=5295, open_out=5175)}


@functools.lru_cache(maxsize=None)
def drive_welded(grids):
    W = wc.drive_model(grids)
    return dict(xyz0=W["xyz0"], nrmw=W["nrmw"], tri=W["tri"], rgba=None)


@functools.lru_cache(maxsize=None)
def drive_components(grids, min_triangles):
    return components_model(drive_welded(grids), min_triangles)
