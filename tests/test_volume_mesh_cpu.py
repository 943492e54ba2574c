"""The TSDF volume's triangle mesh (odo_volume_mesh, odo_volume_upload, api.TsdfVolume.mesh) without a GPU: the ABI, the marching-
tetrahedra table of odometry_amd/csrc/volume_mesh_table.h against a table the model derives geometrically, the numpy model of the
specification (include/odometry_hip.h) pinned to the prose by a plain-loop implementation that does one fp32
operation at a time, the mesh's topological and geometric properties, the model against the synthetic corridor's planes, the
kernels' code-object metadata and the PLY writer.

The model is the yardstick of tests/test_gpu_volume_mesh.py, which asks the GPU for the same bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from test_volume_cpu import (_gradient, bits, centres, empty_grid, extract_model, integrate_model, params, pinned,  # noqa: F401
                             plane_errors, tiny_cases)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

NEW_SYMBOLS = ["odo_volume_mesh", "odo_volume_upload"]
MESH_KERNELS = ["volume_mesh_count_kernel", "volume_mesh_scan_kernel", "volume_mesh_vertex_kernel", "volume_mesh_triangle_kernel"]

DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]       # d_e as (dx, dy, dz)
PATHS = [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]   # corners c = dx + 2 dy + 4 dz


def corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])


# ---- the table, derived geometrically ------------------------------------------------------------------------------------------
def _pattern_triangles(m):
    """The triangles of pattern m (bit p: path position p positive) as triples of edges (path position, path position), unwound."""
    pos = [p for p in range(4) if (m >> p) & 1]
    neg = [p for p in range(4) if not (m >> p) & 1]
    if len(pos) in (1, 3):
        s = pos[0] if len(pos) == 1 else neg[0]
        r = [p for p in range(4) if p != s]
        return pos, neg, [[(s, r[0]), (s, r[1]), (s, r[2])]]
    if len(pos) == 2:
        (a, b), (c, d) = pos, neg
        V = [(a, c), (a, d), (b, d), (b, c)]
        return pos, neg, [[V[0], V[1], V[2]], [V[0], V[2], V[3]]]
    return pos, neg, []


def _owner(path, x, y):
    """The edge between path positions x and y as (corner of the owner voxel, e)."""
    lo, hi = min(x, y), max(x, y)
    d = corner_xyz(path[hi]) - corner_xyz(path[lo])
    assert (d >= 0).all() and d.any()      # every edge of every tetrahedron is one of the seven directions from its lower corner
    return path[lo], DIRS.index(tuple(int(v) for v in d))


def model_table():
    """TABLE[t][m] = [triangle ...], a triangle = three (corner, e); counter-clockwise seen from the positive side, found from the
    determinant of the triangle at alpha = 1/2 with the direction from the negative corners' centroid to the positive ones'."""
    table = []
    for path in PATHS:
        P = [corner_xyz(c).astype(np.float64) for c in path]
        row = []
        for m in range(16):
            pos, neg, tris = _pattern_triangles(m)
            out = []
            for tri in tris:
                mid = [(P[x] + P[y]) / 2 for x, y in tri]
                towards = np.mean([P[x] for x in pos], 0) - np.mean([P[x] for x in neg], 0)
                det = np.linalg.det(np.array([mid[1] - mid[0], mid[2] - mid[0], towards]))
                assert abs(det) > 1e-3, (path, m, det)
                if det < 0:
                    tri = [tri[0], tri[2], tri[1]]
                out.append(tuple(_owner(path, x, y) for x, y in tri))
            row.append(out)
        table.append(row)
    return table


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _shift(a, c):
    """a at corner c of every cell: shape (nz - 1, ny - 1, nx - 1)."""
    dx, dy, dz = corner_xyz(c)
    nz, ny, nx = a.shape
    return a[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def mesh_model(q, w, p, detail=False):
    """The mesh of the volume: (n, 4) x y z e, (n, 4) nx ny nz weight, (m, 3) int32 indices. detail: also the vertices' keys
    (voxel * 7 + e) and the triangles' ((cell * 6 + tetrahedron) * 2 + triangle), both ascending."""
    nz, ny, nx = q.shape
    vs = f32(p["vs"])
    cen = centres(p)
    Q = q.astype(f32)
    obs = w > 0
    g, has = _gradient(Q, obs)
    keys, pts, nrm = [], [], []
    for e, (dx, dy, dz) in enumerate(DIRS):
        sa = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        sb = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        m = obs[sa] & obs[sb] & ((q[sa] > 0) != (q[sb] > 0))
        k, j, i = np.nonzero(m)
        qa, qb = Q[sa][m], Q[sb][m]
        alpha = qa / (qa - qb)
        step = alpha * vs
        P = np.zeros((len(alpha), 4), f32)
        P[:, 0], P[:, 1], P[:, 2], P[:, 3] = cen[0][i], cen[1][j], cen[2][k], f32(e)
        for c, d in enumerate((dx, dy, dz)):
            if d:
                P[:, c] = P[:, c] + step
        ga, gb = g[sa][m], g[sb][m]
        both = has[sa][m] & has[sb][m]
        n = ga + alpha[:, None] * (gb - ga)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        good = both & (ln > 0)
        N = np.zeros((len(alpha), 4), f32)
        with np.errstate(all="ignore"):
            N[:, :3] = np.where(good[:, None], n / ln[:, None], f32(0.0))
        N[:, 3] = np.minimum(w[sa][m], w[sb][m]).astype(f32)
        keys.append(((k.astype(np.int64) * ny + j) * nx + i) * 7 + e)
        pts.append(P)
        nrm.append(N)
    vkeys = np.concatenate(keys)
    order = np.argsort(vkeys, kind="stable")
    vkeys = vkeys[order]
    xyz0, nrmw = np.concatenate(pts)[order], np.concatenate(nrm)[order]
    # triangles
    live = np.ones((nz - 1, ny - 1, nx - 1), bool)
    pos8 = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for c in range(8):
        live &= _shift(obs, c)
        pos8 |= (_shift(q, c) > 0).astype(np.int64) << c
    k, j, i = np.nonzero(live & (pos8 != 0) & (pos8 != 255))
    cell = (k.astype(np.int64) * ny + j) * nx + i
    pos = pos8[k, j, i]
    table = model_table()
    tkeys, tris = [], []
    for t, path in enumerate(PATHS):
        m4 = (pos & 1) | (((pos >> path[1]) & 1) << 1) | (((pos >> path[2]) & 1) << 2) | (((pos >> 7) & 1) << 3)
        for m in range(1, 15):
            at = np.nonzero(m4 == m)[0]
            if not len(at):
                continue
            for r, tri in enumerate(table[t][m]):
                ids = []
                for c, e in tri:
                    owner = cell[at] + (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny
                    key = owner * 7 + e
                    where = np.minimum(np.searchsorted(vkeys, key), len(vkeys) - 1)
                    assert (vkeys[where] == key).all()      # a live cell's sign-changing edge has its vertex
                    ids.append(where)
                ids = np.stack(ids, 1)
                first = ids.argmin(1)
                ids = np.take_along_axis(ids, (first[:, None] + np.arange(3)[None, :]) % 3, 1)   # the smallest index first
                tkeys.append((cell[at] * 6 + t) * 2 + r)
                tris.append(ids)
    if tris:
        tkeys = np.concatenate(tkeys)
        order = np.argsort(tkeys, kind="stable")
        tkeys, tri = tkeys[order], np.concatenate(tris)[order].astype(np.int32)
    else:
        tkeys, tri = np.zeros(0, np.int64), np.zeros((0, 3), np.int32)
    return (xyz0, nrmw, tri, vkeys, tkeys) if detail else (xyz0, nrmw, tri)


# ---- the same, one fp32 operation at a time --------------------------------------------------------------------------------------
def mesh_loop(q, w, p):
    nz, ny, nx = q.shape
    vs = f32(p["vs"])
    o = [f32(v) for v in p["origin"]]
    dims = (nx, ny, nz)
    half, two = f32(0.5), f32(2.0)

    def Q(v):
        return f32(int(q[v[2], v[1], v[0]]))

    def W(v):
        return int(w[v[2], v[1], v[0]])

    def usable(v):
        return all(0 <= v[c] < dims[c] for c in range(3)) and W(v) > 0

    def grad(v):
        out = []
        for c in range(3):
            vp, vm = list(v), list(v)
            vp[c] += 1
            vm[c] -= 1
            if usable(vp) and usable(vm):
                out.append(f32(Q(vp) - Q(vm)))
            elif usable(vp):
                out.append(f32(two * f32(Q(vp) - Q(v))))
            elif usable(vm):
                out.append(f32(two * f32(Q(v) - Q(vm))))
            else:
                return None
        return out

    index = {}
    pts, nrm = [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                a = (i, j, k)
                for e, d in enumerate(DIRS):
                    b = tuple(a[c] + d[c] for c in range(3))
                    if any(b[c] >= dims[c] for c in range(3)) or not (W(a) > 0 and W(b) > 0):
                        continue
                    if (Q(a) > 0) == (Q(b) > 0):
                        continue
                    alpha = f32(Q(a) / f32(Q(a) - Q(b)))
                    P = [f32(o[c] + f32(f32(f32(a[c]) + half) * vs)) for c in range(3)]
                    for c in range(3):
                        if d[c]:
                            P[c] = f32(P[c] + f32(alpha * vs))
                    ga, gb = grad(a), grad(b)
                    n = [f32(0.0)] * 3
                    if ga is not None and gb is not None:
                        m = [f32(ga[c] + f32(alpha * f32(gb[c] - ga[c]))) for c in range(3)]
                        ln = np.sqrt(f32(f32(f32(m[0] * m[0]) + f32(m[1] * m[1])) + f32(m[2] * m[2])))
                        if ln > 0:
                            n = [f32(m[c] / ln) for c in range(3)]
                    index[(a, e)] = len(pts)
                    pts.append(P + [f32(e)])
                    nrm.append(n + [f32(min(W(a), W(b)))])
    tris = []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                corner = [(i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1)) for c in range(8)]
                if not all(W(v) > 0 for v in corner):
                    continue
                for path in PATHS:
                    node = [corner[c] for c in path]
                    positive = [Q(v) > 0 for v in node]
                    pos = [x for x in range(4) if positive[x]]
                    neg = [x for x in range(4) if not positive[x]]
                    if len(pos) in (1, 3):
                        s = pos[0] if len(pos) == 1 else neg[0]
                        r = [x for x in range(4) if x != s]
                        found = [[(s, r[0]), (s, r[1]), (s, r[2])]]
                    elif len(pos) == 2:
                        V = [(pos[0], neg[0]), (pos[0], neg[1]), (pos[1], neg[1]), (pos[1], neg[0])]
                        found = [[V[0], V[1], V[2]], [V[0], V[2], V[3]]]
                    else:
                        found = []
                    for tri in found:
                        # winding in integers: twice the midpoints, their cross product against the direction from the negative
                        # corners to the positive ones
                        mid = [[node[x][c] + node[y][c] for c in range(3)] for x, y in tri]
                        u = [mid[1][c] - mid[0][c] for c in range(3)]
                        v = [mid[2][c] - mid[0][c] for c in range(3)]
                        n = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
                        to = [len(neg) * sum(node[x][c] for x in pos) - len(pos) * sum(node[x][c] for x in neg) for c in range(3)]
                        dot = sum(n[c] * to[c] for c in range(3))
                        assert dot != 0
                        if dot < 0:
                            tri = [tri[0], tri[2], tri[1]]
                        ids = []
                        for x, y in tri:
                            lo, hi = min(x, y), max(x, y)
                            d = tuple(node[hi][c] - node[lo][c] for c in range(3))
                            ids.append(index[(node[lo], DIRS.index(d))])
                        first = ids.index(min(ids))
                        tris.append(ids[first:] + ids[:first])
    return (np.array(pts, f32).reshape(-1, 4), np.array(nrm, f32).reshape(-1, 4), np.array(tris, np.int32).reshape(-1, 3))


# ---- grids -----------------------------------------------------------------------------------------------------------------------
GRID_K = (40.0, 15.5, 11.5)


def grid_params(dims, vs=0.05, origin=(-0.3, 0.2, 0.7)):
    return params(GRID_K, 1000.0, (24, 32), dims=dims, vs=vs, origin=origin, mu=0.3, max_depth=8.0, max_weight=65535)


def random_grid(dims, seed, holes=0.0, zeros=0.0, negative=0.5, shell=False):
    """(q, w) of shape (nz, ny, nx): random signs (`negative` = their share below zero) and |q| in 1 .. 32767, weights 1 .. 5, a share
    `holes` of the nodes unobserved and a share `zeros` with q == 0; shell: the outer layer of nodes forced positive."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    mag = rng.integers(1, 32768, (nz, ny, nx))
    q = np.where(rng.uniform(size=mag.shape) < negative, -mag, mag)
    if shell:
        for s_ in (np.s_[0], np.s_[-1], np.s_[:, 0], np.s_[:, -1], np.s_[:, :, 0], np.s_[:, :, -1]):
            q[s_] = np.abs(q[s_])
    q[rng.uniform(size=mag.shape) < zeros] = 0
    w = rng.integers(1, 6, mag.shape)
    w[rng.uniform(size=mag.shape) < holes] = 0
    return q.astype(np.int16), w.astype(np.uint16)


def pattern_grid(seed=5):
    """48 x 48 x 2: 256 isolated 2 x 2 x 2 cells on a 3-voxel pitch, w = 0 between them, cell n with the sign pattern n."""
    rng = np.random.default_rng(seed)
    q = np.zeros((2, 48, 48), np.int16)
    w = np.zeros((2, 48, 48), np.uint16)
    for n in range(256):
        x, y = 3 * (n % 16), 3 * (n // 16)
        for c in range(8):
            dx, dy, dz = corner_xyz(c)
            mag = int(rng.integers(1, 32768))
            q[dz, y + dy, x + dx] = mag if (n >> c) & 1 else -mag
            w[dz, y + dy, x + dx] = int(rng.integers(1, 6))
    return q, w


def live_patterns(q, w):
    live = np.ones(tuple(n - 1 for n in q.shape), bool)
    pos8 = np.zeros(live.shape, np.int64)
    for c in range(8):
        live &= _shift(w > 0, c)
        pos8 |= (_shift(q, c) > 0).astype(np.int64) << c
    return live, pos8


def tiny_grids():
    """tiny_cases() integrated: [(p, q, w)]."""
    out = []
    for p, frames in tiny_cases():
        q, w = empty_grid(p)
        for raw, pose in frames:
            q, w, _, _ = integrate_model(q, w, raw, pose, p)
        out.append((p, q, w))
    return out


def small_grids():
    """The grids the model is pinned on and whose e < 3 rows are held to extract_model: name -> (p, q, w)."""
    out = {f"tiny {n}": g for n, g in enumerate(tiny_grids())}
    for seed in range(3):
        dims = [(6, 5, 4), (5, 7, 3), (4, 4, 6)][seed]
        out[f"random {seed}"] = (grid_params(dims),) + random_grid(dims, seed, holes=0.15, zeros=0.1)
    return out


def property_grids():
    out = {}
    for seed in range(3):
        out[f"closed {seed}"] = (grid_params((9, 8, 7)),) + random_grid((9, 8, 7), 20 + seed, shell=True)
        out[f"holed {seed}"] = (grid_params((9, 8, 7)),) + random_grid((9, 8, 7), 30 + seed, holes=0.1)
    out["patterns"] = (grid_params((48, 48, 2)),) + pattern_grid()
    return out


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    for name in ("mesh", "upload", "save_mesh_ply"):
        assert callable(getattr(api.TsdfVolume, name))
    assert callable(api.write_ply_mesh)


def test_mesh_and_upload_validate_before_touching_a_device():
    from odometry_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(8)   # never dereferenced: every case below is refused by the argument checks
    counts = (C.c_long * 4)()
    buf = (C.c_float * 4)()
    idx = (C.c_int32 * 3)()
    q = (C.c_int16 * 1)()
    w = (C.c_uint16 * 1)()
    bad = [(None, 0, 0, None, None, None, counts), (fake, 0, 0, None, None, None, None), (fake, -1, 0, None, None, None, counts),
           (fake, 0, -1, None, None, None, counts), (fake, (1 << 28) + 1, 0, buf, buf, None, counts),
           (fake, 0, (1 << 28) + 1, None, None, idx, counts), (fake, 1, 0, None, buf, None, counts), (fake, 1, 0, buf, None, None, counts),
           (fake, 0, 1, None, None, None, counts), (fake, 1, 1, buf, buf, None, counts)]
    for args in bad:
        assert lib.odo_volume_mesh(*args) == -1, args[1:3]
        assert "odo_volume_mesh" in L.last_error()
    for args in ((None, q, w), (fake, None, w), (fake, q, None), (fake, None, None)):
        assert lib.odo_volume_upload(*args) == -1
        assert "odo_volume_upload" in L.last_error()


# ---- the table -------------------------------------------------------------------------------------------------------------------
def test_header_table_equals_the_geometrically_derived_one(tmp_path):
    exe = str(tmp_path / "volume_mesh_table_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "volume_mesh_table_harness.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
    rows = [ln.split() for ln in out.stdout.splitlines()]
    assert [tuple(int(v) for v in r[2:]) for r in rows if r[0] == "path"] == PATHS
    assert [int(r[2]) for r in rows if r[0] == "dir"] == [dx + 2 * dy + 4 * dz for dx, dy, dz in DIRS]
    table = model_table()
    shape = {0: 0, 1: 0, 2: 0}
    entries = [r for r in rows if r[0] == "entry"]
    assert len(entries) == 96
    for r in entries:
        t, m, n = int(r[1]), int(r[2]), int(r[3])
        v = [int(x) for x in r[4:]]
        got = [tuple((v[6 * k + 2 * x], v[6 * k + 2 * x + 1]) for x in range(3)) for k in range(n)]
        assert got == table[t][m], (t, m, got, table[t][m])
        shape[n] += 1
    assert shape == {0: 12, 1: 48, 2: 36}, shape
    cells = {int(r[1]): int(r[2]) for r in rows if r[0] == "cell"}
    for pos8 in range(256):
        want = 0 if pos8 in (0, 255) else sum(len(table[t][(pos8 & 1) | (((pos8 >> p[1]) & 1) << 1) | (((pos8 >> p[2]) & 1) << 2) |
                                                          (((pos8 >> 7) & 1) << 3)]) for t, p in enumerate(PATHS))
        assert cells[pos8] == want, pos8


# ---- the model against the prose -------------------------------------------------------------------------------------------------
def test_vectorised_model_equals_the_loop_model_bit_for_bit():
    n_vert = n_tri = n_zero = n_coincident = 0
    for name, (p, q, w) in small_grids().items():
        X, N, T = mesh_model(q, w, p)
        Xl, Nl, Tl = mesh_loop(q, w, p)
        assert X.shape == Xl.shape and T.shape == Tl.shape, (name, X.shape, Xl.shape, T.shape, Tl.shape)
        assert np.array_equal(bits(X), bits(Xl)) and np.array_equal(bits(N), bits(Nl)), name
        assert np.array_equal(T, Tl), name
        n_vert += len(X)
        n_tri += len(T)
        n_zero += int((N[:, :3] == 0).all(1).sum())
        n_coincident += len(X) - len(np.unique(bits(X)[:, :3], axis=0))
    print(f"{n_vert} vertices, {n_tri} triangles, {n_zero} zero normals, {n_coincident} coincident vertices")
    assert n_vert > 500 and n_tri > 300 and 0 < n_zero < n_vert and n_coincident > 0


def test_rows_of_the_three_axis_edges_are_the_extracted_points():
    total = 0
    for name, (p, q, w) in {**small_grids(), **property_grids()}.items():
        X, N, _ = mesh_model(q, w, p)
        P, Np = extract_model(q, w, p)
        axis = X[:, 3] < 3
        got = X[axis].copy()
        got[:, 3] = 0
        assert got.shape == P.shape, (name, got.shape, P.shape)
        assert np.array_equal(bits(got), bits(P)) and np.array_equal(bits(N[axis]), bits(Np)), name
        total += len(P)
    assert total > 3000, total


# ---- properties ------------------------------------------------------------------------------------------------------------------
def _directed_edges(T):
    e = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]]).astype(np.int64)
    return e[:, 0] * (1 << 32) + e[:, 1], e[:, 1] * (1 << 32) + e[:, 0]


def _lattice(q, vkeys, tkeys, T):
    """fp64, per triangle and relative to its cell's corner 0: the three vertices on the unit lattice (alpha from the integers) and
    the gradient of the tetrahedron's linear interpolant."""
    nz, ny, nx = q.shape

    def ijk(vox):
        return np.stack([vox % nx, (vox // nx) % ny, vox // (nx * ny)], 1)

    vox, e = vkeys // 7, vkeys % 7
    a = ijk(vox)
    d = np.array(DIRS)[e]
    b = a + d
    qa = q[a[:, 2], a[:, 1], a[:, 0]].astype(np.float64)
    qb = q[b[:, 2], b[:, 1], b[:, 0]].astype(np.float64)
    alpha = qa / (qa - qb)
    cell, t = tkeys // 12, (tkeys // 2) % 6
    c0 = ijk(cell)
    V = [(a[T[:, x]] - c0) + alpha[T[:, x], None] * d[T[:, x]] for x in range(3)]
    path = np.array(PATHS)[t]                                              # (m, 4) corners
    off = np.stack([path & 1, (path >> 1) & 1, (path >> 2) & 1], 2)        # (m, 4, 3)
    node = c0[:, None, :] + off
    val = q[node[..., 2], node[..., 1], node[..., 0]].astype(np.float64)   # (m, 4)
    A = (off[:, 1:, :] - off[:, :1, :]).astype(np.float64)
    grad = np.linalg.solve(A, (val[:, 1:] - val[:, :1])[..., None])[..., 0]
    return V, grad


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fully_observed_volume_gives_a_closed_consistently_wound_surface(seed):
    p, q, w = property_grids()[f"closed {seed}"]
    assert (w > 0).all() and (q != 0).all()
    X, N, T, vkeys, tkeys = mesh_model(q, w, p, detail=True)
    fwd, rev = _directed_edges(T)
    uf, cf = np.unique(fwd, return_counts=True)
    assert (cf == 1).all()                                        # every directed edge exactly once ...
    assert np.array_equal(uf, np.unique(rev))                     # ... and its reverse exactly once
    V, E, F = len(X), len(uf) // 2, len(T)
    print(f"seed {seed}: {V} vertices, {E} edges, {F} triangles, Euler characteristic {V - E + F}")
    assert (V - E + F) % 2 == 0
    assert len(np.unique(T)) == V                                 # no unreferenced vertex
    P, grad = _lattice(q, vkeys, tkeys, T)
    n = np.cross(P[1] - P[0], P[2] - P[0])
    ln, lg = np.linalg.norm(n, axis=1), np.linalg.norm(grad, axis=1)
    assert (ln > 0).all() and (lg > 0).all()
    # fp64 on operands below 2 in magnitude (positions relative to the cell): differences carry ~4e-16, the cross product ~3e-15 of
    # absolute error whatever its length, the gradient comes from integers through a unimodular matrix. So the sine of the angle is
    # held to 1e-13 / |n|, thirty times that error
    sine = np.linalg.norm(np.cross(n, grad), axis=1) / (ln * lg)
    print(f"seed {seed}: smallest normal {ln.min():.2e} lattice units^2, largest sine of the angle to the gradient {sine.max():.2e}")
    assert (sine * ln < 1e-13).all(), (sine * ln).max()
    assert ((n * grad).sum(1) > 0).all()                          # counter-clockwise seen from where Q grows: no triangle excluded


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_with_unobserved_nodes_the_surface_has_boundaries_but_no_doubled_edge(seed):
    p, q, w = property_grids()[f"holed {seed}"]
    X, N, T, vkeys, tkeys = mesh_model(q, w, p, detail=True)
    fwd, _ = _directed_edges(T)
    assert len(np.unique(fwd)) == len(fwd)
    assert T.min() >= 0 and T.max() < len(X)
    # a vertex is referenced iff a live cell holds both ends of its edge (every such pair is an edge of the Kuhn split)
    nz, ny, nx = q.shape
    live, _ = live_patterns(q, w)
    vox, e = vkeys // 7, vkeys % 7
    i, j, k = vox % nx, (vox // nx) % ny, vox // (nx * ny)
    want = np.zeros(len(X), bool)
    for n in range(len(X)):
        d = DIRS[e[n]]
        for ci in range(i[n] - 1 + d[0], i[n] + 1):
            for cj in range(j[n] - 1 + d[1], j[n] + 1):
                for ck in range(k[n] - 1 + d[2], k[n] + 1):
                    if 0 <= ci < nx - 1 and 0 <= cj < ny - 1 and 0 <= ck < nz - 1 and live[ck, cj, ci]:
                        want[n] = True
    got = np.zeros(len(X), bool)
    got[np.unique(T)] = True
    print(f"seed {seed}: {len(X)} vertices, {int((~got).sum())} unreferenced, {len(T)} triangles")
    assert np.array_equal(got, want) and 0 < (~got).sum() < len(X)


def test_every_sign_pattern_of_a_cell():
    p, q, w = property_grids()["patterns"]
    live, pos8 = live_patterns(q, w)
    assert live.sum() == 256 and sorted(pos8[live].tolist()) == list(range(256))
    X, N, T = mesh_model(q, w, p)
    print(f"256 patterns: {len(X)} vertices, {len(T)} triangles")
    assert (len(X), len(T)) == (2432, 1920)


# ---- the model against the ground truth -----------------------------------------------------------------------------------------
def test_pinned_case_against_the_corridors_planes(pinned):   # noqa: F811
    """True poses, ten frames. Measured with this model: 151 864 vertices, 298 220 triangles in 1 114 375 live cells; distance to the
    nearest plane per direction e = 0 .. 6 at most 0.131 / 0.170 / 0.000 / 0.171 / 0.133 / 0.178 / 0.178 voxel, medians <= 0.022."""
    p, q, w, _ = pinned
    X, N, T = mesh_model(q, w, p)
    live, _ = live_patterns(q, w)
    dist, dots, ln, zero = plane_errors(X, N, p["vs"])
    print(f"true poses, model: {len(X)} vertices, {int(live.sum())} live cells, {len(T)} triangles; zero normals {int(zero.sum())}")
    for e in range(7):
        d = dist[X[:, 3] == e]
        print(f"  e = {e}: {len(d)} vertices; distance / voxel median {np.median(d) if len(d) else 0:.3f} max {d.max() if len(d) else 0:.3f}")
    assert len(X) > 100_000 and len(T) > 200_000
    assert dist.max() <= 0.5, dist.max()                       # EVERY vertex within half a voxel of a plane
    assert T.min() >= 0 and T.max() < len(X)


# ---- code object, PLY -----------------------------------------------------------------------------------------------------------
def test_mesh_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        for k in MESH_KERNELS:
            if re.fullmatch(r"_ZN3odo%d%sE\w+" % (len(k), k), name):      # the mangled odo::<k>(...): the name matched exactly
                found[k] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                            int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
                print(k, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
    assert sorted(found) == sorted(MESH_KERNELS), found
    assert all(v == (0, 0) for v in found.values()), found


def read_ply_mesh(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[-1])
    nf = int([ln for ln in lines if ln.startswith("element face")][0].split()[-1])
    assert [ln.split()[-1] for ln in lines if ln.startswith("property float")] == ["x", "y", "z", "nx", "ny", "nz"]
    assert "property list uchar int vertex_indices" in lines
    assert lines.index("element vertex %d" % nv) < lines.index("element face %d" % nf)
    assert len(body) == 24 * nv + 13 * nf
    vert = np.frombuffer(body[:24 * nv], "<f4").reshape(nv, 6)
    face = np.frombuffer(body[24 * nv:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert (face["n"] == 3).all()
    return vert, face["v"]


def test_ply_mesh_writer_round_trips(tmp_path):
    from odometry_amd import api
    rng = np.random.default_rng(2)
    xyz0 = rng.normal(size=(41, 4)).astype(f32)
    nrmw = rng.normal(size=(41, 4)).astype(f32)
    tri = rng.integers(0, 41, (77, 3)).astype(np.int32)
    path = str(tmp_path / "mesh.ply")
    api.write_ply_mesh(path, xyz0, nrmw, tri)
    vert, face = read_ply_mesh(path)
    assert np.array_equal(vert[:, :3], xyz0[:, :3]) and np.array_equal(vert[:, 3:], nrmw[:, :3]) and np.array_equal(face, tri)
    api.write_ply_mesh(path, np.zeros((0, 4), f32), np.zeros((0, 4), f32), np.zeros((0, 3), np.int32))
    vert, face = read_ply_mesh(path)
    assert len(vert) == 0 and len(face) == 0
