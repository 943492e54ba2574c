"""The moving TSDF volume (odo_volume_shift, _follow, the spill store; api.TsdfVolume.shift / follow / spilled) without a GPU: the ABI
and the refusals, the numpy model of the specification (include/odometry_hip.h) pinned to the prose by
plain-loop versions, the partition of the surface into what is spilled and what stays, the origin rule, the shared header as a
stand-alone program under sanitizers, a synthetic drive that leaves the box it started in, and the kernels' code-object metadata.

The model is the existing one plus a mask: shift_model moves the arrays, spill_model is test_volume_cpu.extract_model and
test_volume_colour_cpu.point_colours_model on the pre-shift grid with the predicate "a or b leaves" applied to their rows.
It is the yardstick of tests/test_gpu_volume_shift.py, which asks the GPU for the same bits."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from test_volume_cpu import (bits, empty_grid, extract_loop, extract_model, integrate_model, params, plane_errors, tiny_cases, words)
from test_volume_colour_cpu import edge_colours_loop, point_colours_model, random_colour

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DIRS3 = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
MAX_OFF = 1 << 24

NEW_SYMBOLS = ["odo_volume_shift", "odo_volume_window", "odo_volume_enable_spill", "odo_volume_spill_points", "odo_volume_set_follow",
               "odo_volume_follow", "odo_volume_shift_time", "odo_debug_volume_spill_guard"]
SHIFT_KERNELS = ["volume_shift_kernel", "volume_spill_count_kernel", "volume_spill_scan_kernel", "volume_spill_scatter_kernel",
                 "volume_spill_advance_kernel"]


# ---- the model -----------------------------------------------------------------------------------------------------------------
def origin_model(origin0, off, vs):
    """The window's origin: origin0 + (float)off * vs, one fp32 product and one fp32 sum."""
    return (np.asarray(origin0, f32) + np.asarray(off, np.int64).astype(f32) * f32(vs)).astype(f32)


def window(p, off):
    """The model parameters of the window `off` voxels from where p (origin = origin0) was created."""
    return dict(p, origin=tuple(origin_model(p["origin"], off, p["vs"])))


def _ranges(n, d):
    """Destination and source slices of one axis: new i = old i + d where both lie in [0, n)."""
    lo, hi = max(0, -d), min(n, n - d)
    return (slice(lo, hi), slice(lo + d, hi + d)) if lo < hi else (slice(0, 0), slice(0, 0))


def shift_model(q, w, col, d):
    """The grids (nz, ny, nx) and the colour grid (nz, ny, nx, 4) or None after a shift by d = (dx, dy, dz): new voxel (i, j, k) = old
    voxel (i + dx, j + dy, k + dz) inside the old grid, else 0."""
    nz, ny, nx = q.shape
    (xd, xs), (yd, ys), (zd, zs) = _ranges(nx, d[0]), _ranges(ny, d[1]), _ranges(nz, d[2])
    out = []
    for a in (q, w, col):
        if a is None:
            out.append(None)
            continue
        b = np.zeros_like(a)
        b[zd, yd, xd] = a[zs, ys, xs]
        out.append(b)
    return tuple(out)


def leaves_model(shape, d):
    """(nz, ny, nx) bool: old voxel v leaves iff v_c - d_c lies outside [0, n_c) on some axis."""
    nz, ny, nx = shape
    ax = [((np.arange(n) - dc < 0) | (np.arange(n) - dc >= n)) for n, dc in ((nx, d[0]), (ny, d[1]), (nz, d[2]))]
    return ax[2][:, None, None] | ax[1][None, :, None] | ax[0][None, None, :]


def edge_list(q, w):
    """(n, 4) int64 i, j, k, axis of extract_model's points, row for row (its mask and its order)."""
    nz, ny, nx = q.shape
    obs = w > 0
    keys, rows = [], []
    for c, ax in ((0, 2), (1, 1), (2, 0)):
        sa = [slice(None)] * 3
        sb = [slice(None)] * 3
        sa[ax], sb[ax] = slice(0, -1), slice(1, None)
        sa, sb = tuple(sa), tuple(sb)
        k, j, i = np.nonzero(obs[sa] & obs[sb] & ((q[sa] > 0) != (q[sb] > 0)))
        keys.append(((k.astype(np.int64) * ny + j) * nx + i) * 3 + c)
        rows.append(np.stack([i, j, k, np.full(len(i), c)], 1).astype(np.int64))
    order = np.argsort(np.concatenate(keys), kind="stable")
    return np.concatenate(rows)[order]


def spill_mask(q, w, d):
    """Which of extract_model's points a shift by d spills: the edge's voxel a or its voxel b leaves. Also the two flags."""
    e = edge_list(q, w)
    lv = leaves_model(q.shape, d)
    b = e[:, :3].copy()
    b[np.arange(len(e)), e[:, 3]] += 1
    la, lb = lv[e[:, 2], e[:, 1], e[:, 0]], lv[b[:, 2], b[:, 1], b[:, 0]]
    return la | lb, la, lb


def spill_model(q, w, col, p, d):
    """What a shift by d of the grid (q, w, col) in the window p appends to the store: xyz0, nrmw and rgba (None without colour)."""
    P, N = extract_model(q, w, p)
    m = spill_mask(q, w, d)[0]
    return P[m], N[m], (point_colours_model(q, w, col)[m] if col is not None else None)


def follow_model(pose, p, off, focus, threshold):
    """The shift that the 4x4 camera-to-world pose asks of the window `off` voxels from p's origin, 3 ints; None: a non-finite pose.
    fp64 from the fp32 entries."""
    A = np.asarray(pose, f32).astype(np.float64)
    if not np.isfinite(A).all():
        return None
    n = np.array(p["dims"], np.float64)
    vs = np.float64(f32(p["vs"]))
    o = origin_model(p["origin"], off, p["vs"]).astype(np.float64)
    pt = A[:3, 3] + np.float64(f32(focus)) * A[:3, 2]
    e = (pt - (o + (0.5 * n) * vs)) / vs
    if np.abs(e).max() < threshold:
        return (0, 0, 0)
    return tuple(int(x) for x in np.clip(np.rint(e), -n, n))


def offset_model(off, d):
    """off + d, or None when an axis would pass 2^24."""
    s = [int(a) + int(b) for a, b in zip(off, d)]
    return None if any(abs(x) > MAX_OFF for x in s) else tuple(s)


# ---- the same as plain loops -------------------------------------------------------------------------------------------------------
def shift_loop(q, w, col, d):
    nz, ny, nx = q.shape
    out = [None if a is None else np.zeros_like(a) for a in (q, w, col)]
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                s = (i + d[0], j + d[1], k + d[2])
                if 0 <= s[0] < nx and 0 <= s[1] < ny and 0 <= s[2] < nz:
                    for a, b in zip((q, w, col), out):
                        if a is not None:
                            b[k, j, i] = a[s[2], s[1], s[0]]
    return tuple(out)


def _leaves(v, d, dims):
    return any(not 0 <= v[c] - d[c] < dims[c] for c in range(3))


_loop_points = {}


def spill_loop(q, w, col, p, d):
    """extract_loop's points with the predicate decided edge by edge; also how many edges had a staying and b leaving. (The points of
    a grid are computed once: they do not depend on d.)"""
    nz, ny, nx = q.shape
    dims = (nx, ny, nz)
    key = (id(q), id(w), id(col))
    if key not in _loop_points:
        _loop_points[key] = extract_loop(q, w, p) + (edge_colours_loop(q, w, col, DIRS3) if col is not None else None,)
    P, N, rgba = _loop_points[key]
    keep, a_stays_b_leaves = [], 0
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for c in range(3):
                    b = [i, j, k]
                    b[c] += 1
                    if b[c] >= dims[c] or not (w[k, j, i] > 0 and w[b[2], b[1], b[0]] > 0) or (q[k, j, i] > 0) == (q[b[2], b[1], b[0]] > 0):
                        continue
                    la, lb = _leaves((i, j, k), d, dims), _leaves(b, d, dims)
                    keep.append(la or lb)
                    a_stays_b_leaves += int(lb and not la)
    keep = np.array(keep, bool)
    return P[keep], N[keep], (rgba[keep] if col is not None else None), a_stays_b_leaves


def follow_loop(pose, p, off, focus, threshold):
    A = [[float(f32(pose[r][c])) for c in range(4)] for r in range(4)]
    if not all(np.isfinite(x) for row in A for x in row):
        return None
    e = []
    for c in range(3):
        o = float(f32(f32(p["origin"][c]) + f32(f32(int(off[c])) * f32(p["vs"]))))
        vs = float(f32(p["vs"]))
        pt = A[c][3] + float(f32(focus)) * A[c][2]
        e.append((pt - (o + 0.5 * float(p["dims"][c]) * vs)) / vs)
    if max(abs(x) for x in e) < threshold:
        return (0, 0, 0)
    return tuple(int(max(-p["dims"][c], min(p["dims"][c], round(e[c])))) for c in range(3))   # (round: ties to even, as nearbyint)


# ---- the rows ----------------------------------------------------------------------------------------------------------------------
def shifts_for(dims):
    """The shifts every grid is put through: one voxel either way on each axis, a mixed one, all but one layer, everything, beyond."""
    nx, ny, nz = dims
    return [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (3, -2, 5), (nx - 1, 0, 0), (0, -(ny - 1), 0),
            (0, 0, nz - 1), (nx, 0, 0), (0, -ny, 0), (0, 0, nz + 3), (-1, -1, -1)]


def random_grid(dims, seed):
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    q = rng.integers(-32767, 32768, (nz, ny, nx)).astype(np.int16)
    w = rng.integers(1, 300, (nz, ny, nx)).astype(np.uint16)
    w[rng.uniform(size=w.shape) < 0.2] = 0
    q[w == 0] = 0
    return q, w


@functools.lru_cache(maxsize=None)
def grids():
    """name -> (p, q, w, col): three random grids with 20 % never observed (2 x 2 x 2; 64 x 4 x 4: a whole wave per row; 65 x 5 x 4:
    one word more, nx % 4 != 0) and the four tiny volumes of test_volume_cpu after their frames. All coloured at random; the window's
    origin0 is the case's origin."""
    out = {}
    for n, (dims, vs, origin) in enumerate([((2, 2, 2), 0.5, (0.25, -0.5, 1.0)), ((64, 4, 4), 0.04, (-1.3, 0.1, 0.7)),
                                             ((65, 5, 4), 0.04, (-1.3, 0.1, 0.7))]):
        p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=dims, vs=vs, origin=origin)
        q, w = random_grid(dims, 11 + n)
        out["random %dx%dx%d" % dims] = (p, q, w, random_colour(q.shape, 21 + n))
    for n, (p, frames) in enumerate(tiny_cases()):
        q, w = empty_grid(p)
        for raw, pose in frames:
            q, w, _, _ = integrate_model(q, w, raw, pose, p)
        out["tiny %d" % n] = (p, q, w, random_colour(q.shape, 31 + n))
    return out


def rows():
    """(name, p, q, w, col, d) for every grid and every shift."""
    return [(name, p, q, w, col, d) for name, (p, q, w, col) in grids().items() for d in shifts_for(p["dims"])]


# ---- ABI and refusals ------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    for name in ("enable_spill", "shift", "window", "set_follow", "follow", "spilled", "save_ply", "track"):
        assert callable(getattr(api.TsdfVolume, name))
    assert C.sizeof(_lib.VolumeFollowParams) == 8


def test_bad_arguments_are_refused_before_touching_a_device():
    """Every case below is refused by the validation alone: the volume's handle is a fake that is never dereferenced."""
    from odometry_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(8)
    d = (C.c_int * 3)(1, 0, 0)
    n = C.c_long(0)
    buf = np.zeros(8, f32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.odo_volume_shift(None, d) == -1 and lib.odo_volume_shift(fake, None) == -1
    assert "odo_volume_shift" in L.last_error()
    assert lib.odo_volume_window(None, None, None) == -1
    assert lib.odo_volume_shift_time(None, d, 1, fp) == -1 and lib.odo_volume_shift_time(fake, None, 1, fp) == -1
    assert lib.odo_volume_shift_time(fake, d, 1, None) == -1
    for reps in (0, -1, 10001):
        assert lib.odo_volume_shift_time(fake, d, reps, fp) == -1 and "reps" in L.last_error(), reps
    for cap in (0, -1, (1 << 28) + 1):
        assert lib.odo_volume_enable_spill(fake, cap) == -1 and "capacity" in L.last_error(), cap
    assert lib.odo_volume_enable_spill(None, 16) == -1
    assert lib.odo_volume_spill_points(None, 1, fp, fp, None, C.byref(n), None, 0) == -1
    assert lib.odo_volume_spill_points(fake, 1, fp, fp, None, None, None, 0) == -1         # no n_points
    assert lib.odo_volume_spill_points(fake, -1, fp, fp, None, C.byref(n), None, 0) == -1
    assert lib.odo_volume_spill_points(fake, (1 << 28) + 1, fp, fp, None, C.byref(n), None, 0) == -1
    assert lib.odo_volume_spill_points(fake, 2, None, fp, None, C.byref(n), None, 0) == -1   # a capacity without its buffers
    assert "odo_volume_spill_points" in L.last_error()
    for focus, th in ((-0.5, 4), (float("nan"), 4), (float("inf"), 4), (1.0, 0), (1.0, -3)):
        assert lib.odo_volume_set_follow(fake, C.byref(L.VolumeFollowParams(focus, th))) == -1, (focus, th)
        assert "odo_volume_set_follow" in L.last_error()
    assert lib.odo_volume_set_follow(None, None) == -1
    pose = np.eye(4, dtype=f32).T.reshape(16).copy()
    assert lib.odo_volume_follow(None, pose.ctypes.data_as(C.POINTER(C.c_float)), d) == -1
    assert lib.odo_volume_follow(fake, None, d) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        for at in (0, 9, 13, 15):
            A = pose.copy()
            A[at] = bad
            assert lib.odo_volume_follow(fake, A.ctypes.data_as(C.POINTER(C.c_float)), d) == -1 and "non-finite" in L.last_error()
    assert tuple(d) == (1, 0, 0)


# ---- the model against the prose ---------------------------------------------------------------------------------------------------
def test_vectorised_model_equals_the_loop_model_bit_for_bit():
    """Every grid under every shift. The reasons the rows are here for, as predicates on the model alone: a spilled edge whose a
    stays and whose b leaves (the edge is found from a's side only); a point that stays and whose normal changes (a neighbour of
    its gradient left: why the partition below leaves normals out); a spill that is neither empty nor the whole extraction; a
    shift that keeps one layer and one that keeps nothing."""
    met = dict(a_stays_b_leaves=0, normal_changes=0, proper_spill=0, one_layer=0, nothing_stays=0, coloured_points=0, rows=0)
    for name, p, q, w, col, d in rows():
        got = shift_model(q, w, col, d)
        ref = shift_loop(q, w, col, d)
        assert all(np.array_equal(a, b) for a, b in zip(got, ref)), (name, d)
        P, N, rgba = spill_model(q, w, col, p, d)
        Pl, Nl, rl, n_ab = spill_loop(q, w, col, p, d)
        assert P.shape == Pl.shape and np.array_equal(bits(P), bits(Pl)) and np.array_equal(bits(N), bits(Nl)) and \
            np.array_equal(rgba, rl), (name, d)
        m, la, lb = spill_mask(q, w, d)
        assert int((lb & ~la).sum()) == n_ab
        lv = leaves_model(q.shape, d)
        stays = int((~lv).sum())
        assert stays == int(np.prod([max(0, n - abs(dc)) for n, dc in zip(p["dims"], d)]))
        assert (got[1][~_entered(q.shape, d)] == w[~lv]).all()                 # what stays is what the new grid holds, in order
        total = len(edge_list(q, w))
        met["a_stays_b_leaves"] += n_ab
        met["proper_spill"] += int(0 < len(P) < total)
        met["one_layer"] += int(0 < stays <= max(np.prod(p["dims"]) // min(p["dims"]), 1) and max(abs(x) for x in d) > 1)
        met["nothing_stays"] += int(stays == 0 and len(P) == total and not got[1].any() and not got[2].any())
        met["coloured_points"] += int((rgba[:, 3] == 255).sum())
        met["rows"] += 1
        # the points that stay, before and after: same edges; normals compared
        Pb, Nb = extract_model(q, w, p)
        Pa, Na = extract_model(got[0], got[1], window(p, d))
        assert len(Pa) == total - len(P), (name, d)
        met["normal_changes"] += int((bits(Nb[~m][:, :3]) != bits(Na[:, :3])).any(1).sum())
        assert np.array_equal(Nb[~m][:, 3], Na[:, 3])                          # the weights never change
    print(met)
    assert all(v > 0 for v in met.values()), met


def _entered(shape, d):
    """(nz, ny, nx) bool: the NEW voxels that no old voxel fills."""
    return leaves_model(shape, tuple(-x for x in d))


def test_follow_model_equals_the_loop_model_on_poses_around_the_threshold():
    rng = np.random.default_rng(5)
    p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=(12, 8, 10), vs=0.25, origin=(-1.5, -1.0, 0.25))
    met = dict(stays=0, moves=0, clamped=0, tie=0)
    poses = []
    for n in range(300):
        A = np.eye(4)
        th = rng.uniform(-0.4, 0.4, 3)
        A[:3, :3] = _rot(*th)
        A[:3, 3] = rng.uniform(-1, 1, 3) * (0.5 if n % 3 else 6.0) + (0.0, 0.0, 0.0)
        poses.append(A)
    tie = np.eye(4)                       # e = (2.5, 0, 3.5): nearbyint gives (2, 0, 4)
    tie[:3, 3] = (0.625, 0.0, 1.5 + 0.875 - 1.0)
    poses.append(tie)
    for A in poses:
        for off in ((0, 0, 0), (3, -2, 7)):
            for focus, th in ((1.0, 2), (0.0, 1), (2.5, 6)):
                d = follow_model(A, p, off, focus, th)
                assert d == follow_loop(A, p, off, focus, th)
                met["stays" if d == (0, 0, 0) else "moves"] += 1
                met["clamped"] += int(any(abs(x) == n for x, n in zip(d, p["dims"])))
    assert follow_model(tie, p, (0, 0, 0), 1.0, 2) == (2, 0, 4)
    met["tie"] = 1
    bad = np.eye(4)
    bad[1, 1] = np.nan
    assert follow_model(bad, p, (0, 0, 0), 1.0, 2) is None and follow_loop(bad, p, (0, 0, 0), 1.0, 2) is None
    assert all(v > 0 for v in met.values()), met


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


# ---- partition -------------------------------------------------------------------------------------------------------------------
def test_spill_and_what_stays_partition_the_extraction():
    """Dyadic grids (vs = 2^-4, the origin a multiple of it): every voxel centre is exact in either window, so a point has the same
    bits before and after. As multisets of the (x, y, z, w) bit patterns, spill + extraction-after = extraction-before: nothing is
    lost and nothing is doubled. Normals are left out on purpose: a staying voxel's gradient reads neighbours that may have left, so
    a surviving point's normal can change or vanish (the rows above hold that it does) while its position and weight cannot."""
    def rec(P, N):
        a = np.concatenate([bits(P[:, :3]), bits(N[:, 3:4])], 1)
        return a[np.lexsort(a.T[::-1])]

    n_rows = 0
    for dims, seed in (((16, 6, 5), 3), ((9, 8, 10), 4), ((65, 5, 4), 5)):
        p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=dims, vs=2.0 ** -4, origin=(-0.5, 3.0 / 16, 1.25))
        q, w = random_grid(dims, seed)
        cen = origin_model(p["origin"], (0, 0, 0), p["vs"]).astype(np.float64)
        for d in shifts_for(dims):
            pw = window(p, d)
            assert np.array_equal(np.asarray(pw["origin"], np.float64), cen + np.array(d) / 16.0)     # exact
            q2, w2, _ = shift_model(q, w, None, d)
            Ps, Ns, _ = spill_model(q, w, None, p, d)
            Pa, Na = extract_model(q2, w2, pw)
            Pb, Nb = extract_model(q, w, p)
            assert np.array_equal(rec(np.concatenate([Ps, Pa]), np.concatenate([Ns, Na])), rec(Pb, Nb)), (dims, d)
            n_rows += 1
    assert n_rows == 42


# ---- origin rule -----------------------------------------------------------------------------------------------------------------
def test_origin_rule_restores_the_origin_where_an_accumulated_sum_does_not():
    """origin = origin0 + (float)off * vs from the cumulative shift: d then -d gives off = 0 and the first origin's bits, for every d.
    The naive rule, origin += (float)d * vs shift by shift, does not: with origin0 = 0.1 and vs = 0.04 a shift of 2 and back leaves
    it one ulp away (pinned below, and counted over d = 1 .. 64)."""
    origin0 = np.array([0.1, -3.3, 1.2345678], f32)    # full mantissas
    vs = f32(0.04)
    naive_off = 0
    for d in range(1, 65):
        dd = (d, -d, 2 * d)
        off = offset_model((0, 0, 0), dd)
        moved = origin_model(origin0, off, vs)
        assert (moved != origin0).all()
        back = origin_model(origin0, offset_model(off, tuple(-x for x in dd)), vs)
        assert np.array_equal(bits(back), bits(origin0)), d
        naive = (origin0 + np.array(dd, f32) * vs).astype(f32)
        naive = (naive + np.array([-x for x in dd], f32) * vs).astype(f32)
        naive_off += int((bits(naive) != bits(origin0)).any())
    print("naive accumulation misses the origin for", naive_off, "of 64 shifts")
    step = f32(f32(2) * vs)
    there = f32(f32(0.1) + step)
    assert f32(there + f32(f32(-2) * vs)) != f32(0.1)
    assert naive_off == 62      # (IEEE fp32 arithmetic of the naive rule alone: the same on every machine)
    # and the same cumulative shift reached along two routes gives the same window
    assert np.array_equal(bits(origin_model(origin0, offset_model(offset_model((0, 0, 0), (5, 1, -2)), (2, -1, 9)), vs)),
                          bits(origin_model(origin0, (7, 0, 7), vs)))
    assert offset_model((MAX_OFF - 1, 0, 0), (1, 0, 0)) == (MAX_OFF, 0, 0) and offset_model((MAX_OFF, 0, 0), (1, 0, 0)) is None
    assert offset_model((0, -MAX_OFF, 0), (0, -1, 0)) is None


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------
ROW = np.dtype([("pose", "<f4", 16), ("origin0", "<f4", 3), ("off", "<i4", 3), ("n", "<i4", 3), ("vs", "<f4"), ("focus", "<f4"),
                ("threshold", "<i4"), ("d_try", "<i4", 3)])
OUT = np.dtype([("origin", "<f4", 3), ("follow_ok", "<i4"), ("d", "<i4", 3), ("offset_ok", "<i4"), ("off_new", "<i4", 3),
                ("origin_new", "<f4", 3)])


def test_shared_header_equals_the_loop_models_under_sanitizers(tmp_path):
    """odometry_amd/csrc/volume_shift_math.h and host_fp.h's window_origin — the lines the device and the library compile — as a
    stand-alone g++ program with AddressSanitizer and UBSan: the shift and the predicate of every row against the loop models, the
    follow rule, the origin rule and the bound on the cumulative shift on poses round the threshold, non-finite poses, shifts of
    INT_MAX and off at 2^24, all byte for byte."""
    exe = str(tmp_path / "volume_shift_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "volume_shift_harness.cpp"), "-o", exe])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")

    def run(mode, blob):
        open(src, "wb").write(blob)
        out = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
        return open(dst, "rb").read()

    big = [(2 ** 31 - 1, 0, 0), (0, -2 ** 31, 0)]
    for name, p, q, w, col, d in rows() + [("tiny 0",) + grids()["tiny 0"] + (d,) for d in big]:
        nx, ny, nz = p["dims"]
        n = nx * ny * nz
        for with_col in (False, True):
            blob = run("shift", np.array([nx, ny, nz, *d, int(with_col)], "<i4").tobytes() + words(q, w).astype("<u4").tobytes() +
                       (col.tobytes() if with_col else b""))
            q2, w2, c2 = shift_loop(q, w, col if with_col else None, d) if max(abs(x) for x in d) < 2 ** 20 else \
                (np.zeros_like(q), np.zeros_like(w), np.zeros_like(col) if with_col else None)
            assert np.array_equal(np.frombuffer(blob[:4 * n], "<u4"), words(q2, w2)), (name, d)
            at = 4 * n
            if with_col:
                assert blob[at:at + 4 * n] == c2.tobytes(), (name, d)
                at += 4 * n
            lv = np.array([[[_leaves((i, j, k), d, (nx, ny, nz)) for i in range(nx)] for j in range(ny)] for k in range(nz)], np.uint8)
            assert blob[at:] == lv.tobytes(), (name, d)
    # follow, origin, bound
    rng = np.random.default_rng(9)
    p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=(12, 8, 10), vs=0.04, origin=(0.1, -3.3, 1.2345678))
    recs = []
    tries = [(1, 0, 0), (-1, -1, -1), (0, 0, 0), (2 ** 31 - 1, 0, 0), (0, -2 ** 31, 0)]
    offs = [(0, 0, 0), (3, -2, 7), (MAX_OFF, -MAX_OFF, MAX_OFF - 1), (-MAX_OFF, 1, 0)]
    for n in range(240):
        A = np.eye(4)
        A[:3, :3] = _rot(*rng.uniform(-0.4, 0.4, 3))
        A[:3, 3] = rng.uniform(-1, 1, 3) * (0.3 if n % 3 else 2.0) + (0.3, -3.1, 1.4)
        if n % 40 == 7:
            A[rng.integers(0, 4), rng.integers(0, 4)] = (np.nan, np.inf, -np.inf)[n % 3]
        recs.append((A, offs[n % 4] if n % 5 == 0 else offs[n % 2], (1.0, 0.0, 0.2)[n % 3], (2, 1, 6)[n % 3], tries[n % 5]))
    arr = np.zeros(len(recs), ROW)
    for r, (A, off, focus, th, d_try) in zip(arr, recs):
        r["pose"], r["origin0"], r["off"], r["n"] = np.asarray(A, f32).T.reshape(16), p["origin"], off, p["dims"]
        r["vs"], r["focus"], r["threshold"], r["d_try"] = p["vs"], focus, th, d_try
    got = np.frombuffer(run("follow", np.array([len(recs)], "<i4").tobytes() + arr.tobytes()), OUT)
    met = dict(refused=0, stays=0, moves=0, bound=0)
    for g, (A, off, focus, th, d_try) in zip(got, recs):
        assert np.array_equal(bits(g["origin"]), bits(origin_model(p["origin"], off, p["vs"])))
        d = follow_loop(A, p, off, focus, th)
        assert bool(g["follow_ok"]) == (d is not None)
        if d is None:
            met["refused"] += 1
        else:
            assert tuple(g["d"]) == d and d == follow_model(A, p, off, focus, th)
            met["stays" if d == (0, 0, 0) else "moves"] += 1
        new = offset_model(off, d_try)
        assert bool(g["offset_ok"]) == (new is not None)
        if new is None:
            met["bound"] += 1
        else:
            assert tuple(g["off_new"]) == new and np.array_equal(bits(g["origin_new"]), bits(origin_model(p["origin"], new, p["vs"])))
    print(met)
    assert all(v > 0 for v in met.values()), met


# ---- a drive that leaves its box ---------------------------------------------------------------------------------------------------
DRIVE = dict(frames=30, size=(120, 160), fwd_range=(0.45, 0.7), dims=(112, 64, 56), vs=0.1, origin=(-5.6, -3.23, 3.0), mu=0.3,
             max_depth=8.0, focus=5.8, threshold=10)


@functools.lru_cache(maxsize=None)
def drive_case():
    """The `natural` corridor at 120 x 160 driven 0.45 - 0.7 m per frame for 30 frames, true poses, into a window 11.2 x 6.4 x 5.6 m —
    a third as deep as the drive is long — that starts 3 m in front of the camera, where the 60-degree view first meets the floor, and
    follows the point 5.8 m in front of it (the window's centre at frame 0), moving once that is 1 m off. The origin's y is chosen
    so that neither the floor (y = 1.65) nor the ceiling (y = -3) passes through voxel centres: there q is 0 up to rounding, the
    sign of a rounding error decides which edge carries the point, and the half-voxel bound is met with equality. integrate_model and
    follow_model alternate as the attached tracker does it: follow, then integrate. Returns the frames and, from the model: the
    window's track, the spills, the final grid, and the grid of a second volume that never moves."""
    from odometry_amd import synth
    rows_, cols = DRIVE["size"]
    K = (525.0 * cols / 640.0, (cols - 1) / 2.0, (rows_ - 1) / 2.0)
    scene = synth.drive_scene("natural", 0)
    poses = synth.trajectory(DRIVE["frames"], 0, fwd_range=DRIVE["fwd_range"], max_offset=1.0)
    depth = [synth.sensor_depth(scene.render(T, rows_, cols, *K)[1], 1000.0, 30.0) for T in poses]
    p = params(K, 1000.0, DRIVE["size"], dims=DRIVE["dims"], vs=DRIVE["vs"], origin=DRIVE["origin"], mu=DRIVE["mu"],
               max_depth=DRIVE["max_depth"])
    q, w = empty_grid(p)
    qf, wf = empty_grid(p)
    off, shifts, spills = (0, 0, 0), [], []
    for raw, T in zip(depth, poses):
        d = follow_model(T, p, off, DRIVE["focus"], DRIVE["threshold"])
        if d != (0, 0, 0):
            Ps, Ns, _ = spill_model(q, w, None, window(p, off), d)
            q, w, _ = shift_model(q, w, None, d)
            off = offset_model(off, d)
            spills.append((Ps, Ns))
        shifts.append(d)
        q, w, _, _ = integrate_model(q, w, raw, T, window(p, off))
        qf, wf, _, _ = integrate_model(qf, wf, raw, T, p)
    return dict(p=p, depth=depth, poses=poses, shifts=shifts, spills=spills, off=off, q=q, w=w, fixed=(qf, wf))


def test_a_drive_that_leaves_its_box_keeps_its_surface():
    """Measured with this model: see the printed line. Every point of spill + final extraction lies within half a voxel of its
    nearest plane, DESIGN.md section 9.4's bound for true poses, although most of them left the grid long before the end."""
    c = drive_case()
    p = c["p"]
    moved = [d for d in c["shifts"] if d != (0, 0, 0)]
    assert len(moved) >= 3 and len(c["spills"]) == len(moved)
    assert all(len(Ps) > 0 for Ps, _ in c["spills"]), [len(Ps) for Ps, _ in c["spills"]]
    lo = np.asarray(p["origin"], np.float64)
    hi = lo + np.array(p["dims"]) * p["vs"]
    cam = c["poses"][-1][:3, 3]
    assert not ((cam >= lo) & (cam < hi)).all(), cam                       # the camera has left the box it started in
    length = cam[2] - c["poses"][0][2, 3]
    assert 2.5 <= length / (p["dims"][2] * p["vs"]) <= 3.5, length         # the grid is about a third as deep as the drive is long
    Pa, Na = extract_model(c["q"], c["w"], window(p, c["off"]))
    P = np.concatenate([Ps for Ps, _ in c["spills"]] + [Pa])
    N = np.concatenate([Ns for _, Ns in c["spills"]] + [Na])
    dist, dots, ln, zero = plane_errors(P, N, p["vs"])
    Pf, _ = extract_model(*c["fixed"], p)
    print(f"{len(moved)} shifts {moved[:4]} ...; window ends at off {c['off']}; spilled {len(P) - len(Pa)} + extracted {len(Pa)} = {len(P)} "
          f"points, a volume that never moves ends with {len(Pf)}; distance / voxel median {np.median(dist):.3f} "
          f"p99 {np.percentile(dist, 99):.3f} max {dist.max():.3f}")
    assert dist.max() <= 0.5, dist.max()
    assert len(Pf) < len(P)


# ---- code object -------------------------------------------------------------------------------------------------------------------
def test_shift_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
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
        for k in SHIFT_KERNELS:
            if k in name:
                found.setdefault(k, []).append((int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                                                int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))))
                print(name, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
    assert sorted(found) == sorted(SHIFT_KERNELS), found
    assert len(found["volume_shift_kernel"]) == 2                              # the 16-byte and the dword build
    assert all(v == (0, 0) for vs in found.values() for v in vs), found
