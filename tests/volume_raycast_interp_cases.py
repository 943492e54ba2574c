"""The numpy model of the ray-cast's trilinear colour sampling (include/odometry_hip.h, odo_volume_set_colour_sampling; DESIGN.md
section 9.11), shared by tests/test_volume_raycast_interp_cpu.py and tests/test_gpu_volume_raycast_interp.py: the vectorised rule
over the model of tests/test_volume_raycast_cpu.py (whose depth, raw and normals it returns as they are), the same as a plain loop
that does one fp32 operation at a time and tallies its branches, the rows made for each branch, the random grids and the pinned
sequences' model frames under the rule."""
import numpy as np

from test_volume_cpu import _pose, empty_grid
from test_volume_colour_cpu import empty_colour, integrate_colour_model
from test_volume_raycast_cpu import (EXACT, TALLIES, _cell_loop, _cells, _interp, _interp_loop, default_view, plane_grid, random_volume,
                                     ray_loop, raycast_frame, raycast_model, view)

f32 = np.float32
INTERP_TALLIES = ("hit", "invalid_cell", "none", "zero_cover", "coloured", "one", "partial", "all8", "m_one", "frac0", "tie", "clamp")


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _directions(pose, p, rp):
    """e and the rays' g (3, rows * cols), as raycast_model forms them."""
    rows, cols = rp["size"]
    f, cx, cy = (f32(v) for v in rp["K"])
    e, G = raycast_frame(pose, p)
    with np.errstate(all="ignore"):
        dx = np.tile((np.arange(cols, dtype=f32) - cx) / f, rows)
        dy = np.repeat((np.arange(rows, dtype=f32) - cy) / f, cols)
        g = np.stack([(G[r, 0] * dx + G[r, 1] * dy) + G[r, 2] for r in range(3)])
    return e, g


def corner_words(col, bi):
    """The colour words (N, 4) of the eight corners of the cells bi, in the corner order of the cell (bit 0 = x, 1 = y, 2 = z)."""
    nz, ny, nx = col.shape[:3]
    base = (bi[2] * ny + bi[1]) * nx + bi[0]
    flat = col.reshape(-1, 4)
    return [flat.take(base + ((d >> 2) * ny + ((d >> 1) & 1)) * nx + (d & 1), axis=0) for d in range(8)]


def colour_interp(col, ok, fr, bi):
    """The rule for N cell evaluations: (N, 4) uint8 and the coverage M."""
    cw = corner_words(col, bi)
    m = [(c[:, 3] > 0).astype(f32) for c in cw]
    out = np.zeros((len(ok), 4), np.uint8)
    with np.errstate(all="ignore"):
        M = _interp(m, fr)[0]
        has = ok & (M > f32(0.0))
        for k in range(3):
            P = _interp([m[d] * cw[d][:, k].astype(f32) for d in range(8)], fr)[0]
            out[:, k] = np.where(has, np.minimum(f32(255.0), np.rint(P / M)), f32(0.0)).astype(np.uint8)
    out[:, 3] = np.where(has, 255, 0)
    return out, M


def raycast_interp_model(q, w, col, pose, p, rp, detail=False):
    """raycast_model's depth, raw and nrmw, and the colour frame of the trilinear mode; detail: also the hits' indices, cell validity,
    points, fractions, cells and coverage."""
    depth, raw, nrmw, _ = raycast_model(q, w, None, pose, p, rp)
    rows, cols = rp["size"]
    rgba = np.zeros((rows * cols, 4), np.uint8)
    ih = np.nonzero(depth.reshape(-1) > 0)[0]         # a hit has z > t_prev >= 0
    e, g = _directions(pose, p, rp)
    more = dict(ih=ih)
    if len(ih):
        with np.errstate(all="ignore"):
            ok, _, fr, pt, bi, _ = _cells(q, w, e, g[:, ih], depth.reshape(-1)[ih])
        rgba[ih], M = colour_interp(col, ok, fr, bi)
        more.update(ok=ok, pt=pt, fr=fr, bi=bi, M=M)
    out = depth, raw, nrmw, rgba.reshape(rows, cols, 4)
    return out + (more,) if detail else out


# ---- the same, one fp32 operation at a time --------------------------------------------------------------------------------------
def ray_interp_loop(q, w, col, e, g, t_min, step, n_steps, scale, met, imet, spans=None):
    """One ray: ray_loop's z, raw and normal, and the colour of the trilinear mode; imet counts the branches of the rule; spans
    collects (colour, smallest and largest value per channel among the coloured corners) of every coloured pixel."""
    before = met["hit"]
    z, raw, nrm, _ = ray_loop(q, w, None, e, g, t_min, step, n_steps, scale, met)
    rgba = [0] * 4
    if met["hit"] == before:
        return z, raw, nrm, rgba
    imet["hit"] += 1
    cell = _cell_loop(q, w, e, g, z)
    if cell is None:
        imet["invalid_cell"] += 1
        return z, raw, nrm, rgba
    _, fr, _, bi, _ = cell
    cw = [col[bi[2] + (d >> 2), bi[1] + ((d >> 1) & 1), bi[0] + (d & 1)] for d in range(8)]
    m = [f32(1.0) if int(c[3]) > 0 else f32(0.0) for c in cw]
    n = sum(int(c[3]) > 0 for c in cw)
    with np.errstate(all="ignore"):
        M = _interp_loop(m, fr)[0]
        imet["frac0"] += int(all(x == 0 for x in fr))
        if not M > f32(0.0):
            imet["none" if n == 0 else "zero_cover"] += 1
            return z, raw, nrm, rgba
        imet["coloured"] += 1
        imet["one" if n == 1 else "all8" if n == 8 else "partial"] += 1
        imet["m_one"] += int(M == f32(1.0))
        tie = clamp = False
        for k in range(3):
            P = _interp_loop([f32(m[d] * f32(int(cw[d][k]))) for d in range(8)], fr)[0]
            v = f32(P / M)
            r = np.rint(v)
            tie |= bool(v - np.floor(v) == f32(0.5))
            clamp |= bool(r >= f32(255.0))
            rgba[k] = int(min(f32(255.0), r))
        rgba[3] = 255
        imet["tie"] += int(tie)
        imet["clamp"] += int(clamp)
    if spans is not None:
        on = [c for c in cw if int(c[3]) > 0]
        spans.append((rgba[:3], [min(int(c[k]) for c in on) for k in range(3)], [max(int(c[k]) for c in on) for k in range(3)]))
    return z, raw, nrm, rgba


def raycast_interp_loop(q, w, col, pose, p, rp, spans=None):
    """raycast_interp_model as plain loops over scalars; also ray_loop's tallies and those of the rule."""
    rows, cols = rp["size"]
    f, cx, cy = (f32(v) for v in rp["K"])
    e, G = raycast_frame(pose, p)
    met = {k: 0 for k in TALLIES}
    imet = {k: 0 for k in INTERP_TALLIES}
    depth, raw = np.zeros((rows, cols), f32), np.zeros((rows, cols), np.uint16)
    nrmw, rgba = np.zeros((rows, cols, 4), f32), np.zeros((rows, cols, 4), np.uint8)
    for y in range(rows):
        for x in range(cols):
            with np.errstate(all="ignore"):
                dx, dy = f32(f32(f32(x) - cx) / f), f32(f32(f32(y) - cy) / f)
                g = [f32(f32(f32(G[r, 0] * dx) + f32(G[r, 1] * dy)) + G[r, 2]) for r in range(3)]
            depth[y, x], raw[y, x], nrmw[y, x], rgba[y, x] = ray_interp_loop(q, w, col, e, g, f32(rp["t_min"]), f32(rp["step"]),
                                                                             rp["n_steps"], f32(p["depth_scale"]), met, imet, spans)
    return depth, raw, nrmw, rgba, met, imet


# ---- grids -----------------------------------------------------------------------------------------------------------------------
def random_views():
    """(tag, p, q, w, col, pose, view): random 9 x 8 x 7 and 65 x 5 x 2 grids with 10 % unobserved voxels and 30 % wc == 0."""
    out = []
    for seed in range(3):
        p, q, w, col = random_volume((9, 8, 7), seed)
        for pose, step in ((_pose((0.05 * seed, -0.1, 0.02), (0.0, 0.01, 0.0)), 0.02), (_pose((0.4, 0.3, -0.2), (-0.3, -0.25, 0.2)), 0.07)):
            out.append((f"9x8x7 seed {seed}", p, q, w, col, pose, view(p["size"], p["K"], 0.0, step, 40)))
        dims = (65, 5, 2)
        p, q, w, col = random_volume(dims, seed)
        centre = (np.asarray(p["origin"]) + 0.5 * p["vs"] * np.asarray(dims)).tolist()
        for pose, step in ((_pose((0.0, 0.3, 0.0), (centre[0] - 0.2, centre[1], centre[2] - 0.6)), 0.011),
                           (_pose((0.05 * seed, -0.1, 0.02), (0.0, 0.01, 0.0)), 0.02)):
            out.append((f"65x5x2 seed {seed}", p, q, w, col, pose, view(p["size"], p["K"], 0.0, step, 80)))
    return out


def full_colour(shape, seed):
    """Random colours, every voxel coloured."""
    rng = np.random.default_rng(seed)
    col = rng.integers(0, 256, tuple(shape) + (4,)).astype(np.uint8)
    col[..., 3] = rng.integers(1, 256, shape)
    return col


def holed(col, seed, share=0.3):
    """The grid with a share of its voxels never coloured."""
    out = col.copy()
    out[np.random.default_rng(seed).uniform(size=col.shape[:3]) < share] = 0
    return out


def interp_branch_rows():
    """(name, p, q, w, col, pose, view, predicate on the rule's tallies, check(rgba, nearest mode's rgba, detail) or None): each row is
    there for the branch its predicate names. The grid is section 9.7's dyadic one: voxel centres at multiples of 0.25. With the plane
    at h = 1 the field is 0 on the layer z = 4 and every ray hits at p_z = 4 exactly (fr_z = 0); with h = 0.875 the field is +-8192
    on the layers 3 and 4, the sample at p_z = 3.5 has F == 0 and every ray hits there (fr_z = 0.5). A camera moved by half a voxel
    has its principal ray at fr = 0.5."""
    rows = []
    p1, q1, w1 = plane_grid(**EXACT)
    ph, qh, wh = plane_grid(**dict(EXACT, h=0.875))
    shape = q1.shape
    size, K = (3, 5), (40.0, 2.0, 1.0)                # the principal point is pixel (2, 1)
    narrow = view(size, K, 0.0, 0.125, 16)
    wide = view((5, 7), (8.0, 3.0, 2.0), 0.0, 0.125, 16)   # p_x in 2.5 +- 1.31, p_y in 2.5 +- 0.88: cells 1 .. 3
    half = _pose(t=(0.125, 0.125, 0.0))               # e = (2.5, 2.5, 0)

    full = full_colour(shape, 3)
    rows.append(("all eight corners coloured", p1, q1, w1, full, _pose(), narrow,
                 lambda m: m["all8"] == m["m_one"] == m["hit"] == 15, None))
    for d in range(8):
        one = np.zeros(shape + (4,), np.uint8)
        c = (10 + 20 * d, 255 - 7 * d, 3 * d, 1 + d)
        one[3 + (d >> 2), 2 + ((d >> 1) & 1), 2 + (d & 1)] = c
        rows.append((f"corner {d} alone coloured", ph, qh, wh, one, half, narrow, lambda m: m["one"] == m["hit"] == 15,
                     lambda rgba, near, more, c=c: (rgba == np.array(c[:3] + (255,), np.uint8)).all()))
    rows.append(("no corner coloured", ph, qh, wh, np.zeros(shape + (4,), np.uint8), half, narrow,
                 lambda m: m["none"] == m["hit"] == 15, lambda rgba, near, more: not rgba.any()))
    gap = w1.copy()
    gap[5] = 0                                        # section 9.7's row: the crossing lies in a cell that is not valid
    rows.append(("a hit whose normal cell is invalid", p1, q1, gap, full, _pose(), view(size, K, 0.0, 0.75, 4),
                 lambda m: m["invalid_cell"] > 0 and m["invalid_cell"] + m["coloured"] == m["hit"],
                 lambda rgba, near, more: (rgba[more["ih"][~more["ok"]] // 5, more["ih"][~more["ok"]] % 5] == 0).all()))
    rows.append(("every fraction exactly 0", p1, q1, w1, full, _pose(), narrow, lambda m: m["frac0"] == 1,
                 lambda rgba, near, more: rgba[1, 2].tolist() == near[1, 2].tolist() == full[4, 2, 2, :3].tolist() + [255]))
    tie = full.copy()
    i = np.arange(shape[2])
    tie[..., 0], tie[..., 1], tie[..., 2] = 4 + 3 * i, 5 + 3 * i, 18 + i    # voxels 2 and 3: 10 | 13, 11 | 14, 20 | 21
    rows.append(("a fraction of exactly 0.5 and means that tie", p1, q1, w1, tie, _pose(t=(0.125, 0.0, 0.0)), narrow,
                 lambda m: m["tie"] > 0 and m["all8"] == m["hit"], lambda rgba, near, more: rgba[1, 2].tolist() == [12, 12, 20, 255]))
    const = np.zeros(shape + (4,), np.uint8)
    const[...] = (77, 3, 200, 9)
    rows.append(("a constant colour grid with holes", ph, qh, wh, holed(const, 5), half, wide,
                 lambda m: m["partial"] > 0 and m["coloured"] == m["hit"] == 35,
                 lambda rgba, near, more: (rgba[rgba[..., 3] == 255] == np.array((77, 3, 200, 255), np.uint8)).all()))
    ramp = full.copy()
    kk, jj, ii = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    ramp[..., 0], ramp[..., 1], ramp[..., 2] = 8 * ii, 8 * jj, 8 * kk

    def ramp_check(rgba, near, more):                 # l = 8 b + fr 8 is 8 p exactly, the lerps over equal values return them
        want = np.stack([np.rint(8.0 * more["pt"][c].astype(np.float64)) for c in range(3)], 1)
        return len(more["ih"]) == 35 and np.array_equal(rgba.reshape(-1, 4)[more["ih"], :3], want.astype(np.uint8))
    rows.append(("a ramp of 8 per voxel along every axis", ph, qh, wh, ramp, half, wide, lambda m: m["all8"] == m["hit"] == 35, ramp_check))
    sat = np.zeros(shape + (4,), np.uint8)
    sat[...] = (255, 0, 255, 200)
    rows.append(("channels at 0 and 255 under partial coverage", ph, qh, wh, holed(sat, 6), half, wide,
                 lambda m: m["clamp"] == m["coloured"] > 0 and m["partial"] > 0,
                 lambda rgba, near, more: (rgba[rgba[..., 3] == 255] == np.array((255, 0, 255, 255), np.uint8)).all()))
    return rows


def last_cell_views():
    """(tag, p, q, w, col, pose, view, the cell every hit lies in): the dyadic grid with the plane between the last two layers of an
    axis, seen along that axis from a camera over the last cell of the other two, so that every hit lies in the cell with b + 1 ==
    dim - 1 on all three axes and the last pair of the cell evaluation ends on the last word of either grid."""
    dims = (5, 5, 9)
    out = []
    for axis, (n, h) in enumerate(((5, 0.375), (5, 0.375), (9, 1.875))):   # the crossing half a voxel below the last centre
        p, _, w = plane_grid(**dict(EXACT, h=h))
        centres = f32(EXACT["origin"][axis]) + (np.arange(n) + 0.5) * EXACT["vs"]
        line = np.rint(32767.0 * np.clip((h - centres) / EXACT["mu"], -1.0, 1.0)).astype(np.int16)
        q = np.broadcast_to(np.moveaxis(line[:, None, None], 0, 2 - axis), w.shape).copy()
        # the camera looks along +axis: its z axis is the world's `axis`, its centre over the middle of the last cell of the other two
        R = np.roll(np.eye(3), axis + 1, axis=0)                            # camera (x, y, z) -> world axes (axis + 1, axis + 2, axis)
        t = np.array([EXACT["origin"][c] + (dims[c] - 1) * EXACT["vs"] for c in range(3)])   # e_c = dim_c - 1.5
        t[axis] = EXACT["origin"][axis] + 0.5 * EXACT["vs"]                # voxel centre 0 of the axis: e = 0
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = R, t
        cell = tuple(d - 2 for d in dims)
        out.append((f"last cell, along axis {axis}", p, q, w, full_colour(w.shape, 40 + axis), pose.astype(f32),
                    view((3, 5), (40.0, 2.0, 1.0), 0.0, 0.125, 4 * n), cell))
    return out


# ---- the pinned sequences under the rule --------------------------------------------------------------------------------------------
def photo_models_both(seq, frames=range(1, 7)):
    """volume_icp_photo_cases.photo_models with both colour frames: per k (depth, nrmw, rgba of the nearest mode, rgba of the
    trilinear mode), ray-cast from pose k - 1 through the volume of frames 0 .. k - 1."""
    from volume_icp_photo_cases import _grey_colour
    p = seq["p"]
    q, w = empty_grid(p)
    col = empty_colour(p)
    rp = default_view(p)
    out = {}
    for k in range(0, max(frames)):
        q, w, col = integrate_colour_model(q, w, col, seq["depth"][k], _grey_colour(seq["gray"][k]), seq["poses"][k], p)[:3]
        if k + 1 in frames:
            depth, _, nrmw, near = raycast_model(q, w, col, seq["poses"][k], p, rp)
            out[k + 1] = (depth, nrmw, near, raycast_interp_model(q, w, col, seq["poses"][k], p, rp)[3])
    return out
