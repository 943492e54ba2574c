"""The numpy model of the photometric term of frame-to-model tracking (include/odometry_hip.h), shared by
tests/test_volume_icp_photo_cpu.py and tests/test_gpu_volume_icp_photo.py: the vectorised rows, the same as a plain loop that does
one fp32 operation at a time and tallies its branches, the 31 sums, the whole alignment, the rows made for each branch and the two
pinned sequences with their coloured volumes. The geometric half is the model of tests/test_volume_icp_cpu.py, used as it is."""
import numpy as np

from test_volume_cpu import _pose, empty_grid, params
from test_volume_colour_cpu import empty_colour, integrate_colour_model
from test_volume_icp_cpu import (EXACT_K, RIBBED_GRID, RIBBED_SCENE, SMALL, acc_matrix, exact_frame, icp, icp_frame, icp_lane_sums,
                                 icp_rows_loop, icp_rows_model, icp_step_py, icp_tiles, mul4, small_K)
from test_volume_raycast_cpu import default_view, raycast_model

f32 = np.float32
NACC = 31
WEIGHTS = (0.001, 0.003, 0.01, 0.03)       # the grid of the defaults' rule: metres per grey level
HUBERS = (0.0, 4.0, 12.0, 36.0)            # grey levels; 0: no robust weight
PHOTO_TALLIES = ("no_point", "nan_proj", "off_left", "off_right", "off_top", "off_bottom", "model_hole", "gated", "on_gate", "tap00",
                 "tap01", "tap10", "tap11", "flat", "huber_below", "huber_on", "huber_above", "pairs", "geo_only", "photo_only",
                 "both", "neither", "lattice")


def grey_of(rgba):
    """The front end's integer rule on (..., 4) uint8: float32 grey levels."""
    c = np.asarray(rgba).astype(np.int64)
    return ((c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) >> 14).astype(f32)


# ---- the model: rows -------------------------------------------------------------------------------------------------------------
def icp_photo_rows_model(raw, grey, depth_m, nrmw_m, rgba_m, M, Cm, p, stride, dist_max, huber_delta, weight, photo_huber):
    """(rows, cols, 16) float32: {J0 .. J5, res, w} of the geometric row, then of the photometric row — zeros where a row is missing —
    and the masks of the geometric and of the photometric pairs."""
    rows, cols = p["size"]
    geo, mask_g = icp_rows_model(raw, depth_m, nrmw_m, M, Cm, p, stride, dist_max, huber_delta)
    f, cx, cy = (f32(v) for v in p["K"])
    scale, maxd = f32(p["depth_scale"]), f32(p["max_depth"])
    dist_max, lam, ph = f32(dist_max), f32(weight), f32(photo_huber)
    Cm = np.asarray(Cm, f32)
    ys, xs = np.arange(0, rows, stride), np.arange(0, cols, stride)
    X, Y = [a.reshape(-1) for a in np.meshgrid(xs, ys)]
    G = grey_of(rgba_m)
    A = np.asarray(rgba_m)[..., 3]
    with np.errstate(all="ignore"):
        r = np.asarray(raw, np.uint16)[Y, X]
        ok = r != 0
        D = r.astype(f32) / scale
        ok &= ~(D > maxd)
        dx, dy = (X.astype(f32) - cx) / f, (Y.astype(f32) - cy) / f
        pt = [dx * D, dy * D, D]
        pm = [((Cm[k, 0] * pt[0] + Cm[k, 1] * pt[1]) + Cm[k, 2] * pt[2]) + Cm[k, 3] for k in range(3)]
        ok &= pm[2] > f32(0.0)
        u, v = f * (pm[0] / pm[2]) + cx, f * (pm[1] / pm[2]) + cy
        x0, y0 = np.floor(u), np.floor(v)
        ok &= (x0 >= f32(0.0)) & (x0 < f32(cols - 1)) & (y0 >= f32(0.0)) & (y0 < f32(rows - 1))      # as floats; NaN fails
        xi, yi = np.floor(u + f32(0.5)), np.floor(v + f32(0.5))
        xj, yj = np.where(ok, xi, f32(0.0)).astype(np.int64), np.where(ok, yi, f32(0.0)).astype(np.int64)
        zm = np.asarray(depth_m, f32)[yj, xj]
        ok &= (zm > f32(0.0)) & (np.abs(pm[2] - zm) <= dist_max)
        xa, ya = np.where(ok, x0, f32(0.0)).astype(np.int64), np.where(ok, y0, f32(0.0)).astype(np.int64)
        xb, yb = np.minimum(xa + 1, cols - 1), np.minimum(ya + 1, rows - 1)      # (only read where ok, and there xa + 1 <= cols - 1)
        ok &= (A[ya, xa] != 0) & (A[ya, xb] != 0) & (A[yb, xa] != 0) & (A[yb, xb] != 0)
        g00, g01, g10, g11 = G[ya, xa], G[ya, xb], G[yb, xa], G[yb, xb]
        ax, ay = u - x0, v - y0
        dt, db = g01 - g00, g11 - g10
        top, bot = g00 + ax * dt, g10 + ax * db
        val = top + ay * (bot - top)
        gx = dt + ay * (db - dt)
        gy = bot - top
        res = lam * (val - np.asarray(grey, f32)[Y, X])
        a = (lam * f) / pm[2]
        jx, jy = a * gx, a * gy
        jz = -((jx * pm[0] + jy * pm[1]) / pm[2])
        J = [jx, jy, jz, pm[1] * jz - pm[2] * jy, pm[2] * jx - pm[0] * jz, pm[0] * jy - pm[1] * jx]
        if ph > 0:
            d = lam * ph
            w = np.where(np.abs(res) <= d, f32(1.0), d / np.abs(res))
        else:
            w = np.ones(len(res), f32)
        row = np.stack(J + [res, w], 1).astype(f32)
    out = np.zeros((rows, cols, 16), f32)
    out[..., :8] = geo
    out[Y, X, 8:] = np.where(ok[:, None], row, f32(0.0))
    mask_p = np.zeros((rows, cols), bool)
    mask_p[Y, X] = ok
    return out, mask_g, mask_p


def _terms28(r):
    """The 28 exact fp64 terms of rows {J0 .. J5, res, w}, one row of 28 per row."""
    with np.errstate(all="ignore"):
        jw = (r[:, :6] * r[:, 7:8]).astype(f32).astype(np.float64)
        rw = (r[:, 6] * r[:, 7]).astype(f32).astype(np.float64)
        Jd, rd = r[:, :6].astype(np.float64), r[:, 6].astype(np.float64)
        cols = [jw[:, a] * Jd[:, b] for a in range(6) for b in range(a, 6)] + [jw[:, a] * rd for a in range(6)] + [rw * rd]
    return np.stack(cols, 1) if len(r) else np.zeros((0, 28))


def icp_photo_acc(rows16, mask_g, mask_p):
    """The 31 sums in fp64 (numpy's pairwise order), per sum the sum of the terms' magnitudes, and the number of rows."""
    tg, tp = _terms28(rows16[..., :8][mask_g]), _terms28(rows16[..., 8:][mask_p])
    t = np.concatenate([tg, tp])
    acc = np.concatenate([t.sum(0), [float(len(tg)), float(len(tp)), tp[:, 27].sum()]])
    mag = np.concatenate([np.abs(t).sum(0), [float(len(tg)), float(len(tp)), np.abs(tp[:, 27]).sum()]])
    return acc, mag, len(tg) + len(tp)


def icp_photo_acc_kernel_order(rows16, mask_g, mask_p, stride):
    """The 31 sums in the kernels' order: per block of the rows kernel 512 rows, the geometric ones of its 256 threads and then the
    photometric ones (all-zero where a row is missing), through icp_lane_sums — sums 0 .. 27 over all 512, the geometric count over
    the first 256, the photometric count and cost over the last 256 — then the blocks' partials through icp_lane_sums again. The
    device's bits."""
    partials = []
    for r, mg, mp in icp_tiles(stride, rows16, mask_g, mask_p):
        tg, tp = _terms28(r[:, :8]), _terms28(r[:, 8:])
        partials.append(np.concatenate([icp_lane_sums(np.concatenate([tg, tp])),
                                        [icp_lane_sums(mg), icp_lane_sums(mp), icp_lane_sums(tp[:, 27])]]))
    return icp_lane_sums(np.array(partials))


# ---- the same, one fp32 operation at a time --------------------------------------------------------------------------------------
def icp_photo_rows_loop(raw, grey, depth_m, nrmw_m, rgba_m, M, Cm, p, stride, dist_max, huber_delta, weight, photo_huber):
    """icp_photo_rows_model as plain loops over scalars; also the 31 sums in raster order (per pixel the geometric row, then the
    photometric one) and how often each branch of the photometric row was taken. The geometric rows are icp_rows_loop's."""
    rows, cols = p["size"]
    geo, _, _ = icp_rows_loop(raw, depth_m, nrmw_m, M, Cm, p, stride, dist_max, huber_delta)
    f, cx, cy = (f32(v) for v in p["K"])
    scale, maxd = f32(p["depth_scale"]), f32(p["max_depth"])
    dist_max, lam, ph = f32(dist_max), f32(weight), f32(photo_huber)
    Cm = np.asarray(Cm, f32)
    half, zero = f32(0.5), f32(0.0)
    out = np.zeros((rows, cols, 16), f32)
    out[..., :8] = geo
    acc = [0.0] * NACC
    met = {k: 0 for k in PHOTO_TALLIES}

    def add(row, photometric):
        J, res, w = [f32(c) for c in row[:6]], f32(row[6]), f32(row[7])
        jw = [float(f32(J[a] * w)) for a in range(6)]
        k = 0
        for a in range(6):
            for b in range(a, 6):
                acc[k] += jw[a] * float(J[b])
                k += 1
        for a in range(6):
            acc[21 + a] += jw[a] * float(res)
        cost = float(f32(res * w)) * float(res)
        acc[27] += cost
        if photometric:
            acc[29] += 1.0
            acc[30] += cost
        else:
            acc[28] += 1.0

    def photo(x, y):
        r = int(raw[y, x])
        if r == 0:
            return "no_point"
        D = f32(f32(r) / scale)
        if D > maxd:
            return "no_point"
        dx, dy = f32(f32(f32(x) - cx) / f), f32(f32(f32(y) - cy) / f)
        pt = [f32(dx * D), f32(dy * D), D]
        pm = [f32(f32(f32(f32(Cm[k, 0] * pt[0]) + f32(Cm[k, 1] * pt[1])) + f32(Cm[k, 2] * pt[2])) + Cm[k, 3]) for k in range(3)]
        if not pm[2] > zero:
            return "no_point"
        u = f32(f32(f * f32(pm[0] / pm[2])) + cx)
        v = f32(f32(f * f32(pm[1] / pm[2])) + cy)
        x0, y0 = np.floor(u), np.floor(v)
        if np.isnan(x0) or np.isnan(y0):
            return "nan_proj"
        if not x0 >= zero:
            return "off_left"
        if not x0 < f32(cols - 1):
            return "off_right"
        if not y0 >= zero:
            return "off_top"
        if not y0 < f32(rows - 1):
            return "off_bottom"
        xi, yi = int(np.floor(f32(u + half))), int(np.floor(f32(v + half)))
        zm = f32(depth_m[yi, xi])
        if not zm > zero:
            return "model_hole"
        gap = np.abs(f32(pm[2] - zm))
        if not gap <= dist_max:
            return "gated"
        met["on_gate"] += int(gap == dist_max)
        xa, ya = int(x0), int(y0)
        taps = [rgba_m[ya, xa], rgba_m[ya, xa + 1], rgba_m[ya + 1, xa], rgba_m[ya + 1, xa + 1]]
        missing = [name for name, c in zip(("tap00", "tap01", "tap10", "tap11"), taps) if int(c[3]) == 0]
        if missing:
            for name in missing:
                met[name] += 1
            return "tap"
        g00, g01, g10, g11 = (f32((int(c[0]) * 4899 + int(c[1]) * 9617 + int(c[2]) * 1868 + 8192) >> 14) for c in taps)
        ax, ay = f32(u - x0), f32(v - y0)
        dt, db = f32(g01 - g00), f32(g11 - g10)
        top, bot = f32(g00 + f32(ax * dt)), f32(g10 + f32(ax * db))
        val = f32(top + f32(ay * f32(bot - top)))
        gx = f32(dt + f32(ay * f32(db - dt)))
        gy = f32(bot - top)
        met["flat"] += int(gx == 0 and gy == 0)
        res = f32(lam * f32(val - f32(grey[y, x])))
        a = f32(f32(lam * f) / pm[2])
        jx, jy = f32(a * gx), f32(a * gy)
        jz = f32(-f32(f32(f32(jx * pm[0]) + f32(jy * pm[1])) / pm[2]))
        J = [jx, jy, jz, f32(f32(pm[1] * jz) - f32(pm[2] * jy)), f32(f32(pm[2] * jx) - f32(pm[0] * jz)),
             f32(f32(pm[0] * jy) - f32(pm[1] * jx))]
        w = f32(1.0)
        if ph > 0:
            d, mag = f32(lam * ph), np.abs(res)
            met["huber_below" if mag < d else "huber_on" if mag == d else "huber_above"] += 1
            if not mag <= d:
                w = f32(d / mag)
        return J + [res, w]

    with np.errstate(all="ignore"):
        for y in range(0, rows, stride):
            for x in range(0, cols, stride):
                met["lattice"] += 1
                has_g = bool(geo[y, x, 7] != 0)                  # a pair's weight is 1 or delta / |res|, never 0
                row = photo(x, y)
                if isinstance(row, str):
                    if row != "tap":
                        met[row] += 1
                    row = None
                else:
                    out[y, x, 8:] = row
                    met["pairs"] += 1
                if has_g:
                    add(out[y, x, :8], False)
                if row is not None:
                    add(out[y, x, 8:], True)
                met["both" if has_g and row is not None else "geo_only" if has_g else "photo_only" if row is not None else "neither"] += 1
    return out, np.array(acc), met


# ---- the whole loop --------------------------------------------------------------------------------------------------------------
def photo(weight=None, huber_delta=None):
    """The model's odo_icp_photo_params; the defaults of api.TsdfVolume.photo_params."""
    from odometry_amd import api
    return dict(weight=api.TsdfVolume.ICP_PHOTO_WEIGHT if weight is None else weight,
                huber_delta=api.TsdfVolume.ICP_PHOTO_HUBER if huber_delta is None else huber_delta)


def icp_photo_align_model(raw, grey, depth_m, nrmw_m, rgba_m, P_m, P_init, p, ic, ph, step=icp_step_py, sums=None):
    """icp_align_model with the photometric rows: the same dict, plus photo_pairs and photo_cost; a trace entry's acc has 31 sums.
    The step sees the first 29."""
    M, Cm = icp_frame(P_m, P_init)
    status, n, trace, acc = 0, 0, [], None
    for level, (stride, iters) in enumerate(zip(ic["strides"], ic["iters"])):
        for _ in range(iters):
            if status:
                break
            rows16, mg, mp = icp_photo_rows_model(raw, grey, depth_m, nrmw_m, rgba_m, M, Cm, p, stride, ic["dist_max"], ic["huber_delta"],
                                                  ph["weight"], ph["huber_delta"])
            acc = sums(rows16, mg, mp) if sums else icp_photo_acc(rows16, mg, mp)[0]
            failed, converged, delta, Cm = step(acc[:29], Cm, ic["min_pairs"], ic["eps_t"], ic["eps_r"])
            trace.append((level, acc, delta, Cm))
            n += 1
            status = 1 if failed else 0
            if converged:
                break
    out = dict(status=status, iterations=n, pairs=0.0, cost=0.0, eig_min=0.0, eig_max=0.0, photo_pairs=0.0, photo_cost=0.0, C=Cm, trace=trace)
    if acc is not None:
        ev = np.linalg.eigvalsh(acc_matrix(acc)) if np.isfinite(acc).all() else np.full(6, np.nan)
        out.update(pairs=acc[28], cost=acc[27], eig_min=ev[0], eig_max=ev[-1], photo_pairs=acc[29], photo_cost=acc[30])
    if out["status"] == 0 and not np.isfinite(Cm).all():
        out["status"] = 1
    if out["status"] == 0 and (acc is None or out["eig_min"] < float(f32(ic["min_eig_ratio"])) * out["eig_max"]):
        out["status"] = 2 if acc is not None else 1
    out["abs_pose"] = mul4(P_m, Cm) if out["status"] == 0 else np.full((4, 4), np.nan, f32)
    return out


# ---- frames --------------------------------------------------------------------------------------------------------------------
def random_photo_frames(seed, size=(24, 32), *more):
    """test_volume_icp_cpu.random_frames (more: its K and motion) with a random grey frame and a random colour frame with holes:
    (p, raw, grey, depth, nrmw, rgba, P_m, P_init)."""
    from test_volume_icp_cpu import random_frames
    p, raw, depth, nrmw, P_m, P_init = random_frames(seed, size, *more)
    rng = np.random.default_rng(700 + seed)
    base = 120 + 60 * np.sin(np.arange(size[1]) / 3.0)[None, :] * np.cos(np.arange(size[0]) / 2.5)[:, None]
    rgba = np.clip(base[..., None] + rng.normal(0, 12, size + (4,)), 0, 255).astype(np.uint8)
    rgba[..., 3] = 255
    rgba[rng.uniform(size=size) < 0.08] = 0
    grey = np.clip(base + rng.normal(0, 6, size), 0, 255).astype(f32)
    return p, raw, grey, depth, nrmw, rgba, P_m, P_init


def tiny_photo_views():
    """The tiny volumes' coloured ray-casts from their own poses as model frames, their frames' raw depth as sensor frames and a seeded
    grey frame: (p, raw, grey, depth, nrmw, rgba, P_m, P_init)."""
    from test_volume_cpu import tiny_cases
    from test_volume_raycast_cpu import tiny_volumes
    out = []
    rng = np.random.default_rng(31)
    for (p, q, w, col, poses), (_, frames) in zip(tiny_volumes(), tiny_cases()):
        rp = default_view(p, n_steps=30)
        for k, pose in enumerate(poses):
            depth, _, nrmw, rgba = raycast_model(q, w, col, pose, p, rp)
            raw, other = frames[(k + 1) % len(frames)]
            out.append((p, raw, rng.uniform(0, 255, p["size"]).astype(f32), depth, nrmw, rgba, pose, other))
    return out


def exact_photo_frame(size=(4, 6), zm=3.5, grey=50.0):
    """test_volume_icp_cpu.exact_frame with a colour frame whose grey is 10 x + 3 y (R = G = B, so the integer rule returns it) and a
    constant grey frame: with a translation of 2 along z, u = x / 2 + t_x and v = y / 2 + t_y."""
    p, raw, depth, nrmw = exact_frame(size, zm)
    g = (10 * np.arange(size[1])[None, :] + 3 * np.arange(size[0])[:, None]) % 256
    rgba = np.stack([g, g, g, np.full(size, 255)], -1).astype(np.uint8)
    return p, raw, np.full(size, grey, f32), depth, nrmw, rgba


def boundary_colours():
    """(R, G, B) whose weighted sum plus 8192 is a multiple of 16384, and ones a single unit below it: the integer rule's `>> 14` turns
    over between them."""
    out = {0: [], 16383: []}
    R, G = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for B in range(256):
        rem = (R * 4899 + G * 9617 + B * 1868 + 8192) % 16384
        for want in out:
            for r, g in zip(*np.nonzero(rem == want)):
                if len(out[want]) < 12:
                    out[want].append((int(r), int(g), B))
    return out[0] + out[16383]


def photo_branch_rows():
    """(name, p, raw, grey, depth, nrmw, rgba, M, C, stride, dist_max, huber_delta, weight, photo_huber, predicate on the loop's
    tallies): each row is there for the branch its predicate names."""
    out = []
    eye = np.eye(4, dtype=f32)

    def fwd(tx=0.0, ty=0.0):
        return _pose(t=(tx, ty, 2.0)).astype(f32)            # pm = (x / 2 + tx, y / 2 + ty, 4): u = pm_x, v = pm_y

    def add(name, fr, Cm, pred, stride=1, dist_max=1.0, huber=0.0, weight=0.25, photo_huber=0.0):
        p, raw, grey, depth, nrmw, rgba = fr
        out.append((name, p, raw, grey, depth, nrmw, rgba, eye, Cm, stride, dist_max, huber, weight, photo_huber, pred))

    add("x0 = -1 with xi = 0", exact_photo_frame(), fwd(tx=-0.25), lambda m: m["off_left"] == 4 and m["geo_only"] == 4 and m["pairs"] > 0)
    p, raw, grey, depth, nrmw, rgba = exact_photo_frame()
    flat_n = nrmw.copy()
    flat_n[:2, :3, :3] = 0
    add("a zero normal, four coloured taps", (p, raw, grey, depth, flat_n, rgba), fwd(), lambda m: m["photo_only"] > 0 and m["both"] > 0)
    add("x0 = cols - 1 and y0 = rows - 1", exact_photo_frame(), fwd(tx=3.0, ty=2.0),
        lambda m: m["off_right"] == 2 * 4 and m["off_bottom"] == 4 * 2 and m["pairs"] == 4 * 2)
    for name, (hy, hx), (tx, ty) in (("tap00", (0, 0), (0.0, 0.0)), ("tap01", (0, 5), (2.0, 0.0)), ("tap10", (3, 0), (0.0, 1.0)),
                                     ("tap11", (3, 5), (2.0, 1.0))):
        hole = rgba.copy()
        hole[hy, hx] = (9, 9, 9, 0)                          # coloured bytes, no weight: A alone decides
        add(f"{name} alone with A = 0", (p, raw, grey, depth, nrmw, hole), fwd(tx, ty),
            lambda m, name=name: m[name] > 0 and sum(m[k] for k in ("tap00", "tap01", "tap10", "tap11")) == m[name] and m["pairs"] > 0)
    gap = depth.copy()
    gap[0, :2] = 0
    add("model depth 0 at the nearest pixel", (p, raw, grey, gap, nrmw, rgba), fwd(), lambda m: m["model_hole"] > 0 and m["pairs"] > 0)
    step = depth.copy()
    step[:, :2] = 3.25                                      # |pm_z - zm| = 0.75 there, 0.5 = dist_max elsewhere
    add("|pm_z - zm| exactly on the gate", (p, raw, grey, step, nrmw, rgba), fwd(),
        lambda m: m["gated"] > 0 and m["on_gate"] == m["pairs"] > 0, dist_max=0.5)
    nanC = fwd()
    nanC[0, 0], nanC[0, 2] = 3e38, -3e38
    add("a NaN projection", exact_photo_frame(), nanC, lambda m: m["nan_proj"] > 0)
    const = rgba.copy()
    const[..., :3] = 77
    add("a flat patch", (p, raw, grey, depth, nrmw, const), fwd(), lambda m: m["flat"] == m["pairs"] > 0)
    tone = np.full(raw.shape, 77.0, f32)
    tone[:, 0], tone[:, 1], tone[:, 2:] = 76.0, 75.0, 73.0   # |res| = lambda {1, 2, 4} = 0.25, 0.5, 1 against lambda huber = 0.5
    add("photo_huber below, on and above", (p, raw, tone, depth, nrmw, const), fwd(),
        lambda m: m["huber_below"] > 0 and m["huber_on"] > 0 and m["huber_above"] > 0, photo_huber=2.0)
    for size in ((1, 1), (1, 64)):
        add(f"{size[0]} x {size[1]}: no photometric pair", exact_photo_frame(size), fwd(),
            lambda m: m["pairs"] == 0 and m["geo_only"] > 0 and m["off_top"] + m["off_bottom"] + m["off_right"] == m["lattice"])
    for s in (1, 2, 4, 16):
        add(f"stride {s} on 17 x 23", exact_photo_frame((17, 23)), fwd(),
            lambda m, s=s: m["lattice"] == (-(-17 // s)) * (-(-23 // s)) and m["pairs"] > 0, stride=s, dist_max=4.0)
    edge = np.zeros((4, 6, 4), np.uint8)
    cols24 = boundary_colours()
    edge.reshape(-1, 4)[:, :3] = cols24
    edge[..., 3] = 255
    add("colours on the boundary of >> 14", (p, raw, grey, depth, nrmw, edge), fwd(), lambda m: m["pairs"] > 0 and m["flat"] < m["pairs"])
    return out


# ---- the pinned sequences with colour ---------------------------------------------------------------------------------------------
def _grey_colour(grey):
    g = np.asarray(grey).astype(np.uint8)
    return np.ascontiguousarray(np.stack([g, g, g], -1))


def ribbed_photo_sequence(n=7):
    """test_volume_icp_cpu.ribbed_sequence with Scene.render's grey frames."""
    from odometry_amd import synth
    scene = synth.Scene(0, **RIBBED_SCENE)
    poses = synth.trajectory(n, 0, fwd_range=(0.1, 0.2), max_offset=1.0)
    f, cx, cy = small_K()
    frames = [scene.render(T, SMALL[0], SMALL[1], f, cx, cy) for T in poses]
    return dict(depth=[synth.sensor_depth(Z, 1000.0, 30.0) for _, Z in frames], gray=[img for img, _ in frames], poses=poses,
                p=params((f, cx, cy), 1000.0, SMALL, **RIBBED_GRID))


def corridor_photo_sequence(n=7):
    """test_volume_icp_cpu.corridor_sequence with its rendered grey frames."""
    from odometry_amd import synth
    f, cx, cy = small_K()
    seq = synth.make_rgbd_sequence(n, seed=0, rows=SMALL[0], cols=SMALL[1], f=f, cx=cx, cy=cy)
    return dict(depth=seq["depth"], gray=seq["gray"], poses=seq["poses"], p=params(seq, size=SMALL))


def photo_models(seq, frames=range(1, 7)):
    """Frames 0 .. k - 1 fused with their grey replicated into R, G and B at their true poses, the coloured ray-cast from pose k - 1:
    per k the model frame (depth, nrmw, rgba)."""
    p = seq["p"]
    q, w = empty_grid(p)
    col = empty_colour(p)
    rp = default_view(p)
    out = {}
    for k in range(0, max(frames)):
        q, w, col = integrate_colour_model(q, w, col, seq["depth"][k], _grey_colour(seq["gray"][k]), seq["poses"][k], p)[:3]
        if k + 1 in frames:
            depth, _, nrmw, rgba = raycast_model(q, w, col, seq["poses"][k], p, rp)
            out[k + 1] = (depth, nrmw, rgba)
    return out


def photo_frame_to_model(seq, models, ic, ph, step=icp_step_py, frames=range(1, 7)):
    """Frame k aligned from pose k - 1 against the model frame of pose k - 1, with the photometric term: per k the model's result."""
    return {k: icp_photo_align_model(seq["depth"][k], seq["gray"][k], *models[k], seq["poses"][k - 1], seq["poses"][k - 1], seq["p"], ic, ph,
                                     step=step) for k in frames}
