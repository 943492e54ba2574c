"""The dense stereo matcher's specification as code (include/odometry_hip.h, odo_stereo_depth_create), shared
by tests/test_stereo_depth_cpu.py and tests/test_gpu_stereo_depth.py: the launch constants read out of the kernels' header, the numpy
model (vectorised: a cost volume with a sentinel for inadmissible candidates, the box sum by summed-area table, np.float32 division
and np.rint), a plain-loop second implementation written independently of it (per pixel, per candidate, per tap, Python integers),
and the rows — each with the situation it is in the table for as a predicate on the model's outputs. Nothing here loads the GPU
library.

A row is (name, L, R, params, predicate). params: dict(dmin, dmax, A, uniq, lr_max, max_raw, fx, baseline, depth_scale); the rule's
one float is k = float32(16 fx baseline depth_scale). The model can be told to get one of four things wrong (SWITCHES); CAUGHT_BY
names, for each, the rows that are in the table to notice. Frames and model results are computed once per process and shared.

Two situations of the specification's list cannot occur and have no row. den == 0 at a winner: cm > c0 always, because dl is the
SMALLEST candidate of minimal cost (with cm == c0 the candidate dl - 1 would have won), so den = (cm - c0) + (cp - c0) >= 1; the rule's
`den <= 0` guard is exercised through sd_subpixel directly by the harness. Exactly one interior pixel with two or three candidates:
the interior pixel at the smallest column always has one candidate, the next one two; the degenerate rows are the frames with one,
two and three interior pixels, whose candidates number 1, 1 .. 2 and 1 .. 3."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "odometry_amd", "csrc")
BIG = 1 << 30                 # the sentinel of an inadmissible candidate: above every cost
NO_RIGHT = 255
STATS = ("interior", "matched", "rej_unique", "rej_lr", "rej_range", "sum_q")
SWITCHES = ("largest_wins", "exclude_winner_only", "subpixel_at_dmax", "half_away")
LOOP_WORK = 1_500_000         # rows whose pixels x candidates x taps stay below this go through the loop


def constants():
    """{kName: value} of every `constexpr int kName = <integer>;` line of stereo_depth_math.h and stereo_depth.hip.h."""
    out = {}
    for name in ("stereo_depth_math.h", "stereo_depth.hip.h"):
        for m in re.finditer(r"^constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, name)).read(), re.M):
            out[m.group(1)] = int(m.group(2))
    return out


def geometry(size, k=None):
    """launch_stereo_depth_stage's grid and store path for a frame (8-byte aligned outputs)."""
    k = k or constants()
    rows, cols = size
    return dict(blocks_x=-(-cols // k["kSdTileW"]), blocks_y=-(-rows // k["kSdTileH"]), vec=cols % 4 == 0)


def params(dmin=1, dmax=20, A=2, uniq=10, lr_max=1, max_raw=65535, fx=100.0, baseline=0.5, depth_scale=1000.0, k=None):
    """k, if given, is reached exactly: fx = k / 16, baseline = depth_scale = 1."""
    if k is not None:
        fx, baseline, depth_scale = float(k) / 16.0, 1.0, 1.0
    return dict(dmin=dmin, dmax=dmax, A=A, uniq=uniq, lr_max=lr_max, max_raw=max_raw, fx=fx, baseline=baseline, depth_scale=depth_scale)


def k_of(p):
    return np.float32(16.0 * p["fx"] * p["baseline"] * p["depth_scale"])


# ---- the model ------------------------------------------------------------------------------------------------------------------
def census(img):
    """rows x cols uint64, 0 outside the census domain. The bit order is this function's own: only Hamming distances are observable."""
    img = np.asarray(img, np.float32)
    rows, cols = img.shape
    out = np.zeros((rows, cols), np.uint64)
    if rows < 7 or cols < 9:
        return out
    c = img[3:rows - 3, 4:cols - 4]
    w = np.zeros(c.shape, np.uint64)
    bit = 0
    with np.errstate(invalid="ignore"):
        for dy in range(-3, 4):
            for dx in range(-4, 5):
                if dy == 0 and dx == 0:
                    continue
                n = img[3 + dy:rows - 3 + dy, 4 + dx:cols - 4 + dx]
                w |= (n < c).astype(np.uint64) << np.uint64(bit)
                bit += 1
    out[3:rows - 3, 4:cols - 4] = w
    return out


def _box(H, A):
    """Sum of H over (2A + 1)^2 windows by summed-area table, zero outside; H is (D, rows, cols)."""
    if A == 0:
        return H.copy()
    D, rows, cols = H.shape
    S = np.zeros((D, rows + 2 * A + 1, cols + 2 * A + 1), np.int64)
    S[:, A + 1:A + 1 + rows, A + 1:A + 1 + cols] = H
    S = S.cumsum(1).cumsum(2)
    n = 2 * A + 1
    return (S[:, n:, n:] - S[:, :-n, n:] - S[:, n:, :-n] + S[:, :-n, :-n]).astype(np.int32)


def stereo_model(L, R, p, largest_wins=False, exclude_winner_only=False, subpixel_at_dmax=False, half_away=False, details=False):
    """(depth uint16, q uint16, stats dict) of one pair, and with details=True a dict of the per-pixel intermediates."""
    L, R = np.asarray(L, np.float32), np.asarray(R, np.float32)
    rows, cols = L.shape
    dmin, dmax, A = p["dmin"], p["dmax"], p["A"]
    k = k_of(p)
    D = dmax - dmin + 1
    DD = D + 1                                                   # one more plane, d = dmax + 1, read by the subpixel_at_dmax switch only
    cl, cr = census(L), census(R)
    H = np.zeros((DD, rows, cols), np.int32)
    for i in range(DD):
        d = dmin + i
        if cols - 4 > d + 4:
            H[i, :, d + 4:cols - 4] = np.bitwise_count(cl[:, d + 4:cols - 4] ^ cr[:, 4:cols - 4 - d])
    C = _box(H, A)
    y, x = np.mgrid[0:rows, 0:cols]
    inner = (x >= A + 4) & (x < cols - A - 4) & (y >= A + 3) & (y < rows - A - 3)
    ds = dmin + np.arange(DD)
    adm = inner[None] & (x[None] - ds[:, None, None] >= A + 4)
    cost_all = np.where(adm, C, BIG)
    cost = cost_all[:D]

    def winner(cv):
        """Index of the winning plane and its cost; ties to the smallest d (the largest under the switch)."""
        if largest_wins:
            return cv.shape[0] - 1 - np.argmin(cv[::-1], axis=0), cv.min(axis=0)
        return np.argmin(cv, axis=0), cv.min(axis=0)

    il, c0 = winner(cost)
    interior = c0 < BIG
    dl = il + dmin
    idx = np.arange(D)[:, None, None]
    excluded = np.abs(idx - il[None]) <= (0 if exclude_winner_only else 1)
    c2 = np.where(excluded, BIG, cost).min(axis=0)
    unique = (c2 < BIG) & (c2.astype(np.int64) * (100 - p["uniq"]) > c0.astype(np.int64) * 100)
    # the right image's winners: CR(x', y, d) = C(x' + d, y, d)
    cright = np.full((D, rows, cols), BIG, np.int32)
    for i in range(D):
        d = dmin + i
        if d < cols:
            cright[i, :, :cols - d] = cost[i, :, d:]
    ir, cr0 = winner(cright)
    dr = np.where(cr0 < BIG, ir + dmin, NO_RIGHT).astype(np.uint8)
    if p["lr_max"] >= 0:
        drx = dr[y, np.clip(x - dl, 0, cols - 1)].astype(np.int64)
        lr_ok = np.abs(drx - dl) <= p["lr_max"]
    else:
        lr_ok = np.ones((rows, cols), bool)
    # sub-pixel
    take = lambda plane: np.take_along_axis(cost_all, np.clip(plane, 0, DD - 1)[None], axis=0)[0]
    cm = np.where(il >= 1, take(il - 1), BIG)
    cp = take(il + 1)
    if not subpixel_at_dmax:
        cp = np.where(il + 1 <= D - 1, cp, BIG)
    have = (cm < BIG) & (cp < BIG)
    den = np.where(have, cm.astype(np.int64) - 2 * c0 + cp, 0)
    num = np.where(have, cm.astype(np.int64) - cp, 0)
    dpos = np.maximum(den, 1)
    f = np.where(den > 0, np.sign(num) * ((16 * np.abs(num) + dpos) // (2 * dpos)), 0)
    qv = 16 * dl + f
    with np.errstate(over="ignore"):
        ratio = k / np.maximum(qv, 1).astype(np.float32)
    assert ratio.dtype == np.float32
    raw = np.floor(ratio.astype(np.float64) + 0.5) if half_away else np.rint(ratio).astype(np.float64)
    in_range = raw <= p["max_raw"]
    outcome = np.zeros((rows, cols), np.int8)                    # 0 not interior, 1 matched, 2 / 3 / 4 rejected by unique / lr / range
    outcome[interior] = 1
    outcome[interior & ~unique] = 2
    outcome[interior & unique & ~lr_ok] = 3
    outcome[interior & unique & lr_ok & ~in_range] = 4
    matched = outcome == 1
    depth = np.where(matched, raw, 0).astype(np.uint16)
    q = np.where(matched, qv, 0).astype(np.uint16)
    stats = dict(interior=int(interior.sum()), matched=int(matched.sum()), rej_unique=int((outcome == 2).sum()),
                 rej_lr=int((outcome == 3).sum()), rej_range=int((outcome == 4).sum()), sum_q=int(q.astype(np.int64).sum()))
    if not details:
        return depth, q, stats
    n_cand = adm[:D].sum(axis=0)
    return depth, q, stats, dict(outcome=outcome, dl=dl, f=f, c0=c0, c2=c2, cm=cm, cp=cp, den=den, num=num, raw=raw, ratio=ratio, dr=dr,
                                 n_cand=n_cand, x=x, y=y, qv=qv, k=k)


def stereo_loop(L, R, p):
    """The rules read off the prose, one pixel, one candidate and one tap at a time in Python integers: (depth, q, stats)."""
    import math
    L, R = np.asarray(L, np.float32), np.asarray(R, np.float32)
    rows, cols = L.shape
    dmin, dmax, A, uniq, lr_max, max_raw = (p[n] for n in ("dmin", "dmax", "A", "uniq", "lr_max", "max_raw"))
    k = k_of(p)

    def descriptors(img):
        px = [[float(v) for v in r] for r in img]
        out = {}
        for yy in range(3, rows - 3):
            for xx in range(4, cols - 4):
                c, w = px[yy][xx], 0
                for dy in range(-3, 4):
                    for dx in range(-4, 5):
                        if (dy, dx) != (0, 0):
                            w = (w << 1) | (1 if px[yy + dy][xx + dx] < c else 0)       # (a NaN compares false)
                out[(xx, yy)] = w
        return out

    cl, cr = descriptors(L), descriptors(R)

    def is_interior(xx, yy):
        return A + 4 <= xx < cols - A - 4 and A + 3 <= yy < rows - A - 3

    def admissible(xx, yy):
        return [d for d in range(dmin, dmax + 1) if xx - d >= A + 4] if is_interior(xx, yy) else []

    def C(xx, yy, d):
        return sum(bin(cl[(xx + i, yy + j)] ^ cr[(xx + i - d, yy + j)]).count("1") for j in range(-A, A + 1) for i in range(-A, A + 1))

    def right_winner(xr, yy):
        cands = [d for d in range(dmin, dmax + 1) if xr + d < cols and d in admissible(xr + d, yy)]
        costs = [C(xr + d, yy, d) for d in cands]
        return cands[costs.index(min(costs))]

    depth, q = np.zeros((rows, cols), np.uint16), np.zeros((rows, cols), np.uint16)
    n = dict.fromkeys(STATS, 0)
    for yy in range(rows):
        for xx in range(cols):
            cands = admissible(xx, yy)
            if not cands:
                continue
            n["interior"] += 1
            costs = {d: C(xx, yy, d) for d in cands}
            c0 = min(costs.values())
            dl = min(d for d in cands if costs[d] == c0)
            others = [costs[d] for d in cands if abs(d - dl) > 1]
            if not others or not (min(others) * (100 - uniq) > c0 * 100):
                n["rej_unique"] += 1
                continue
            if lr_max >= 0 and abs(right_winner(xx - dl, yy) - dl) > lr_max:
                n["rej_lr"] += 1
                continue
            f = 0
            if dl != dmin and dl != dmax and dl - 1 in costs and dl + 1 in costs:
                cm, cp = costs[dl - 1], costs[dl + 1]
                den, num = cm - 2 * c0 + cp, cm - cp
                if den > 0:
                    f = (16 * abs(num) + den) // (2 * den)
                    f = -f if num < 0 else f
            qq = 16 * dl + f
            ratio = float(k / np.float32(qq))                    # one fp32 division
            lo = math.floor(ratio)
            frac = ratio - lo
            raw = lo + 1 if frac > 0.5 or (frac == 0.5 and lo % 2 == 1) else lo
            if raw > max_raw:
                n["rej_range"] += 1
                continue
            n["matched"] += 1
            n["sum_q"] += qq
            depth[yy, xx], q[yy, xx] = raw, qq
    return depth, q, n


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def noise_image(seed, size):
    """Integers 0 .. 255 as fp32, smoothed a little so that neighbouring census words are related."""
    rng = np.random.default_rng([0x57E7E0, seed, size[0], size[1]])
    a = rng.integers(0, 256, (size[0] + 2, size[1] + 2)).astype(np.float64)
    a = (a[:-2, 1:-1] + a[2:, 1:-1] + a[1:-1, :-2] + a[1:-1, 2:] + 2 * a[1:-1, 1:-1]) / 6.0
    return np.rint(a).astype(np.float32)


def shifted_pair(seed, size, d):
    """left[y, x] = right[y, x - d] with an integer d; the left image's first d columns are other texture."""
    rows, cols = size
    wide = noise_image(seed, (rows, cols + d))
    return np.ascontiguousarray(wide[:, :cols]), np.ascontiguousarray(wide[:, d:])     # left[x] = wide[x]; right[x] = wide[x + d]


def half_pixel_pair(seed, size, d):
    """The left image lies between the right image shifted by d and by d + 1, nearer to one or the other from column to column."""
    rows, cols = size
    wide = noise_image(seed, (rows, cols + d + 1)).astype(np.float64)
    right = wide[:, d + 1:]
    a = 0.2 + 0.6 * (np.arange(cols) // 16 % 2)                  # weight of the d + 1 shift
    left = (1 - a) * wide[:, 1:cols + 1] + a * wide[:, :cols]
    return left.astype(np.float32), np.ascontiguousarray(right.astype(np.float32))


def periodic_pair(seed, size, period, d):
    rows, cols = size
    cell = noise_image(seed, (rows, period))
    right = np.tile(cell, (1, cols // period + 2))
    return np.ascontiguousarray(right[:, period - d % period:][:, :cols]), np.ascontiguousarray(right[:, period:][:, :cols])


def occluding_step(seed, size, d_back=4, d_front=12):
    """A foreground strip (disparity d_front) in front of a background (d_back): beside the strip the left image sees background that
    the right image does not."""
    rows, cols = size
    back = noise_image(seed, (rows, cols + d_back))
    front = noise_image(seed + 1, (rows, cols + d_front))
    xa, xb = cols // 2 - 8, cols // 2 + 14
    left, right = back[:, :cols].copy(), back[:, d_back:].copy()  # left[x] = back[x], right[x'] = back[x' + d_back]: left[x] = right[x - d_back]
    left[:, xa:xb] = front[:, xa:xb]
    right[:, xa - d_front:xb - d_front] = front[:, xa:xb]
    return left, right


def non_finite_pair(seed, size, d):
    left, right = shifted_pair(seed, size, d)
    spots = [(12, 30), (14, 41), (16, 52)]
    for (yy, xx), v in zip(spots, (np.nan, np.inf, -np.inf)):
        left[yy, xx] = v
        right[yy + 6, xx - 9] = v
    return left, right


@functools.lru_cache(maxsize=None)
def rendered_pair(drive="natural"):
    """(left, right, Z, fx, baseline): frame 0 of the drive's scene at 188 x 620 with the KITTI intrinsics halved."""
    from odometry_amd import synth
    scene = synth.drive_scene(drive, 0)
    T = synth.drive_trajectory(drive, 1, 0)[0]
    f, cx, cy = synth.KITTI_F / 2, synth.KITTI_CX / 2, synth.KITTI_CY / 2
    left, Z = scene.render(T, 188, 620, f, cx, cy, 0.0)
    right, _ = scene.render(T, 188, 620, f, cx, cy, synth.KITTI_BASELINE)
    for a in (left, right, Z):
        a.setflags(write=False)
    return np.asarray(left, np.float32), np.asarray(right, np.float32), Z, f, synth.KITTI_BASELINE


def rendered_params(A=2):
    from odometry_amd import synth
    return params(dmin=1, dmax=63, A=A, uniq=10, lr_max=1, fx=synth.KITTI_F / 2, baseline=synth.KITTI_BASELINE, depth_scale=1000.0)


@functools.lru_cache(maxsize=None)
def integer_pair():
    from odometry_amd import synth
    return synth.integer_disparity_pair(seed=1, rows=96, cols=320, band=24, dmin=3, dmax=60)


# ---- the rows ---------------------------------------------------------------------------------------------------------------------
def _m(T, code=1):
    return T["outcome"] == code


@functools.lru_cache(maxsize=None)
def rows():
    kc = constants()
    TW, TH = kc["kSdTileW"], kc["kSdTileH"]
    out = []

    def add(name, pair, p, pred):
        L, R = (np.ascontiguousarray(a, np.float32) for a in pair[:2])
        for a in (L, R):
            a.setflags(write=False)
        out.append((name, L, R, p, pred))

    # degenerate frames
    add("no census window: 6 x 8", shifted_pair(1, (6, 8), 2), params(A=0), lambda s, T: s["interior"] == 0)
    add("no interior pixel: 12 x 12 at A = 2", shifted_pair(1, (12, 12), 2), params(A=2), lambda s, T: s["interior"] == 0)
    for n in (1, 2, 3):
        add(f"{n} interior pixel(s) with 1 .. {n} candidates", shifted_pair(2, (7, 9 + n), 1), params(A=0, dmin=1, dmax=3),
            lambda s, T, n=n: s["interior"] == n and sorted(T["n_cand"][T["n_cand"] > 0]) == list(range(1, n + 1)) and s["rej_unique"] >= min(n, 2)
            and (T["outcome"][T["n_cand"] == 1] == 2).all())
    add("cols 50 below dmax 60", shifted_pair(3, (40, 50), 7), params(dmax=60),
        lambda s, T: s["matched"] > 0 and T["n_cand"].max() < 60 - 1 + 1)
    # launch geometry: either side of the tile's width and height, every cols % 4, several workgroups each way
    for r_, c_ in ((3 * TH, TW - 1), (3 * TH, TW), (3 * TH, TW + 1), (3 * TH - 1, TW), (3 * TH + 1, TW), (3 * TH, 2 * TW - 1),
                   (3 * TH, 2 * TW), (3 * TH + 1, 2 * TW + 1), (3 * TH + 1, TW + 2), (3 * TH + 2, TW + 3)):
        g = geometry((r_, c_), kc)
        add(f"tile geometry {r_} x {c_}", shifted_pair(4, (r_, c_), 5), params(A=1),
            lambda s, T, g=g, r_=r_, c_=c_: s["matched"] > 0 and g["blocks_x"] == -(-c_ // TW) and g["blocks_y"] == -(-r_ // TH)
            and _m(T)[:, -(1 + 4 + 1)].any() and _m(T)[-(1 + 3 + 1), :].any())
    # ties and rejections
    add("constant images, L == R", (np.full((20, 40), 7.0), np.full((20, 40), 7.0)), params(),
        lambda s, T: s["interior"] > 0 and s["rej_unique"] == s["interior"] and (T["c0"][T["outcome"] > 0] == 0).all())
    add("constant images, L != R", (np.full((20, 40), 3.0), np.full((20, 40), 200.0)), params(uniq=0),
        lambda s, T: s["interior"] > 0 and s["rej_unique"] == s["interior"])
    for period in (5, 17):
        add(f"right image of period {period}", periodic_pair(5, (24, 90), period, 3), params(dmin=1, dmax=40),
            lambda s, T, period=period: ((T["c0"] == 0) & (T["c2"] == 0) & (T["outcome"] == 2)).any()
            and (T["dl"][(T["c0"] == 0) & (T["c2"] == 0)] <= period).all() and s["matched"] < s["interior"] // 4)
    # known answers
    add("integer disparity pair 96 x 320", integer_pair(), params(dmin=1, dmax=63), lambda s, T: s["matched"] > s["interior"] // 2)
    # sub-pixel edges
    add("winner at dmin", shifted_pair(6, (30, 70), 4), params(dmin=4, dmax=20),
        lambda s, T: (_m(T) & (T["dl"] == 4)).sum() > 100 and (T["f"][T["dl"] == 4] == 0).all())
    add("winner at dmax", shifted_pair(6, (30, 70), 9), params(dmin=2, dmax=9),
        lambda s, T: (_m(T) & (T["dl"] == 9)).sum() > 100 and (T["f"][T["dl"] == 9] == 0).all())
    add("num of both signs", half_pixel_pair(7, (30, 100), 6), params(dmin=1, dmax=20),
        lambda s, T: (_m(T) & (T["f"] > 0)).sum() > 20 and (_m(T) & (T["f"] < 0)).sum() > 20 and T["f"].min() >= -8 and T["f"].max() <= 8)
    add("winner's neighbour inadmissible at the left edge", shifted_pair(8, (30, 70), 6), params(A=1, dmin=1, dmax=20),
        lambda s, T: (_m(T) & (T["dl"] == T["x"] - 1 - 4) & (T["dl"] < 20) & (T["dl"] > 1) & (T["f"] == 0)).any())
    # left-right
    for lr in (-1, 0, 1, 3):
        add(f"occluding step, lr_max {lr}", occluding_step(9, (40, 120)), params(dmin=1, dmax=24, lr_max=lr),
            lambda s, T, lr=lr: (s["rej_lr"] == 0) if lr < 0 else (s["rej_lr"] > 0 or lr == 3))
    # range and rounding: the pair's disparity is 8, so q = 128 where f = 0
    for tag, max_raw in (("at", 500), ("one below", 499), ("one above", 501)):
        add(f"max_raw {tag} a pixel's raw", shifted_pair(10, (24, 70), 8), params(dmin=1, dmax=20, max_raw=max_raw, k=128 * 500.0),
            lambda s, T, max_raw=max_raw: ((T["raw"] == 500) & (T["outcome"] == (4 if max_raw < 500 else 1))).sum() > 100)
    for half in (500.5, 502.5):
        add(f"k / q = {half}", shifted_pair(10, (24, 70), 8), params(dmin=1, dmax=20, k=128 * half),
            lambda s, T, half=half: (_m(T) & (T["qv"] == 128) & (T["raw"] == half - 0.5)).sum() > 100 and float(T["k"]) == 128 * half)
    add("NaN, +inf and -inf pixels", non_finite_pair(11, (36, 80), 5), params(dmin=1, dmax=20),
        lambda s, T: s["matched"] > 0 and np.isfinite(T["raw"]).all() and (finite_q(11, (36, 80), 5) != T["qv"] * _m(T)).sum() > 6)
    # every A on the rendered pair
    for A in (0, 1, 2, 3):
        add(f"rendered pair natural 188 x 620, A = {A}", rendered_pair("natural"), rendered_params(A),
            lambda s, T: s["matched"] > s["interior"] // 2 and s["rej_lr"] > 0 and s["rej_unique"] > 0)
    return out


@functools.lru_cache(maxsize=None)
def finite_q(seed, size, d):
    """The q frame of non_finite_pair's pair without its non-finite pixels."""
    return stereo_model(*shifted_pair(seed, size, d), params(dmin=1, dmax=20))[1]


def row_ids():
    return [r[0] for r in rows()]


@functools.lru_cache(maxsize=None)
def model_of(index, switch=None):
    """(depth, q, stats, details) of row `index` from the vectorised model (details only without a switch); read-only."""
    _, L, R, p, _ = rows()[index]
    res = stereo_model(L, R, p, details=switch is None, **({switch: True} if switch else {}))
    for a in res[:2]:
        a.setflags(write=False)
    return res


def loop_work(index):
    _, L, _, p, _ = rows()[index]
    return L.size * (p["dmax"] - p["dmin"] + 1) * (2 * p["A"] + 1) ** 2


def neighbour_decides_uniqueness(index):
    """True iff some interior pixel's uniqueness verdict turns when the winner's neighbours dl - 1 and dl + 1 are let into c2: worked
    out of the unswitched model's costs, not by running the switch."""
    p = rows()[index][3]
    T = model_of(index)[3]
    c0, c2 = T["c0"].astype(np.int64), T["c2"].astype(np.int64)
    c2n = np.minimum(c2, np.minimum(T["cm"], T["cp"]))
    verdict = lambda c: (c < BIG) & (c * (100 - p["uniq"]) > c0 * 100)
    return bool(((T["outcome"] > 0) & (verdict(c2) != verdict(c2n))).any())


# For each switch of the model, the rows that are in the table to notice it (test_stereo_depth_cpu.py holds the table to this): a list
# of names, or a function of the row's index.
_RENDERED = [f"rendered pair natural 188 x 620, A = {A}" for A in range(4)]
CAUGHT_BY = {
    # exact ties for the lead: a period apart (the winner is rejected either way, but the right image's winner moves and with it the
    # left-right verdicts), and between neighbouring candidates in flat tiles
    "largest_wins": ["right image of period 5", "right image of period 17", "integer disparity pair 96 x 320"] + _RENDERED,
    "exclude_winner_only": neighbour_decides_uniqueness,
    # a matched winner at dmax whose candidate dmax + 1 has a cost
    "subpixel_at_dmax": ["winner at dmax", "occluding step, lr_max -1", _RENDERED[0]],
    "half_away": ["k / q = 500.5", "k / q = 502.5"],
}
