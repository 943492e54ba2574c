"""Images and depth maps the pyramid kernels (P1 / P2: image_pyramid_fused_kernel and its wide build, blur3x3_kernel, pyrdown_kernel,
median3x3_kernel, decimate_odd_kernel, depth_pyramid_fused_kernel) are held to at their tile seams and edges
(tests/test_pyramid_cases_cpu.py, tests/test_gpu_pyramid_cases.py): the table of rows — each a kind (image / depth / median), a size, a
number of levels, a seeded numpy builder of its content and the cases it is in the table for, as names of predicates that are evaluated
on models alone (the replay of the fused kernel's index arithmetic, the launch geometry, the row's own input) and never on what the
oracle or the GPU returns. Nothing here imports the GPU library.

The launch constants (tile, halo widths, the 64 x 4 launch blocks, the tile count from which the wide build runs) are read out of
kernels.hip.h and odometry_hip.hip. replay_axis follows image_pyramid_fused_kernel_body line by line along one axis (the two axes are
independent: every index the kernel forms is a function of one coordinate).

Out of scope, on purpose: subnormal and NaN pixel values (the blur and pyrDown arithmetic of rows (a) - (e) neither overflows nor
reaches subnormals: magnitudes 2^-20 ... 2^20 through weights that sum to 1), and NaN or -0.0 in the median rows — a median is a
selection and its bits are defined only where the order of the nine values is: fminf / fmaxf and a comparison sort agree on every other
float, +-inf included, but not on which zero or which NaN they return. The batched tracker's pyramid (image_pyramid_batch_kernel) and
the trackers' internal pyramids have no accessor; they stay covered by the pose parity tests."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def constants():
    k = open(os.path.join(ROOT, "odometry_amd", "csrc", "kernels.hip.h")).read()
    h = open(os.path.join(ROOT, "odometry_amd", "csrc", "odometry_hip.hip")).read()
    out = {}
    for name in ("kPT", "kPIn", "kPInS", "kPL1", "kPL2", "kPyrThreads", "kPyrThreadsWide"):
        out[name] = int(re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, k).group(1))
    m = re.search(r"const int iy0 = kPT \* ty - (\d+), ix0 = kPT \* tx - (\d+);", k)
    assert m.group(1) == m.group(2)
    out["origin"] = -int(m.group(1))
    m = re.search(r"x1lo = max\(16 \* tx - (\d+), 0\);\s*const int y1hi = min\(16 \* ty \+ (\d+), R1 - 1\), x1hi = min\(16 \* tx \+ (\d+), C1 - 1\)", k)
    assert m.group(2) == m.group(3)
    out["l1lo"], out["l1hi"] = -int(m.group(1)), int(m.group(2))
    m = re.search(r"x2lo = max\(8 \* tx - (\d+), 0\);\s*const int y2hi = min\(8 \* ty \+ (\d+), R2 - 1\), x2hi = min\(8 \* tx \+ (\d+), C2 - 1\)", k)
    assert m.group(2) == m.group(3)
    out["l2lo"], out["l2hi"] = -int(m.group(1)), int(m.group(2))
    m = re.search(r"grid2d\(int cols, int rows, int z = 1\) \{ return dim3\(\(cols \+ (\d+)\) / (\d+), \(rows \+ (\d+)\) / (\d+), z\); \}", h)
    assert int(m.group(1)) == int(m.group(2)) - 1 and int(m.group(3)) == int(m.group(4)) - 1
    out["grid_x"], out["grid_y"] = int(m.group(2)), int(m.group(4))
    out["wide_from"] = int(re.search(r'getenv\("ODO_PYR_WIDE_FROM"\) \? atoi\(getenv\("ODO_PYR_WIDE_FROM"\)\) : (\d+);', h).group(1))
    out["fused_max_levels"] = int(re.search(r"if \(p->levels <= (\d+) && !unfused\)", h).group(1))
    out["max_levels"] = int(re.search(r"^#define\s+ODO_MAX_LEVELS_K\s+(\d+)", k, re.M).group(1))
    return out


K = constants()
PT = K["kPT"]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def level_dims(rows, cols, levels):
    return [(rows >> l, cols >> l) for l in range(levels)]


def legal(rows, cols, levels):
    """What pyr_alloc accepts: 1 ... max_levels levels, none of them empty."""
    return 1 <= levels <= K["max_levels"] and rows >> (levels - 1) >= 1 and cols >> (levels - 1) >= 1


def n_tiles(rows, cols):
    return -(-rows // PT) * -(-cols // PT)


# ---- the index arithmetic of both implementations --------------------------------------------------------------------------------
def reflect101(i, n, trips=None):
    """reflect101 of kernels.hip.h; trips (a list) receives how many times the loop ran."""
    k = 0
    if n != 1:
        while i < 0 or i >= n:
            i = -i if i < 0 else 2 * n - 2 - i
            k += 1
    else:
        i = 0
    if trips is not None:
        trips.append(k)
    return i


def reflect_index(n, lo, hi):
    """reflect101(i, n) for i = lo ... hi - 1 as an index array."""
    return np.array([reflect101(i, n) for i in range(lo, hi)], np.int64)


def replay_axis(n, levels, smooth=True, **mut):
    """image_pyramid_fused_kernel_body along one axis of n pixels: per tile the halo origin, lo / hi of levels 1 and 2 and every
    `reflect101(...) - origin` the kernel forms, checked against what the phase that filled that LDS array wrote. Returns (violations,
    facts): violations a list of strings (empty for the kernel as it is), facts what the predicates of the table look at. **mut replaces
    launch constants (the mutants of the CPU test)."""
    c = dict(K, **mut)
    pin, pl1, pl2, org = c["kPIn"], c["kPL1"], c["kPL2"], c["origin"]
    assert legal(n, n, levels) and levels <= c["fused_max_levels"]
    N = [n >> l for l in range(4)]
    tiles = -(-n // PT)
    bad = []
    own = [np.zeros(max(N[l], 0), np.int64) for l in range(levels)]
    facts = dict(tiles=tiles, last_tile_width=n - PT * (tiles - 1), n1=[], n2=[], l1_far_clipped=[], full_halo_tiles=[], max_trips=0,
                 input_unreflected=[])
    trips = []

    def inside(what, t, idx, width):
        if not 0 <= idx < width:
            bad.append(f"n={n} levels={levels} tile {t}: {what} index {idx} outside [0, {width})")

    for t in range(tiles):
        i0 = PT * t + org
        for j in range(pin):
            reflect101(i0 + j, N[0], trips)                  # always a pixel of the image: reflect101 returns 0 ... n - 1
        facts["input_unreflected"].append(i0 >= 0 and i0 + pin - 1 <= N[0] - 1)
        for x in range(PT * t, min(PT * t + PT, N[0])):      # level 0: the owned pixels, three taps when smoothing
            j = x - i0
            for d in ((-1, 0, 1) if smooth else (0,)):
                inside("level-0 tap, input halo", t, j + d, pin)
            own[0][x] += 1
        if levels < 2:
            continue
        lo1, hi1 = max(16 * t + c["l1lo"], 0), min(16 * t + c["l1hi"], N[1] - 1)
        n1 = hi1 - lo1 + 1
        facts["n1"].append(n1)
        if 16 * t + c["l1hi"] > N[1] - 1:
            facts["l1_far_clipped"].append(t)
        if not 1 <= n1 <= pl1:
            bad.append(f"n={n} levels={levels} tile {t}: level-1 halo of {n1} entries, kPL1 = {pl1}")
        for jx in range(n1):
            x1 = lo1 + jx
            for k in range(5):
                inside("level-1 tap, input halo", t, reflect101(2 * x1 - 2 + k, N[0], trips) - i0, pin)
            if 16 * t <= x1 < 16 * t + 16:
                own[1][x1] += 1
        if levels < 3:
            continue
        lo2, hi2 = max(8 * t + c["l2lo"], 0), min(8 * t + c["l2hi"], N[2] - 1)
        n2 = hi2 - lo2 + 1
        facts["n2"].append(n2)
        if not 1 <= n2 <= pl2:
            bad.append(f"n={n} levels={levels} tile {t}: level-2 halo of {n2} entries, kPL2 = {pl2}")
        if 0 < t < tiles - 1 and n1 == K["kPL1"] and n2 == K["kPL2"] and facts["input_unreflected"][t]:
            facts["full_halo_tiles"].append(t)
        for jx in range(n2):
            x2 = lo2 + jx
            for k in range(5):
                inside("level-2 tap, level-1 halo", t, reflect101(2 * x2 - 2 + k, N[1], trips) - lo1, min(n1, pl1))
            if 8 * t <= x2 < 8 * t + 8:
                own[2][x2] += 1
        if levels < 4:
            continue
        for jx in range(4):
            x3 = 4 * t + jx
            if x3 < N[3]:
                for k in range(5):
                    inside("level-3 tap, level-2 halo", t, reflect101(2 * x3 - 2 + k, N[2], trips) - lo2, min(n2, pl2))
                own[3][x3] += 1
    for l in range(levels):
        if not (own[l] == 1).all():
            bad.append(f"n={n} levels={levels}: level {l} pixels {np.flatnonzero(own[l] != 1)[:8].tolist()} are owned {own[l][own[l] != 1][:8].tolist()} times")
    facts["max_trips"] = max(trips)
    return bad, facts


def pyramid_trips(n, levels):
    """The largest number of trips reflect101 makes for a tap of the blur (level 0) or of a pyrDown (reading levels 0 ... levels - 2)
    along an axis of n pixels — the same in every implementation of the definition."""
    trips = []
    for x in (0, n - 1):
        reflect101(x - 1, n, trips)
        reflect101(x + 1, n, trips)
    for l in range(levels - 1):
        m = n >> l
        for x in range(m // 2):
            for k in range(5):
                reflect101(2 * x - 2 + k, m, trips)
    return max(trips)


# ---- models ----------------------------------------------------------------------------------------------------------------------
def integer_model(img, levels):
    """Levels 0 (smoothed), 1 and 2 of an image of integers 0 ... 255 as exact fractions, numerators in int64 with reflect-101 indices:
    blur = S / 16, level 1 = S / 256, level 2 = S / 65 536. Every float32 intermediate of either implementation is exact at these
    magnitudes (numerators below 2^24), so both must return exactly these values."""
    a = np.asarray(img).astype(np.int64)
    assert np.array_equal(a, img) and a.min() >= 0 and a.max() <= 255
    rows, cols = a.shape

    def blur_axis(v, n, axis):
        return 2 * v + np.take(v, reflect_index(n, -1, n - 1), axis) + np.take(v, reflect_index(n, 1, n + 1), axis)

    def down_axis(v, n, axis):
        out = 0
        for k, w in enumerate((1, 4, 6, 4, 1)):
            idx = np.array([reflect101(2 * x - 2 + k, n) for x in range(n // 2)], np.int64)
            out = out + w * np.take(v, idx, axis)
        return out

    out = [(blur_axis(blur_axis(a, cols, 1), rows, 0)).astype(np.float64) / 16.0]
    num, den = a, 1
    for l in range(1, min(levels, 3)):
        r, c = num.shape
        num, den = down_axis(down_axis(num, c, 1), r, 0), den * 256
        assert num.max(initial=0) < 2 ** 24
        out.append(num.astype(np.float64) / den)
    return [o.astype(f32) for o in out]


def np_blur(img):
    """The oracle's blur, step by step in float32: mid * 0.5 + (prev + next) * 0.25 along the rows, then along the columns."""
    s = np.asarray(img, f32)
    rows, cols = s.shape
    t = s * f32(0.5) + (s[:, reflect_index(cols, -1, cols - 1)] + s[:, reflect_index(cols, 1, cols + 1)]) * f32(0.25)
    return t * f32(0.5) + (t[reflect_index(rows, -1, rows - 1)] + t[reflect_index(rows, 1, rows + 1)]) * f32(0.25)


def np_pyrdown(img):
    """... its pyrDown: ((s2 * 6 + (s1 + s3) * 4) + s0) + s4 along the rows, the same along the columns, times 1 / 256."""
    s = np.asarray(img, f32)
    rows, cols = s.shape
    cx = [np.array([reflect101(2 * x - 2 + k, cols) for x in range(cols // 2)], np.int64) for k in range(5)]
    t = ((s[:, cx[2]] * f32(6) + (s[:, cx[1]] + s[:, cx[3]]) * f32(4)) + s[:, cx[0]]) + s[:, cx[4]]
    ry = [np.array([reflect101(2 * y - 2 + k, rows) for y in range(rows // 2)], np.int64) for k in range(5)]
    return (((t[ry[2]] * f32(6) + (t[ry[1]] + t[ry[3]]) * f32(4)) + t[ry[0]]) + t[ry[4]]) * (f32(1) / f32(256))


def np_median(img):
    """The nine replicated-border shifts, sorted, element 4."""
    s = np.asarray(img, f32)
    rows, cols = s.shape
    p = np.pad(s, 1, mode="edge")
    nine = np.stack([p[dy:dy + rows, dx:dx + cols] for dy in range(3) for dx in range(3)])
    return np.sort(nine, axis=0)[4]


def np_decimate(img):
    rows, cols = img.shape
    return np.ascontiguousarray(img[1::2, 1::2][:rows // 2, :cols // 2])


def np_pyramid(kind, img, levels, smooth):
    img = np.asarray(img, f32)
    if kind == "image":
        out, prev = [np_blur(img) if smooth else img.copy()], img
        for _ in range(1, levels):
            prev = np_pyrdown(prev)
            out.append(prev)
        return out
    out = [np_median(img) if smooth else img.copy()]
    for _ in range(1, levels):
        out.append(np_decimate(out[-1]))
    return out


def sorted_neighbourhoods(img):
    s = np.asarray(img, f32)
    rows, cols = s.shape
    p = np.pad(s, 1, mode="edge")
    return np.sort(np.stack([p[dy:dy + rows, dx:dx + cols] for dy in range(3) for dx in range(3)]), axis=0)


# ---- content ---------------------------------------------------------------------------------------------------------------------
def integers(rng, rows, cols):
    return rng.integers(0, 256, (rows, cols)).astype(f32)


def mantissa(rng, rows, cols):
    """Full-mantissa float32 in [0, 255)."""
    return np.minimum((rng.random((rows, cols)) * 255.0).astype(f32), np.nextafter(f32(255), f32(0)))


def signed(rng, rows, cols):
    """Either sign, magnitudes 2^-20 ... 2^20 with random mantissas."""
    v = np.exp2(rng.uniform(-20.0, 20.0, (rows, cols))) * rng.choice([-1.0, 1.0], (rows, cols))
    return np.clip(v, -2.0 ** 20, 2.0 ** 20).astype(f32)


def impulse(y, x):
    def build(rng, rows, cols):
        a = np.zeros((rows, cols), f32)
        a[y % rows, x % cols] = 255.0
        return a
    return build


def constant(rng, rows, cols):
    return np.full((rows, cols), 255, f32)


def holes(fraction):
    def build(rng, rows, cols):
        d = rng.uniform(0.1, 30.0, (rows, cols)).astype(f32)
        d[rng.random((rows, cols)) < fraction] = 0.0
        return d
    return build


def plateaus(rng, rows, cols):
    return rng.integers(1, 4, (rows, cols)).astype(f32) * f32(0.375)


ZERO_CLASSES = ((0, 0), (1, 1), (2, 2), (0, 2), (1, 0))      # residues (y % 3, x % 3): every 3 x 3 window holds each class once


def zero_classes(n_zero):
    def build(rng, rows, cols):
        """n_zero of the nine residue classes (y % 3, x % 3) are 0, the rest distinct positives: every neighbourhood that lies inside
        the image holds exactly n_zero zeros."""
        d = (rng.permutation(rows * cols).reshape(rows, cols) + 1).astype(f32) * f32(0.03125)
        yy, xx = np.mgrid[0:rows, 0:cols]
        for cy, cx in ZERO_CLASSES[:n_zero]:
            d[(yy % 3 == cy) & (xx % 3 == cx)] = 0.0
        return d
    return build


def negatives(rng, rows, cols):
    d = rng.integers(-6, 7, (rows, cols)).astype(f32) * f32(1.25)
    d[d == 0] = f32(0.0)                                       # +0.0 only
    return d


def infinities(rng, rows, cols):
    d = rng.uniform(-50.0, 50.0, (rows, cols)).astype(f32)
    u = rng.random((rows, cols))
    d[u < 0.3] = np.inf
    d[u > 0.7] = -np.inf
    d[d == 0] = f32(1.0)
    return d


def closed_four_zeros(img):
    """Four zeros and five distinct positives: the median (the fifth smallest) is the smallest positive. Interior pixels only."""
    a = np.where(img > 0, img, np.inf).astype(f32)
    rows, cols = a.shape
    return np.min(np.stack([a[dy:rows - 2 + dy, dx:cols - 2 + dx] for dy in range(3) for dx in range(3)]), axis=0)


def closed_five_zeros(img):
    return np.zeros((img.shape[0] - 2, img.shape[1] - 2), f32)


# ---- predicates: (row, image) -> bool, on models alone ---------------------------------------------------------------------------
def _axes(r):
    return {"rows": r["size"][0], "cols": r["size"][1]}


def _fused(r):
    return r["kind"] == "image" and r["levels"] <= K["fused_max_levels"]


def _facts(r, axis):
    return replay_axis(_axes(r)[axis], r["levels"])[1]


PREDICATES = {
    # "a tap reflects twice": reflect101 runs its loop twice for a tap of this row (an axis of two pixels read by a pyrDown)
    "reflects_twice": lambda r, img: max(pyramid_trips(n, r["levels"]) for n in r["size"]) >= 2,
    "one_pixel_level": lambda r, img: min(r["size"]) >> (r["levels"] - 1) == 1,        # reflect101(n == 1) applies if it is read
    "single_tile": lambda r, img: _fused(r) and n_tiles(*r["size"]) == 1,
    "several_tiles": lambda r, img: _fused(r) and n_tiles(*r["size"]) > 1,
    # "tile t's level-1 halo is clipped on the far side", t not the last tile of its axis
    "l1_far_clip_before_last": lambda r, img: _fused(r) and any(
        any(t < _facts(r, a)["tiles"] - 1 for t in _facts(r, a)["l1_far_clipped"]) for a in ("rows", "cols")),
    # "an interior tile with halos 25 / 11": input halo unreflected, level-1 and level-2 halos at full width, on either axis
    "interior_full_halo": lambda r, img: _fused(r) and r["levels"] >= 3 and any(_facts(r, a)["full_halo_tiles"] for a in ("rows", "cols")),
    "last_tile_one_row": lambda r, img: _fused(r) and r["size"][0] % PT == 1,
    "last_tile_one_col": lambda r, img: _fused(r) and r["size"][1] % PT == 1,
    "early_return": lambda r, img: _fused(r) and r["levels"] < 4,
    "level_by_level": lambda r, img: r["levels"] > K["fused_max_levels"],
    "wide": lambda r, img: _fused(r) and n_tiles(*r["size"]) >= K["wide_from"],                # ">= wide_from tiles"
    "just_below_wide": lambda r, img: _fused(r) and n_tiles(*r["size"]) == K["wide_from"] - 1,
    # the 64 x 4 launch blocks of the level-by-level kernels: a last block of one thread, a full one, one short of full
    "grid_edge": lambda r, img: any((c % K["grid_x"] in (0, 1, K["grid_x"] - 1)) and (rr % K["grid_y"] in (0, 1, K["grid_y"] - 1))
                                    for rr, c in level_dims(r["size"][0], r["size"][1], r["levels"])[:2]),
    "median_tied": lambda r, img: bool(((sorted_neighbourhoods(img)[4] == sorted_neighbourhoods(img)[3])
                                        | (sorted_neighbourhoods(img)[4] == sorted_neighbourhoods(img)[5])).mean() > 0.5),
    "four_zeros": lambda r, img: min(img.shape) < 3 or bool(((sorted_neighbourhoods(img) == 0).sum(0)[1:-1, 1:-1] == 4).all()),
    "five_zeros": lambda r, img: min(img.shape) < 3 or bool(((sorted_neighbourhoods(img) == 0).sum(0)[1:-1, 1:-1] == 5).all()),
    "has_negatives": lambda r, img: bool((img < 0).any()) and not np.signbit(img[img == 0]).any(),
    "has_infinities": lambda r, img: bool(np.isposinf(img).any() and np.isneginf(img).any()),
    "one_pixel_wide": lambda r, img: min(img.shape) == 1,
    "zeros_60": lambda r, img: img.size < 400 or 0.5 < (img == 0).mean() < 0.7,
    "zeros_90": lambda r, img: 0.85 < (img == 0).mean() < 0.95,
    "zeros_99": lambda r, img: 0.97 < (img == 0).mean() < 1.0,
    "integer": lambda r, img: bool(np.array_equal(img, np.floor(img)) and img.min() >= 0 and img.max() <= 255),
    "impulse": lambda r, img: int((img != 0).sum()) == 1 and img.max() == 255,
}


# ---- the table -------------------------------------------------------------------------------------------------------------------
SWEEP = list(range(8, 104))


def partner(s, mul, add):
    """The size paired with s: a fixed permutation of SWEEP, so each axis sees every size without a square-only table."""
    return SWEEP[((s - SWEEP[0]) * mul + add) % len(SWEEP)]


def sweep_cases(rows, cols):
    """The cases a sweep shape is in the table for, from the ranges the sweep was laid out by (not from the replay: the CPU test
    holds the two against each other)."""
    out = ["single_tile" if rows <= 32 and cols <= 32 else "several_tiles"]
    if min(rows, cols) <= 11:
        out.append("reflects_twice")
    if min(rows, cols) <= 15:
        out.append("one_pixel_level")
    if any(33 <= n <= 37 or 65 <= n <= 69 or 97 <= n <= 101 for n in (rows, cols)):      # a last tile of at most five pixels
        out.append("l1_far_clip_before_last")
    if max(rows, cols) >= 71:
        out.append("interior_full_halo")
    if rows % 32 == 1 and rows > 32:
        out.append("last_tile_one_row")
    if cols % 32 == 1 and cols > 32:
        out.append("last_tile_one_col")
    return out


def row(name, group, kind, size, levels, build, cases, seed=0, closed=None):
    assert legal(size[0], size[1], levels), name
    return dict(name=name, group=group, kind=kind, size=size, levels=levels, build=build, cases=tuple(cases), seed=seed, closed=closed)


def _table():
    t = []
    # every size 8 ... 103 on each axis at four levels, three times with three contents and three pairings
    for tag, build, mul, add, extra in (("b", mantissa, 37, 11, []), ("a", integers, 59, 5, ["integer"]), ("c", signed, 13, 50, [])):
        for s in SWEEP:
            size = (s, partner(s, mul, add))
            t.append(row(f"sweep-{tag}-{size[0]}x{size[1]}", f"sweep-{tag}", "image", size, 4, build, sweep_cases(*size) + extra, seed=s))
    # (d) one 255 on a zero image: the corners and the four pixels round the first tile corner
    for size in ((40, 72), (33, 65), (65, 33)):
        for y, x in ((0, 0), (-1, -1), (31, 31), (31, 32), (32, 31), (32, 32)):
            t.append(row(f"impulse-{size[0]}x{size[1]}-at-{y % size[0]}-{x % size[1]}", "impulse", "image", size, 4, impulse(y, x),
                         ["impulse", "integer", "several_tiles"]))
    # (e) a constant
    for size in ((8, 8), (33, 65), (72, 103), (50, 31)):
        t.append(row(f"constant-{size[0]}x{size[1]}", "constant", "image", size, 4, constant, ["integer"]))
    # one, two and three levels: the early returns
    for size in ((1, 1), (1, 9), (9, 1), (2, 2), (3, 2), (4, 5), (7, 7), (33, 65)):
        for levels in (1, 2, 3):
            if legal(size[0], size[1], levels):
                for tag, build, extra in (("a", integers, ["integer"]), ("b", mantissa, [])):
                    cases = ["early_return"] + extra
                    if min(size) >> (levels - 1) == 1:
                        cases.append("one_pixel_level")
                    if levels > 1 and any(n >> (levels - 2) == 2 for n in size):
                        cases.append("reflects_twice")
                    t.append(row(f"small-{tag}-{size[0]}x{size[1]}-l{levels}", "small", "image", size, levels, build, cases, seed=levels))
    # more levels than the fused kernel takes: 130 -> 1 and 257 -> 2 at eight
    for levels in (5, 8):
        for tag, build, extra in (("a", integers, ["integer"]), ("b", mantissa, []), ("c", signed, [])):
            t.append(row(f"deep-{tag}-130x257-l{levels}", "deep", "image", (130, 257), levels, build,
                         ["level_by_level"] + extra + (["one_pixel_level", "reflects_twice"] if levels == 8 else []), seed=levels))
    # the 64 x 4 launch blocks: level 0 (blur, median, the fused depth kernel) and level 1 (pyrDown, the decimation)
    for kind, build in (("image", mantissa), ("depth", holes(0.6))):
        for size in [(rr, c) for rr in (3, 4, 5) for c in (63, 64, 65)] + [(6, 127), (8, 128), (10, 130), (10, 127), (6, 130)]:
            t.append(row(f"grid-{kind}-{size[0]}x{size[1]}", f"grid-{kind}", kind, size, 2, build,
                         ["grid_edge"] + (["zeros_60"] if kind == "depth" else ["early_return"]), seed=size[1]))
    # the wide build's threshold on the default path: 31 x 33 = 1 023 tiles and 32 x 32 = 1 024
    t.append(row("threshold-below-992x1056", "threshold", "image", (992, 1056), 4, mantissa, ["just_below_wide", "interior_full_halo"]))
    t.append(row("threshold-at-1024x1024", "threshold", "image", (1024, 1024), 4, integers, ["wide", "integer", "interior_full_halo"]))
    # depth maps: 60 %, 90 % and 99 % exact zeros
    for s in SWEEP[::8] + [103]:
        size = (s, partner(s, 37, 11))
        for pct in (60, 90, 99):
            if pct == 60 or size[0] * size[1] >= 2000:
                t.append(row(f"depth-{pct}-{size[0]}x{size[1]}", "depth", "depth", size, 4, holes(pct / 100.0), [f"zeros_{pct}"], seed=s))
    for size in ((1, 1), (1, 9), (9, 1), (2, 2), (3, 2), (4, 5), (7, 7), (33, 65)):
        for levels in (1, 2, 3):
            if legal(size[0], size[1], levels):
                t.append(row(f"depth-small-{size[0]}x{size[1]}-l{levels}", "depth-small", "depth", size, levels, holes(0.6), ["zeros_60"],
                             seed=levels))
    for levels in (5, 8):
        for pct in (60, 90, 99):
            t.append(row(f"depth-deep-{pct}-130x257-l{levels}", "depth-deep", "depth", (130, 257), levels, holes(pct / 100.0),
                         [f"zeros_{pct}", "level_by_level"], seed=levels))
    # the median (DepthPyramid with smooth = true)
    med = (("plateaus", plateaus, ["median_tied"], None), ("four-zeros", zero_classes(4), ["four_zeros"], closed_four_zeros),
           ("five-zeros", zero_classes(5), ["five_zeros", "median_tied"], closed_five_zeros), ("negatives", negatives, ["has_negatives"], None),
           ("infinities", infinities, ["has_infinities"], None))
    for size, levels in (((1, 1), 1), ((2, 2), 2), ((1, 9), 1), ((9, 1), 1), ((1, 70), 1), ((70, 1), 1), ((5, 65), 2), ((13, 67), 3), ((64, 64), 4)):
        for tag, build, cases, closed in med:
            cases = list(cases) + (["one_pixel_wide"] if min(size) == 1 else [])
            if size == (1, 1):
                cases = [c for c in cases if c in ("one_pixel_wide",)]
            if tag == "infinities" and size[0] * size[1] < 9:
                continue
            if tag == "negatives" and size == (2, 2):
                continue
            t.append(row(f"median-{tag}-{size[0]}x{size[1]}", f"median-{tag}", "median", size, levels, build, cases, seed=size[0] + size[1],
                         closed=closed if min(size) >= 3 else None))
    return t


TABLE = _table()
BY_NAME = {r["name"]: r for r in TABLE}
assert len(BY_NAME) == len(TABLE)
GROUPS = sorted({r["group"] for r in TABLE})
SMOOTH = (True, False)


def group_rows(group):
    return [r for r in TABLE if r["group"] == group]


# ---- a row's image and oracle result, once per process ---------------------------------------------------------------------------
_images, _refs = {}, {}


def image(r):
    if r["name"] not in _images:
        a = r["build"](np.random.default_rng(r["seed"]), *r["size"])
        assert a.shape == tuple(r["size"]) and a.dtype == f32
        assert not np.isnan(a).any() and not np.signbit(a[a == 0]).any()
        a.setflags(write=False)
        _images[r["name"]] = a
    return _images[r["name"]]


def reference(r, smooth):
    """The oracle's levels of the row (read-only arrays)."""
    from oracle import oracle as O
    key = (r["name"], bool(smooth))
    if key not in _refs:
        if r["kind"] == "image":
            lv = O.image_pyramid(image(r), r["levels"], smooth)
        else:
            lv = O.depth_pyramid(image(r), r["levels"], smooth=smooth)
        lv = [np.array(a) for a in lv]
        for a in lv:
            a.setflags(write=False)
        _refs[key] = lv
    return _refs[key]


def key(r, smooth, level):
    """Name of a level in the .npz a child process writes."""
    return f"{r['name']}|{int(bool(smooth))}|{level}"
