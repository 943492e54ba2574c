"""Stereo pairs the depth estimator's selection and scan kernels are held to on ties and edges (tests/test_depth_cases_cpu.py,
tests/test_gpu_depth_cases.py): the table of rows — each a seeded numpy builder, an image size, the estimator's parameters, the counts
that show how often the pair reaches the branch it is in the table for (a predicate on the ORACLE's outputs, with the floor the test
holds it to and the count measured when the row was written), and, where one exists, a closed form of the answer that does not come
from the oracle. Nothing here imports the GPU library.

The launch constants (selection cap, threads of the selection workgroup, its key bound) are read out of kernels.hip.h; the replay of
which of the scan's three loops handles a candidate column (scan_path) follows depth_disparity_kernel_body line by line. A row's pair,
its oracle result and its analysis are computed once per process."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
WAVE = 64


def constants():
    src = open(os.path.join(ROOT, "odometry_amd", "csrc", "kernels.hip.h")).read()
    out = {m.group(1): int(m.group(2)) for m in re.finditer(r"^constexpr\s+int\s+(kSel\w+)\s*=\s*(\d+)\s*;", src, re.M)}
    out["kSelThreads"] = int(re.search(r"^#define\s+ODO_SEL_THREADS\s+(\d+)", src, re.M).group(1))
    out["scan_unroll"] = int(re.search(r"^#define\s+ODO_SCAN_UNROLL\s+(\d+)", src, re.M).group(1))
    return out


K = constants()
CAP, CHUNK, MAX_KEYS = K["kSelCap"], K["kSelThreads"], K["kSelMaxElems"]
MAIN_TRIP = 4 * WAVE                     # candidates per trip of the scan's first loop (four per lane)
PAIR_TRIP = K["scan_unroll"] * WAVE      # ... of its second loop


def tile_dims(rows, cols, bnd):
    return (cols - 2 * bnd) // 32, (rows - 2 * bnd) // 16


def size_for(bw, bh, bnd=4, extra=(0, 0)):
    """(rows, cols) whose selection tiles are bw x bh; extra = (rows, cols) left over behind the last tile."""
    return 16 * bh + 2 * bnd + extra[0], 32 * bw + 2 * bnd + extra[1]


def scan_lo(x, bnd, max_disparity):
    lo = np.full_like(x, bnd)
    if max_disparity > 0:
        lo = np.maximum(lo, x - max_disparity)
    return lo


def scan_path(n_cand, off):
    """Which loop of depth_disparity_kernel_body evaluates candidate lo + off of a point with n_cand = x - lo candidates:
    ("main", trip, lane, u) — the 256-per-trip loop, candidate u of the lane's four;
    ("pair", trip, lane, u) — the loop of ODO_SCAN_UNROLL candidates per lane and trip; ("single", trip, lane, 0) — the last loop."""
    assert 0 <= off < n_cand
    n_main = n_cand // MAIN_TRIP
    if off < n_main * MAIN_TRIP:
        return ("main", off // MAIN_TRIP, (off % MAIN_TRIP) // 4, off % 4)
    rest, o = n_cand - n_main * MAIN_TRIP, off - n_main * MAIN_TRIP
    lane, rx, trip = o % WAVE, o % WAVE, 0
    while rx + (PAIR_TRIP - WAVE) < rest:                    # for (; rx + (UNROLL - 1) * 64 < x; rx += UNROLL * 64)
        if rx <= o < rx + PAIR_TRIP:
            return ("pair", trip, lane, (o - rx) // WAVE)
        rx += PAIR_TRIP
        trip += 1
    return ("single", (o - rx) // WAVE, lane, 0)


def mag_image(Lb):
    """|grad| of the blurred left image as DisparityDepthEstimate forms it: float32, one rounding per operation."""
    Lb = np.asarray(Lb, f32)
    g = np.zeros_like(Lb)
    gx = f32(0.5) * (Lb[1:-1, 2:] - Lb[1:-1, :-2])
    gy = f32(0.5) * (Lb[2:, 1:-1] - Lb[:-2, 1:-1])
    g[1:-1, 1:-1] = np.sqrt(gx * gx + gy * gy)
    return g


def ssd_candidates(Lb, Rb, x, y, lo):
    """The 8-tap SSD of every candidate column lo .. x - 1 of point (x, y) in float32 with the reference's adder tree."""
    taps = ((0, 2), (-1, 1), (2, 0), (0, 0), (-2, 0), (1, -1), (-1, -1), (0, -2))     # (dx, dy) in lane order
    c = np.arange(lo, x)
    s = []
    for dx, dy in taps:
        d = Lb[y + dy, x + dx] - Rb[y + dy, c + dx]
        s.append(d * d)
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))


# ---- builders -------------------------------------------------------------------------------------------------------------------
def quantised(levels, step, shift=5):
    def build(rng, rows, cols):
        L = (rng.integers(0, levels, (rows, cols)) * step).astype(f32)
        return L, np.roll(L, -shift, axis=1)
    return build


def ramp_noise(rng, rows, cols):
    """A plane plus noise of a few thousandths of a grey level: the magnitudes of a tile cluster inside a few hundred float32 steps."""
    yy, xx = np.mgrid[0:rows, 0:cols]
    L = (0.5 * xx + 0.25 * yy + rng.integers(-8, 9, (rows, cols)) / 4096.0).astype(f32)
    return L, np.roll(L, -3, axis=1)


def flat_and_textured(bnd=4):
    def build(rng, rows, cols):
        """Tiles of a checkerboard are flat (every magnitude of the tile 0: the texture of their neighbours keeps three pixels away
        from them) or textured."""
        bw, bh = tile_dims(rows, cols, bnd)
        L = np.full((rows, cols), 64, f32)
        for b in range(512):
            ty, tx = b // 32, b % 32
            if (ty + tx) % 2:
                sy, sx = bnd + ty * bh, bnd + tx * bw
                L[sy + 3:sy + bh - 3, sx + 3:sx + bw - 3] = rng.integers(0, 256, (bh - 6, bw - 6))
        return L, np.roll(L, -2, axis=1)
    return build


def bumps(rng, rows, cols):
    """Single pixels of 160 grey levels on a flat image: each puts exactly four magnitudes of 20 (its four neighbours) over a
    threshold of 16 and nothing else (the next largest is 14.1; pixels four apart cancel each other's gradients on the line between
    them), and fewer than half of a tile's magnitudes are non-zero, so its median is 0. A tile's count over the threshold is four
    per pixel inside it, three for one in its first column, one for one just outside. Only tiles of even tile columns carry a
    design; design k (of CAP_DESIGNS) goes to every tile with (tile row * 16 + tile column / 2) % len == k."""
    bnd = 4
    bw, bh = tile_dims(rows, cols, bnd)
    assert bw >= 24 and bh >= 32
    L = np.zeros((rows, cols), f32)
    for ty in range(16):
        for tc in range(16):
            sy, sx = bnd + ty * bh, bnd + 2 * tc * bw
            n, r0, edge_first, step = CAP_DESIGNS[(ty * 16 + tc) % len(CAP_DESIGNS)]
            rws = list(range(r0, bh - 1, step))
            rem = n % 4
            if rem:   # the odd remainder on a raster row of its own: in front of the others or right behind them
                er = rws.pop(0 if edge_first else -(-(n // 4) // 5))
                for lx in {1: (-1,), 2: (-1, bw), 3: (0,)}[rem]:
                    L[sy + er, sx + lx] = 160.0
            left = n // 4
            for r in rws:
                for lx in (2, 6, 10, 14, 18):
                    if left:
                        L[sy + r, sx + lx] = 160.0
                        left -= 1
            assert left == 0, (n, r0)
    return L, np.roll(L, -7, axis=1)


# (pixels over the threshold, raster row of the first single pixel, whether the odd remainder's row comes first, rows between pixels)
CAP_DESIGNS = [(79, 2, False, 4), (80, 2, False, 4), (81, 2, False, 4), (82, 1, True, 4), (83, 3, False, 5), (84, 2, False, 4),
               (96, 2, False, 5), (79, 4, True, 4), (81, 1, True, 5), (40, 23, False, 4), (75, 2, False, 4), (78, 3, True, 4),
               (80, 10, False, 4), (19, 24, True, 4), (100, 1, False, 4), (81, 3, False, 4), (77, 2, False, 5), (81, 9, True, 4),
               (88, 8, False, 4)]


def all_tie(rng, rows, cols):
    return rng.integers(0, 256, (rows, cols)).astype(f32), np.full((rows, cols), 128, f32)


def periodic(p, d):
    def build(rng, rows, cols):
        base = rng.integers(0, 256, (rows, p)).astype(f32)
        xx = np.arange(cols)
        return base[:, (xx - d) % p].copy(), base[:, xx % p].copy()
    return build


TRIP_BANDS = (1, 1, 2, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 260, 300, 511)


def trip_bands(rng, rows, cols):
    """Tile row k (a band of rows) is the right image moved by TRIP_BANDS[k] columns; what the move uncovers is fresh noise."""
    bw, bh = tile_dims(rows, cols, 4)
    R = rng.integers(0, 256, (rows, cols)).astype(f32)
    L = rng.integers(0, 256, (rows, cols)).astype(f32)
    for k, d in enumerate(TRIP_BANDS):
        y0, y1 = (0 if k == 0 else 4 + k * bh), (rows if k == 15 else 4 + (k + 1) * bh)
        L[y0:y1, d:] = R[y0:y1, :cols - d]
    return L, R


def integer_noise(rng, rows, cols):
    """Integer grey levels, the left image the right one moved by 6 columns plus noise of -2 .. 2: every blurred value is a multiple
    of 1/16 and every SSD a multiple of 1/256, so many points share their best SSD exactly."""
    R = (rng.integers(0, 64, (rows, cols)) * 4).astype(f32)
    L = np.roll(R, 6, axis=1) + rng.integers(-2, 3, (rows, cols)).astype(f32)
    return L.astype(f32), R


def huge_amplitudes(rng, rows, cols):
    L = (2.0e5 + 1.0e3 * rng.integers(0, 256, (rows, cols))).astype(f32)
    R = (1.0e3 * rng.integers(0, 256, (rows, cols))).astype(f32)
    return L, R


def textured_pair(shift):
    def build(rng, rows, cols):
        R = rng.integers(0, 256, (rows, cols)).astype(f32)
        return np.roll(R, shift, axis=1), R
    return build


# ---- the table ------------------------------------------------------------------------------------------------------------------
def row(name, group, size, build, floors, grad_th=8.0, ssd_th=900.0, boundary=4, max_disparity=0, closed=None, why="", seed=0, **kw):
    """floors: {count name: (floor the CPU test holds the count to, count measured with the oracle when the row was written — the
    smallest of them where a loop writes several rows)}. A floor of (0, 0) says that the row cannot reach that branch."""
    return dict(name=name, group=group, size=size, build=build, floors=floors, closed=closed, why=why, seed=seed,
                params=dict(grad_th=grad_th, ssd_th=ssd_th, boundary=boundary, max_disparity=max_disparity, any_size=1), **kw)


def _with_md(rows_):
    """Each row at max_disparity 0 (the reference's range) and 128."""
    out = []
    for r in rows_:
        for md in (0, 128):
            out.append(dict(r, name=f"{r['name']}-md{md}", params=dict(r["params"], max_disparity=md),
                            floors=r["floors"] if md == 0 else r.get("floors_md128", r["floors"])))
    return out


# closed forms: (analysis of the row, outputs dict(val, disp, dep, n_selected, n_matched)) -> raises AssertionError
def closed_all_tie(A, out):
    """Every candidate has the same SSD: the first one (lo) wins, disp = x - lo; a point at x == lo has no candidate."""
    ys, xs = np.nonzero(out["val"])
    lo = scan_lo(xs, A["bnd"], A["params"]["max_disparity"])
    assert np.array_equal(out["disp"][ys, xs], (xs - lo).astype(f32))
    assert out["n_matched"] == int((xs > lo).sum()) and out["n_selected"] == len(xs)
    assert (xs == lo).sum() > 0 and not out["dep"][ys, xs][xs == lo].any()


def closed_periodic(p):
    def check(A, out):
        """The right image has period p along the scan: a column at or behind lo + p repeats the SSD of the one p in front of it and
        cannot be the first minimum; a point with a whole period of candidates finds its own eight taps, SSD 0."""
        ys, xs = np.nonzero(out["val"])
        lo = scan_lo(xs, A["bnd"], A["params"]["max_disparity"])
        disp = out["disp"][ys, xs]
        full = xs - lo >= p
        assert (disp[full] > 0).all(), "a point with a whole period of candidates is unmatched"
        m = disp > 0
        col = xs[m] - disp[m].astype(np.int64)
        assert ((col >= lo[m]) & (col < lo[m] + p)).all()
    return check


def closed_flat(neg):
    def check(A, out):
        """A flat tile's magnitudes are all 0 = its median: with grad_th = 0 nothing is strictly above, with a negative grad_th every
        pixel is and the first 80 in raster order are taken."""
        rows, cols = A["size"]
        bw, bh = tile_dims(rows, cols, A["bnd"])
        want = np.zeros(bw * bh, np.uint8)
        if neg:
            want[:CAP] = 1
        n = 0
        for b in range(512):
            ty, tx = b // 32, b % 32
            if (ty + tx) % 2 == 0:
                sy, sx = A["bnd"] + ty * bh, A["bnd"] + tx * bw
                assert np.array_equal(out["val"][sy:sy + bh, sx:sx + bw].ravel(), want), f"flat tile {b}"
                n += 1
        assert n == 256
    return check


def closed_bumps(A, out):
    """Tiles of even tile columns hold min(n, 80) selected pixels, n the design's count (builder `bumps`)."""
    rows, cols = A["size"]
    bw, bh = tile_dims(rows, cols, 4)
    for ty in range(16):
        for tc in range(16):
            sy, sx = 4 + ty * bh, 4 + 2 * tc * bw
            n = CAP_DESIGNS[(ty * 16 + tc) % len(CAP_DESIGNS)][0]
            assert int(out["val"][sy:sy + bh, sx:sx + bw].sum()) == min(n, CAP), (ty, tc, n)


def closed_nothing_matched(A, out):
    assert out["n_selected"] == int(out["val"].sum()) > 0 and out["n_matched"] == 0
    assert not out["disp"].any() and not out["dep"].any()


def closed_generic(A, out):
    """Holds on every row: disp and dep are zero off the mask, disp is a whole number of columns inside the point's range, and dep is
    the one float32 division disp / (f0 * baseline)."""
    from oracle import oracle as O
    val, disp, dep = out["val"], out["disp"], out["dep"]
    assert not disp[val == 0].any() and not dep[val == 0].any()
    ys, xs = np.nonzero(val)
    d = disp[ys, xs]
    assert np.array_equal(d, np.floor(d)) and (d >= 0).all() and (d <= xs - scan_lo(xs, A["bnd"], A["params"]["max_disparity"])).all()
    assert np.array_equal(dep[ys, xs], d / f32(f32(718.856) * f32(O.KITTI_BASELINE)))
    assert out["n_selected"] == len(xs) and out["n_matched"] == int((d > 0).sum())


Q3 = quantised(3, 18, shift=9)
SELECTION = [
    row("tied-median-2-levels", "tied-median", size_for(10, 7), quantised(2, 32), dict(tiles_tied=(400, 483), tiles_inside_run=(150, 209)),
        grad_th=0.0, why="two grey levels: a handful of distinct magnitudes per tile"),
    row("tied-median-3-levels", "tied-median", size_for(10, 7), quantised(3, 16), dict(tiles_tied=(300, 359), tiles_inside_run=(50, 80)),
        grad_th=0.0),
    row("tied-median-5-levels", "tied-median", size_for(10, 7), quantised(5, 8), dict(tiles_tied=(150, 185), tiles_inside_run=(10, 18)),
        grad_th=0.0),
    row("radix-pass", "radix-pass", size_for(38, 23, extra=(0, 17)), ramp_noise,
        dict(tiles_share8=(512, 512), tiles_share16=(512, 512), tiles_share24=(512, 512)), grad_th=0.0,
        why="KITTI's size; the fourth pass of the radix select decides"),
    row("flat-and-textured", "flat-and-textured", size_for(10, 9), flat_and_textured(), dict(tiles_flat=(256, 256), tiles_flat_empty=(256, 256)),
        grad_th=0.0, closed=closed_flat(False)),
    row("flat-and-textured-negative", "flat-and-textured", size_for(10, 9), flat_and_textured(),
        dict(tiles_flat=(256, 256), tiles_flat_capped=(256, 256)), grad_th=-1.0, closed=closed_flat(True),
        why="grad_th < 0: every pixel of a flat tile is above its threshold, 90 of them, 80 taken"),
    row("on-threshold", "on-threshold", size_for(10, 7), quantised(2, 32), dict(on_threshold=(32, 181), on_threshold_selected=(0, 0)),
        grad_th=1.0, why="magnitudes and medians are exact: pixels with mag == median + 1 exist and none may be selected"),
    row("cap", "cap", size_for(24, 32), bumps,
        dict(tiles_79=(20, 28), tiles_80=(20, 27), tiles_81=(40, 54), tiles_first_in_later_chunk=(40, 50), tiles_cap_in_later_chunk=(40, 53),
             tiles_80_81_same_wave=(40, 55), tiles_80_81_other_wave=(60, 81)), grad_th=16.0, closed=closed_bumps,
        why="tiles of 768 keys (two chunks of 512), counts around the cap by design"),
]
TILE_SIZES = [
    row(f"tiles-{bw * bh}-keys", "tile-size", size_for(bw, bh), Q3, dict(tiles_tied=(512, 512), chunks=(ch, ch)), grad_th=0.0,
        why=f"{bw}x{bh} tiles, {ch} chunk(s) of 512 keys, three grey levels")
    for bw, bh, ch in ((32, 16, 1), (27, 19, 2), (32, 32, 2), (41, 25, 3), (64, 64, 8))
]
SCAN = _with_md([
    row("all-tie", "all-tie", size_for(10, 7, extra=(0, 12)), all_tie, dict(points_without_candidates=(20, 25), points_all_tied=(8000, 8765)),
        ssd_th=1.0e9, closed=closed_all_tie, why="constant right image: every candidate of every point has the same SSD"),
] + [
    row(f"periodic-p{p}-d{d}", "periodic", size_for(bw, 7, extra=(0, 12)), periodic(p, d), dict(points_tied_one_period_on=fl, **{tag: fl}),
        floors_md128=dict(points_tied_one_period_on=fl if p <= 64 else (0, 0), **{tag128: fl if p <= 64 else (0, 0)}), closed=closed_periodic(p), period=p,
        why=why)
    for p, bw, fl, tag, tag128, why in (
        (5, 10, (6000, 7111), "tied_other_lane", "tied_other_lane", "ties in different lanes"),
        (16, 10, (6000, 6351), "tied_other_row_of_16", "tied_other_row_of_16", "ties in different rows of 16 lanes"),
        (64, 10, (5000, 5113), "tied_same_lane_last_loops", "tied_same_lane_last_loops", "ties in the same lane of the last loops"),
        (256, 24, (7000, 7306), "tied_same_lane_main_loop", "tied_same_lane_main_loop",
         "ties in the same lane of the first loop, a trip apart (+-128 px: no candidate a period on, the count is 0)"))
    for d in (3, 11)
]) + [
    row("trip-edges", "trip-edges", size_for(17, 10, extra=(0, 8)), trip_bands,
        dict(min_on_first=(40, 40), min_on_last=(40, 40), min_on_last_of_main_trip=(40, 40), min_on_first_of_next_main_trip=(5, 10),
             min_in_pair_loop=(40, 40), min_in_single_loop=(40, 40), trip_edge_lengths=(16, 16)), grad_th=0.0,
        why="a disparity per band of rows: the unique minimum lands on every edge of the three loops"),
    row("on-ssd-threshold", "on-ssd-threshold", size_for(10, 7, extra=(0, 12)), integer_noise,
        dict(best_on_threshold=(1, 10), best_next_above=(1, 6)), ssd_th="median of the oracle's best SSDs",
        why="ssd_th is the best SSD of a point: equality is a hit, the next larger value a miss"),
    row("never-below-start", "never-below-start", size_for(10, 7, extra=(0, 12)), huge_amplitudes, dict(best_at_start=(17000, 17401)),
        closed=closed_nothing_matched, why="every SSD is above the 1e10 the minimum starts at"),
] + [
    row(f"tap-edges-b{b}-c{c}", "tap-edges", size_for(10, 6, bnd=b, extra=(0, c)), textured_pair(40),
        dict(points_top_row=(100, 140), points_first_column=(30, 40), points_scanned_from_lo=(14000, 14791), points_bottom_row=(100, 140),
             points_last_column=(30, 40) if c == 0 else (0, 0), points_main_loop=(2500, 2959)), grad_th=0.0, boundary=b,
        why=f"boundary {b}, cols % 4 == {c}" + ("" if c else ", tiles reach the last legal row and column"))
    for b in (2, 4) for c in (0, 1, 2, 3)
]
TABLE = SELECTION + TILE_SIZES + SCAN
BY_NAME = {r["name"]: r for r in TABLE}
assert len(BY_NAME) == len(TABLE)
# what the started-ahead / prepared test and the batched test run (tests/test_gpu_depth_cases.py)
AHEAD_ROWS = ("all-tie-md0", "cap")
BATCH = dict(rows=("periodic-p16-d3-md0", "tied-median-3-levels"), size=size_for(10, 7, extra=(0, 12)), levels=3,
             params=dict(grad_th=0.0, ssd_th=900.0, boundary=4, max_disparity=0, min_depth=1.0e-3, max_depth=1.0e4, photo_th=15.0))


BATCH_BASELINE = 0.537


def batch_intrinsics():
    rows, cols = BATCH["size"]
    return (718.856 * cols / 1241.0, (cols - 1) / 2.0, (rows - 1) / 2.0)


def batch_oracle_params():
    return dict(BATCH["params"], f0=batch_intrinsics()[0], baseline=BATCH_BASELINE)


def batch_tracker_args():
    """Keyword overrides of api.Tracker / api.TrackerBatch for the batched rows."""
    rows, cols = BATCH["size"]
    return dict(BATCH["params"], rows=rows, cols=cols, levels=BATCH["levels"], lm_max_iters=(10, 20, 30), K=batch_intrinsics(), any_size=1,
                baseline=BATCH_BASELINE)


# ---- a row's pair, oracle result and analysis, once per process -----------------------------------------------------------------
_pairs, _refs, _analyses = {}, {}, {}


def pair(r, size=None):
    key = (r["name"], size)
    if key not in _pairs:
        rows, cols = size or r["size"]
        L, R = r["build"](np.random.default_rng(r["seed"]), rows, cols)
        assert L.shape == R.shape == (rows, cols) and L.dtype == R.dtype == f32
        L.setflags(write=False)
        R.setflags(write=False)
        _pairs[key] = (L, R)
    return _pairs[key]


def resolve(r):
    """The row's parameters as numbers: the on-ssd-threshold row takes its ssd_th from the oracle's scan of its own pair — the median
    of the selected points' best SSDs, an exact float32."""
    from oracle import oracle as O
    prm = dict(r["params"])
    if isinstance(prm["ssd_th"], str):
        L, R = pair(r)
        first = O.compute_depth(L, R, O.depth_params(**dict(prm, ssd_th=1.0e9)), stage=1)
        s = O.disparity_scan(O.blur3x3(L), O.blur3x3(R), first["val"], boundary=prm["boundary"], ssd_th=1.0e9,
                             max_disparity=prm["max_disparity"])
        ys, xs = np.nonzero(first["val"])
        best = np.sort(s["best_ssd"][ys, xs][xs > prm["boundary"]])
        prm["ssd_th"] = float(best[len(best) // 2])
    return prm


def reference(r):
    """(L, R, resolved parameters, the oracle's stage-1 result) of the row."""
    from oracle import oracle as O
    if r["name"] not in _refs:
        L, R = pair(r)
        prm = resolve(r)
        _refs[r["name"]] = (L, R, prm, O.compute_depth(L, R, O.depth_params(**prm), stage=1))
    return _refs[r["name"]]


def outputs_of(ref):
    return {k: ref[k] for k in ("val", "disp", "dep", "n_selected", "n_matched")}


def analysis(r):
    """Everything the predicates and closed forms look at: the pair, the oracle's mask / disparities / best SSD and column per
    point, the blurred images, the magnitude image and every tile's sorted keys."""
    from oracle import oracle as O
    if r["name"] in _analyses:
        return _analyses[r["name"]]
    L, R, prm, ref = reference(r)
    rows, cols = L.shape
    bnd = prm["boundary"]
    Lb, Rb = O.blur3x3(L), O.blur3x3(R)
    scan = O.disparity_scan(Lb, Rb, ref["val"], boundary=bnd, ssd_th=prm["ssd_th"], max_disparity=prm["max_disparity"])
    assert np.array_equal(scan["disp"], ref["disp"]) and scan["n_matched"] == ref["n_matched"]
    A = dict(row=r, size=(rows, cols), bnd=bnd, params=prm, L=L, R=R, Lb=Lb, Rb=Rb, ref=ref, scan=scan, mag=mag_image(Lb))
    _analyses[r["name"]] = A
    return A


def tiles(A):
    """Per selection tile: origin, magnitudes in raster order, the sorted keys, the median (rank bsz / 2) and the threshold."""
    rows, cols = A["size"]
    bnd = A["bnd"]
    bw, bh = tile_dims(rows, cols, bnd)
    gth = f32(A["params"]["grad_th"])
    for b in range(512):
        sy, sx = bnd + (b // 32) * bh, bnd + (b % 32) * bw
        m = A["mag"][sy:sy + bh, sx:sx + bw].ravel()
        s = np.sort(m)
        med = s[(bw * bh) // 2]
        yield dict(b=b, sy=sy, sx=sx, bw=bw, bh=bh, mag=m, sorted=s, median=med, th=f32(med + gth))


def selection_counts(A):
    """How many tiles (or pixels) of the row reach each branch of depth_select_kernel_body."""
    c = dict.fromkeys(("tiles_tied", "tiles_inside_run", "tiles_share8", "tiles_share16", "tiles_share24", "tiles_flat",
                       "tiles_flat_empty", "tiles_flat_capped", "on_threshold", "on_threshold_selected", "tiles_79", "tiles_80",
                       "tiles_81", "tiles_over_cap", "tiles_first_in_later_chunk", "tiles_cap_in_later_chunk",
                       "tiles_80_81_same_wave", "tiles_80_81_other_wave"), 0)
    sub = np.zeros((4, 4), np.int64)        # [pass, chosen digit % 4]
    val = A["ref"]["val"]
    for t in tiles(A):
        bsz, k = t["bw"] * t["bh"], (t["bw"] * t["bh"]) // 2
        s, med = t["sorted"], t["median"]
        first, last = np.searchsorted(s, med, "left"), np.searchsorted(s, med, "right") - 1
        c["tiles_tied"] += last > first
        c["tiles_inside_run"] += first < k < last
        bits, mb = s.view(np.uint32), int(np.asarray(med).view(np.uint32))
        other = bits != mb
        for n in (8, 16, 24):
            c[f"tiles_share{n}"] += bool((other & ((bits >> (32 - n)) == (mb >> (32 - n)))).any())
        for p in range(4):
            sub[p, ((mb >> (24 - 8 * p)) & 255) % 4] += 1
        picked = val[t["sy"]:t["sy"] + t["bh"], t["sx"]:t["sx"] + t["bw"]].ravel()
        if s[0] == s[-1]:
            c["tiles_flat"] += 1
            c["tiles_flat_empty"] += not picked.any()
            c["tiles_flat_capped"] += bsz > CAP and int(picked.sum()) == CAP and bool(picked[:CAP].all())
        on = t["mag"] == t["th"]
        c["on_threshold"] += int(on.sum())
        c["on_threshold_selected"] += int(picked[on].sum())
        idx = np.flatnonzero(t["mag"] > t["th"])
        n = len(idx)
        c["tiles_79"] += n == CAP - 1
        c["tiles_80"] += n == CAP
        c["tiles_81"] += n == CAP + 1
        c["tiles_over_cap"] += n > CAP
        if n:
            c["tiles_first_in_later_chunk"] += idx[0] >= CHUNK
        if n >= CAP:
            c["tiles_cap_in_later_chunk"] += idx[CAP - 1] // CHUNK > idx[0] // CHUNK
        if n > CAP:
            same = idx[CAP - 1] // WAVE == idx[CAP] // WAVE
            c["tiles_80_81_same_wave"] += same
            c["tiles_80_81_other_wave"] += not same
    c = {k: int(v) for k, v in c.items()}
    c["chunks"] = -(-(t["bw"] * t["bh"]) // CHUNK)
    c["keys"] = t["bw"] * t["bh"]
    for p in range(4):
        for q in range(4):
            c[f"pass{p}_bin{q}"] = int(sub[p, q])
    return c


TRIP_EDGE_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513)


def scan_counts(A, unique_limit=40):
    """How many selected points of the row reach each branch of depth_disparity_kernel_body."""
    from oracle import oracle as O
    rows, cols = A["size"]
    bnd, prm, scan = A["bnd"], A["params"], A["scan"]
    ys, xs = np.nonzero(A["ref"]["val"])
    lo = scan_lo(xs, bnd, prm["max_disparity"])
    best, col = scan["best_ssd"][ys, xs], scan["best_col"][ys, xs]
    n_cand = xs - lo
    hit = ~(best > f32(prm["ssd_th"]))
    c = dict(points=len(xs), points_without_candidates=int((n_cand == 0).sum()), matched=int((hit & (n_cand > 0)).sum()),
             best_at_start=int((best == f32(1e10)).sum()),
             trip_edge_lengths=len(set(TRIP_EDGE_LENGTHS) & set(n_cand.tolist())),
             points_top_row=int((ys == bnd).sum()), points_bottom_row=int((ys == rows - bnd - 1).sum()),
             points_first_column=int((xs == bnd).sum()), points_last_column=int((xs == cols - bnd - 1).sum()),
             points_scanned_from_lo=int(((lo == bnd) & (n_cand > 0)).sum()), points_main_loop=int((n_cand >= MAIN_TRIP).sum()))
    # equality with the threshold, and the next value above it
    c["best_on_threshold"] = int((best == f32(prm["ssd_th"])).sum())
    above = best[best > f32(prm["ssd_th"])]
    c["best_next_above"] = int((best == above.min()).sum()) if len(above) else 0
    # ties: every candidate (all-tie), or one period further on
    c["points_all_tied"] = 0
    if A["row"]["group"] == "all-tie":
        c["points_all_tied"] = sum(1 for i in np.flatnonzero(n_cand > 1)
                                   if np.ptp(ssd_candidates(A["Lb"], A["Rb"], xs[i], ys[i], lo[i])) == 0)
    p = A["row"].get("period")
    tied = dict.fromkeys(("points_tied_one_period_on", "tied_other_lane", "tied_other_row_of_16", "tied_same_lane_last_loops",
                          "tied_same_lane_main_loop"), 0)
    if p:
        Lb, Rb = A["Lb"], A["Rb"]
        for i in np.flatnonzero(hit & (col >= 0) & (col + p < xs)):
            x, y = int(xs[i]), int(ys[i])
            Lp = [Lb[y + 2, x], Lb[y + 1, x - 1], Lb[y, x + 2], Lb[y, x], Lb[y, x - 2], Lb[y - 1, x + 1], Lb[y - 1, x - 1], Lb[y - 2, x]]
            if O.ssd8_at(Lp, Rb, int(col[i]) + p, y) != best[i]:
                continue
            tied["points_tied_one_period_on"] += 1
            a, b = scan_path(int(n_cand[i]), int(col[i] - lo[i])), scan_path(int(n_cand[i]), int(col[i] - lo[i]) + p)
            tied["tied_other_lane"] += a[2] != b[2]
            tied["tied_other_row_of_16"] += a[2] // 16 != b[2] // 16
            tied["tied_same_lane_last_loops"] += a[2] == b[2] and a[0] != "main" and b[0] != "main"
            tied["tied_same_lane_main_loop"] += a[2] == b[2] and a[0] == b[0] == "main" and a[1] != b[1]
    c.update({k: int(v) for k, v in tied.items()})
    # where the UNIQUE minimum falls (checked against every candidate's SSD, at most unique_limit points per class)
    cls = dict.fromkeys(("min_on_first", "min_on_last", "min_on_last_of_main_trip", "min_on_first_of_next_main_trip",
                         "min_in_pair_loop", "min_in_single_loop", "min_in_main_loop"), 0)
    if A["row"]["group"] == "trip-edges":
        for i in np.flatnonzero(hit & (n_cand > 0)):
            n, off = int(n_cand[i]), int(col[i] - lo[i])
            path = scan_path(n, off)
            mine = [k for k, ok in (("min_on_first", off == 0), ("min_on_last", off == n - 1),
                                    ("min_on_last_of_main_trip", path[0] == "main" and off % MAIN_TRIP == MAIN_TRIP - 1),
                                    ("min_on_first_of_next_main_trip", path[0] == "main" and path[1] > 0 and off % MAIN_TRIP == 0),
                                    ("min_in_pair_loop", path[0] == "pair"), ("min_in_single_loop", path[0] == "single"),
                                    ("min_in_main_loop", path[0] == "main")) if ok and cls[k] < unique_limit]
            if mine and int((ssd_candidates(A["Lb"], A["Rb"], int(xs[i]), int(ys[i]), int(lo[i])) == best[i]).sum()) == 1:
                for k in mine:
                    cls[k] += 1
    c.update(cls)
    return c


def counts(r):
    A = analysis(r)
    if "counts" not in A:
        A["counts"] = dict(selection_counts(A), **scan_counts(A))
    return A["counts"]
