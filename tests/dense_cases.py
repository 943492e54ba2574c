"""Models and cases of tests/test_dense_cases_cpu.py and tests/test_gpu_dense_cases.py.

Two things the per-pixel tests (tests/test_gpu_devmath.py) do not pin:

* which pixels a block of the dense evaluation visits (dense.hip.h: dense_level_geometry, dense_block_run and the unit walk of
  dense_eval_block_pipelined) and how a block's sums are joined. `geometry`, `block_run`, `run_units` and `block_pixels` restate the
  index arithmetic in Python integers; CASES is a table of small frames and grid caps at which every situation of that arithmetic
  occurs (tests/test_dense_cases_cpu.py asserts that it does);
* the t-distribution scale iteration over stored residuals (kernels.hip.h: lm_tdist_scale_kernel in both orders,
  lm_tdist_scale_multi_kernel). `tdist_model` is the iteration with every pass's sum taken exactly (math.fsum); the kernels add the
  same fp32 terms in fp64 in some order, which stays within n 2^-52 S of that sum, and for the committed residual sets that interval
  holds ONE float sigma at every pass (asserted on the CPU), so the device's result is known bit for bit whatever its order.
"""
import functools
import math
import os
import re

import numpy as np

from fine_gather_cases import _texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _header(name):
    with open(os.path.join(ROOT, "odometry_amd", "csrc", name)) as f:
        return f.read()


def constant(header, name):
    """An integer constant of a header, e.g. `constexpr int kDenseBlock = 256, kDenseWaves = 4;`."""
    return int(re.search(r"\b" + name + r" = (\d+)\b", _header(header)).group(1))


DENSE_BLOCK = constant("dense.hip.h", "kDenseBlock")
GRID_CAP = constant("dense.hip.h", "kDenseGridCap")
R = DENSE_BLOCK // 64                     # rows of a unit: one per wavefront of a block
NACC = 29


# ---- A. the dense scan's work decomposition ----------------------------------------------------------------------------------------
def geometry(rows, cols, cap, block=DENSE_BLOCK):
    """dense_level_geometry: (n_strips, n_rg, nblk)."""
    r = block // 64
    iw, ih = cols - 8, rows - 8
    if iw <= 0 or ih <= 0:
        return 0, 0, 1
    n_strips, n_rg = (iw + 63) // 64, (ih + r - 1) // r
    return n_strips, n_rg, max(1, min(n_strips * n_rg, cap))


def block_run(n_strips, n_rg, nblk, b):
    """dense_block_run: (strip, rg, rg0, rg1, count) of block b. The device computes in unsigned 32-bit: every intermediate is checked."""
    def u32(v):
        assert 0 <= v < 1 << 32, "32-bit overflow in dense_block_run"
        return v
    G = min(nblk, 8)
    g, j = b % G, b // G
    nj = u32(nblk - g + G - 1) // G
    rg0, rg1 = u32(g * n_rg) // G, u32((g + 1) * n_rg) // G
    nrg = rg1 - rg0
    U = u32(nrg * n_strips)
    u0, u1 = u32(j * U) // nj, u32((j + 1) * U) // nj
    return (u0 // nrg if nrg else 0, rg0 + u0 % nrg if nrg else 0, rg0, rg1, u1 - u0)


def run_units(run):
    """The (strip, row group) pairs a block walks: `if (++rg == rg1) { rg = rg0; strip++; }`."""
    strip, rg, rg0, rg1, count = run
    out = []
    for _ in range(count):
        out.append((strip, rg))
        rg += 1
        if rg == rg1:
            rg, strip = rg0, strip + 1
    return out


def unit_pixels(rows, cols, strip, rg, block=DENSE_BLOCK):
    """Flat indices y * cols + x of the in-image pixels of a unit: x = 4 + 64 strip + lane < cols - 4, y = 4 + R rg + wave < rows - 4."""
    r = block // 64
    xs = np.arange(4 + 64 * strip, min(4 + 64 * strip + 64, cols - 4))
    ys = np.arange(4 + r * rg, min(4 + r * rg + r, rows - 4))
    return (ys[:, None] * cols + xs[None, :]).reshape(-1)


def block_pixels(rows, cols, cap):
    """Per block: the flat indices of its pixels, in the model's walk order."""
    n_strips, n_rg, nblk = geometry(rows, cols, cap)
    out = []
    for b in range(nblk):
        px = [unit_pixels(rows, cols, s, g) for s, g in run_units(block_run(n_strips, n_rg, nblk, b))]
        out.append(np.concatenate(px) if px else np.zeros(0, np.int64))
    return out


def runs(rows, cols, cap):
    n_strips, n_rg, nblk = geometry(rows, cols, cap)
    return np.array([block_run(n_strips, n_rg, nblk, b) for b in range(nblk)], np.int32).reshape(nblk, 5)


def wraps(run):
    """A run that goes from the bottom of one strip to the top of the next and on."""
    strip, rg, rg0, rg1, count = run
    return count >= 2 and (rg - rg0) + count > (rg1 - rg0)


WIDTHS = (1, 63, 64, 65, 128, 129)               # interior widths: below, at and above one and two 64-pixel strips
HEIGHTS = (1, 3, 4, 5, 8, 9, 31, 32, 33)         # interior heights: below, at and above one, two and eight row groups of R = 4


def _cases():
    out = []
    # every interior width x height, one unit per block (the product's decomposition of a small level)
    for ih in HEIGHTS:
        for iw in WIDTHS:
            out.append((ih + 8, iw + 8, GRID_CAP))
    # no interior: one block, a partial row of zeros
    out += [(8, 72, GRID_CAP), (40, 8, GRID_CAP), (8, 8, 3)]
    # small caps: what the product reaches above 1024 units — runs of several units, odd and even, wrapping from strip to strip
    for (rows, cols), caps in (((33 + 8, 129 + 8), (1, 2, 3, 5, 7, 8, 9, 13, 16, 17)),
                             ((31 + 8, 128 + 8), (3, 8, 9, 13)),
                             ((32 + 8, 65 + 8), (5, 8, 9, 16)),
                             ((9 + 8, 129 + 8), (2, 7, 8)),
                             ((5 + 8, 129 + 8), (4, 5)),          # n_rg = 2 < G: bands without row groups
                             ((4 + 8, 128 + 8), (2,)),            # n_rg = 1 < G = 2
                             ((81 + 8, 129 + 8), (5, 13, 16, 17, 64)),
                             ((81 + 8, 1 + 8), (3, 8, 9))):
        for cap in caps:
            out.append((rows, cols, cap))
    return out


CASES = _cases()


def case_id(case):
    return "%dx%d_cap%d" % case


def case_inputs(rows, cols, seed=0):
    """(I1, I2, D1, k = (fl, cx, cy, bilinear), T 4x4 row-major) of a frame: the texture of fine_gather_cases.py, an inverse depth with
    pseudo-random holes and a few |d| > 4096 pixels (waves that leave the shared-reciprocal path inside a level that takes it), a pose
    with motion (pixels warp out of the image), a principal point on an interior pixel (x == cx, y == cy occur)."""
    rng = np.random.default_rng(1000 * rows + cols + seed)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    I1 = _texture(x, y).astype(f32)
    I2 = _texture(x + 2.0, y + 1.0).astype(f32)
    D1 = rng.uniform(0.05, 2.0, (rows, cols)).astype(f32)
    D1[rng.random((rows, cols)) < 0.2] = 0.0
    D1[rng.random((rows, cols)) < 0.02] = f32(0.005)                    # below the validity threshold without being zero
    big = rng.random((rows, cols)) < 0.01
    D1[big] = np.where(rng.random(int(big.sum())) < 0.5, f32(5000.0), f32(-6000.0))
    if (rows - 8) * (cols - 8) == 1:
        D1[4, 4] = f32(0.05)                                             # a single interior pixel: a far point, which lands inside
    elif rows > 8 and cols > 8:
        D1[4 + (rows - 8) // 2, 4 + (cols - 8) // 2] = f32(4096.5)     # at least one unguarded pixel, in the middle unit
    fl = 60.0 if cols - 8 >= 31 else 10.0                                # (a narrow frame: a shorter lens, or nothing lands inside it)
    k = (fl, float(4 + (cols - 8) // 2), float(4 + (rows - 8) // 2), 0)
    T = np.eye(4, dtype=f32)
    a, b = 0.03, -0.02
    T[:3, :3] = (np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]) @
                 np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])).astype(f32)
    T[0, 3], T[1, 3], T[2, 3] = 0.15, -0.05, -0.02
    return I1, I2, D1, k, T


def sum_bound(terms, n):
    """|any-order fp64 sum of the exact terms - their exact sum| <= n 2^-52 sum |terms| (each of the n - 1 additions rounds once:
    (n - 1) 2^-53 to first order; 2^-52 covers the higher orders for every n below 2^50)."""
    return n * 2.0 ** -52 * math.fsum(np.abs(terms))


# ---- B. the t-distribution scale ------------------------------------------------------------------------------------------------------
LM_BLOCK = constant("kernels.hip.h", "kLmBlock")
FINE_KMAX = constant("kernels.hip.h", "kFineKMax")
CHUNKS_MAX = constant("kernels.hip.h", "kTdistChunksMax")
TS_THREADS, TS_PER_THREAD, TS_MAX_WG = (constant("kernels.hip.h", n) for n in ("kTsThreads", "kTsPerThread", "kTsMaxWg"))
MAX_PASSES = constant("kernels.hip.h", "kTdistMaxPasses")
LIST_MAX = 2 * FINE_KMAX * LM_BLOCK                 # 16384: the last size the product gives to the list order
SINGLE_LIST_MAX = 64 * CHUNKS_MAX                   # 40960: the last size the single-workgroup kernel holds in registers
FITS_MAX = TS_MAX_WG * TS_THREADS * TS_PER_THREAD   # 2097152: the last size the multi-workgroup kernel holds in registers
ORDER_LIST, ORDER_STRIDED, ORDER_PRODUCT = 0, 1, 2
WROTE_LIST, WROTE_STRIDED, WROTE_MULTI = 0, 1, 2


def scale_plan(n):
    """tdist_scale_plan (kernels.hip.h): (list, G, fits, single_order)."""
    per_wg = TS_THREADS * 8
    G = max(2, min(TS_MAX_WG, (n + per_wg - 1) // per_wg))
    return int(n <= LIST_MAX), G, int(n <= G * TS_THREADS * TS_PER_THREAD), int(n <= SINGLE_LIST_MAX)


def product_writer(n):
    """Which kernel the product's launch sequence lets write sigma when no multi-workgroup launch gives up."""
    lst, G, fits, single = scale_plan(n)
    if lst:
        return WROTE_LIST
    if not fits:
        return WROTE_LIST if single else WROTE_STRIDED
    return WROTE_MULTI


SCALE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, LIST_MAX, LIST_MAX + 1, 20480, 20481, SINGLE_LIST_MAX, SINGLE_LIST_MAX + 1,
               524288, 524289, FITS_MAX, FITS_MAX + 1)
SCALE_KINDS = ("mixed", "mixed1", "all_nan", "nan_tail", "valid", "const")
SCALE_SEEDS = {}                                    # (n, kind) -> seed, for a case whose interval is not one float under its default seed


def scale_cases():
    return [(0, "valid")] + [(n, kind) for n in SCALE_SIZES[1:] for kind in SCALE_KINDS]


@functools.lru_cache(maxsize=8)
def residuals(n, kind):
    """mixed / mixed1: standard_t(3) * 12 with 30 % NaN (seeds 0 and 1); all_nan; nan_tail: NaN only in the second half of the last
    64-residual chunk; valid: no NaN; const: one value everywhere."""
    seed = SCALE_SEEDS.get((n, kind), 1 if kind == "mixed1" else 0)
    rng = np.random.default_rng([seed, n])
    if kind == "all_nan":
        return np.full(n, np.nan, f32)
    if kind == "const":
        return np.full(n, 7.25, f32)
    r = (rng.standard_t(3, n) * 12.0).astype(f32)
    if kind in ("mixed", "mixed1"):
        r[rng.random(n) < 0.3] = np.nan
    elif kind == "nan_tail" and n:
        first = 64 * ((n - 1) // 64)
        r[first + (n - first) // 2:] = np.nan
    return r


def tdist_terms(e2, sigma):
    """tdist_term per residual in float32, in its operation order: e2 * 201 / (200 + e2 / sigma^2) (-ffp-contract=off, correctly
    rounded fp32 division: numpy's float32 operations are the device's)."""
    s2 = f32(sigma) * f32(sigma)
    return (e2 * f32(201.0)) / (f32(200.0) + e2 / s2)


def _next_sigma(total, n):
    return np.sqrt(f32(total / float(n)))


def tdist_model(res):
    """The scale iteration with exact sums. Returns (sigma^2 as float32, passes, single): single = at every pass the interval of sums an
    fp64 summation of the terms in any order can give, S (1 +- n 2^-52), holds one float sigma."""
    res = np.ascontiguousarray(res, f32)
    r = res[~np.isnan(res)]
    n = len(r)
    cur = f32(5.0)
    if n == 0:
        return f32(25.0), 0, True
    e2 = r * r
    single = True
    passes = 0
    for passes in range(1, MAX_PASSES + 1):
        S = math.fsum(tdist_terms(e2, cur).astype(np.float64))
        slack = n * 2.0 ** -52 * S
        nxt = _next_sigma(S, n)
        single = single and _next_sigma(S - slack, n) == nxt == _next_sigma(S + slack, n)
        done = not (abs(f32(nxt - cur)) >= f32(1e-3))
        cur = nxt
        if done:
            break
    return f32(cur * cur), passes, single


@functools.lru_cache(maxsize=None)
def scale_expected(n, kind):
    return tdist_model(residuals(n, kind))


# ---- through the public API ----------------------------------------------------------------------------------------------------------
def row_products(r, w, J):
    """The 29 products odo::accumulate_row (odo_math.h) adds for each row, formed exactly: fl32(J w) and fl32(r w) in float32, every
    product of two float32 values exact in float64. [n, 29]."""
    r, w, J = np.asarray(r, f32), np.asarray(w, f32), np.asarray(J, f32)
    jw = (J * w[:, None]).astype(f32).astype(np.float64)
    Jd, rd = J.astype(np.float64), r.astype(np.float64)
    out = np.zeros((len(r), NACC))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            out[:, k] = jw[:, a] * Jd[:, b]
            k += 1
    out[:, 21:27] = jw * rd[:, None]
    out[:, 27] = (r * w).astype(f32).astype(np.float64) * rd
    out[:, 28] = 1.0
    return out


# (rows, cols, pyramid levels) of the frames that go through lm.accumulate. 41 x 137 and 24 x 40 end on a level without interior
# (5 x 17, 6 x 10); 4108 x 72 is 1 strip x 1025 row groups, the smallest frame at which the product's own cap (1024) builds runs of
# more than one unit.
API_FRAMES = ((12, 72, 1), (9, 9, 1), (41, 137, 4), (24, 40, 3), (4108, 72, 1))
LIST_FRAME = (150, 196)          # interior 142 x 188 = 26 696 points: a point-list level above LIST_MAX (the multi-workgroup scale)


def list_inputs():
    """LIST_FRAME with every interior pixel a point, a small sideways motion and the principal point near a corner of the image.
    The corner is what makes `rtol` on the 28 sums a statement about sigma: with the principal point in the middle the cross sums
    cancel (sum |terms| / |sum| up to 19 000 for this frame) and the oracle's OWN fp64 summation is 5e-11 off the exact sum, above
    the 1e-11 the test asks for; near the corner x - cx and y - cy keep their sign, no sum cancels by more than 11 and the oracle
    is within 2e-14 of the exact sums (tests/test_dense_cases_cpu.py asserts both)."""
    rows, cols = LIST_FRAME
    I1, I2, D1, k, _ = case_inputs(rows, cols, seed=7)
    inv = np.where(np.abs(D1) < 0.01, f32(0.3), np.minimum(np.abs(D1), f32(2.0))).astype(f32)
    T = np.eye(4, dtype=f32)
    T[0, 3] = 0.01
    return I1, I2, inv, (k[0], 10.0, 6.0), T


def api_inputs(rows, cols):
    """(I1, I2, inverse depth, intrinsics (f0, cx0, cy0), pose) of a frame for the library and the oracle: case_inputs' images, depth
    and pose."""
    I1, I2, D1, k, T = case_inputs(rows, cols, seed=7)
    return I1, I2, D1, (k[0], k[1], k[2]), T
