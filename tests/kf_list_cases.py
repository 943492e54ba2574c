"""Models and cases of tests/test_kf_list_cases_cpu.py and tests/test_gpu_kf_list_cases.py.

The route every semi-dense Solve reads its points through: kf_count_kernel / kf_fill_kernel (kernels.hip.h) compact the valid interior
pixels of all levels of a keyframe into point lists, `load_point` reads them back in lm_residual_list_kernel /
lm_residual_only_list_kernel and in the coarse, persistent and step launches.

* A. The lists. A list is make_point (odo_math.h) of the level's valid interior pixels in raster order. `expected` builds every byte
  the two kernels may write — rowcnt, npts and the four arrays of every level, with the 0xAB fill where they must not write — from
  the thirteen floats per pixel of `Ops.make_points`; CASES places small frames at the edges of the kernels' index arithmetic (a row's
  256-pixel chunks, the 256-row trips of the row-offset prefix, the ballot at lanes 0 and 63, levels without interior, every one of
  pl0 .. pl7, both sides of both inequalities of the dense_above skip). Three deliberately wrong models (`variant`) show that the
  cases would notice the mistakes they are placed for.
* B. What reads a list. `partial_rows` restates lm_residual_list_kernel's summation — a thread's points in ascending grid-stride
  order, block_reduce_acc's 32 additions per (quantity, segment) and its 8-lane tree — in numpy float64, whose additions are the
  device's; every term is exact in fp64 (dense_cases.row_products), so the partial rows are known bit for bit.
"""
import functools
import os
import re

import numpy as np

import dense_cases as Dc
from fine_gather_cases import _texture

ROOT = Dc.ROOT
f32 = np.float32
MAX_LEVELS = 8                                   # ODO_MAX_LEVELS_K
CHUNK = 256                                      # threads of a kf_count / kf_fill block: pixels of a row per trip, rows per prefix trip
FILL32 = np.uint32(0xABABABAB)
K = (96.0, 20.5, 6.25)                           # (f0, cx0, cy0) of every list case
SPARE = 3                                        # list entries behind a level's interior size


def valid(d):
    """depth_valid (odo_math.h): !(fabsf(d) < 0.01f). The code's rule, NaN included: NaN is valid and is listed."""
    return ~(np.abs(np.asarray(d, f32)) < f32(0.01))


LO, HI = np.nextafter(f32(0.01), f32(0)), np.nextafter(f32(0.01), f32(1))
# (inverse depth, valid?) at the validity test: the threshold and its float32 neighbours, its negative, both zeros, a denormal, negative
# depths, |d| > 4096, both infinities, NaN
EDGE_DEPTHS = ((f32(0.01), True), (LO, False), (HI, True), (f32(-0.01), True), (-LO, False), (f32(0.0), False), (f32(-0.0), False),
               (f32(1e-40), False), (f32(-1e-40), False), (f32(-0.5), True), (f32(-3.0), True), (f32(5000.0), True), (f32(-6000.0), True),
               (f32(np.inf), True), (f32(-np.inf), True), (f32(np.nan), True), (f32(0.3), True))


# ---- A. contents of a level ------------------------------------------------------------------------------------------------------------
def level_content(rows, cols, pattern, seed=0):
    """(I1, D1) of one level. The 4-pixel border holds no depth unless the pattern says so. Patterns, over the interior (iw x ih):
    all / none; first_col (x = 4) / last_col (x = cols - 5); lane0 / lane63 (only that lane of every wave); last_chunk (only the last
    256-pixel chunk of a row); alt (alternating); empty_row (row 1 empty between full ones); border (valid depths all over the border,
    half of the interior); random (40 %); edge (EDGE_DEPTHS in turn); count:N (exactly N valid pixels, scattered)."""
    rng = np.random.default_rng([seed, rows, cols])
    y, x = np.mgrid[0:rows, 0:cols]
    I1 = _texture(x.astype(np.float64) + 3.0 * seed, y.astype(np.float64)).astype(f32)
    depth = rng.uniform(0.05, 2.0, (rows, cols)).astype(f32)
    iw, ih = cols - 8, rows - 8
    D1 = np.zeros((rows, cols), f32)
    if iw <= 0 or ih <= 0:
        return I1, depth                                             # no interior: depths everywhere, none may be listed
    xi, yi = x[4:rows - 4, 4:cols - 4] - 4, y[4:rows - 4, 4:cols - 4] - 4
    if pattern.startswith("count:"):
        keep = np.zeros(iw * ih, bool)
        keep[rng.permutation(iw * ih)[:int(pattern[6:])]] = True
        keep = keep.reshape(ih, iw)
    else:
        keep = {"all": lambda: np.ones((ih, iw), bool), "none": lambda: np.zeros((ih, iw), bool), "first_col": lambda: xi == 0,
                "last_col": lambda: xi == iw - 1, "lane0": lambda: xi % 64 == 0, "lane63": lambda: xi % 64 == 63,
                "last_chunk": lambda: xi >= CHUNK * ((iw - 1) // CHUNK), "alt": lambda: (xi + yi) % 2 == 0,
                "empty_row": lambda: yi != 1, "border": lambda: rng.random((ih, iw)) < 0.5, "random": lambda: rng.random((ih, iw)) < 0.4,
                "edge": lambda: np.ones((ih, iw), bool)}[pattern]()
    if pattern == "border":
        D1[...] = depth
    inner = D1[4:rows - 4, 4:cols - 4]
    inner[...] = np.where(keep, depth[4:rows - 4, 4:cols - 4], f32(0.0))
    if pattern == "edge":
        vals = np.array([v for v, _ in EDGE_DEPTHS], f32)
        inner[...] = vals[(xi + 5 * yi) % len(vals)]
    return I1, D1


def _case(name, levels, dense_above=0):
    """levels: [(rows, cols, pattern)]."""
    return dict(id=name, levels=tuple(levels), dense_above=dense_above)


WIDTHS = (1, 63, 64, 65, 255, 256, 257, 513)      # interior widths: a wave, a chunk (the chunk loop ends exactly), a second chunk of one pixel, three chunks
# interior heights. Row my's offset is the sum of rowcnt[0 .. my): thread t adds rows t, t + 256, ... — the second trip of
# `for (i = t; i < my; i += 256)` first happens at my = 257 (height 258), the third at my = 513 (height 514).
HEIGHTS = (1, 256, 257, 258, 513, 514)
SKIP_POINTS = ((128, 1), (129, 128), (129, 129), (129, 0), (256, 255), (256, 256))   # (total, dense_above) on an interior of 256


def _cases():
    out = []
    for iw in WIDTHS:
        for pat in ("all", "random"):
            out.append(_case("w%d_%s" % (iw, pat), [(3 + 8, iw + 8, pat)]))
    for ih in HEIGHTS:
        for iw, pat in ((1, "all"), (3, "random")):
            out.append(_case("h%d_w%d_%s" % (ih, iw, pat), [(ih + 8, iw + 8, pat)]))
    for pat in ("all", "none", "first_col", "last_col", "lane0", "lane63", "last_chunk", "alt", "empty_row", "border"):
        out.append(_case("pat_" + pat, [(3 + 8, 513 + 8, pat)]))
    out.append(_case("pat_lane63_w64", [(2 + 8, 64 + 8, "lane63")]))
    out.append(_case("edge_depths", [(3 + 8, len(EDGE_DEPTHS) + 8, "edge")]))
    out.append(_case("levels4_last_rows8", [(14, 40, "random"), (11, 24, "all"), (10, 13, "alt"), (8, 20, "all")]))
    out.append(_case("levels3_mid_cols8", [(12, 20, "random"), (12, 8, "all"), (11, 12, "all")]))
    out.append(_case("levels3_first_rows5", [(5, 30, "all"), (12, 12, "random"), (10, 11, "all")]))
    out.append(_case("levels8", [(9 + l % 3, 10 + (5 * l) % 7, "random" if l % 2 else "all") for l in range(MAX_LEVELS)]))
    for total, above in SKIP_POINTS:
        out.append(_case("skip_%d_above%d" % (total, above), [(12, 72, "count:%d" % total)], above))
    out.append(_case("skip_0_filled_1", [(12, 72, "count:129"), (12, 72, "count:128")], 1))
    out.append(_case("filled_0_skip_1", [(12, 72, "count:128"), (12, 72, "count:129")], 1))
    out.append(_case("skip_tall", [(258 + 8, 1 + 8, "all")], 1))      # the skip's own sum over the level's rows takes a second trip
    out.append(_case("skip_mixed_levels", [(12, 72, "count:200"), (8, 72, "all"), (10, 20, "all"), (11, 30, "count:9")], 20))
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def contents(case_id, seed=0):
    """[(I1, D1)] of a case's levels (seed 1: the second table entry of the by-reference launch, other contents in the same shapes)."""
    case = next(c for c in CASES if c["id"] == case_id)
    out = []
    for l, (rows, cols, pat) in enumerate(case["levels"]):
        I1, D1 = level_content(rows, cols, pat if seed == 0 or pat.startswith("count:") else "random", seed=10 * seed + l)
        I1.setflags(write=False)
        D1.setflags(write=False)
        out.append((I1, D1))
    return out


# ---- A. the model ---------------------------------------------------------------------------------------------------------------------
def cx_level(c, level):
    v = f32(c)
    for _ in range(level):
        v = (v + f32(0.5)) / f32(2.0) + f32(0.5)
    return v


def make_points_np(I1, D1, K, level):
    """make_point (odo_math.h) of every pixel restated on numpy float32, operation by operation: [rows, cols, 13]."""
    rows, cols = D1.shape
    fl = float(f32(K[0])) / 2.0 ** level
    flf, cx, cy = f32(fl), cx_level(K[1], level), cx_level(K[2], level)
    y, x = np.mgrid[0:rows, 0:cols].astype(f32)
    d = np.asarray(D1, f32)
    with np.errstate(all="ignore"):
        z = f32(1.0) / d
        X, Y, Z = (z * (x - cx)) / flf, (z * (y - cy)) / flf, z
        fx_z = flf / Z
        xy, xx, yy, zz = X * Y, X * X, Y * Y, Z * Z
        jw02, jw03 = (-fx_z * X) / Z, (-fx_z * xy) / Z
        jw04 = (fl * (1.0 + (xx / zz).astype(np.float64))).astype(f32)
        jw05, jw12 = -fx_z * Y, (-fx_z * Y) / Z
        jw13 = (-fl * (1.0 + (yy / zz).astype(np.float64))).astype(f32)
        jw14, jw15 = -jw03, fx_z * X
    out = np.stack([X, Y, Z, np.asarray(I1, f32), fx_z, jw02, jw03, jw04, jw05, jw12, jw13, jw14, jw15], axis=2)
    assert out.dtype == f32
    return out


def interior(rows, cols):
    return (rows - 8, cols - 8) if rows > 8 and cols > 8 else (0, 0)


def skip_verdict(total, n_interior, dense_above, variant=None):
    """kf_fill_kernel_body's skip — the host's rule in lm_take_counts read the other way round."""
    if dense_above <= 0:
        return False
    a = total >= dense_above if variant == "skip_ge_total" else total > dense_above
    b = 2 * total >= n_interior if variant == "skip_ge_half" else 2 * total > n_interior
    return bool(a and b)


def host_use_list(npts, n_interior, fuse_dense_max, mode=0):
    """lm_take_counts (odometry_hip.hip): does the level run on its list?"""
    return bool(mode == 2 or (n_interior > 0 and 2 * npts <= n_interior) or (mode == 0 and 0 < npts <= fuse_dense_max))


VARIANTS = ("chunk_restart", "prefix_256", "skip_ge_total", "skip_ge_half")


def expected(levels, points, dense_above=0, spare=SPARE, variant=None):
    """Every byte of a list build. levels = [(I1, D1)], points = [make_points of each level]. Returns dict(rowcnt [rows_total + 1] int32,
    npts [8] int32, lists = 8 x [interior + spare, 13] float32, skipped = [bool per level]), unwritten parts holding the 0xAB fill.
    variant None: the contract — entries [0, npts) are the valid interior pixels' points in raster order. The wrong models:
    chunk_restart (a row's second chunk starts at the row's base again), prefix_256 (a row's offset counts only the first 256 rows
    above it), skip_ge_total / skip_ge_half (`>=` in one of the skip's inequalities)."""
    rowcnt, npts, lists, skipped = [], np.zeros(MAX_LEVELS, np.int32), [], []
    for l in range(MAX_LEVELS):
        ih, iw = interior(*levels[l][1].shape) if l < len(levels) else (0, 0)
        out = np.full((ih * iw + spare, 13), FILL32, np.uint32).view(f32)
        lists.append(out)
        if ih == 0:
            skipped.append(False)
            continue
        D1 = levels[l][1]
        V = valid(D1[4:-4, 4:-4])
        pts = points[l][4:-4, 4:-4]
        cnt = V.sum(1).astype(np.int64)
        rowcnt += [int(c) for c in cnt]
        skip = skip_verdict(int(cnt.sum()), ih * iw, dense_above, variant)
        skipped.append(skip)
        if skip:
            npts[l] = cnt.sum()
            continue
        if variant is None:
            out[:cnt.sum()] = pts[V]                                 # numpy's compaction in raster order
            npts[l] = cnt.sum()
            continue
        before = np.concatenate([[0], np.cumsum(cnt)[:-1]])          # the row's offset
        if variant == "prefix_256":
            before = np.array([cnt[:min(my, CHUNK)].sum() for my in range(ih)], np.int64)
        in_row = np.cumsum(V, 1) - 1                                  # the pixel's place in its row
        if variant == "chunk_restart":
            for x0 in range(CHUNK, iw, CHUNK):
                in_row[:, x0:x0 + CHUNK] -= V[:, :x0].sum(1, keepdims=True)
        pos = before[:, None] + in_row
        out[pos[V]] = pts[V]                                          # in raster order: a later write to the same entry wins
        npts[l] = before[-1] + cnt[-1]
    rc = np.full(len(rowcnt) + 1, FILL32, np.uint32).view(np.int32)
    rc[:len(rowcnt)] = rowcnt
    return dict(rowcnt=rc, npts=npts, lists=lists, skipped=skipped)


def same_build(a, b):
    """Two list builds (rowcnt, npts, lists) byte for byte, NaNs as NaNs."""
    if not (np.array_equal(a["rowcnt"], b["rowcnt"]) and np.array_equal(a["npts"], b["npts"])):
        return False
    for x, y in zip(a["lists"], b["lists"]):
        xb, yb = np.ascontiguousarray(x, f32).view(np.uint32), np.ascontiguousarray(y, f32).view(np.uint32)
        if x.shape != y.shape or not ((xb == yb) | (np.isnan(x) & np.isnan(y))).all():
            return False
    return True


def situations(case, levels):
    """What a case reaches: chunk trips of a row, rows whose later chunk starts behind points of an earlier one (hand-overs of base_sh
    that carry something), trips of the row-offset prefix, rows whose offset needs rows >= 256 that hold points, waves whose ballot
    is lane 0 alone / lane 63 alone, levels without interior, the skip's verdicts."""
    s = dict(chunk_trips=0, carries=0, prefix_trips=0, prefix_late=0, lane0_only=0, lane63_only=0, no_interior=0, skipped=[], exact_end=0,
             levels_with_points=0, border_depths=0)
    for rows, cols, _ in case["levels"]:
        if interior(rows, cols) == (0, 0):
            s["no_interior"] += 1
    for (I1, D1), (rows, cols, _) in zip(levels, case["levels"]):
        ih, iw = interior(rows, cols)
        if ih == 0:
            continue
        V = valid(D1[4:-4, 4:-4])
        B = valid(D1).copy()
        B[4:-4, 4:-4] = False
        s["border_depths"] += int(B.sum())
        s["levels_with_points"] += int(V.any())
        s["chunk_trips"] = max(s["chunk_trips"], -(-iw // CHUNK))
        s["exact_end"] += int(iw % CHUNK == 0)
        for x0 in range(CHUNK, iw, CHUNK):
            s["carries"] += int((V[:, :x0].any(1) & V[:, x0:x0 + CHUNK].any(1)).sum())
        s["prefix_trips"] = max(s["prefix_trips"], -(-(ih - 1) // CHUNK))
        cnt = V.sum(1)
        s["prefix_late"] += sum(1 for my in range(CHUNK + 1, ih) if cnt[CHUNK:my].any())
        for x0 in range(0, iw, 64):
            w = V[:, x0:x0 + 64]
            one = w.sum(1) == 1
            s["lane0_only"] += int((one & w[:, 0]).sum())
            if w.shape[1] == 64:
                s["lane63_only"] += int((one & w[:, 63]).sum())
        s["skipped"].append(skip_verdict(int(V.sum()), ih * iw, case["dense_above"]))
    return s


# ---- B. what reads the lists ------------------------------------------------------------------------------------------------------------
def _list_max_blocks():
    with open(os.path.join(ROOT, "odometry_amd", "csrc", "odometry_hip.hip")) as f:
        m = re.search(r"constexpr int kLmListMaxBlocks = (\d+);", f.read())
    assert m, "odometry_hip.hip no longer declares `constexpr int kLmListMaxBlocks = <n>;`: the largest list case is placed by it"
    return int(m.group(1))


LIST_MAX_BLOCKS = _list_max_blocks()
LM_BLOCK = Dc.LM_BLOCK
HUBER, SCALE_SQR = 28.0, 30.25


def list_blocks(n):
    """lm_list_blocks (odometry_hip.hip)."""
    return max(1, min(LIST_MAX_BLOCKS, (n + LM_BLOCK - 1) // LM_BLOCK))


# (points, blocks): the product's grid at the edges of one and two blocks, forced small grids for the grid-stride loop, and the
# product's own cap with one point more than a trip of all its blocks
LIST_EVALS = tuple((n, list_blocks(n)) for n in (1, 255, 256, 257, 512, 513)) + ((1000, 1), (513, 2), (2049, 3)) + \
    ((LIST_MAX_BLOCKS * LM_BLOCK + 1, list_blocks(LIST_MAX_BLOCKS * LM_BLOCK + 1)),)
LIST_SEEDS = {}                                   # n -> seed, for a size whose default choice of pixels misses what it is there for


def list_frame(n):
    """The smallest of three frames whose interior holds n points with room to spare."""
    for rows, cols in ((40, 48), (56, 72), (177, 264)):
        if n <= (rows - 8) * (cols - 8) * 19 // 20:
            return rows, cols
    raise ValueError(n)


@functools.lru_cache(maxsize=4)
def list_inputs(n):
    """dense_cases.case_inputs of list_frame(n) — holes, far points, negative depths, a pose with motion — with the inverse depth
    thinned out or filled up to exactly n valid interior pixels."""
    rows, cols = list_frame(n)
    I1, I2, D1, k, T = Dc.case_inputs(rows, cols)
    rng = np.random.default_rng([LIST_SEEDS.get(n, 0), n])
    D1 = D1.copy()
    inner = D1[4:rows - 4, 4:cols - 4]
    V = valid(inner).ravel()
    order = rng.permutation(V.size)
    have = order[V[order]]
    flat = inner.reshape(-1).copy()
    if len(have) > n:
        flat[have[n:]] = f32(0.0)
    else:
        flat[order[~V[order]][:n - len(have)]] = f32(0.3)
    inner[...] = flat.reshape(inner.shape)
    assert int(valid(inner).sum()) == n
    for a in (I1, I2, D1, T):
        a.setflags(write=False)
    return I1, I2, D1, k, T


def list_points(D1, *per_pixel):
    """Per-pixel arrays [rows, cols, ...] -> the list's order: the valid interior pixels in raster order."""
    V = valid(D1[4:-4, 4:-4])
    return [np.asarray(a)[4:-4, 4:-4][V] for a in per_pixel]


def partial_rows(terms, hit, nblk, block=None):
    """lm_residual_list_kernel's partial rows [nblk, 29] from the points' 29 exact terms [n, 29] and their hit flags, in the kernel's
    order: thread t of block b adds its points b 256 + t + j nblk 256 in ascending j from +0 (a point without a residual adds
    nothing); thread (q, s) of block_reduce_acc adds sh[q][8 i + s] for i = 0 .. 31 from +0; the 8-lane xor tree,
    ((v0 + v4) + (v2 + v6)) + ((v1 + v5) + (v3 + v7))."""
    block = block or LM_BLOCK
    terms, hit = np.asarray(terms, np.float64), np.asarray(hit, bool)
    n, stride = len(hit), nblk * block
    trips = max(1, -(-n // stride))
    t_pad, h_pad = np.zeros((trips * stride, Dc.NACC)), np.zeros(trips * stride, bool)
    t_pad[:n], h_pad[:n] = terms, hit
    acc = np.zeros((stride, Dc.NACC))
    for j in range(trips):
        sl = slice(j * stride, (j + 1) * stride)
        acc = np.where(h_pad[sl, None], acc + t_pad[sl], acc)
    A = acc.reshape(nblk, block // 8, 8, Dc.NACC)
    v = np.zeros((nblk, 8, Dc.NACC))
    for i in range(block // 8):
        v = v + A[:, i]
    return ((v[:, 0] + v[:, 4]) + (v[:, 2] + v[:, 6])) + ((v[:, 1] + v[:, 5]) + (v[:, 3] + v[:, 7]))


def list_model(pix, D1, nblk):
    """pix = Ops.pixels(..., mode 0) of the frame: (the model's partial rows, hits among the list's points)."""
    hit, r, w, J = list_points(D1, *pix)
    hit = hit != 0
    terms = np.zeros((len(hit), Dc.NACC))
    terms[hit] = Dc.row_products(r[hit], w[hit], J[hit])
    return partial_rows(terms, hit, nblk), hit


# ---- the hand-over rule through the library ---------------------------------------------------------------------------------------------
HANDOVER = tuple((total, fuse) for total in (128, 129) for fuse in (128, 129))      # on the 12 x 72 level: interior 256


def handover_inputs(total, seed=0):
    """Dc.api_inputs of a 12 x 72 frame with exactly `total` valid interior pixels (ordinary depths)."""
    I1, I2, _, Kk, T = Dc.api_inputs(12, 72)
    D1 = level_content(12, 72, "count:%d" % total, seed=seed)[1]
    return I1, I2, D1, Kk, T
