"""The speckle filter's specification as code (include/odometry_hip.h, odo_speckle_create), shared by
tests/test_speckle_cpu.py and tests/test_gpu_speckle.py: the launch constants read out of the kernels' header, the numpy model (the
connected neighbour pairs found with array operations, then a union-find over them), a breadth-first flood fill in plain Python
written independently of it, and the rows — each with the situation it is in the table for as a predicate on the model's
intermediates. Nothing here loads the GPU library.

A row is (name, K, max_diff, min_size, predicate). The model can be told to get one of four things wrong (SWITCHES); CAUGHT_BY names,
for each, the rows that are in the table to notice. Frames and model results are computed once per process and shared."""
import functools
import os
import re
from collections import deque

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "odometry_amd", "csrc")
STATS = ("pixels", "components", "removed_components", "removed_pixels", "largest", "guard")
SWITCHES = ("eight", "strict", "gt", "zeros_connect")
FLOOD_PIXELS = 12000          # rows with no more pixels than this go through the flood fill


def constants():
    """{kName: value} of every `constexpr int kName = <integer>;` line of speckle_math.h and speckle.hip.h."""
    out = {}
    for name in ("speckle_math.h", "speckle.hip.h"):
        for m in re.finditer(r"^constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, name)).read(), re.M):
            out[m.group(1)] = int(m.group(2))
    return out


def geometry(size, k=None):
    """launch_speckle_stage's grids for a frame: tiles either way and the pixel pairs across the seams."""
    k = k or constants()
    rows, cols = size
    bx, by = -(-cols // k["kSpTileW"]), -(-rows // k["kSpTileH"])
    return dict(blocks_x=bx, blocks_y=by, seam_pairs=(by - 1) * cols + (bx - 1) * rows)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def speckle_model(K, max_diff, min_size, eight=False, strict=False, gt=False, zeros_connect=False):
    """dict(keep, stats, root, size): keep = the pixels that stay (non-zero key, component large enough); root = the smallest linear
    index of each pixel's component, -1 where the pixel belongs to none; size = its component's pixel count, 0 where none. The
    switches: diagonal neighbours connect too; `<` for `<=` in the connection; `>` for `>=` in the survival test; zero keys
    connect like any other key (and are pixels of components)."""
    K = np.asarray(K, np.uint16)
    rows, cols = K.shape
    n = rows * cols
    v = K.astype(np.int64)
    idx = np.arange(n).reshape(rows, cols)
    labelled = np.ones((rows, cols), bool) if zeros_connect else K != 0

    def pairs(sa, sb):
        d = np.abs(v[sa] - v[sb])
        ok = (d < max_diff if strict else d <= max_diff) & labelled[sa] & labelled[sb]
        return idx[sa][ok], idx[sb][ok]

    s_ = np.s_
    slices = [(s_[:, 1:], s_[:, :-1]), (s_[1:, :], s_[:-1, :])]
    if eight:
        slices += [(s_[1:, 1:], s_[:-1, :-1]), (s_[1:, :-1], s_[:-1, 1:])]
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for sa, sb in slices:
        ia, ib = pairs(sa, sb)
        for a, b in zip(ia.tolist(), ib.tolist()):
            ra, rb = find(a), find(b)
            if ra < rb:
                parent[rb] = ra
            elif rb < ra:
                parent[ra] = rb
    root = np.array([find(i) for i in range(n)], np.int64).reshape(rows, cols)
    root[~labelled] = -1
    counts = np.bincount(root[labelled], minlength=n) if labelled.any() else np.zeros(n, np.int64)
    size = np.where(labelled, counts[np.maximum(root, 0)], 0)
    big = size > min_size if gt else size >= min_size
    keep = labelled & big
    is_root = labelled & (root == idx)
    stats = dict(pixels=int((K != 0).sum()), components=int(is_root.sum()), removed_components=int((is_root & ~big).sum()),
                 removed_pixels=int((labelled & ~big).sum()), largest=int(size.max()) if n else 0, guard=0)
    return dict(keep=keep, stats=stats, root=root.astype(np.int32), size=size.astype(np.int32))


def speckle_flood(K, max_diff, min_size):
    """The rule read off the prose, a pixel at a time in Python integers: every unvisited non-zero pixel in raster order starts a
    breadth-first fill over its connected 4-neighbours. (keep, stats, root, size) as lists of lists."""
    px = [[int(v) for v in r] for r in np.asarray(K)]
    rows, cols = len(px), len(px[0])
    root = [[-1] * cols for _ in range(rows)]
    size = [[0] * cols for _ in range(rows)]
    keep = [[False] * cols for _ in range(rows)]
    n = dict.fromkeys(STATS, 0)
    for y0 in range(rows):
        for x0 in range(cols):
            if px[y0][x0] == 0 or root[y0][x0] >= 0:
                continue
            first = y0 * cols + x0                                   # raster order: the smallest index of the component
            root[y0][x0] = first
            todo, members = deque([(y0, x0)]), []
            while todo:
                y, x = todo.popleft()
                members.append((y, x))
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < rows and 0 <= xx < cols and px[yy][xx] != 0 and root[yy][xx] < 0 \
                            and abs(px[yy][xx] - px[y][x]) <= max_diff:
                        root[yy][xx] = first
                        todo.append((yy, xx))
            survives = len(members) >= min_size
            n["pixels"] += len(members)
            n["components"] += 1
            n["largest"] = max(n["largest"], len(members))
            if not survives:
                n["removed_components"] += 1
                n["removed_pixels"] += len(members)
            for y, x in members:
                size[y][x] = len(members)
                keep[y][x] = survives
    return keep, n, root, size


def apply_keep(frame, M):
    """What the filter leaves of a target frame: the non-surviving non-zero-key pixels zeroed, every other value as it was."""
    out = np.array(frame, np.uint16)
    out[(M["root"] >= 0) & ~M["keep"]] = 0
    return out


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def blobs(seed, size, p_zero=0.3):
    """Keys from a few levels one or three apart, so that max_diff 1 joins some neighbours and not others; p_zero of them 0."""
    rng = np.random.default_rng([0x5BEC, seed, size[0], size[1]])
    levels = np.array([100, 101, 103, 104, 200, 201], np.uint16)
    K = levels[rng.integers(0, len(levels), size)]
    K[rng.random(size) < p_zero] = 0
    return K


def serpentine(size, vertical=False):
    """A path one pixel wide that runs along every second row (column) and turns at alternate ends; keys 100, 101, 102, 100 .. along it."""
    rows, cols = size
    if vertical:
        return np.ascontiguousarray(serpentine((cols, rows)).T)
    K = np.zeros(size, np.uint16)
    step = 0
    for i, y in enumerate(range(0, rows, 2)):
        xs = range(cols) if i % 2 == 0 else range(cols - 1, -1, -1)
        for x in xs:
            K[y, x] = 100 + step % 3
            step += 1
        if y + 2 < rows:
            K[y + 1, cols - 1 if i % 2 == 0 else 0] = 100 + step % 3
            step += 1
    return K


def spiral(size):
    """A path one pixel wide that winds inwards from the top left corner with a one-pixel gap between its turns."""
    rows, cols = size
    K = np.zeros(size, np.uint16)
    inside = lambda y, x: 0 <= y < rows and 0 <= x < cols
    free = lambda y, x: not inside(y, x) or K[y, x] == 0
    y = x = step = 0
    dy, dx = 0, 1
    K[0, 0] = 100
    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx                                  # a step is taken if it touches nothing but the pixel it leaves
            if inside(ny, nx) and K[ny, nx] == 0 and all(free(ny + j, nx + i) for j, i in ((-1, 0), (1, 0), (0, -1), (0, 1)) if (ny + j, nx + i) != (y, x)):
                break
            dy, dx = dx, -dy
        else:
            return K
        y, x, step = ny, nx, step + 1
        K[y, x] = 100 + step % 3


def degree(K):
    """Non-zero 4-neighbours of every pixel."""
    m = np.pad(K != 0, 1)
    return (m[:-2, 1:-1].astype(int) + m[2:, 1:-1] + m[1:-1, :-2] + m[1:-1, 2:]) * (K != 0)


@functools.lru_cache(maxsize=None)
def wall_pair():
    """A textured scene at disparity 12 with an untextured patch (grey 128) in the middle, one grey level of noise on either image:
    census bits of the flat patch are the sign of the noise, and what the matcher matches there is mostly wrong."""
    rng = np.random.default_rng(3)
    rows, cols, d = 96, 320, 12
    base = rng.uniform(0, 255, (rows, cols + 64)).astype(np.float32)
    for _ in range(2):
        base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, -1, 0) + np.roll(base, -1, 1)) / 5
    base[28:68, 120:240] = 128.0
    L = (base[:, 32:32 + cols] + rng.normal(0, 1, (rows, cols))).astype(np.float32)
    R = (base[:, 32 + d:32 + d + cols] + rng.normal(0, 1, (rows, cols))).astype(np.float32)
    for a in (L, R):
        a.setflags(write=False)
    return L, R


def wall_params():
    import stereo_depth_cases as sdc
    return sdc.params(dmin=1, dmax=40, A=2)


@functools.lru_cache(maxsize=None)
def wall_match():
    """(depth, q, stats) of the wall scene from the matcher's model."""
    import stereo_depth_cases as sdc
    res = sdc.stereo_model(*wall_pair(), wall_params())
    for a in res[:2]:
        a.setflags(write=False)
    return res


# ---- the rows ---------------------------------------------------------------------------------------------------------------------
def _tiles_of(mask, k):
    ys, xs = np.nonzero(mask)
    return set(zip((ys // k["kSpTileH"]).tolist(), (xs // k["kSpTileW"]).tolist()))


def _sizes(M):
    """The sorted sizes of the components."""
    idx = np.arange(M["root"].size).reshape(M["root"].shape)
    return sorted(M["size"][M["root"] == idx].tolist())


@functools.lru_cache(maxsize=None)
def rows():
    k = constants()
    W, H = k["kSpTileW"], k["kSpTileH"]
    out = []

    def add(name, K, max_diff, min_size, pred):
        K = np.ascontiguousarray(K, np.uint16)
        K.setflags(write=False)
        out.append((name, K, max_diff, min_size, pred))

    s = lambda M: M["stats"]
    # degenerate frames
    add("all zero", np.zeros((H + 4, W + 6)), 4, 3, lambda M, K: s(M)["pixels"] == 0 and s(M)["components"] == 0 and s(M)["largest"] == 0)
    add("1 x 1 kept", [[7]], 0, 1, lambda M, K: s(M)["components"] == 1 and s(M)["removed_pixels"] == 0)
    add("1 x 1 removed", [[7]], 0, 2, lambda M, K: s(M)["components"] == 1 and s(M)["removed_pixels"] == 1)
    add(f"1 x {W + 3}", blobs(1, (1, W + 3), 0.2), 1, 3, lambda M, K: 2 < s(M)["removed_components"] < s(M)["components"])
    add(f"{2 * H + 3} x 1", blobs(2, (2 * H + 3, 1), 0.2), 1, 2, lambda M, K: 0 < s(M)["removed_components"] < s(M)["components"])
    add("one component fills the frame", np.full((2 * H + 3, W + 5), 100), 2, 10,
        lambda M, K: s(M)["components"] == 1 and s(M)["largest"] == K.size and s(M)["removed_pixels"] == 0)
    yy, xx = np.mgrid[0:H + 3, 0:W + 5]
    add("checkerboard: every pixel its own component", 100 + ((yy + xx) % 2) * 4, 3, 2,
        lambda M, K: s(M)["components"] == s(M)["pixels"] == K.size == s(M)["removed_pixels"] and s(M)["largest"] == 1)
    # connection is not transitive
    ramp = 1 + 5 * xx
    add("ramp with steps of exactly max_diff", ramp, 5, 10,
        lambda M, K: s(M)["components"] == 1 and (np.diff(K.astype(int), axis=1) == 5).all() and int(K.max()) - int(K.min()) > 50)
    broken = ramp.copy()
    broken[:, (W + 5) // 2:] += 1
    add("ramp with one step of max_diff + 1", broken, 5, 10,
        lambda M, K: s(M)["components"] == 2 and sorted(set(np.diff(K.astype(int), axis=1).ravel().tolist())) == [5, 6])
    # survival
    bars = np.zeros((7, 20), np.uint16)
    bars[1, 2:13], bars[3, 2:14], bars[5, 2:15] = 50, 50, 50
    add("components of min_size - 1, min_size and min_size + 1", bars, 2, 12,
        lambda M, K: _sizes(M) == [11, 12, 13] and s(M)["removed_components"] == 1 and s(M)["removed_pixels"] == 11)
    # labels that meet late
    u = np.zeros((H + 6, 30), np.uint16)
    u[:, 2], u[:, 20], u[-1, 2:21] = 9, 9, 9
    add("U: two labels until its bottom row", u, 2, 5,
        lambda M, K: s(M)["components"] == 1 and speckle_model(K[:-1], 2, 5)["stats"]["components"] == 2 and len(_tiles_of(K != 0, k)) == 2)
    comb = np.zeros((2 * H + 3, 2 * W + 10), np.uint16)
    comb[:, ::2], comb[-1, :] = 9, 9
    add("comb: teeth that meet in the last row", comb, 2, 5,
        lambda M, K: s(M)["components"] == 1 and speckle_model(K[:-1], 2, 5)["stats"]["components"] == W + 5 and len(_tiles_of(K != 0, k)) == 9)
    # the longest find paths: one path through every tile of a 3 x 3-tile frame
    path = lambda M, K: (s(M)["components"] == 1 and len(_tiles_of(K != 0, k)) == 9 and degree(K).max() == 2
                         and (degree(K)[K != 0] == 1).sum() == 2 and s(M)["largest"] > K.size // 3)
    add("serpentine through 3 x 3 tiles", serpentine((3 * H, 3 * W)), 3, 100, path)
    add("vertical serpentine through 3 x 3 tiles", serpentine((3 * H, 3 * W), vertical=True), 3, 100, path)
    add("spiral through 3 x 3 tiles", spiral((3 * H, 3 * W)), 3, 100, path)
    # roots and seams
    tail = np.zeros((2 * H + 4, 2 * W), np.uint16)
    tail[H + 2:2 * H + 2, W + 4:W + 30] = 300
    tail[3:H + 2, W + 10] = 300
    tail[3, 5:W + 10] = 300
    add("smallest index in another tile than most of the component", tail, 2, 50,
        lambda M, K: s(M)["components"] == 1 and M["root"].max() == 3 * K.shape[1] + 5
        and ((np.nonzero(K)[0] >= H) & (np.nonzero(K)[1] >= W)).mean() > 0.8 and len(_tiles_of(K != 0, k)) == 4)
    for tag, step, comps in (("touch", 6, 1), ("are a key-step apart", 7, 2)):
        seam = np.zeros((2 * H + 2, 2 * W + 2), np.uint16)
        seam[H - 5:H, 10:20] = 400
        seam[H:H + 5, 19:30] = 400 + step                            # meets the block above in column 19 only, across the seam y = H
        seam[2:9, W - 6:W] = 500
        seam[8:12, W:W + 6] = 500 + step                             # meets the block on its left in row 8 only, across the seam x = W
        add(f"two components that {tag} across a seam, both ways", seam, 6, 60,
            lambda M, K, comps=comps: s(M)["components"] == 2 * comps and s(M)["removed_components"] == (0 if comps == 1 else 4)
            and K[H - 1, 19] and K[H, 19] and not K[H, 18] and not K[H - 1, 20] and K[8, W - 1] and K[8, W] and not K[7, W] and not K[9, W - 1])
    corner = np.zeros((2 * H, 2 * W), np.uint16)
    corner[H - 1:H + 1, W - 1:W + 1] = 77
    add("a component across the corner where four tiles meet", corner, 2, 4,
        lambda M, K: s(M)["components"] == 1 and s(M)["largest"] == 4 and len(_tiles_of(K != 0, k)) == 4 and s(M)["removed_pixels"] == 0)
    diag = np.zeros((2 * H, 2 * W), np.uint16)
    diag[H - 3:H, W - 3:W] = 60
    diag[H:H + 3, W:W + 3] = 60                                      # touches the first block at the tiles' corner, diagonally only
    diag[2:4, 2:4] = 60
    diag[4:6, 4:6] = 60                                              # and the same inside a tile
    add("diagonal-only contacts do not connect", diag, 2, 5,
        lambda M, K: s(M)["components"] == 4 and _sizes(M) == [4, 4, 9, 9] and s(M)["removed_pixels"] == 8)
    # launch geometry: either side of the tile's width and height, every cols % 4, one and several workgroups each way
    for r_, c_ in ((H - 1, W - 1), (H, W), (H + 1, W + 1), (H - 1, W + 2), (H + 1, W + 3), (2 * H + 1, 2 * W), (3 * H - 1, 2 * W + 1),
                   (70, 140)):
        add(f"blobs {r_} x {c_}", blobs(3, (r_, c_)), 1, 4,
            lambda M, K: 0 < s(M)["removed_components"] < s(M)["components"] and s(M)["largest"] >= 8 and (K[-1] != 0).any() and (K[:, -1] != 0).any())
    add("dense blobs 70 x 140", blobs(4, (70, 140), 0.05), 3, 30, lambda M, K: s(M)["largest"] > 500 and s(M)["removed_components"] > 10)
    # the ends of the key range
    ends = np.array([[1, 65535, 0, 65535, 1, 1], [0, 0, 0, 0, 0, 0]], np.uint16)
    add("keys 1 and 65535 with max_diff 65534", ends, 65534, 2, lambda M, K: _sizes(M) == [2, 3] and s(M)["removed_pixels"] == 0)
    add("keys 1 and 65535 with max_diff 65533", ends, 65533, 2, lambda M, K: _sizes(M) == [1, 1, 1, 2] and s(M)["removed_pixels"] == 3)
    add("keys 1 and 65535 with max_diff 65535", ends, 65535, 2, lambda M, K: _sizes(M) == [2, 3])
    add("min_size 1 removes nothing", blobs(5, (H + 5, W + 9)), 1, 1,
        lambda M, K: s(M)["removed_pixels"] == 0 and s(M)["removed_components"] == 0 and s(M)["components"] > 50)
    add("min_size above the frame removes everything", blobs(5, (H + 5, W + 9)), 1, 1 << 30,
        lambda M, K: s(M)["removed_pixels"] == s(M)["pixels"] > 0 and s(M)["removed_components"] == s(M)["components"])
    add("max_diff 0", blobs(6, (H + 2, W + 2), 0.1), 0, 3, lambda M, K: 0 < s(M)["removed_components"] < s(M)["components"])
    return out


def row_ids():
    return [r[0] for r in rows()]


@functools.lru_cache(maxsize=None)
def model_of(index, switch=None):
    """The model's result for row `index`; read-only."""
    _, K, max_diff, min_size, _ = rows()[index]
    M = speckle_model(K, max_diff, min_size, **({switch: True} if switch else {}))
    for key in ("keep", "root", "size"):
        M[key].setflags(write=False)
    return M


def differs(index, switch):
    """True iff the switched model leaves other pixels or other counters than the model."""
    a, b = model_of(index), model_of(index, switch)
    return not (np.array_equal(a["keep"], b["keep"]) and a["stats"] == b["stats"])


def diagonal_joins_two_components(index):
    """True iff two diagonal neighbours that differ by at most max_diff lie in different components: worked out of the unswitched
    model's roots, not by running the switch."""
    _, K, max_diff, _, _ = rows()[index]
    v, root = K.astype(np.int64), model_of(index)["root"]
    for (a, b) in ((np.s_[1:, 1:], np.s_[:-1, :-1]), (np.s_[1:, :-1], np.s_[:-1, 1:])):
        if ((K[a] != 0) & (K[b] != 0) & (np.abs(v[a] - v[b]) <= max_diff) & (root[a] != root[b])).any():
            return True
    return False


def has_a_zero_key(index):
    """A zero key that connects is a pixel of some component: the count of components or a size changes wherever there is one."""
    return bool((rows()[index][1] == 0).any())


def a_component_of_exactly_min_size(index):
    return rows()[index][3] in _sizes(model_of(index))


# For each switch of the model, the rows that are in the table to notice it (test_speckle_cpu.py holds the table to this): a list of
# names, or a function of the row's index.
_BLOBS = [f"blobs {r} x {c}" for r, c in ((15, 63), (16, 64), (17, 65), (15, 66), (17, 67), (33, 128), (47, 129), (70, 140))]
CAUGHT_BY = {
    "eight": diagonal_joins_two_components,
    # neighbours exactly max_diff apart whose link is the only one between two parts
    "strict": ["1 x 67", "35 x 1", "ramp with steps of exactly max_diff", "ramp with one step of max_diff + 1",
               "two components that touch across a seam, both ways"] + _BLOBS +
              ["dense blobs 70 x 140", "keys 1 and 65535 with max_diff 65534", "min_size 1 removes nothing",
               "min_size above the frame removes everything", "max_diff 0"],
    "gt": a_component_of_exactly_min_size,
    "zeros_connect": has_a_zero_key,
}
