"""The bilateral depth filter's specification as code (include/odometry_hip.h, odo_depth_filter_create), shared
by tests/test_depth_filter_cpu.py and tests/test_gpu_depth_filter.py: the launch constants read out of the kernel's header, the numpy
model (vectorised, int64), a plain-loop second implementation that tallies which situations it met (and can be told to get one of
three things wrong), the table makers, and the rows — each with the situation it is in the table for as a predicate on the loop's
tallies at the radius it names. Nothing here loads the GPU library.

A row is (name, raw, tables_of, R, predicate): tables_of(radius) gives (ws, wr, shift) for any radius 1 .. 4, so that the GPU test can
run every row at every radius; R is the radius the predicate is about. Frames, model results and loop results are computed once per
process and shared."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "odometry_amd", "csrc")
RADII = (1, 2, 3, 4)
S_BOUND = 4080 * 4095 * 80   # 1 336 608 000: the largest |S| the rule can reach


def constants():
    """{kName: value} of every `constexpr int kName = <integer>;` line of depth_filter.hip.h and depth_filter_math.h."""
    out = {}
    for name in ("depth_filter_math.h", "depth_filter.hip.h"):
        for m in re.finditer(r"^constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, name)).read(), re.M):
            out[m.group(1)] = int(m.group(2))
    return out


def geometry(size, k=None):
    """launch_depth_filter's grid and load path for a frame (8-byte aligned buffers)."""
    k = k or constants()
    rows, cols = size
    return dict(blocks_x=-(-cols // k["kDfTileW"]), blocks_y=-(-rows // k["kDfTileH"]), vec=cols % 4 == 0)


# ---- the model ------------------------------------------------------------------------------------------------------------------
def filter_model(raw, ws, wr, shift):
    """(out uint16, dict(n_valid, n_changed, sum_abs_change)) of one frame; ws is (2R + 1) x (2R + 1)."""
    raw = np.asarray(raw, np.uint16)
    ws, wr, shift = np.asarray(ws, np.int64), np.asarray(wr, np.int64), np.asarray(shift, np.int64)
    R = (ws.shape[0] - 1) // 2
    rows, cols = raw.shape
    c = raw.astype(np.int64)
    pad = np.zeros((rows + 2 * R, cols + 2 * R), np.int64)      # outside the frame: 0, and a 0 never counts
    pad[R:R + rows, R:R + cols] = c
    s = shift[c >> 8]
    S, W = np.zeros_like(c), np.zeros_like(c)
    for dy in range(2 * R + 1):
        for dx in range(2 * R + 1):
            t = pad[dy:dy + rows, dx:dx + cols]
            d = t - c
            k = np.abs(d) >> s
            w = np.where((t != 0) & (k < 256), ws[dy, dx] * wr[np.minimum(k, 255)], 0)
            S += w * d
            W += w
    assert np.abs(S).max(initial=0) <= S_BOUND
    Wd = np.maximum(W, 1)
    q = np.where(S >= 0, (S + Wd // 2) // Wd, -((-S + Wd // 2) // Wd))
    out = np.where(c == 0, 0, c + q)
    assert (W[c != 0] >= 1).all() and out.min(initial=0) >= 0 and out.max(initial=0) <= 65535
    stats = dict(n_valid=int((c != 0).sum()), n_changed=int((out != c).sum()), sum_abs_change=int(np.abs(out - c).sum()))
    return out.astype(np.uint16), stats


def filter_loop(raw, ws, wr, shift, le256=False, toward_zero=False, holes_count=False):
    """The rule read off the prose, one pixel and one tap at a time in Python integers. Returns (out, stats, tallies). The three
    switches are the mutants: `k <= 256` for `k < 256`, the division rounding toward zero, a hole counted as a tap."""
    raw = np.asarray(raw, np.uint16)
    rows, cols = raw.shape
    n = len(ws)
    R = (n - 1) // 2
    px = [[int(v) for v in r] for r in raw]
    ws = [[int(v) for v in r] for r in ws]
    wr, shift = [int(v) for v in wr], [int(v) for v in shift]
    out = np.zeros((rows, cols), np.uint16)
    T = dict(outside=0, holes=0, counted=0, k255=0, k256=0, far=0, centre_zero=0, ties_pos=0, ties_neg=0, max_S=0, min_S=0,
             shifts_used=set(), hole_positions=set(), low_ff=0, low_00=0, zero_ws=0, q_pos=0, q_neg=0, pixels=rows * cols)
    n_valid = n_changed = sum_abs = 0
    for y in range(rows):
        for x in range(cols):
            c = px[y][x]
            if c == 0:
                T["centre_zero"] += 1
                T["hole_positions"].add((0, 0))
                continue
            n_valid += 1
            s = shift[c >> 8]
            T["shifts_used"].add(s)
            T["low_ff"] += (c & 0xFF) == 0xFF
            T["low_00"] += (c & 0xFF) == 0
            S = W = 0
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    yy, xx = y + dy, x + dx
                    if yy < 0 or yy >= rows or xx < 0 or xx >= cols:
                        T["outside"] += 1
                        continue
                    t = px[yy][xx]
                    if t == 0:
                        T["holes"] += 1
                        T["hole_positions"].add((dy, dx))
                        if not holes_count:
                            continue
                    d = t - c
                    k = abs(d) >> s
                    T["k255"] += k == 255
                    T["k256"] += k == 256
                    if k > 256 or (k == 256 and not le256):
                        T["far"] += k > 256
                        continue
                    w = ws[dy + R][dx + R] * wr[min(k, 255)]
                    T["zero_ws"] += ws[dy + R][dx + R] == 0
                    T["counted"] += 1
                    S += w * d
                    W += w
            T["max_S"], T["min_S"] = max(T["max_S"], S), min(T["min_S"], S)
            if W % 2 == 0 and abs(S) % W == W // 2:
                T["ties_pos" if S > 0 else "ties_neg"] += 1
            if toward_zero:
                q = S // W if S >= 0 else -((-S) // W)
            else:
                q = (S + W // 2) // W if S >= 0 else -((-S + W // 2) // W)
            T["q_pos"] += q > 0
            T["q_neg"] += q < 0
            o = c + q
            out[y, x] = o
            n_changed += o != c
            sum_abs += abs(o - c)
    return out, dict(n_valid=n_valid, n_changed=n_changed, sum_abs_change=sum_abs), T


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def default_tables(radius):
    from odometry_amd import api
    return api.depth_filter_tables(radius=radius)


def max_tables(radius):
    n = 2 * radius + 1
    return np.full((n, n), 16, np.uint8), np.full(256, 255, np.uint8), np.full(256, 4, np.uint8)


def identity_tables(radius):
    ws, wr, shift = max_tables(radius)
    ws[:] = 0
    ws[radius, radius] = 1
    return ws, wr, shift


def random_tables(seed, radius):
    rng = np.random.default_rng([0xDF, seed, radius])
    n = 2 * radius + 1
    ws = rng.integers(0, 17, (n, n)).astype(np.uint8)
    ws[radius, radius] = rng.integers(1, 17)
    wr = rng.integers(0, 256, 256).astype(np.uint8)
    wr[0] = rng.integers(1, 256)
    return ws, wr, rng.integers(0, 5, 256).astype(np.uint8)


def flat_shift_tables(s):
    """Every weight large, wr falling from 255 to 128, every shift = s: a tap with k = 255 moves the output, one with k = 256 must not."""
    def of(radius):
        n = 2 * radius + 1
        return np.full((n, n), 16, np.uint8), (255 - np.arange(256) // 2).astype(np.uint8), np.full(256, s, np.uint8)
    return of


def hole_tables(radius):
    """Shift 0 and full weights: a hole read as a tap of value 0 beside a centre below 256 would count."""
    ws, wr, shift = max_tables(radius)
    shift[:] = 0
    return ws, wr, shift


def tie_tables(radius):
    """The centre and its right neighbour with weight 1, wr = 1 everywhere: W = 2 where both count, S = their difference."""
    n = 2 * radius + 1
    ws = np.zeros((n, n), np.uint8)
    ws[radius, radius] = ws[radius, radius + 1] = 1
    return ws, np.ones(256, np.uint8), np.zeros(256, np.uint8)


def sparse_ws_tables(radius):
    """Random tables whose first window row, last window column and (R >= 2) second window column are zero."""
    ws, wr, shift = random_tables(99, radius)
    ws[0, :] = 0
    ws[:, -1] = 0
    if radius >= 2:
        ws[:, 1] = 0
    return ws, np.maximum(wr, 1), shift


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def surface_frame(seed, size, holes=0.1, base=2000):
    """A slanted surface with +-20 raw units of noise and a share of holes: neighbours within the range kernel of one another."""
    rng = np.random.default_rng([0xF7A3E, seed, size[0], size[1]])
    y, x = np.mgrid[0:size[0], 0:size[1]]
    raw = base + 3 * x + 2 * y + rng.integers(-20, 21, size)
    raw[rng.random(size) < holes] = 0
    return raw.astype(np.uint16)


def random_frame(seed, size, holes):
    rng = np.random.default_rng([0xF7A3F, seed])
    raw = rng.integers(1, 65536, size)
    raw[rng.random(size) < holes] = 0
    return raw.astype(np.uint16)


def step_frame(s):
    """Left half c = 1000, right half c + (255 << s) in the upper rows (k = 255: counts) and c + (256 << s) in the lower (k = 256)."""
    raw = np.full((12, 16), 1000, np.int64)
    raw[:6, 8:] = 1000 + (255 << s)
    raw[6:, 8:] = 1000 + (256 << s)
    return raw.astype(np.uint16)


def shift_change():
    """(j, frame): the default tables' shift steps between centres 256 j - 1 and 256 j; the frame holds both, and values round them."""
    shift = default_tables(2)[2]
    j = int(np.flatnonzero(np.diff(shift.astype(int)) != 0)[1]) + 1
    rng = np.random.default_rng(0x5C)
    raw = 256 * j + rng.integers(-40, 41, (12, 24))
    raw[::2, ::3] = 256 * j - 1
    raw[1::2, 1::3] = 256 * j
    return j, raw.astype(np.uint16)


def bound_frame(sign):
    """9 x 9: the centre c against 80 neighbours c + 4095 (sign +1) or c - 4095 (sign -1): with max_tables at R = 4, S = +-S_BOUND."""
    lo, hi = 1000, 1000 + 4095
    raw = np.full((9, 9), hi if sign > 0 else lo, np.uint16)
    raw[4, 4] = lo if sign > 0 else hi
    return raw


def tie_frame():
    raw = np.tile(np.array([100, 101, 100, 99], np.uint16), (3, 5))   # right neighbour +1, -1, -1, +1, ...
    return raw


def single_hole_frame():
    """17 x 17 round 200 (centres below 256) with one hole in the middle: round it, the hole sits at every tap of every window."""
    rng = np.random.default_rng(0x401E)
    raw = 200 + rng.integers(-5, 6, (17, 17))
    raw[8, 8] = 0
    return raw.astype(np.uint16)


# ---- the rows ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows():
    k = constants()
    TW, TH = k["kDfTileW"], k["kDfTileH"]
    out = []

    def add(name, raw, tables_of, R, pred):
        out.append((name, np.ascontiguousarray(raw, np.uint16), tables_of, R, pred))

    def sized(size, R=2, extra=lambda T, g: True, tag=None, holes=0.1):
        g = geometry(size, k)
        add(tag or f"{size[0]}x{size[1]}", surface_frame(1, size, holes), default_tables, R,
            lambda T, g=g, size=size: T["pixels"] == size[0] * size[1] and T["outside"] > 0 and extra(T, g))

    sized((1, 1), extra=lambda T, g: T["counted"] == 1, holes=0.0)
    sized((1, 64), extra=lambda T, g: g["blocks_x"] == 1 and g["vec"])
    sized((64, 1), extra=lambda T, g: g["blocks_y"] == 64 // TH and not g["vec"])
    sized((2, 3), R=4, tag="2x3 smaller than R = 3, 4")
    sized((3, 9), R=4, tag="3x9 shorter than R = 4")
    sized((9, 2), R=3, tag="9x2 narrower than R = 3")
    for dr, dc in ((0, -1), (0, 0), (0, 1), (-1, 0), (1, 0), (1, 1)):
        size = (TH + dr, TW + dc)
        sized(size, extra=lambda T, g, size=size: (g["blocks_y"], g["blocks_x"]) == (1 + (size[0] > TH), 1 + (size[1] > TW)),
              tag=f"tile {TH}{dr:+d} x {TW}{dc:+d}")
    for m in (1, 2, 3):
        sized((5 + m, TW + 4 + m), extra=lambda T, g, m=m: not g["vec"] and (TW + 4 + m) % 4 == m, tag=f"cols % 4 == {m}")
    sized((17, 23), R=3)
    sized((120, 160), extra=lambda T, g: g["vec"] and g["blocks_x"] * g["blocks_y"] > 16 and T["holes"] > 0)
    for share in (30, 90):
        add(f"random frame, {share} % holes", random_frame(share, (33, 70), share / 100), lambda r, share=share: random_tables(share, r), 3,
            lambda T: T["holes"] > 0 and T["far"] > 0 and T["counted"] > T["pixels"] - T["centre_zero"] and T["q_pos"] and T["q_neg"])
    add("all zero", np.zeros((20, 68), np.uint16), default_tables, 2, lambda T: T["centre_zero"] == T["pixels"] and T["counted"] == 0)
    add("all 65535", np.full((20, 68), 65535, np.uint16), max_tables, 2,
        lambda T: T["centre_zero"] == 0 and T["max_S"] == 0 == T["min_S"] and T["far"] == 0)
    for s in range(5):
        add(f"step of 255 << {s} and 256 << {s}", step_frame(s), flat_shift_tables(s), 2,
            lambda T, s=s: T["k255"] > 0 and T["k256"] > 0 and T["shifts_used"] == {s})
    j, raw = shift_change()
    add(f"centres {256 * j - 1} and {256 * j} across a change of shift", raw, default_tables, 2,
        lambda T: len(T["shifts_used"]) == 2 and T["low_ff"] > 0 and T["low_00"] > 0)
    for R in RADII:
        add(f"a hole at every tap, R = {R}", single_hole_frame(), hole_tables, R,
            lambda T, R=R: len(T["hole_positions"]) == (2 * R + 1) ** 2 and T["centre_zero"] == 1)
    add("the overflow bound, S = +1 336 608 000", bound_frame(+1), max_tables, 4, lambda T: T["max_S"] == S_BOUND)
    add("the overflow bound, S = -1 336 608 000", bound_frame(-1), max_tables, 4, lambda T: T["min_S"] == -S_BOUND)
    add("ties at W / 2 in both signs", tie_frame(), tie_tables, 1, lambda T: T["ties_pos"] > 0 and T["ties_neg"] > 0)
    add("ws with zero rows and columns", surface_frame(7, (19, 37)), sparse_ws_tables, 3,
        lambda T: T["zero_ws"] > 0 and T["counted"] > T["zero_ws"])
    return out


def row_ids():
    return [r[0] for r in rows()]


@functools.lru_cache(maxsize=None)
def model_of(index, radius):
    """(out, stats) of row `index` at `radius`, from the vectorised model; read-only."""
    _, raw, tables_of, _, _ = rows()[index]
    out, stats = filter_model(raw, *tables_of(radius))
    out.setflags(write=False)
    return out, stats


@functools.lru_cache(maxsize=None)
def loop_of(index, radius):
    _, raw, tables_of, _, _ = rows()[index]
    out, stats, T = filter_loop(raw, *tables_of(radius))
    out.setflags(write=False)
    return out, stats, T


# ---- the noise case: the ribbed corridor of DESIGN.md section 9.8 with the Kinect axial model ------------------------------------------
NOISE_SEED = 7


@functools.lru_cache(maxsize=None)
def ribbed_scene():
    from odometry_amd import synth
    from test_volume_icp_cpu import RIBBED_SCENE
    return synth.Scene(0, **RIBBED_SCENE)


def ribbed_frame(k, size, noise_seed=None):
    """(Z metres, uint16 sensor frame) of frame k of the ribbed corridor at `size` (TUM intrinsics scaled), clean or with sensor noise."""
    from odometry_amd import synth
    scale = synth.TUM_ROWS // size[0]
    scene = ribbed_scene()
    T = synth.trajectory(k + 1, 0, fwd_range=(0.1, 0.2), max_offset=1.0)[k]
    Z = scene.render(T, size[0], size[1], synth.TUM_F / scale, synth.TUM_CX / scale, synth.TUM_CY / scale)[1]
    Zn = Z if noise_seed is None else synth.sensor_noise(Z, *synth.depth_noise_rng(noise_seed, k))
    return Z, synth.sensor_depth(Zn, 1000.0, 30.0)


def rms_against_clean(frame, clean, Z):
    """RMS of frame - clean in raw units over the pixels with Z <= 5 m that have a reading in both."""
    m = (Z <= 5.0) & (frame != 0) & (clean != 0)
    d = frame[m].astype(np.float64) - clean[m].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))
