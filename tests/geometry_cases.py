"""Launch geometries the map, volume and RGB-D front-end kernels are held to (tests/test_geometry_cpu.py, tests/test_gpu_geometry.py):
the launch constants read out of the kernels' headers, the geometry the host code derives from a problem size, the table of rows —
each with the branch it is in the table for, as a predicate on that geometry —, a replay of the volume's tile walk with a switch that
leaves out one carry, the inputs of every row and the numpy models' results for them. Nothing here imports the GPU library.

The models are the ones of tests/test_volume_cpu.py, tests/test_gpu_map.py and tests/test_rgbd_frontend_cpu.py, imported unchanged. A
row's inputs and model results are computed once per process (the 10.5 M-voxel row takes the longest) and shared by both test files."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "odometry_amd", "csrc")
f32 = np.float32


def constants():
    """{kName: value} of every `constexpr int kName = value;` line of the three kernel headers."""
    out = {}
    for name in ("volume.hip.h", "map.hip.h", "rgbd_frontend.hip.h"):
        for m in re.finditer(r"^constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, name)).read(), re.M):
            out[m.group(1)] = int(m.group(2))
    return out


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- the geometry the host code derives -----------------------------------------------------------------------------------------
def volume_geometry(dims, k=None):
    """volume_integrate's tiles / blocks / step digits and volume_extract_dev's block count (volume_api.hip.h)."""
    k = k or constants()
    nx, ny, nz = dims
    tx, ty = _cdiv(nx, k["kVolTileX"]), _cdiv(ny, k["kVolTileY"])
    tiles = tx * ty * nz
    nblk = min(tiles, k["kVolMaxBlocks"])
    ext = _cdiv(nx * ny * nz, k["kVolExtBlock"])
    return dict(dims=tuple(dims), tiles_x=tx, tiles_y=ty, tiles=tiles, nblk=nblk, step_x=nblk % tx, step_y=(nblk // tx) % ty,
                step_k=(nblk // tx) // ty, ext_blocks=ext, scan_chunks=_cdiv(ext, k["kVolScanThreads"]), n=nx * ny * nz,
                max_blocks=k["kVolMaxBlocks"], scan_threads=k["kVolScanThreads"], ext_block=k["kVolExtBlock"],
                tile=(k["kVolTileX"], k["kVolTileY"]))


def map_geometry(size, k=None):
    """odo_map_create's block count and map_scan_kernel's blocks per scan thread (map_api.hip.h, map_kernels.hip)."""
    k = k or constants()
    n = size[0] * size[1]
    nblk = _cdiv(n, k["kMapBlock"])
    per = _cdiv(nblk, k["kMapScanThreads"])
    return dict(size=tuple(size), n=n, nblk=nblk, per=per, scan_busy=_cdiv(nblk, per), block=k["kMapBlock"],
                scan_threads=k["kMapScanThreads"])


def frontend_geometry(depth_size, size, k=None):
    """launch_rgbd_frontend's three grids: gb grey blocks, rb register blocks, sb resolve blocks."""
    k = k or constants()
    nd, n = depth_size[0] * depth_size[1], size[0] * size[1]
    groups = _cdiv(_cdiv(n, 4), k["kFeBlock"])
    return dict(depth_size=tuple(depth_size), size=tuple(size), nd=nd, n=n, gb=groups, rb=min(_cdiv(nd, k["kFeBlock"]), k["kFeRegBlocksMax"]),
                sb=min(groups, k["kFeResBlocksMax"]), block=k["kFeBlock"], reg_max=k["kFeRegBlocksMax"], res_max=k["kFeResBlocksMax"])


# ---- the tile walk of volume_integrate_kernel, replayed -------------------------------------------------------------------------
def walk(g, x_carry=True, y_carry=True):
    """How often each tile (raster order: x tile fastest, then y tile, then k) is visited by the launch of geometry g: block b starts
    at tile b and adds the stride of nblk tiles digit by digit, as vol_next_tile does. x_carry / y_carry False leaves out the `++*ty`
    / the `++*k`. Returns (visits per tile, whether a block was stopped because it would never have left the grid)."""
    tx_n, ty_n, nz = g["tiles_x"], g["tiles_y"], g["dims"][2]
    visits = np.zeros(g["tiles"], np.int64)
    stuck = False
    for b in range(g["nblk"]):
        tx, r0 = b % tx_n, b // tx_n
        ty, k = r0 % ty_n, r0 // ty_n
        left = 8 * (g["tiles"] // g["nblk"] + 2)     # (a walk that is right visits at most ceil(tiles / nblk) tiles per block)
        while k < nz:
            visits[(k * ty_n + ty) * tx_n + tx] += 1
            tx += g["step_x"]
            if tx >= tx_n:
                tx -= tx_n
                ty += 1 if x_carry else 0
            ty += g["step_y"]
            if ty >= ty_n:
                ty -= ty_n
                k += 1 if y_carry else 0
            k += g["step_k"]
            left -= 1
            if left == 0:
                stuck = True
                break
    return visits, stuck


def wrong_tiles(g, **kw):
    """(tx, ty, k) of the tiles the replay does not visit exactly once."""
    visits, _ = walk(g, **kw)
    t = np.nonzero(visits != 1)[0]
    return [(int(i % g["tiles_x"]), int((i // g["tiles_x"]) % g["tiles_y"]), int(i // (g["tiles_x"] * g["tiles_y"]))) for i in t]


def carries_taken(g):
    """(x carries, y carries) the walk as written takes over the whole launch."""
    tx_n, ty_n, nz = g["tiles_x"], g["tiles_y"], g["dims"][2]
    nxc = nyc = 0
    for b in range(g["nblk"]):
        tx, r0 = b % tx_n, b // tx_n
        ty, k = r0 % ty_n, r0 // ty_n
        while k < nz:
            tx += g["step_x"]
            if tx >= tx_n:
                tx, ty, nxc = tx - tx_n, ty + 1, nxc + 1
            ty += g["step_y"]
            if ty >= ty_n:
                ty, k, nyc = ty - ty_n, k + 1, nyc + 1
            k += g["step_k"]
    return nxc, nyc


# The three grids the GPU suite compared with the model before this table existed (tests/test_gpu_volume.py, tests/test_gpu_shapes.py).
EARLIER_VOLUME_GRIDS = [(240, 128, 200), (101, 75, 83), (121, 67, 99)]

# ---- volume rows ----------------------------------------------------------------------------------------------------------------
SIZES = {"300x420": ((300, 420), (310.0, 207.3, 151.8)), "241x423": ((241, 423), (312.0, 210.6, 119.7))}


def _vrow(name, dims, why, holds, kind="rendered", carry=(), **kw):
    return dict(name=name, dims=dims, why=why, holds=holds, kind=kind, carry=carry, **kw)


def _x_and_y_carry(g):
    nxc, nyc = carries_taken(g)
    return g["step_x"] != 0 and nxc > 0 and nyc > 0


# rendered rows: the natural scene's corridor (ground y = 1.65, walls x = -4 and x = 5) seen by a camera that looks slightly down,
# `frames` poses with rotation about all three axes; vs / origin put a surface through the grid. mw = max_weight.
VOLUME = [
    _vrow("150x50x60", (150, 50, 60), "step_x != 0, x- and y-carries both taken", _x_and_y_carry, carry=("x", "y"),
          vs=0.06, origin=(-4.4, -1.0, 1.5), size="300x420", cam=(0.4, -0.3, 0.0), frames=3, mw=65535),
    _vrow("320x21x300", (320, 21, 300), "step_x != 0 with tiles_x odd > 3, ny % 4 != 0, several passes per block",
          lambda g: _x_and_y_carry(g) and g["tiles_x"] % 2 == 1 and g["tiles_x"] > 3 and g["dims"][1] % g["tile"][1] != 0
          and g["tiles"] >= 4 * g["nblk"], carry=("x", "y"),
          vs=0.03, origin=(-4.6, 1.35, 0.5), size="241x423", cam=(0.4, -0.3, 0.0), frames=3, mw=2),
    _vrow("321x77x41", (321, 77, 41), "nx % 64 == 1: one live lane in the last x tile",
          lambda g: _x_and_y_carry(g) and g["dims"][0] % g["tile"][0] == 1, carry=("x", "y"),
          vs=0.01, origin=(-1.6, 1.2, 3.5), size="300x420", cam=(0.1, -0.3, 0.3), frames=2, mw=65535),
    _vrow("700x150x100", (700, 150, 100), "about 20 tiles per block, 10.5 M voxels, the extraction scan's chunk loop runs 11 times",
          lambda g: _x_and_y_carry(g) and g["tiles"] >= 20 * g["nblk"] and g["scan_chunks"] >= 11, carry=("x", "y"),
          vs=0.014, origin=(-4.6, -0.3, 3.0), size="241x423", cam=(0.4, -0.3, 0.3), frames=2, mw=65535),
    _vrow("130x4x683", (130, 4, 683), "tiles == nblk + 1: exactly one block walks twice",
          lambda g: g["tiles"] == g["nblk"] + 1 == g["max_blocks"] + 1 and g["step_x"] != 0, carry=("x", "y"),
          vs=0.01, origin=(-0.65, 1.63, 0.8), size="300x420", cam=(0.1, -0.3, 0.5), frames=2, mw=65535),
    _vrow("192x4x682", (192, 4, 682), "tiles < kVolMaxBlocks: nblk == tiles, nobody walks",
          lambda g: g["tiles"] == g["nblk"] < g["max_blocks"] and g["tiles"] > g["max_blocks"] - 64,
          vs=0.01, origin=(-0.96, 1.63, 0.8), size="241x423", cam=(0.1, -0.3, 0.5), frames=2, mw=65535),
    _vrow("1024x32x32", (1024, 32, 32), "extraction nblk == kVolScanThreads exactly: one full chunk",
          lambda g: g["ext_blocks"] == g["scan_threads"] and g["n"] == g["ext_blocks"] * g["ext_block"],
          vs=0.009, origin=(-4.5, 1.5, 3.0), size="300x420", cam=(0.4, -0.3, 0.3), frames=2, mw=65535),
    _vrow("1024x600x2", (1024, 600, 2), "step_k == 0: a layer holds more tiles than the launch has blocks, k advances by the y-carry alone",
          lambda g: g["step_k"] == 0 and g["step_y"] != 0 and g["tiles_x"] * g["tiles_y"] > g["max_blocks"], carry=("y",),
          vs=0.009, origin=(-4.6, -3.2, 4.0), size="241x423", cam=(0.4, -0.3, 0.3), frames=2, mw=65535),
    # small rows: the 24 x 32 frames of test_volume_cpu.tiny_cases() (a wavy surface 1 m away, holes, 65535s)
    _vrow("64x4x2", (64, 4, 2), "one full tile in x and y", lambda g: g["dims"][:2] == g["tile"] and g["tiles"] == g["nblk"] == g["dims"][2],
          kind="small", vs=0.01, origin=(-0.32, -0.02, 0.99)),
    _vrow("65x5x2", (65, 5, 2), "one voxel spilling into the next tile on both axes",
          lambda g: g["dims"][0] == g["tile"][0] + 1 and g["dims"][1] == g["tile"][1] + 1 and g["tiles"] == g["nblk"],
          kind="small", vs=0.01, origin=(-0.325, -0.025, 0.99)),
    _vrow("2x2x2", (2, 2, 2), "the smallest legal grid: below one tile, one extraction block of 8 voxels",
          lambda g: g["dims"] == (2, 2, 2) and g["tiles"] == 2 and g["ext_blocks"] == 1, kind="small", vs=0.1, origin=(-0.1, -0.1, 0.9)),
] + [
    _vrow(f"tiny{i}", None, "a skip class of tiny_cases(), below one extraction block", lambda g: g["ext_blocks"] == 1 and g["tiles"] == g["nblk"],
          kind="tiny", index=i) for i in range(4)
]


def volume_row(name):
    for r in VOLUME:
        if r["name"] == name:
            return r
    raise KeyError(name)


def _render_depth(size_id, poses, depth_scale, seed):
    from odometry_amd import synth
    (rows, cols), K = SIZES[size_id]
    scene = synth.drive_scene("natural", 0)
    rng = np.random.default_rng(seed)
    out = []
    for A in poses:
        Z = scene.render(A, rows, cols, *K, 0.0)[1]
        raw = synth.sensor_depth(Z, depth_scale, 30.0)
        raw[rng.uniform(size=raw.shape) < 0.03] = 0
        raw[rng.uniform(size=raw.shape) < 0.02] = 65535
        raw[40:80, 100:180] = 0
        out.append((raw, A))
    return out


def volume_inputs(r):
    """(model parameters, [(raw depth frame, camera-to-world pose) ...]) of a volume row."""
    from test_volume_cpu import _pose, params, tiny_cases
    if r["kind"] == "tiny":
        return tiny_cases()[r["index"]]
    if r["kind"] == "small":
        tc = tiny_cases()
        wavy, near = tc[0][1][0][0], tc[0][1][2][0]
        p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=r["dims"], vs=r["vs"], origin=r["origin"], mu=0.05, max_depth=8.0, max_weight=2)
        return p, [(wavy, _pose()), (near, _pose((0.02, -0.03, 0.01), (0.01, 0.02, -0.03))), (wavy, _pose((0.0, 0.01, 0.0), (0.0, 0.0, 0.004)))]
    size, K = SIZES[r["size"]]
    p = params(K, 5000.0, size, dims=r["dims"], vs=r["vs"], origin=r["origin"], mu=0.2, max_depth=8.0, max_weight=r["mw"])
    cx, cy, cz = r["cam"]
    poses = [_pose((-0.2 - 0.03 * n, -0.05 + 0.05 * n, 0.1 + 0.02 * n), (cx - 0.1 * n, cy + 0.02 * n, cz + 0.15 * n)) for n in range(r["frames"])]
    return p, _render_depth(r["size"], poses, 5000.0, 11 + len(r["name"]))


def edge_keys(q, w):
    """The (voxel, axis) keys of the volume's points, voxel * 3 + axis in ascending order: the order of extract_model's output."""
    nz, ny, nx = q.shape
    obs = w > 0
    keys = []
    for c, ax in ((0, 2), (1, 1), (2, 0)):
        sa = [slice(None)] * 3
        sb = [slice(None)] * 3
        sa[ax], sb[ax] = slice(0, -1), slice(1, None)
        sa, sb = tuple(sa), tuple(sb)
        k, j, i = np.nonzero(obs[sa] & obs[sb] & ((q[sa] > 0) != (q[sb] > 0)))
        keys.append(((k.astype(np.int64) * ny + j) * nx + i) * 3 + c)
    return np.sort(np.concatenate(keys))


def mid_voxel_capacity(keys):
    """A capacity that cuts the extraction inside a voxel: the index of the first point of a voxel with >= 2 edges, plus one; None
    when no voxel carries two points."""
    vox = keys // 3
    same = np.nonzero(vox[1:] == vox[:-1])[0]
    if len(same) == 0:
        return None
    pick = same[len(same) // 2]
    while pick > 0 and vox[pick - 1] == vox[pick]:
        pick -= 1
    return int(pick) + 1


_volume_cache = {}


def volume_run(name):
    """The model over a volume row: dict(p, frames, counts [(updated, in band) per frame], first / last = (q, w) after the first / the
    last frame, points = extract_model of the last, keys = edge_keys, mid = mid_voxel_capacity)."""
    if name not in _volume_cache:
        from test_volume_cpu import empty_grid, extract_model, integrate_model
        r = volume_row(name)
        p, frames = volume_inputs(r)
        q, w = empty_grid(p)
        counts, first = [], None
        for raw, A in frames:
            q, w, upd, band = integrate_model(q, w, raw, A, p)
            counts.append((upd, band))
            if first is None:
                first = (q, w)
        keys = edge_keys(q, w)
        _volume_cache[name] = dict(row=r, p=p, frames=frames, counts=counts, first=first, last=(q, w), points=extract_model(q, w, p),
                                   keys=keys, mid=mid_voxel_capacity(keys), geometry=volume_geometry(p["dims"]))
    return _volume_cache[name]


# ---- map rows -------------------------------------------------------------------------------------------------------------------
def _mrow(size, why, holds):
    return dict(size=size, why=why, holds=holds, name=f"{size[0]}x{size[1]}")


MAP = [
    _mrow((1, 1), "one pixel: one live lane in the only wave", lambda g: g["n"] == 1),
    _mrow((1, 63), "below one wave", lambda g: g["n"] < 64),
    _mrow((3, 85), "one lane short of a block", lambda g: g["n"] == g["block"] - 1),
    _mrow((16, 16), "one block exactly", lambda g: g["n"] == g["block"] and g["nblk"] == 1),
    _mrow((1, 257), "one pixel into the second block", lambda g: g["n"] == g["block"] + 1 and g["nblk"] == 2),
    _mrow((512, 512), "nblk == kMapScanThreads: every scan thread busy, per == 1", lambda g: g["nblk"] == g["scan_threads"] and g["per"] == 1),
    _mrow((512, 513), "per steps to 2, about half the scan threads idle",
          lambda g: g["per"] == 2 and g["scan_threads"] < g["nblk"] <= g["scan_threads"] + 2 and g["scan_busy"] <= g["scan_threads"] // 2 + 1),
    _mrow((361, 1243), "n % 64 != 0 in a full-size frame", lambda g: g["n"] % 64 == 19 and g["per"] == 2),
    _mrow((1032, 2056), "per >= 3", lambda g: g["per"] == 9),
]
MAP_RANDOM_BELOW = 10_000      # pixels: smaller frames are random arrays, larger ones renderings of the natural scene
MAP_SPECIAL_SIZES = [(240, 424), (3, 85)]
MAP_VOXEL = 0.05


def map_row(name):
    for r in MAP:
        if r["name"] == name:
            return r
    raise KeyError(name)


def map_K(size):
    rows, cols = size
    if rows * cols < MAP_RANDOM_BELOW:
        return (40.0, (cols - 1) / 2.0, (rows - 1) / 2.0)
    return (718.856 * cols / 1241.0, (cols - 1) / 2.0, (rows - 1) / 2.0)


_map_inputs = {}


def map_inputs(size, n=3):
    """[(mask, inverse depth, image, pose) ...] of n insertions at a frame size. Small frames: random inverse depths (some inside the
    0.01 validity threshold, some zero, some negative), a random mask and image; large ones: the natural scene's semi-dense inverse
    depth, no mask."""
    key = (tuple(size), n)
    if key in _map_inputs:
        return _map_inputs[key]
    from odometry_amd import synth
    from test_volume_cpu import _pose
    rows, cols = size
    out = []
    if rows * cols < MAP_RANDOM_BELOW:
        rng = np.random.default_rng(rows * 10007 + cols)
        for k in range(n):
            dep = rng.uniform(-0.1, 0.6, size).astype(f32)
            u = rng.uniform(size=size)
            dep[u < 0.1] = rng.uniform(-0.0099, 0.0099, size).astype(f32)[u < 0.1]
            dep[(u >= 0.1) & (u < 0.15)] = 0.0
            if rows * cols == 1:
                dep[:] = (0.25, 0.005, 0.4)[k % 3]
            val = (rng.uniform(size=size) < 0.8).astype(np.uint8)
            if rows * cols == 1:
                val[:] = 1
            img = rng.integers(0, 256, size).astype(f32)
            A = _pose((0.02 * k, -0.03 * k, 0.01 * k), (0.05 * k, -0.02 * k, 0.3 * k)).astype(f32)
            out.append((val, dep, img, A))
    else:
        f, cx, cy = map_K(size)
        scene = synth.drive_scene("natural", 0)
        for A in synth.drive_trajectory("natural", n, 0):
            L, Z = scene.render(A, rows, cols, f, cx, cy, 0.0)
            out.append((None, synth.semi_dense_inverse_depth(Z, L), L, np.asarray(A, f32)))
    _map_inputs[key] = out
    return out


def map_capacity(size):
    return 4096 if size[0] * size[1] < MAP_RANDOM_BELOW else 1_000_000


def ref_map(size, capacity, voxel):
    from test_gpu_map import RefMap
    return RefMap(capacity, voxel, cols=size[1], k=map_K(size))


def map_model(size, capacity, voxel, inputs):
    """RefMap after each insertion: [(deep copy of the statistics, number of points)], and the final RefMap."""
    ref = ref_map(size, capacity, voxel)
    trail = []
    for val, dep, img, A in inputs:
        ref.insert(val, dep, img, A)
        trail.append((dict(ref.st), len(ref.xyzi)))
    return trail, ref


def shifted(inputs, by):
    """The same insertions with the poses' translation moved by `by` metres on every axis."""
    out = []
    for val, dep, img, A in inputs:
        B = np.array(A, f32)
        B[:3, 3] += f32(by)
        out.append((val, dep, img, B))
    return out


def with_mask(inputs, seed=5):
    rng = np.random.default_rng(seed)
    return [((rng.uniform(size=dep.shape) < 0.7).astype(np.uint8) if val is None else val, dep, img, A) for val, dep, img, A in inputs]


def survivors(ref, ins):
    """Pixel indices of insertion `ins`'s points in the model's map, ascending."""
    return ref.kp[ref.kp[:, 0] == ins, 1].astype(np.int64)


def capacity_cuts(size):
    """{name: (capacity, insertions)} of the capacity rows at a frame size, from the survivor list of an unbounded model map with
    the filter on: the cut (a) right after the last survivor of a wave, (b) right after the last survivor of a block, both inside the
    first insertion where the frame has more than one wave / block, (c) with room for exactly one point of the second insertion,
    (d) exactly at the end of the second insertion, (e) capacity 1."""
    k = constants()
    inputs = map_inputs(size)
    _, big = map_model(size, 1 << 24, MAP_VOXEL, inputs)
    p0, p1 = survivors(big, 0), survivors(big, 1)

    def boundary(unit, other=None):
        j = np.nonzero(p0[1:] // unit != p0[:-1] // unit)[0]
        if other:
            inner = j[p0[j + 1] // other == p0[j] // other]
            j = inner if len(inner) else j
        return int(j[len(j) // 2]) + 1 if len(j) else len(p0)   # (no boundary inside: the end of the insertion is the unit's end)

    return dict(wave=(boundary(64, k["kMapBlock"]), 3), block=(boundary(k["kMapBlock"]), 3), one=(len(p0) + 1, 3),
                end=(len(p0) + len(p1), 3), single=(1, 2)), (p0, p1)


# ---- front-end rows -------------------------------------------------------------------------------------------------------------
def _frow(depth_size, size, why, holds, tiny=False):
    return dict(depth_size=depth_size, size=size, why=why, holds=holds, tiny=tiny, name=f"{depth_size[0]}x{depth_size[1]}-{size[0]}x{size[1]}")


FRONTEND = [
    _frow((13, 17), (3, 5), "one register block with a partial last wave, one resolve block",
          lambda g: g["rb"] == 1 and g["sb"] == 1 and g["nd"] % 64 != 0, tiny=True),
    _frow((20, 28), (20, 28), "three register blocks, the last one partial", lambda g: g["rb"] == 3 and g["nd"] % g["block"] != 0, tiny=True),
    _frow((171, 224), (480, 640), "fewer register rows than resolve threads: threads of the last block without a row to sum",
          lambda g: 1 < g["rb"] < g["block"] and g["sb"] == g["res_max"]),
    _frow((256, 512), (256, 512), "nd == n == rb * 256: one pass exactly in register and in resolve",
          lambda g: g["rb"] == g["reg_max"] and g["nd"] == g["rb"] * g["block"] and g["n"] == 4 * g["sb"] * g["block"]),
    _frow((257, 511), (255, 514), "one 255-pixel block past a full pass; n % 4 == 2",
          lambda g: g["rb"] == g["reg_max"] and g["nd"] == g["rb"] * g["block"] + g["block"] - 1 and g["n"] % 4 == 2),
    _frow((479, 641), (479, 641), "nd % 64 == 31", lambda g: g["rb"] == g["reg_max"] and g["nd"] % 64 == 31 and g["n"] % 4 == 3),
]
FRONTEND_VARIANTS = ("flipped", "near_plane", "magnify", "scale_out")


def frontend_row(name):
    for r in FRONTEND:
        if r["name"] == name:
            return r
    raise KeyError(name)


_frontend_cache = {}


def frontend_inputs(name, variant=None):
    """dict(rig, colour (4 channels; the first three are the 3-channel frame), raw, scale_in, scale_out) of a front-end row. Full-size
    rows: rig A's extrinsic with the focal lengths scaled to the row, frame 5 of the natural drive. Tiny rows: random readings with
    holes; `variant` one of FRONTEND_VARIANTS, the cases of test_rgbd_frontend_cpu's twin test."""
    key = (name, variant)
    if key in _frontend_cache:
        return _frontend_cache[key]
    from odometry_amd import synth
    from test_rgbd_frontend_cpu import _small_raw, raw_sequence, rig
    r = frontend_row(name)
    (dr, dc), (rows, cols) = r["depth_size"], r["size"]
    if not r["tiny"]:
        assert variant is None
        g = rig(r["depth_size"], 385.0 * dc / 640.0, r["size"], 525.0 * cols / 640.0, (15.0, 0.5, -0.3), (2.0, -3.0, 1.0))
        seq = raw_sequence(g, 6, frames=[5], channels=4, tint_seed=3)
        out = dict(rig=g, colour=seq["colour"][0], raw=seq["raw_depth"][0], scale_in=1000.0, scale_out=1000.0)
    else:
        # the twin test's rig, its depth imager scaled to the row: 30 / 31 pixels focal length at 28 columns, 40 for a target as wide
        fd = 30.0 * dc / 28.0
        g = dict(depth_size=r["depth_size"], depth_K=(fd, fd * 31.0 / 30.0, (dc - 1) / 2.0, (dr - 1) / 2.0), size=r["size"],
                 K=(fd * 4.0 / 3.0 * cols / dc, (cols - 1) / 2.0, (rows - 1) / 2.0),
                 E=synth.rig_extrinsic((0.015, 0.0005, -0.0003), (0.002, -0.003, 0.001)))
        raw = _small_raw(3, dr, dc)
        s_out = 1000.0
        if variant == "flipped":
            g["E"] = synth.rig_extrinsic((0.0, 0.0, 0.0), (0.0, np.pi, 0.0))
        elif variant == "near_plane":
            g["E"] = synth.rig_extrinsic((0.0, 0.0, -1.0), (0.3, 0.2, 0.0))
            raw = _small_raw(4, dr, dc, lo=900, hi=2000)   # (the twin's 1200 would leave nothing in front far enough to land)
        elif variant == "magnify":        # footprints of 4 to 5 pixels, a target half as large again
            g["size"] = (rows * 3 // 2, cols * 3 // 2)
            g["K"] = (fd * 122.0 / 30.0, (g["size"][1] - 1) / 2.0, (g["size"][0] - 1) / 2.0)
        elif variant == "scale_out":
            s_out = 30000.0
        else:
            assert variant is None, variant
        rng = np.random.default_rng(dr * dc + len(variant or ""))
        out = dict(rig=g, colour=rng.integers(0, 256, g["size"] + (4,)).astype(np.uint8), raw=raw, scale_in=1000.0, scale_out=s_out)
    _frontend_cache[key] = out
    return out


def frontend_cases():
    """(row name, variant) of every front-end comparison."""
    out = []
    for r in FRONTEND:
        out.append((r["name"], None))
        if r["tiny"]:
            out += [(r["name"], v) for v in FRONTEND_VARIANTS]
    return out


def frontend_want(name, variant=None):
    from test_rgbd_frontend_cpu import frontend_model
    x = frontend_inputs(name, variant)
    return frontend_model(x["colour"], x["raw"], x["rig"], x["scale_in"], x["scale_out"])
