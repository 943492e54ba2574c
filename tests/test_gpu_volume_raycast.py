"""The ray-cast of the TSDF volume on the GPU (odo_volume_raycast_dev, odo_volume_raycast, api.TsdfVolume.raycast) against the numpy
model of tests/test_volume_raycast_cpu.py: depth, raw, normals and colours bit for bit, with no tolerance anywhere, across frame sizes
round the launch tile, grids, every pose class of the model's branch rows, the pinned case, coloured volumes, every subset of
outputs, the volume's state round a ray-cast, the refusals and a volume attached to an RgbdTracker mid-drive."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_gpu_volume import _grid_equal, _run, _standalone, _tracker, _volume, second_rig
from test_rgbd_cpu import drive
from test_volume_colour_cpu import empty_colour, integrate_colour_model, random_frame
from test_volume_cpu import _pose, bits, empty_grid, integrate_model, params
from test_volume_mesh_cpu import grid_params, random_grid
from test_volume_raycast_cpu import (EXACT, branch_rows, default_view, frames_equal, plane_grid, random_volume, raycast_model, tiny_volumes,
                                     view)

pytestmark = pytest.mark.gpu
f32 = np.float32
NAMES = ("depth", "raw", "nrmw", "rgba")


@pytest.fixture(scope="module")
def seq():
    return drive()


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _uploaded(ctx, p, q, w, col=None):
    vol = _volume(ctx, p)
    vol.upload(q, w)
    if col is not None:
        vol.enable_colour(3, False, 255)
        vol.upload_colour(col)
    return vol


def _cast(vol, pose, rp, colour):
    """The host call: (depth, raw, nrmw, rgba), rgba zeros for a volume without colour (what the model returns for it)."""
    got = vol.raycast(pose, size=rp["size"], K=rp["K"], t_min=rp["t_min"], step=rp["step"], n_steps=rp["n_steps"], raw=True, colour=colour)
    depth, nrmw, raw = got[:3]
    rgba = got[3] if colour else np.zeros(depth.shape + (4,), np.uint8)
    assert depth.dtype == f32 and raw.dtype == np.uint16 and nrmw.dtype == f32 and rgba.dtype == np.uint8
    return depth, raw, nrmw, rgba


def _check(vol, q, w, col, pose, p, rp, tag):
    want = raycast_model(q, w, col, pose, p, rp)
    frames_equal(_cast(vol, pose, rp, col is not None), want, tag)
    return want


def _c_params(rp):
    from odometry_amd import _lib as L
    return L.RaycastParams(rp["size"][0], rp["size"][1], *rp["K"], rp["t_min"], rp["step"], rp["n_steps"])


def _cast_dev(ctx, vol, pose, rp, which):
    """odo_volume_raycast_dev into buffers of the caller filled with 0xAB bytes beforehand: {name: array} of the outputs asked for."""
    rows, cols = rp["size"]
    shapes = dict(depth=((rows, cols), f32), raw=((rows, cols), np.uint16), nrmw=((rows, cols, 4), f32), rgba=((rows, cols, 4), np.uint8))
    dev = {k: ctx.upload(np.full(shapes[k][0], 0xAB, np.uint8).repeat(np.dtype(shapes[k][1]).itemsize)) for k in which}
    A = np.ascontiguousarray(np.asarray(pose, f32).T).reshape(16)
    st = vol.lib.odo_volume_raycast_dev(vol.h, C.byref(_c_params(rp)), A.ctypes.data_as(C.POINTER(C.c_float)), *[dev.get(k) for k in NAMES])
    vol.sync()                                                             # odo_volume_sync covers the ray-cast
    out = {k: ctx.download(dev[k], *shapes[k]) for k in which}
    for h in dev.values():
        ctx.free(h)
    return st, out


# ---- frame sizes round the launch tile (a wave is 8 x 8 pixels, a block 16 x 16) ------------------------------------------------------
SIZES = [(1, 1), (8, 8), (9, 8), (8, 9), (16, 16), (17, 16), (16, 17), (17, 23), (64, 1), (1, 64), (65, 33)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_sizes_round_the_launch_tile(ctx, size):
    p, q, w, col, poses = tiny_volumes()[3]
    rows, cols = size
    f = 1.3 * max(rows, cols)                                              # looking 0.3 / 0.2 off the axis: past the hole in the middle
    rp = view(size, (f, (cols - 1) / 2 - 0.3 * f, (rows - 1) / 2 - 0.2 * f), 0.0, 0.15, 30)
    vol = _uploaded(ctx, p, q, w, col)
    hits = 0
    for pose in poses:
        want = _check(vol, q, w, col, pose, p, rp, f"{size}")
        hits += int((want[0] > 0).sum())
        st, dev = _cast_dev(ctx, vol, pose, rp, NAMES)                     # every pixel and nothing else is written
        assert st == 0
        frames_equal([dev[k] for k in NAMES], want, f"{size} dev")
    assert hits > 0
    vol.close()


# ---- grids ---------------------------------------------------------------------------------------------------------------------------
def test_two_by_two_by_two(ctx):
    p = grid_params((2, 2, 2), vs=0.5, origin=(-0.5, -0.5, 0.5))
    hits = 0
    for seed in range(4):
        q, w = random_grid((2, 2, 2), seed)
        q[0] = np.abs(q[0])
        q[1] = -np.abs(q[1])                                               # a surface between the two layers
        vol = _uploaded(ctx, p, q, w)
        for pose in (_pose(), _pose((0.1, -0.2, 0.3), (0.1, 0.05, 0.2))):
            rp = view((12, 16), (20.0, 7.5, 5.5), 0.0, 0.05, 40)
            hits += int((_check(vol, q, w, None, pose, p, rp, f"2x2x2 seed {seed}")[0] > 0).sum())
        vol.close()
    assert hits > 50


def test_tiny_volumes_from_their_own_poses(ctx):
    hits = zero = 0
    for n, (p, q, w, col, poses) in enumerate(tiny_volumes()):
        vol = _uploaded(ctx, p, q, w, col)
        for k, pose in enumerate(poses):                                   # the 3e38 poses among them: inf / NaN positions, all invalid
            want = _check(vol, q, w, col, pose, p, default_view(p, n_steps=30), f"tiny {n} pose {k}")
            hits += int((want[0] > 0).sum())
            zero += int(((want[0] > 0) & (want[2][..., 3] == 0)).sum())
        vol.close()
    assert hits > 500 and zero > 0


@pytest.mark.parametrize("dims", [(9, 8, 7), (65, 5, 2)], ids=lambda d: "x".join(map(str, d)))
def test_uploaded_random_grids(ctx, dims):
    hits = coloured = 0
    for seed in range(3):
        p, q, w, col = random_volume(dims, seed)
        vol = _uploaded(ctx, p, q, w, col)
        centre = (np.asarray(p["origin"]) + 0.5 * p["vs"] * np.asarray(dims)).tolist()
        for pose, step in ((_pose((0.05 * seed, -0.1, 0.02), (0.0, 0.01, 0.0)), 0.02), (_pose((0.4, 0.3, -0.2), (-0.3, -0.25, 0.2)), 0.07),
                           (_pose((0.0, 0.3, 0.0), (centre[0] - 0.2, centre[1], centre[2] - 0.6)), 0.011)):
            want = _check(vol, q, w, col, pose, p, view((24, 32), (30.0, 15.5, 11.5), 0.0, step, 80), f"{dims} seed {seed}")
            hits += int((want[0] > 0).sum())
            coloured += int((want[3][..., 3] > 0).sum())
        vol.close()
    print(f"{dims}: {hits} hits, {coloured} coloured")
    assert hits > 100 and 0 < coloured < hits


# ---- poses ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", branch_rows(), ids=lambda r: r[0])
def test_every_pose_class_of_the_models_rows(ctx, row):
    name, p, q, w, col, pose, rp, _ = row
    vol = _uploaded(ctx, p, q, w, col)
    _check(vol, q, w, col, pose, p, rp, name)
    vol.close()


def test_looking_away_far_off_and_a_step_longer_than_the_grid(ctx):
    p, q, w = plane_grid(**EXACT)
    vol = _uploaded(ctx, p, q, w)
    size, K = (20, 28), (25.0, 13.5, 9.5)
    away = _check(vol, q, w, None, _pose((0.0, np.pi, 0.0), (0.0, 0.0, 0.3)), p, view(size, K, 0.0, 0.05, 100), "looking away")
    assert not away[0].any() and not away[2].any()
    # from 1 000 m a pixel of f = 2 000 is 0.5 m wide: the principal ray and its neighbours on one side reach the grid and find the plane
    far = _check(vol, q, w, None, _pose(t=(0.0, 0.0, -1000.0)), p, view(size, (2000.0, 14.0, 10.0), 999.0, 0.05, 100), "1 000 m off")
    assert (far[0] > 1000).any() and far[0][10, 14] > 1000
    long = _check(vol, q, w, None, _pose(), p, view(size, K, 0.0, 2.5, 10), "a step longer than the grid")
    assert not long[0].any()                                               # one sample inside at most: never two to bracket a crossing
    wide = _check(vol, q, w, None, _pose(), p, view(size, K, 0.5, 1.0, 3), "samples either side of the surface, a cell apart")
    assert (wide[0] > 0).any()
    vol.close()


# ---- the pinned case -----------------------------------------------------------------------------------------------------------------
PINNED_VIEWS = ["pose 0", "pose 9", "rotated", "120x160"]


@pytest.fixture(scope="module")
def pinned_grids(seq):
    """The pinned case (true poses) after 1 and 10 integrations: {n: (q, w)} and the parameters."""
    p = params(seq)
    q, w = empty_grid(p)
    out = {}
    for k in range(10):
        q, w, _, _ = integrate_model(q, w, seq["depth"][k], seq["poses"][k], p)
        if k + 1 in (1, 10):
            out[k + 1] = (q, w)
    return p, out


@pytest.fixture(scope="module")
def pinned_volumes(ctx, pinned_grids):
    p, grids = pinned_grids
    vols = {n: _uploaded(ctx, p, q, w) for n, (q, w) in grids.items()}
    yield vols
    for v in vols.values():
        v.close()


@pytest.mark.parametrize("which", PINNED_VIEWS)
@pytest.mark.parametrize("n", [1, 10])
def test_pinned_case_matches_the_model_bit_for_bit(seq, pinned_grids, pinned_volumes, n, which):
    p, grids = pinned_grids
    q, w = grids[n]
    rp = default_view(p, n_steps=140)
    pose = seq["poses"][9 if which == "pose 9" else 0]
    if which == "rotated":                                                 # off the path: turned towards a wall and the floor, moved aside
        pose = np.asarray(seq["poses"][4], np.float64) @ _pose((0.25, -0.4, 0.1), (0.3, -0.2, 0.1))
    if which == "120x160":
        f, cx, cy = p["K"]
        rp = default_view(p, n_steps=140, size=(120, 160), K=(f / 4, (cx - 1.5) / 4, (cy - 1.5) / 4))
    want = _check(pinned_volumes[n], q, w, None, pose, p, rp, f"pinned after {n}, {which}")
    hit = want[0] > 0
    print(f"after {n}, {which}: {int(hit.sum())} hits of {hit.size}, {int((hit & (want[2][..., 3] == 0)).sum())} without a normal")
    assert hit.sum() > 1000


# ---- colour --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cmax", [255, 3])
def test_second_rig_coloured(ctx, cmax):
    p, frames = second_rig()
    vol = _volume(ctx, p)
    vol.enable_colour(4, True, cmax)
    q, w = empty_grid(p)
    col = empty_colour(p)
    for n, (raw, A) in enumerate(frames):
        frame = random_frame(p, 4, 31 + n)
        vol.integrate(raw, A, colour=frame)
        q, w, col, _, _, _ = integrate_colour_model(q, w, col, raw, frame, A, p, 4, True, cmax)
    rows, cols = p["size"]
    f, cx, cy = p["K"]
    rp = default_view(p, size=(rows // 4, cols // 4), K=(f / 4, (cx - 1.5) / 4, (cy - 1.5) / 4))
    for k in (0, 5):
        want = _check(vol, q, w, col, frames[k][1], p, rp, f"second rig, colour weight {cmax}, pose {k}")
        hit = want[0] > 0
        assert hit.sum() > 300 and (want[3][hit][:, 3] == 255).any() and (want[3][~hit] == 0).all()
    vol.close()


# ---- outputs and state -----------------------------------------------------------------------------------------------------------------
def test_every_subset_of_outputs_equals_the_full_call(ctx):
    p, q, w, col = random_volume((9, 8, 7), 2)
    vol = _uploaded(ctx, p, q, w, col)
    pose, rp = _pose((0.05, -0.1, 0.02), (0.0, 0.01, 0.0)), view((19, 21), (30.0, 10.0, 9.0), 0.0, 0.02, 60)
    want = dict(zip(NAMES, raycast_model(q, w, col, pose, p, rp)))
    assert (want["depth"] > 0).sum() > 20
    for r in range(5):
        for which in itertools.combinations(NAMES, r):
            st, got = _cast_dev(ctx, vol, pose, rp, which)
            assert st == 0, which
            frames_equal([got[k] for k in which], [want[k] for k in which], f"outputs {which}")
    # raw against the formula
    assert np.array_equal(want["raw"], np.where(want["depth"] > 0, np.minimum(f32(65535.0), np.rint(want["depth"] * f32(p["depth_scale"]))), 0))
    # the host call with fewer outputs
    A = np.ascontiguousarray(np.asarray(pose, f32).T).reshape(16)
    raw = np.zeros(rp["size"], np.uint16)
    assert vol.lib.odo_volume_raycast(vol.h, C.byref(_c_params(rp)), A.ctypes.data_as(C.POINTER(C.c_float)), None,
                                      raw.ctypes.data_as(C.POINTER(C.c_uint16)), None, None) == 0
    assert np.array_equal(raw, want["raw"])
    vol.close()


def test_grid_and_counters_are_unchanged_and_empty_volumes_give_zeros(ctx, seq):
    p = params(seq, dims=(32, 16, 24), vs=0.08, origin=(-1.28, 0.9, 3.6))   # the ground, 3.6 to 5.5 m ahead, crosses it
    vol = _volume(ctx, p)
    vol.enable_colour(3, False, 255)
    rp = default_view(p, size=(60, 80), K=(p["K"][0] / 8, (p["K"][1] - 3.5) / 8, (p["K"][2] - 3.5) / 8))
    empty = _check(vol, *empty_grid(p), empty_colour(p), seq["poses"][0], p, rp, "empty")
    assert not any(a.any() for a in empty)
    q, w = empty_grid(p)
    col = empty_colour(p)
    from odometry_amd import synth
    for k in range(2):
        frame = synth.colour_from_gray(seq["gray"][k], 3, False, tint_seed=1)
        vol.integrate(seq["depth"][k], seq["poses"][k], colour=frame)
        q, w, col, _, _, _ = integrate_colour_model(q, w, col, seq["depth"][k], frame, seq["poses"][k], p)
    before = vol.stats()
    want = _check(vol, q, w, col, seq["poses"][1], p, rp, "two frames")
    assert (want[0] > 0).sum() > 50 and (want[3][..., 3] == 255).sum() > 50
    assert vol.stats() == before
    _grid_equal(vol, q, w, "after the ray-casts")
    assert np.array_equal(vol.colour_grid(), col)
    # an integration behind a ray-cast that has not been waited for is ordered behind it, and the next ray-cast behind that
    d = ctx.upload(seq["depth"][2])
    st, first = _cast_dev_nowait(ctx, vol, seq["poses"][1], rp)
    vol.integrate(d, seq["poses"][2])
    q2, w2, _, _ = integrate_model(q, w, seq["depth"][2], seq["poses"][2], p)
    second = _cast(vol, seq["poses"][1], rp, True)
    frames_equal([first()], [want[0]], "a ray-cast in front of an integration")
    frames_equal(second, raycast_model(q2, w2, col, seq["poses"][1], p, rp), "a ray-cast behind an integration")
    ctx.free(d)
    vol.clear()
    cleared = _cast(vol, seq["poses"][1], rp, True)
    assert not any(a.any() for a in cleared)
    vol.close()


def _cast_dev_nowait(ctx, vol, pose, rp):
    """The depth output only, not waited for: (status, a function that waits, downloads and frees)."""
    rows, cols = rp["size"]
    dev = ctx.upload(np.full((rows, cols), np.nan, f32))
    A = np.ascontiguousarray(np.asarray(pose, f32).T).reshape(16)
    st = vol.lib.odo_volume_raycast_dev(vol.h, C.byref(_c_params(rp)), A.ctypes.data_as(C.POINTER(C.c_float)), dev, None, None, None)
    assert st == 0

    def finish():
        vol.sync()
        out = ctx.download(dev, (rows, cols), f32)
        ctx.free(dev)
        return out
    return st, finish


def test_refusals_enqueue_nothing(ctx):
    from odometry_amd import _lib as L
    p, q, w, _ = random_volume((9, 8, 7), 0)
    vol = _uploaded(ctx, p, q, w)                                          # no colour grid
    rp = view((12, 16), (30.0, 7.5, 5.5), 0.0, 0.02, 40)
    before = vol.stats()
    with pytest.raises(L.OdoError, match="no colour grid"):
        vol.raycast(_pose(), size=rp["size"], K=rp["K"], step=0.02, n_steps=40, colour=True)
    st, got = _cast_dev(ctx, vol, _pose(), rp, ("depth", "rgba"))
    assert st == -1 and "no colour grid" in L.last_error()
    assert (got["depth"].view(np.uint8) == 0xAB).all() and (got["rgba"] == 0xAB).all()   # nothing was written
    for bad in (dict(n_steps=0), dict(n_steps=4097), dict(step=0.0), dict(step=float("nan")), dict(t_min=-1.0), dict(size=(0, 16)),
                dict(size=(12, 4097)), dict(K=(0.0, 7.5, 5.5)), dict(K=(30.0, float("inf"), 5.5))):
        st, got = _cast_dev(ctx, vol, _pose(), dict(rp, **bad), ())
        assert st == -1 and "odo_volume_raycast_dev" in L.last_error(), bad
        with pytest.raises(L.OdoError, match="odo_volume_raycast:"):
            vol.raycast(_pose(), **dict(rp, **bad))
    for v in (np.nan, np.inf, -np.inf):
        A = np.eye(4, dtype=f32)
        A[1, 3] = v
        st, got = _cast_dev(ctx, vol, A, rp, ("depth",))
        assert st == -1 and "non-finite" in L.last_error() and (got["depth"].view(np.uint8) == 0xAB).all()
        with pytest.raises(L.OdoError, match="non-finite"):
            vol.raycast(A, size=rp["size"], K=rp["K"], step=0.02, n_steps=40)
    assert vol.stats() == before
    _grid_equal(vol, q, w, "after the refused calls")
    frames_equal(_cast(vol, _pose(), rp, False), raycast_model(q, w, None, _pose(), p, rp), "after the refused calls")
    vol.close()


def test_defaults_of_the_python_call(ctx):
    p, q, w, col, poses = tiny_volumes()[3]
    vol = _uploaded(ctx, p, q, w)
    rp = default_view(p)                                                   # the volume's size and K, mu / 2, reaching max_depth + mu
    c = vol.raycast_params()
    assert (c.rows, c.cols) == p["size"] and c.n_steps == rp["n_steps"] and f32(c.step) == f32(rp["step"]) and c.t_min == 0.0
    assert rp["step"] * (rp["n_steps"] - 1) >= p["max_depth"] + p["mu"] > rp["step"] * (rp["n_steps"] - 2)
    depth, nrmw = vol.raycast(poses[0])
    frames_equal([depth, nrmw], [raycast_model(q, w, None, poses[0], p, rp)[k] for k in (0, 2)], "defaults")
    vol.close()


# ---- attached to a tracker -----------------------------------------------------------------------------------------------------------
def test_raycast_of_an_attached_volume_mid_drive(seq):
    p = params(seq)
    plain = _tracker(seq)
    want_rows = _run(plain, [(plain.upload_frame(g), plain.upload_depth(d)) for g, d in zip(seq["gray"][:6], seq["depth"][:6])], False)
    plain.close()
    trk = _tracker(seq)
    vol = _volume(trk, p)
    trk.attach_volume(vol)
    dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"][:6], seq["depth"][:6])]
    f, cx, cy = p["K"]
    rp = default_view(p, n_steps=140, size=(120, 160), K=(f / 4, (cx - 1.5) / 4, (cy - 1.5) / 4))
    trk.init(*dev[0])
    rows = [dict(abs_pose=np.eye(4, dtype=f32), solve_status=0)]
    casts = {}
    for k in range(1, 6):
        rows.append(trk.track(*dev[k]))
        if k in (3, 5):                                                    # behind the integrations enqueued so far, the drive goes on
            casts[k] = _cast(vol, rows[k]["abs_pose"], rp, False)
    for k in range(1, 6):
        for key in ("pose_to_keyframe", "abs_pose"):
            assert np.array_equal(bits(rows[k][key]), bits(want_rows[k][key])), f"frame {k}: {key} differs"
        assert rows[k]["new_keyframe"] == want_rows[k]["new_keyframe"] and rows[k]["solve_status"] == 0
    for k, got in casts.items():
        ref = _standalone(trk, p, dev[:k + 1], rows[:k + 1])
        frames_equal(got, _cast(ref, rows[k]["abs_pose"], rp, False), f"attached after {k + 1} frames against a standalone volume")
        q, w = ref.grid()
        frames_equal(got, raycast_model(q, w, None, rows[k]["abs_pose"], p, rp), f"attached after {k + 1} frames against the model")
        assert (got[0] > 0).sum() > 1000
        ref.close()
    assert vol.stats()["frames"] == 6
    vol.close()
    trk.close()
