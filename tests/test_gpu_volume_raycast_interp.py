"""The trilinear colour sampling of the volume's ray-cast on the GPU (odo_volume_set_colour_sampling, api.TsdfVolume
.set_colour_sampling) against the numpy model of tests/volume_raycast_interp_cases.py: every output bit for bit, with no tolerance
anywhere, into buffers pre-filled with 0xAB, across frame sizes round the launch tile, grids, the last cell of a grid, every branch
row, the handling of the mode, the pinned coloured case, track(grey=...) under the mode, the volume's state round a ray-cast, a volume
attached to an RgbdTracker mid-drive and the refusals."""
import itertools

import numpy as np
import pytest

import volume_icp_photo_cases as pc
import volume_raycast_interp_cases as ic
from test_gpu_volume import _grid_equal, _volume
from test_gpu_volume_raycast import NAMES, _cast, _cast_dev, _uploaded
from test_rgbd_cpu import drive
from test_volume_cpu import _pose, bits, params
from test_volume_icp_cpu import pose_error
from test_volume_mesh_cpu import grid_params, random_grid
from test_volume_colour_cpu import random_colour
from test_volume_raycast_cpu import default_view, frames_equal, random_volume, raycast_model, tiny_volumes, view
from test_volume_raycast_interp_cpu import (MEASURED_CORRIDOR_R_DEG, MEASURED_CORRIDOR_T_M, MEASURED_RIBBED_R_DEG, MEASURED_RIBBED_T_M,
                                            TRILINEAR_LINES)

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _trilinear(ctx, p, q, w, col):
    vol = _uploaded(ctx, p, q, w, col)
    assert vol.colour_sampling == "nearest"                                # the state at create
    vol.set_colour_sampling("trilinear")
    assert vol.colour_sampling == "trilinear"
    return vol


def _check(ctx, vol, q, w, col, pose, p, rp, tag):
    """The host call and odo_volume_raycast_dev (into buffers pre-filled with 0xAB) against the model of the trilinear mode."""
    want = ic.raycast_interp_model(q, w, col, pose, p, rp)
    frames_equal(_cast(vol, pose, rp, True), want, tag)
    st, dev = _cast_dev(ctx, vol, pose, rp, NAMES)
    assert st == 0
    frames_equal([dev[k] for k in NAMES], want, tag + " dev")
    return want


# ---- frame sizes round the launch tile (a wave is 8 x 8 pixels, a block 16 x 16) ------------------------------------------------------
SIZES = [(1, 1), (8, 8), (9, 8), (8, 9), (16, 16), (17, 16), (16, 17), (17, 23), (64, 1), (1, 64), (65, 33)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_sizes_round_the_launch_tile(ctx, size):
    p, q, w, col, poses = tiny_volumes()[3]
    rows, cols = size
    f = 1.3 * max(rows, cols)                                              # looking 0.3 / 0.2 off the axis: past the hole in the middle
    rp = view(size, (f, (cols - 1) / 2 - 0.3 * f, (rows - 1) / 2 - 0.2 * f), 0.0, 0.15, 30)
    vol = _trilinear(ctx, p, q, w, col)
    coloured = 0
    for pose in poses:
        coloured += int((_check(ctx, vol, q, w, col, pose, p, rp, f"{size}")[3][..., 3] > 0).sum())
    assert coloured > 0
    vol.close()


# ---- grids ---------------------------------------------------------------------------------------------------------------------------
def test_two_by_two_by_two(ctx):
    p = grid_params((2, 2, 2), vs=0.5, origin=(-0.5, -0.5, 0.5))
    coloured = 0
    for seed in range(4):
        q, w = random_grid((2, 2, 2), seed)
        q[0] = np.abs(q[0])
        q[1] = -np.abs(q[1])                                               # a surface between the two layers
        col = random_colour((2, 2, 2), 90 + seed, holes=0.3)
        vol = _trilinear(ctx, p, q, w, col)
        for pose in (_pose(), _pose((0.1, -0.2, 0.3), (0.1, 0.05, 0.2))):
            want = _check(ctx, vol, q, w, col, pose, p, view((12, 16), (20.0, 7.5, 5.5), 0.0, 0.05, 40), f"2x2x2 seed {seed}")
            coloured += int((want[3][..., 3] > 0).sum())
        vol.close()
    assert coloured > 50


def test_tiny_volumes_from_their_own_poses(ctx):
    coloured = 0
    for n, (p, q, w, col, poses) in enumerate(tiny_volumes()):
        vol = _trilinear(ctx, p, q, w, col)
        for k, pose in enumerate(poses):                                   # the 3e38 poses among them
            coloured += int((_check(ctx, vol, q, w, col, pose, p, default_view(p, n_steps=30), f"tiny {n} pose {k}")[3][..., 3] > 0).sum())
        vol.close()
    assert coloured > 500


def test_uploaded_random_grids(ctx):
    hits = coloured = 0
    for tag, p, q, w, col, pose, rp in ic.random_views():
        vol = _trilinear(ctx, p, q, w, col)
        want = _check(ctx, vol, q, w, col, pose, p, rp, tag)
        hits += int((want[0] > 0).sum())
        coloured += int((want[3][..., 3] > 0).sum())
        vol.close()
    print(f"{hits} hits, {coloured} coloured")
    assert hits > 100 and 100 < coloured <= hits                           # (a hit with any coloured corner has a colour)


@pytest.mark.parametrize("case", ic.last_cell_views(), ids=lambda c: c[0])
def test_hits_in_the_last_cell_of_every_axis(ctx, case):
    """The last pair of the cell evaluation ends on the last word of the voxel grid and of the colour grid."""
    tag, p, q, w, col, pose, rp, cell = case
    vol = _trilinear(ctx, p, q, w, col)
    want = _check(ctx, vol, q, w, col, pose, p, rp, tag)
    assert (want[3][..., 3] == 255).all()
    vol.close()


@pytest.mark.parametrize("row", ic.interp_branch_rows(), ids=lambda r: r[0])
def test_every_branch_row(ctx, row):
    name, p, q, w, col, pose, rp, _, _ = row
    vol = _trilinear(ctx, p, q, w, col)
    _check(ctx, vol, q, w, col, pose, p, rp, name)
    vol.close()


# ---- the mode ------------------------------------------------------------------------------------------------------------------------
def test_nearest_then_trilinear_then_nearest_and_every_subset_of_outputs(ctx):
    p, q, w, col = random_volume((9, 8, 7), 2)
    vol = _uploaded(ctx, p, q, w, col)
    pose, rp = _pose((0.05, -0.1, 0.02), (0.0, 0.01, 0.0)), view((19, 21), (30.0, 10.0, 9.0), 0.0, 0.02, 60)
    near = raycast_model(q, w, col, pose, p, rp)
    tri = ic.raycast_interp_model(q, w, col, pose, p, rp)
    assert (tri[3][..., 3] > 0).sum() > 20 and not np.array_equal(near[3], tri[3])
    first = _cast(vol, pose, rp, True)
    vol.set_colour_sampling("trilinear")
    second = _cast(vol, pose, rp, True)
    vol.clear()                                                            # odo_volume_clear leaves the mode
    assert vol.colour_sampling == "trilinear"
    vol.upload(q, w)
    vol.upload_colour(col)
    frames_equal(_cast(vol, pose, rp, True), tri, "after clear and upload")
    vol.set_colour_sampling("nearest")
    third = _cast(vol, pose, rp, True)
    frames_equal(first, near, "nearest")
    frames_equal(second, tri, "trilinear")
    frames_equal(third, near, "nearest again")
    want = {mode: dict(zip(NAMES, frames)) for mode, frames in (("nearest", near), ("trilinear", tri))}
    for mode in ("trilinear", "nearest"):
        vol.set_colour_sampling(mode)
        for r in range(1, 5):
            for which in itertools.combinations(NAMES, r):                 # rgba alone, with every other output, and without it
                st, got = _cast_dev(ctx, vol, pose, rp, which)
                assert st == 0, which
                frames_equal([got[k] for k in which], [want[mode][k] for k in which], f"{mode} outputs {which}")
    for k in ("depth", "raw", "nrmw"):                                     # (the modes share every output but rgba, bit for bit)
        a, b = want["nearest"][k], want["trilinear"][k]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
    vol.close()


# ---- the pinned coloured case --------------------------------------------------------------------------------------------------------
def test_pinned_coloured_case_at_120x160(ctx):
    """The pinned drive's ten frames fused with their colour on the device at their true poses; the ray-casts at 120 x 160 with the
    intrinsics divided by four, from poses 0 and 9, against the model on the grids as the device holds them. Grid, colour grid and
    stats() are unchanged by them, and two calls are bit-identical."""
    from odometry_amd import synth
    seq = drive(10)
    p = params(seq)
    vol = _volume(ctx, p)
    vol.enable_colour(3, False, 255)
    for k in range(10):
        vol.integrate(seq["depth"][k], seq["poses"][k], colour=synth.colour_from_gray(seq["gray"][k], 3, False, tint_seed=1))
    vol.set_colour_sampling("trilinear")
    q, w = vol.grid()
    col, stats = vol.colour_grid(), vol.stats()
    f, cx, cy = p["K"]
    rp = default_view(p, n_steps=140, size=(120, 160), K=(f / 4, (cx - 1.5) / 4, (cy - 1.5) / 4))
    for k in (0, 9):
        want = _check(ctx, vol, q, w, col, seq["poses"][k], p, rp, f"pinned, pose {k}")
        near = raycast_model(q, w, col, seq["poses"][k], p, rp)
        differ = int((want[3] != near[3]).any(-1).sum())
        print(f"pose {k}: {int((want[0] > 0).sum())} hits, {int((want[3][..., 3] > 0).sum())} coloured, {differ} differ from the nearest mode")
        assert (want[3][..., 3] > 0).sum() > 1000 and differ > 100
        frames_equal(_cast(vol, seq["poses"][k], rp, True), want, "again")
    assert vol.stats() == stats
    _grid_equal(vol, q, w, "after the ray-casts")
    assert np.array_equal(vol.colour_grid(), col)
    vol.close()


# ---- track(grey=...) -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sequences():
    return dict(corridor=pc.corridor_photo_sequence(), ribbed=pc.ribbed_photo_sequence())


def test_track_equals_trilinear_raycast_plus_align_and_changes_nothing(ctx, sequences):
    seq, k = sequences["ribbed"], 2
    vol = _volume(ctx, seq["p"])
    vol.enable_colour()
    for n in range(k):
        vol.integrate(seq["depth"][n], seq["poses"][n], colour=pc._grey_colour(seq["gray"][n]))
    q, w = vol.grid()
    col, stats = vol.colour_grid(), vol.stats()
    P_m, raw, grey = seq["poses"][k - 1], seq["depth"][k], seq["gray"][k]
    n_pose, n_res = vol.track(raw, P_m, grey=grey)
    g_pose, g_res = vol.track(raw, P_m)
    vol.set_colour_sampling("trilinear")
    depth, nrmw, rgba = vol.raycast(P_m, colour=True)
    frames_equal([depth, nrmw, rgba], [ic.raycast_interp_model(q, w, col, P_m, seq["p"], default_view(seq["p"]))[i] for i in (0, 2, 3)], "model frame")
    a_pose, a_res = vol.align(raw, depth, nrmw, P_m, P_m, grey=grey, model_rgba=rgba)
    t_pose, t_res = vol.track(raw, P_m, grey=grey)
    assert a_res["status"] == 0 and np.array_equal(bits(a_pose), bits(t_pose))
    for key in ("status", "iterations", "pairs", "cost", "eig_min", "eig_max", "photo_pairs", "photo_cost"):
        assert a_res[key] == t_res[key], key
    assert np.array_equal(bits(a_res["C"]), bits(t_res["C"])) and t_res["photo_pairs"] > 0
    assert not np.array_equal(bits(t_pose), bits(n_pose))                  # the mode reaches the alignment
    p_pose, p_res = vol.track(raw, P_m)                                    # the geometric track does not depend on it
    assert np.array_equal(bits(p_pose), bits(g_pose)) and p_res["cost"] == g_res["cost"]
    again, _ = vol.track(raw, P_m, grey=grey)
    assert np.array_equal(bits(again), bits(t_pose))
    _grid_equal(vol, q, w, "after ray-cast, align and track")
    assert np.array_equal(vol.colour_grid(), col) and vol.stats() == stats
    vol.close()


@pytest.mark.parametrize("name", ["corridor", "ribbed"])
def test_pinned_cases_give_the_cpu_tests_lines(ctx, sequences, name):
    """The CPU test's procedure on the GPU under the trilinear mode: frames 0 .. k - 1 fused with their colour at their true poses,
    frame k tracked from pose k - 1 with its grey frame, k = 1 .. 6: its six lines digit for digit, inside its bounds."""
    seq = sequences[name]
    bound_t, bound_r = dict(corridor=(MEASURED_CORRIDOR_T_M, MEASURED_CORRIDOR_R_DEG), ribbed=(MEASURED_RIBBED_T_M, MEASURED_RIBBED_R_DEG))[name]
    vol = _volume(ctx, seq["p"])
    vol.enable_colour()
    vol.set_colour_sampling("trilinear")
    lines = []
    for k in range(1, 7):
        vol.integrate(seq["depth"][k - 1], seq["poses"][k - 1], colour=pc._grey_colour(seq["gray"][k - 1]))
        pose, res = vol.track(seq["depth"][k], seq["poses"][k - 1], grey=seq["gray"][k])
        et, er = pose_error(pose, seq["poses"][k])
        lines.append(f"{name} frame {k}: {et * 1e3:.2f} mm {er:.3f} deg, pairs {res['pairs']:.0f} + {res['photo_pairs']:.0f}, steps {res['iterations']}")
        print(lines[-1])
        assert res["status"] == 0
        assert et <= 2 * bound_t and er <= 2 * bound_r
    assert lines == TRILINEAR_LINES[name]
    vol.close()


# ---- attached to a tracker -----------------------------------------------------------------------------------------------------------
def test_setter_on_an_attached_volume_mid_drive():
    """An RgbdTracker at 120 x 160 with a coloured volume attached, the mode set and set back while the drive goes on: the tracker's
    rows are those of a run without a volume, and the ray-casts between the frames are the model's on a standalone volume fed the
    same frames."""
    import shape_cases as S
    from odometry_amd import api, synth
    c = dict(S.find("rgbd", 120, 160, 3), frames=5)
    seq = S.render(c)
    p = params(seq, size=(120, 160), dims=(101, 75, 83), vs=0.07, origin=(-3.1, -3.2, 1.0), mu=0.2, max_depth=8.0, max_weight=3)
    p["K"] = tuple(S.intrinsics(c))
    colour = [synth.colour_from_gray(g, 3, False, tint_seed=2) for g in seq["gray"]]

    def run(with_volume):
        trk = api.RgbdTracker(0, **S.tracker_args(c))
        dev = [(trk.upload_frame(g), trk.upload_depth(d)) for g, d in zip(seq["gray"], seq["depth"])]
        cdev = [trk.upload_colour(a) for a in colour]
        vol, casts = None, {}
        if with_volume:
            vol = _volume(trk, p)
            vol.enable_colour(3, False, 255)
            trk.attach_volume(vol)
            trk.frame_colour(cdev[0])
        trk.init(*dev[0])
        rows = [dict(abs_pose=np.eye(4, dtype=f32))]
        for k in range(1, c["frames"]):
            if with_volume:
                trk.frame_colour(cdev[k])
            rows.append(trk.track(*dev[k]))
            if with_volume:
                vol.set_colour_sampling("trilinear" if k % 2 else "nearest")   # while attached, behind the integrations enqueued so far
                assert vol.colour_sampling == ("trilinear" if k % 2 else "nearest")
                casts[k] = _cast(vol, rows[k]["abs_pose"], default_view(p), True)
        return trk, vol, dev, cdev, rows, casts

    plain, _, _, _, want_rows, _ = run(False)
    plain.close()
    trk, vol, dev, cdev, rows, casts = run(True)
    for k in range(1, c["frames"]):
        for key in ("pose_to_keyframe", "abs_pose"):
            assert np.array_equal(bits(rows[k][key]), bits(want_rows[k][key])), f"frame {k}: {key} differs"
        assert rows[k]["new_keyframe"] == want_rows[k]["new_keyframe"] and rows[k]["solve_status"] == want_rows[k]["solve_status"] == 0
    ref = _volume(trk, p)
    ref.enable_colour(3, False, 255)
    coloured = 0
    for k in range(c["frames"]):
        ref.integrate(dev[k][1], rows[k]["abs_pose"], colour=cdev[k])
        if k in casts:
            q, w = ref.grid()
            col = ref.colour_grid()
            model = ic.raycast_interp_model if k % 2 else raycast_model
            want = model(q, w, col, rows[k]["abs_pose"], p, default_view(p))
            frames_equal(casts[k], want, f"attached after {k + 1} frames, {'trilinear' if k % 2 else 'nearest'}")
            coloured += int((want[3][..., 3] > 0).sum())
    assert coloured > 1000 and vol.stats()["frames"] == c["frames"]
    ref.close()
    vol.close()
    trk.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_volume(ctx):
    from odometry_amd import _lib as L
    p, q, w, col = random_volume((9, 8, 7), 0)
    pose, rp = _pose(), view((12, 16), (30.0, 7.5, 5.5), 0.0, 0.02, 40)
    plain = _uploaded(ctx, p, q, w)                                        # no colour grid
    before = plain.stats()
    assert plain.lib.odo_volume_set_colour_sampling(plain.h, 1) == -1 and "no colour grid" in L.last_error()
    with pytest.raises(L.OdoError, match="no colour grid"):
        plain.set_colour_sampling("trilinear")
    assert plain.colour_sampling == "nearest" and plain.stats() == before
    frames_equal(_cast(plain, pose, rp, False), raycast_model(q, w, None, pose, p, rp), "after the refused calls")
    plain.close()
    vol = _uploaded(ctx, p, q, w, col)
    vol.set_colour_sampling("trilinear")
    for mode in (2, -1, 7):
        assert vol.lib.odo_volume_set_colour_sampling(vol.h, mode) == -1 and "mode" in L.last_error(), mode
        assert vol.colour_sampling == "trilinear"                          # the mode is unchanged
    with pytest.raises(ValueError):
        vol.set_colour_sampling("cubic")
    frames_equal(_cast(vol, pose, rp, True), ic.raycast_interp_model(q, w, col, pose, p, rp), "after the refused calls")
    _grid_equal(vol, q, w, "after the refused calls")
    vol.close()


def test_the_timing_call_runs_in_either_mode_and_changes_nothing(ctx):
    from odometry_amd import _lib as L
    p, q, w, col = random_volume((9, 8, 7), 1)
    pose, rp = _pose((0.05, -0.1, 0.02), (0.0, 0.01, 0.0)), view((17, 23), (30.0, 10.0, 9.0), 0.0, 0.02, 40)
    kw = dict(size=rp["size"], K=rp["K"], t_min=rp["t_min"], step=rp["step"], n_steps=rp["n_steps"])
    vol = _uploaded(ctx, p, q, w, col)
    stats = vol.stats()
    for mode in ("nearest", "trilinear"):
        vol.set_colour_sampling(mode)
        assert vol.raycast_time(pose, colour=True, reps=3, **kw) > 0 and vol.raycast_time(pose, reps=2, **kw) > 0
    frames_equal(_cast(vol, pose, rp, True), ic.raycast_interp_model(q, w, col, pose, p, rp), "after the timing calls")
    _grid_equal(vol, q, w, "after the timing calls")
    assert np.array_equal(vol.colour_grid(), col) and vol.stats() == stats
    vol.close()
    plain = _uploaded(ctx, p, q, w)
    with pytest.raises(L.OdoError, match="no colour grid"):
        plain.raycast_time(pose, colour=True, reps=2, **kw)
    assert plain.raycast_time(pose, reps=2, **kw) > 0
    plain.close()
