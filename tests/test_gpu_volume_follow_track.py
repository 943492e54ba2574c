"""The closed loop of the TSDF volume on the GPU: TsdfVolume.track(..., integrate=True) on a volume with set_follow on, every frame
started from the pose the frame before it returned, against the composed model of tests/volume_follow_track_cases.py frame by frame
and bit for bit: drive A (the window leaves its box, one blind frame) with the point store, drive B (out and back) with and without
the re-entry store, refusals inside a following drive, track against the explicit calls it stands for on the geometric and the
photometric path, and host frames against device handles. The only tolerance in this file is the eigenvalues' (Jacobi on the device's
host side, LAPACK in the model), as in tests/test_gpu_volume_icp.py."""
import time

import numpy as np
import pytest

import volume_follow_track_cases as F
import volume_icp_photo_cases as pc
from test_gpu_volume_reentry import _state_equals
from test_gpu_volume_shift import _store_equals, _volume, _window_equals
from test_volume_cpu import bits
from test_volume_follow_track_cpu import MEASURED
from test_volume_icp_cpu import pose_error

pytestmark = pytest.mark.gpu
f32 = np.float32
NO_RATIO = 0.5      # a min_eig_ratio that no frame of the drives can meet: theirs lie between 4e-3 and 2e-2


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx):
    """The depth frames of both drives, uploaded once: name -> device handles."""
    out = {name: [ctx.upload(np.ascontiguousarray(d)) for d in F.drive(name)["depth"]] for name in ("A", "B")}
    yield out
    for handles in out.values():
        for h in handles:
            ctx.free(h)


@pytest.fixture(scope="module")
def models():
    t = time.time()
    out = {("A", False): F.model("A", spill=True), ("B", False): F.model("B", spill=True), ("B", True): F.model("B", reentry=True, spill=True)}
    print(f"the three models took {time.time() - t:.1f} s")
    return out


def _start(ctx, c, frame0, reentry=False, colour=None):
    """A following volume with the point store (and the re-entry store) behind frame 0: the follow step for its true pose, then its
    integration, as drive_case() does it."""
    vol = _volume(ctx, c["p"], colour=colour is not None, spill=F.SPILL_CAPACITY)
    if reentry:
        vol.enable_reentry(F.REENTRY_CAPACITY)
    vol.set_follow(c["follow"]["focus"], c["follow"]["threshold"])
    assert vol.follow(c["poses"][0]) == (0, 0, 0)
    vol.integrate(frame0, c["poses"][0], colour=colour)
    return vol


def _result_equals(res, pose, want, tag):
    """What track returned against the model's frame: the pose's bits (NaNs when refused), status, iterations, pairs, C and cost by
    bits, the eigenvalues within 1e-9 eig_max."""
    assert res["status"] == want["status"], (tag, res["status"], want["status"])
    assert res["iterations"] == want["iterations"] and res["pairs"] == want["pairs"], (tag, res["iterations"], res["pairs"])
    assert np.array_equal(bits(res["C"]), bits(want["C"])), f"{tag}: C differs"
    assert np.float64(res["cost"]).tobytes() == np.float64(want["cost"]).tobytes(), (tag, res["cost"], want["cost"])
    for key in ("eig_min", "eig_max"):
        assert abs(res[key] - want[key]) <= 1e-9 * want["eig_max"], (tag, key, res[key], want[key])
    assert pose.dtype == f32 and pose.shape == (4, 4)
    if want["status"] == 0:
        assert np.array_equal(bits(pose), bits(want["pose"])), f"{tag}: the pose differs by {np.abs(pose - want['pose']).max():.3e}"
    else:
        assert np.isnan(pose).all(), tag


def _grid_equals(vol, grid, tag):
    gq, gw = vol.grid()
    assert np.array_equal(gw, grid[1]) and np.array_equal(gq, grid[0]), f"{tag}: the grid differs"


def _drive(vol, frames, c, m, waits, last=None):
    """Frames 1 .. last through track(integrate=True), each from the pose the frame before it returned, against the model. Without
    waits the test touches nothing on the device between two tracks (window() reads the host's state): the poses and results, and
    the window behind every frame. With waits also stats() behind every frame and the grid behind the model's checkpoints. Returns
    the last good pose and [(k, pose)] of the frames with status 0."""
    good, tracked = c["poses"][0], []
    n = len(m["frames"]) if last is None else last + 1
    for k in range(1, n):
        want = m["frames"][k]
        pose, res = vol.track(frames[k], good, integrate=True)
        _result_equals(res, pose, want, f"frame {k}")
        _window_equals(vol, c["p"], want["off"], f"frame {k}")
        if waits:
            assert vol.stats()["frames"] == want["fused"], (k, vol.stats())
            if "grid" in want:
                _grid_equals(vol, want["grid"], f"frame {k}")
        if res["status"] == 0:
            good = pose
            tracked.append((k, pose))
    return good, tracked


def _end_equals(vol, c, m, tag):
    """The window, the grid, the counters and the stores behind the drive's last frame."""
    _window_equals(vol, c["p"], m["off"], tag)
    _grid_equals(vol, (m["q"], m["w"]), tag)
    assert vol.stats()["frames"] == m["frames"][-1]["fused"]
    pts = m["points"]
    _store_equals(vol, pts["xyz0"], pts["nrmw"], None, tag, dropped=pts["dropped"])
    if m["reentry"] is not None:
        _state_equals(vol, c["p"], (m["q"], m["w"], None, m["off"], m["reentry"]), tag, behind=False)


def _truth(c, tracked, key):
    """The returned poses against the true ones: inside twice what the CPU tests measured with the model."""
    e = [pose_error(pose, c["poses"][k]) for k, pose in tracked]
    print(f"{key}: largest {max(t for t, _ in e) * 1e3:.3f} mm {max(r for _, r in e):.4f} deg over {len(e)} frames")
    assert len(e) == len(c["poses"]) - 1 - len(c["blind"])
    assert max(t for t, _ in e) <= 2 * MEASURED[key][0] and max(r for _, r in e) <= 2 * MEASURED[key][1]


# ---- the drives against the model ------------------------------------------------------------------------------------------------
def test_drive_a_frame_by_frame(ctx, dev, models):
    """26 frames, the ninth blind, 23 shifts, the window ends 68 voxels deep in a grid of 60: once with nothing but track between the
    frames, once with the counters behind every frame and the grid behind frames 1, 8, 9 (the blind one: unchanged), 10 and the
    last."""
    c, m = F.drive("A"), models[("A", False)]
    for waits in (False, True):
        vol = _start(ctx, c, dev["A"][0])
        tracked = _drive(vol, dev["A"], c, m, waits)[1]
        _end_equals(vol, c, m, f"drive A, waits {waits}")
        vol.close()
    assert m["shifts"] >= 20 and m["off"][2] >= c["p"]["dims"][2] and len(m["points"]["xyz0"]) > 0
    _truth(c, tracked, ("A", False))


@pytest.mark.parametrize("reentry", [False, True])
def test_drive_b_out_and_back(ctx, dev, models, reentry):
    c, m = F.drive("B"), models[("B", reentry)]
    for waits in (False, True):
        vol = _start(ctx, c, dev["B"][0], reentry=reentry)
        tracked = _drive(vol, dev["B"], c, m, waits)[1]
        _end_equals(vol, c, m, f"drive B, re-entry {reentry}, waits {waits}")
        vol.close()
    assert m["off"] == (0, 0, 0)
    _truth(c, tracked, ("B", reentry))


def test_the_reentry_store_changes_the_return_leg_where_the_models_say(ctx, dev, models):
    """Two volumes side by side, one with the re-entry store: their poses are the same bits exactly on the frames on which the two
    models' are, and they differ on some."""
    c = F.drive("B")
    plain, store = models[("B", False)]["frames"], models[("B", True)]["frames"]
    vols = [_start(ctx, c, dev["B"][0], reentry=r) for r in (False, True)]
    good = [c["poses"][0], c["poses"][0]]
    differ = []
    for k in range(1, len(plain)):
        got = [v.track(dev["B"][k], g, integrate=True) for v, g in zip(vols, good)]
        assert got[0][1]["status"] == got[1][1]["status"] == 0
        same = np.array_equal(bits(got[0][0]), bits(got[1][0])) and got[0][1]["pairs"] == got[1][1]["pairs"]
        want = np.array_equal(bits(plain[k]["pose"]), bits(store[k]["pose"])) and plain[k]["pairs"] == store[k]["pairs"]
        assert same == want, k
        differ.append(not same)
        good = [g[0] for g in got]
    assert any(differ) and not differ[0] and differ[-1]
    assert vols[1].reentry_stats()["restored"] > 0
    assert not np.array_equal(vols[0].grid()[1], vols[1].grid()[1])
    for v in vols:
        v.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _snapshot(vol):
    q, w = vol.grid()
    pts = vol.spilled(with_dropped=True)
    off, origin = vol.window()
    return dict(off=off, origin=origin.tobytes(), q=q.tobytes(), w=w.tobytes(), points=(len(pts[0]), pts[0].tobytes(), pts[1].tobytes(), pts[2]),
                stats=vol.stats())


def test_refused_frames_inside_a_following_drive_change_nothing(ctx, dev, models):
    """Drive A to frame 3; frame 4 under a min_eig_ratio that it cannot meet (status 2: the alignment itself is the model's), then
    frame 4 as the drive has it; on to the blind frame 9 (status 1) and the frame behind it. Each refusal returns a NaN pose and
    leaves the window, both grids, the point store and the counters as they were, and the next track from the last good pose is the
    model's."""
    c, m = F.drive("A"), models[("A", False)]
    vol = _start(ctx, c, dev["A"][0])
    good = _drive(vol, dev["A"], c, m, False, last=3)[0]
    before = _snapshot(vol)
    pose, res = vol.track(dev["A"][4], good, integrate=True, params=vol.icp_params(min_eig_ratio=NO_RATIO))
    want = m["frames"][4]
    assert res["status"] == 2 and np.isnan(pose).all() and res["eig_min"] < NO_RATIO * res["eig_max"]
    assert res["iterations"] == want["iterations"] and res["pairs"] == want["pairs"] and np.array_equal(bits(res["C"]), bits(want["C"]))
    assert _snapshot(vol) == before
    assert before["stats"]["frames"] == 4 and before["points"][0] > 0 and before["off"] == m["frames"][3]["off"]
    (b,) = c["blind"]
    for k in range(4, b):
        pose, res = vol.track(dev["A"][k], good, integrate=True)
        _result_equals(res, pose, m["frames"][k], f"frame {k}")
        good = pose
    _grid_equals(vol, m["frames"][b - 1]["grid"], f"frame {b - 1}")
    before = _snapshot(vol)
    pose, res = vol.track(dev["A"][b], good, integrate=True)
    _result_equals(res, pose, m["frames"][b], "the blind frame")
    assert res["status"] == 1 and np.isnan(pose).all() and _snapshot(vol) == before
    pose, res = vol.track(dev["A"][b + 1], good, integrate=True)
    _result_equals(res, pose, m["frames"][b + 1], "behind the blind frame")
    _window_equals(vol, c["p"], m["frames"][b + 1]["off"], "behind the blind frame")
    _grid_equals(vol, m["frames"][b + 1]["grid"], "behind the blind frame")
    assert vol.stats()["frames"] == m["frames"][b + 1]["fused"] == b + 1
    vol.close()


# ---- track against the calls it stands for -------------------------------------------------------------------------------------------
RESULT_KEYS = ("status", "iterations", "pairs", "cost", "eig_min", "eig_max")


def _volumes_equal(a, b, colour, tag):
    assert a.window()[0] == b.window()[0] and a.window()[1].tobytes() == b.window()[1].tobytes(), tag
    assert all(np.array_equal(x, y) for x, y in zip(a.grid(), b.grid())), f"{tag}: the grids differ"
    if colour:
        assert np.array_equal(a.colour_grid(), b.colour_grid()), f"{tag}: the colour grids differ"
    sa, sb = a.spilled(colour=colour, with_dropped=True), b.spilled(colour=colour, with_dropped=True)
    assert sa[-1] == sb[-1] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(sa[:-1], sb[:-1])), f"{tag}: the point stores differ"
    assert a.stats() == b.stats(), tag


def test_track_with_integrate_is_raycast_align_follow_integrate(ctx, dev):
    """No model: a second volume driven with the explicit calls ends every one of drive A's first 8 frames with the same pose, result,
    window, grid, store and counters as track(integrate=True)."""
    c = F.drive("A")
    one, two = _start(ctx, c, dev["A"][0]), _start(ctx, c, dev["A"][0])
    good, shifts = c["poses"][0], 0
    for k in range(1, 9):
        pose, res = one.track(dev["A"][k], good, integrate=True)
        depth, nrmw = two.raycast(good)
        pose2, res2 = two.align(dev["A"][k], depth, nrmw, good, good)
        assert res["status"] == res2["status"] == 0 and np.array_equal(bits(pose), bits(pose2)), k
        assert all(res[key] == res2[key] for key in RESULT_KEYS) and np.array_equal(bits(res["C"]), bits(res2["C"])), k
        shifts += two.follow(pose2) != (0, 0, 0)
        two.integrate(dev["A"][k], pose2)
        _volumes_equal(one, two, False, f"frame {k}")
        good = pose
    assert shifts >= 6 and len(one.spilled()[0]) > 0
    one.close()
    two.close()


@pytest.mark.parametrize("mode", ["nearest", "trilinear"])
def test_photometric_track_with_integrate_is_its_explicit_calls(ctx, mode):
    """The same identity on a coloured volume over 4 frames, frames made as volume_icp_photo_cases makes them (Scene.render's grey,
    replicated into R, G and B), from numpy arrays, in either colour sampling mode; the colour grids and the stores' colours are
    compared as well."""
    c = F.drive("A")
    colour = [pc._grey_colour(g) for g in c["gray"][:5]]
    vols = [_start(ctx, c, c["depth"][0], colour=colour[0]) for _ in range(2)]
    one, two = vols
    for v in vols:
        v.set_colour_sampling(mode)
    good, shifts = c["poses"][0], 0
    for k in range(1, 5):
        raw, grey = c["depth"][k], c["gray"][k]
        pose, res = one.track(raw, good, integrate=True, grey=grey, colour=colour[k])
        depth, nrmw, rgba = two.raycast(good, colour=True)
        pose2, res2 = two.align(raw, depth, nrmw, good, good, grey=grey, model_rgba=rgba)
        assert res["status"] == res2["status"] == 0 and np.array_equal(bits(pose), bits(pose2)), k
        assert all(res[key] == res2[key] for key in RESULT_KEYS + ("photo_pairs", "photo_cost")), k
        assert np.array_equal(bits(res["C"]), bits(res2["C"])) and res["photo_pairs"] > 0, k
        shifts += two.follow(pose2) != (0, 0, 0)
        two.integrate(raw, pose2, colour=colour[k])
        _volumes_equal(one, two, True, f"{mode}, frame {k}")
        et, er = pose_error(pose, c["poses"][k])
        print(f"{mode} frame {k}: {et * 1e3:.2f} mm {er:.3f} deg, pairs {res['pairs']:.0f} + {res['photo_pairs']:.0f}, window {one.window()[0]}")
        good = pose
    assert shifts >= 2 and one.colour_grid().any() and len(one.spilled()[0]) > 0
    for v in vols:
        v.close()


def test_host_frames_give_what_device_handles_give(ctx, dev, models):
    """Drive A's first 6 frames from numpy arrays (uploaded into temporaries that each call frees) against the run from device
    handles: the same poses and results, and the same volume at the end; both are the model's."""
    c, m = F.drive("A"), models[("A", False)]
    a, b = _start(ctx, c, dev["A"][0]), _start(ctx, c, c["depth"][0])
    good = c["poses"][0]
    for k in range(1, 7):
        pose, res = a.track(dev["A"][k], good, integrate=True)
        pose2, res2 = b.track(c["depth"][k], good, integrate=True)
        assert np.array_equal(bits(pose), bits(pose2)) and all(res[key] == res2[key] for key in RESULT_KEYS), k
        _result_equals(res2, pose2, m["frames"][k], f"frame {k}")
        good = pose
    _volumes_equal(a, b, False, "host frames")
    a.close()
    b.close()
