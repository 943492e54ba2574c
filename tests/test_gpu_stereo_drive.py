"""What a stereo matcher carries from one pair to the next, and the closed stereo drive, on the GPU against the composed models of
tests/stereo_drive_cases.py, bit for bit (INTEGRATION.md sections 3.15 to 3.17). One StereoDepth lives through the whole sequence
table, mode switches, filter switches and output frames included, and equals after every step the model of that step ALONE; the
same sequence enqueued back to back with nothing read in between; the drive match -> filter -> ray-cast -> align -> follow -> fuse,
every frame started from the pose the frame before it returned, with the matcher's internal frame handed to TsdfVolume.track every
time, for the box matcher and the semi-global mode, with and without host reads between the frames; the same drive into callers'
frames; and mode switches behind runs in flight. tests/test_stereo_drive_cpu.py holds the conditions under which this means
something. The only tolerance in this file is the eigenvalues' of test_gpu_volume_follow_track._result_equals."""
import time

import numpy as np
import pytest

import stereo_drive_cases as D
from test_gpu_depth_filter import Guarded
from test_gpu_stereo_depth import _matcher
from test_gpu_volume_follow_track import _end_equals, _result_equals, _snapshot, _start
from test_gpu_volume_shift import _window_equals
from test_stereo_drive_cpu import MEASURED
from test_volume_icp_cpu import pose_error

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture
def keep():
    """keep(obj) hands a matcher or a volume back and closes it behind the test, passed or failed: an object that a failed test's
    traceback keeps alive must not be destroyed after the module's context, which it points to."""
    made = []

    def keep_(obj):
        made.append(obj)
        return obj

    yield keep_
    for obj in reversed(made):
        obj.close()


@pytest.fixture(scope="module")
def seq_dev(ctx):
    """The sequence table's pairs, uploaded once: name -> (left, right) device handles."""
    out = {name: tuple(ctx.upload(a) for a in pair) for name, pair in D.sequence_pairs().items()}
    yield out
    for pair in out.values():
        for h in pair:
            ctx.free(h)


@pytest.fixture(scope="module")
def drive_dev(ctx):
    """All 16 images of the drive (the two front ends see the same ones), uploaded once: (lefts, rights)."""
    c = D.stereo_drive("box")
    out = [ctx.upload(a) for a in c["left"]], [ctx.upload(a) for a in c["right"]]
    yield out
    for handles in out:
        for h in handles:
            ctx.free(h)


@pytest.fixture(scope="module")
def models():
    t = time.time()
    out = {front: (D.stereo_drive(front), D.stereo_drive_model(front)) for front in D.FRONTS}
    print(f"the drives' models took {time.time() - t:.1f} s")
    return out


# ---- one matcher through the sequence table ---------------------------------------------------------------------------------------
class _Switches:
    """The calls between two steps, as the table says: enable_sgm / disable_sgm when the mode changes, enable_speckle when the filter
    does (min_size 0 takes it off)."""

    def __init__(self, sd):
        self.sd, self.mode, self.speckle = sd, "box", None

    def to(self, mode, speckle):
        if mode != self.mode:
            if D.MODES[mode] is None:
                self.sd.disable_sgm()
            else:
                self.sd.enable_sgm(**D.MODES[mode])
            self.mode = mode
        if speckle != self.speckle:
            self.sd.enable_speckle(*(speckle or (0, 0)))
            self.speckle = speckle


def _matcher_equals(sd, m, tag, speckle=True, volume=True):
    """The matcher's own planes and counters behind a run against the step's model."""
    q = sd.disparity()
    assert np.array_equal(q, m["fq"]), (tag, "q", np.argwhere(q != m["fq"])[:4])
    assert sd.stats() == m["stats"], (tag, sd.stats(), m["stats"])
    if volume and m["S"] is not None:
        S = sd.sgm_volume()
        assert np.array_equal(S, m["S"]), (tag, "S", np.argwhere(S != m["S"])[:4])
    if speckle and m["M"] is not None:
        assert sd.speckle_stats() == m["M"]["stats"] and m["M"]["stats"]["guard"] == 0, (tag, sd.speckle_stats(), m["M"]["stats"])


def test_one_matcher_through_the_sequence(ctx, seq_dev, keep):
    steps = D.sequence_steps()
    sd = keep(_matcher(ctx, D.SEQ_SIZE, D.sequence_params()))
    switches = _Switches(sd)
    internal = np.zeros(D.SEQ_SIZE, np.uint16)                  # the internal frame is zero until the first run that uses it
    t = time.time()
    for i, (pair, mode, speckle, output) in enumerate(steps):
        m, tag = D.step_model(i), f"step {i}: {steps[i]}"
        switches.to(mode, speckle)
        left, right = seq_dev[pair]
        if output == "caller":
            dst = Guarded(ctx, 2 * m["fdepth"].size)
            assert sd.run(left, right, dst.p).value == dst.p.value
            depth = dst.frame(D.SEQ_SIZE).copy()
            dst.free()
        else:
            sd.run(left, right)
            depth = internal = sd.download()
        assert np.array_equal(depth, m["fdepth"]), (tag, "depth", np.argwhere(depth != m["fdepth"])[:4])
        _matcher_equals(sd, m, tag)
        assert np.array_equal(sd.download(), internal), f"{tag}: the internal frame is not the last internal step's"
    print(f"{len(steps)} steps took {time.time() - t:.2f} s")
    sd.close()


def test_the_sequence_with_nothing_read_in_between(ctx, seq_dev, keep):
    """Every step into a guarded frame of its own, the mode and filter switches between them (they may wait internally; the test
    reads nothing): all frames are compared at the end, and the matcher holds the last step's q, statistics and S."""
    steps = D.sequence_steps()
    sd = keep(_matcher(ctx, D.SEQ_SIZE, D.sequence_params()))
    switches = _Switches(sd)
    frames = [Guarded(ctx, 2 * D.SEQ_SIZE[0] * D.SEQ_SIZE[1]) for _ in steps]
    ctx.synchronize()
    for (pair, mode, speckle, _), dst in zip(steps, frames):
        switches.to(mode, speckle)
        sd.run(*seq_dev[pair], dst.p)
    for i, dst in enumerate(frames):
        want = D.step_model(i)["fdepth"]
        got = dst.frame(D.SEQ_SIZE)
        assert np.array_equal(got, want), (i, steps[i], np.argwhere(got != want)[:4])
        dst.free()
    last = D.step_model(len(steps) - 1)
    assert last["S"] is not None
    _matcher_equals(sd, last, "the last step")
    assert not sd.download().any()                                                           # no step used the internal frame
    sd.close()


def test_mode_switch_with_runs_in_flight(ctx, seq_dev, keep):
    """Five semi-global runs, then with no wait disable_sgm (frees the volumes the runs read and write), a box run, enable_speckle
    (allocates the filter's planes) and one more run: seven guarded frames, each its own model."""
    p = D.sequence_params()
    plan = [(name, "sgm8", None) for name in ("shift 17", "occluding step 2/20", "exchanged", "constant", "non-finite")]
    plan += [("occluding step 4/12", "box", None), ("exchanged", "box", (16, 60))]
    want = [D._step_model(*step) for step in plan]
    assert want[-1]["M"]["stats"]["removed_pixels"] > 0 and len({w["fdepth"].tobytes() for w in want}) == len(want)
    sd = keep(_matcher(ctx, D.SEQ_SIZE, p))
    switches = _Switches(sd)
    frames = [Guarded(ctx, 2 * D.SEQ_SIZE[0] * D.SEQ_SIZE[1]) for _ in plan]
    ctx.synchronize()
    for (pair, mode, speckle), dst in zip(plan, frames):
        switches.to(mode, speckle)
        sd.run(*seq_dev[pair], dst.p)
    for step, dst, w in zip(plan, frames, want):
        got = dst.frame(D.SEQ_SIZE)
        assert np.array_equal(got, w["fdepth"]), (step, np.argwhere(got != w["fdepth"])[:4])
        dst.free()
    _matcher_equals(sd, want[-1], "the last run")
    sd.close()


# ---- the closed stereo drive ---------------------------------------------------------------------------------------------------------
def _front(ctx, c, keep):
    """The drive's matcher: the filter on, the semi-global mode for "sgm"."""
    sd = keep(_matcher(ctx, c["left"][0].shape, c["mp"]))
    assert sd.params.max_raw == c["mp"]["max_raw"]
    if c["sg"] is not None:
        sd.enable_sgm(**c["sg"])
    sd.enable_speckle(*c["speckle"])
    return sd


def _stereo_drive(ctx, keep, c, m, dev, waits, own=None):
    """The drive on a fresh matcher and a fresh following volume with the point store. Frame 0: follow(pose0), then
    integrate(sd.run(L0, R0), pose0); frame k: track(sd.run(Lk, Rk), good, integrate=True), the matcher's internal frame every
    time (own: a guarded frame per pair instead). Every result and the window against the model; with waits also the volume's and
    the matcher's counters and the q frame behind every frame, and the volume's whole state round the blind frame. Returns (sd, vol,
    [(k, pose)] of the frames with status 0)."""
    lefts, rights = dev
    sd = _front(ctx, c, keep)
    run = lambda k: sd.run(lefts[k], rights[k]) if own is None else sd.run(lefts[k], rights[k], own[k].p)
    vol = keep(_start(ctx, c, run(0)))
    good, tracked = c["poses"][0], []
    for k in range(1, len(m["frames"])):
        want, tag = m["frames"][k], f"{c['name']}, waits {waits}, frame {k}"
        before = _snapshot(vol) if waits and k in c["blind"] else None
        pose, res = vol.track(run(k), good, integrate=True)
        _result_equals(res, pose, want, tag)
        _window_equals(vol, c["p"], want["off"], tag)
        if waits:
            assert vol.stats()["frames"] == want["fused"], (tag, vol.stats())
            _matcher_equals(sd, c["frames"][k], tag, volume=False)
            if before is not None:
                assert res["status"] == 1 and res["pairs"] == 0 and _snapshot(vol) == before, tag
        if res["status"] == 0:
            good = pose
            tracked.append((k, pose))
    return sd, vol, tracked


def _truth(c, tracked, front):
    e = [pose_error(pose, c["poses"][k]) for k, pose in tracked]
    print(f"{front}: largest {max(t for t, _ in e) * 1e3:.3f} mm {max(r for _, r in e):.4f} deg over {len(e)} frames")
    assert len(e) == len(c["poses"]) - 1 - len(c["blind"])
    assert max(t for t, _ in e) <= 2 * MEASURED[front][0] and max(r for _, r in e) <= 2 * MEASURED[front][1]


@pytest.mark.parametrize("front", D.FRONTS)
def test_stereo_drive_frame_by_frame(ctx, drive_dev, models, keep, front):
    """8 pairs, the fifth blind, 5 shifts: once with nothing but sd.run and track between the frames, once with the counters and the
    q frame read behind every frame."""
    c, m = models[front]
    (b,) = c["blind"]
    assert m["frames"][b]["status"] == 1 and m["frames"][b]["fused"] == m["frames"][b - 1]["fused"] and m["shifts"] >= 4
    for waits in (False, True):
        t = time.time()
        sd, vol, tracked = _stereo_drive(ctx, keep, c, m, drive_dev, waits)
        _end_equals(vol, c, m, f"{c['name']}, waits {waits}")
        _matcher_equals(sd, c["frames"][-1], f"{c['name']}, waits {waits}: the last pair")
        assert np.array_equal(sd.download(), c["frames"][-1]["fdepth"])
        print(f"{front}, waits {waits}: {time.time() - t:.2f} s")
        vol.close()
        sd.close()
    _truth(c, tracked, front)


def test_drive_into_callers_frames(ctx, drive_dev, models, keep):
    """The box drive with sd.run(L, R, own_buffer_k): the same results as into the internal frame (both are the model's), every
    buffer the filtered model frame at the end, and the internal frame never written."""
    c, m = models["box"]
    own = [Guarded(ctx, 2 * a.size) for a in c["left"]]
    sd, vol, tracked = _stereo_drive(ctx, keep, c, m, drive_dev, False, own=own)
    _end_equals(vol, c, m, "callers' frames")
    for k, dst in enumerate(own):
        got = dst.frame(c["left"][k].shape)
        assert np.array_equal(got, c["frames"][k]["fdepth"]), (k, np.argwhere(got != c["frames"][k]["fdepth"])[:4])
        dst.free()
    _matcher_equals(sd, c["frames"][-1], "callers' frames: the last pair")
    assert not sd.download().any()
    _truth(c, tracked, "box")
    vol.close()
    sd.close()
