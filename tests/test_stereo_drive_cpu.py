"""The conditions under which tests/test_gpu_stereo_drive.py means something, asserted on the models of tests/stereo_drive_cases.py
alone (no GPU, no library).

The sequence table: one matcher lives through its steps and carries its planes from one to the next, so a plane that a run failed to
rewrite must not be able to pass for the next step's model. Between every two consecutive steps the q frames, the depth frames, the
statistics and (between two semi-global steps) the aggregate S differ widely, and where the filter is on it removes something.

The drive, for both front ends: every sighted frame tracks, the blind one is refused with an all-zero depth frame and changes
nothing, the window shifts, the matcher and the filter have work on every frame, and the two front ends end in different pose bits.

What the q frames can and cannot show. A q pixel is non-zero exactly where the step matched. The table asks for 200 pixels that go
non-zero -> zero and 200 that go zero -> non-zero between neighbours; the second count is at most the number of unmatched interior
pixels of the earlier step and the first at most that of the later one. Two of the pairs the table must contain match everywhere
but in the two leftmost interior columns, whatever the mode and the order: the exact shift by 5 (90 unmatched interior pixels of
3210) and the constant pair under the semi-global rule (60; under the box rule it matches nothing, and then the other direction
is empty). No neighbour can make those directions reach 200, so for a direction whose limit lies below 200 the test asks instead for
200 pixels matched in BOTH steps whose q differs, which a stale q frame cannot reproduce either; it asserts that this happens for
those two pairs only, and only in the limited direction. Every other direction of every transition holds the 200."""
import numpy as np
import pytest

import stereo_drive_cases as D
import stereo_sgm_cases as sgc
from test_volume_cpu import bits
from test_volume_icp_cpu import pose_error

# Measured with the committed models (test_drives_track prints them): the largest translation (m) and rotation (degrees) error against
# the true poses over a drive, every frame started from the pose the model returned for the frame before it; both at frame 7. The
# stereo depth is quantised to sixteenths of a pixel of disparity (9 cm at 3 m here), hence centimetres where sensor depth gives
# millimetres. tests/test_gpu_stereo_drive.py asserts twice these; here they are informational and held to the same factor.
MEASURED = {"box": (0.09452, 1.9126), "sgm": (0.09239, 2.5806)}
MIN_CHANGED = 200                 # pixels of q, each way, between two consecutive steps
FEW_UNMATCHED = ("shift 5", "constant")
MODEL_SECONDS = 60.0              # a guard against a model that got slow, not a measurement: a drive's models take 4 to 6 s


# ---- the sequence table -----------------------------------------------------------------------------------------------------------
def test_table_covers_modes_filters_frames_and_pairs():
    steps = D.sequence_steps()
    pairs, modes, speckles, outputs = (list(x) for x in zip(*steps))
    assert len(steps) >= 14
    assert set(pairs) == set(D.sequence_pairs()) and all(a.shape == D.SEQ_SIZE for pr in D.sequence_pairs().values() for a in pr)
    assert set(modes) == set(D.MODES) and set(speckles) == set(D.SPECKLES) and set(outputs) == {"internal", "caller"}
    assert (D.MODES["sgm8"], D.MODES["sgm4"]) == (dict(p1=100, p2=600, paths=8), dict(p1=7, p2=900, paths=4))
    # every mode follows every other mode
    follows = set(zip(modes, modes[1:]))
    assert {(a, b) for a in D.MODES for b in D.MODES if a != b} <= follows, follows
    # the filter is switched on, re-parametrised (both ways round would do) and switched off between steps
    turns = set(zip(speckles, speckles[1:]))
    on = [s for s in D.SPECKLES if s]
    assert any((None, s) in turns for s in on) and any((s, None) in turns for s in on) and ((on[0], on[1]) in turns or (on[1], on[0]) in turns)
    # the constant and the exchanged pair each sit between two textured ones
    for i, name in enumerate(pairs):
        if name in ("constant", "exchanged"):
            assert 0 < i < len(pairs) - 1 and pairs[i - 1] in D.TEXTURED and pairs[i + 1] in D.TEXTURED, (i, name)
    assert "constant" in pairs and "exchanged" in pairs
    # a caller's frame is used while the internal one holds an earlier step's result, and the last step is semi-global (its S is read)
    assert outputs[0] == "internal" and any(a == "internal" and b == "caller" for a, b in zip(outputs, outputs[1:]))
    assert modes[-1] != "box"
    L, R = D.sequence_pairs()["exchanged"]
    assert np.array_equal(L, D.sequence_pairs()["occluding step 4/12"][1]) and np.array_equal(R, D.sequence_pairs()["occluding step 4/12"][0])
    assert all(np.ptp(a) == 0 for a in D.sequence_pairs()["constant"])
    assert not np.isfinite(D.sequence_pairs()["non-finite"][0]).all()


def _unmatched(m):
    """Interior pixels whose q is zero behind the step."""
    return m["stats"]["interior"] - int((m["fq"] != 0).sum())


def test_neighbouring_steps_differ_in_every_plane():
    steps = D.sequence_steps()
    models = [D.step_model(i) for i in range(len(steps))]
    smallest, limited = None, []
    for i in range(len(steps) - 1):
        a, b = models[i], models[i + 1]
        gone = int(((a["fq"] != 0) & (b["fq"] == 0)).sum())
        come = int(((a["fq"] == 0) & (b["fq"] != 0)).sum())
        both = int(((a["fq"] != 0) & (b["fq"] != 0) & (a["fq"] != b["fq"])).sum())
        line = f"steps {i} -> {i + 1} ({steps[i][0]}, {steps[i][1]} -> {steps[i + 1][0]}, {steps[i + 1][1]}): q non-zero -> zero {gone}, zero -> non-zero {come}"
        for count, limit, step in ((gone, _unmatched(b), steps[i + 1]), (come, _unmatched(a), steps[i])):
            if limit >= MIN_CHANGED:
                assert count >= MIN_CHANGED, line
                smallest = count if smallest is None else min(smallest, count)
            else:       # (see the module's docstring)
                assert step[0] in FEW_UNMATCHED and both >= MIN_CHANGED, (line, limit, both)
                limited.append((i, step[0], count, limit, both))
        assert gone + come + both >= 2 * MIN_CHANGED, line
        assert not np.array_equal(a["fdepth"], b["fdepth"]) and a["stats"] != b["stats"], line
        if a["S"] is not None and b["S"] is not None:
            adm = b["S"] != sgc.NONE
            share = float(((a["S"] != b["S"]) & adm).sum()) / float(adm.sum())
            assert np.array_equal(a["S"] != sgc.NONE, adm) and share >= 0.10, (line, share)
            line += f", S differs on {100 * share:.1f} % of its admissible entries"
        print(line)
    print(f"{len(steps) - 1} consecutive step pairs; the smallest count of changed pixels held to {MIN_CHANGED}: {smallest}")
    for i, name, count, limit, both in limited:
        print(f"steps {i} -> {i + 1}: '{name}' leaves {limit} interior pixels unmatched, so {count} pixels change that way; {both} pixels matched "
              "in both steps differ")
    assert smallest >= MIN_CHANGED and len(limited) <= 3 and {name for _, name, _, _, _ in limited} <= set(FEW_UNMATCHED)
    assert all(_unmatched(D._step_model(name, mode, None)) < MIN_CHANGED for name in FEW_UNMATCHED for mode in ("sgm8", "sgm4"))
    assert _unmatched(D._step_model("shift 5", "box", None)) < MIN_CHANGED and not D._step_model("constant", "box", None)["fq"].any()


def test_the_filter_has_work_wherever_it_is_on():
    seen = 0
    for i, (pair, mode, speckle, _) in enumerate(D.sequence_steps()):
        m = D.step_model(i)
        if speckle:
            s = m["M"]["stats"]
            assert s["removed_pixels"] > 0 and s["guard"] == 0 and s["pixels"] == m["stats"]["matched"], (i, pair, s)
            assert not np.array_equal(m["fq"], m["q"]) and not np.array_equal(m["fdepth"], m["depth"])
            seen += 1
        else:
            assert m["M"] is None and m["fq"] is m["q"]
    assert seen >= 5


# ---- the drive --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drives():
    return {front: (D.stereo_drive(front), D.stereo_drive_model(front)) for front in D.FRONTS}


def errors(c, m):
    """Per tracked frame with status 0: (k, translation error in metres, rotation error in degrees) against the true pose."""
    return [(k,) + pose_error(r["pose"], c["poses"][k]) for k, r in enumerate(m["frames"]) if k > 0 and r["status"] == 0]


def test_drive_is_the_follow_track_drive_seen_by_two_cameras():
    import volume_follow_track_cases as F
    c, a = D.stereo_drive("box"), F.drive("A")
    assert all(np.array_equal(x, y) for x, y in zip(c["poses"], a["poses"][:D.N_FRAMES])) and c["p"] == a["p"] and c["follow"] == a["follow"]
    assert c["ic"] == a["ic"] and c["ic"]["min_eig_ratio"] == 0.0
    assert all(np.array_equal(x, y) for x, y in zip(c["left"][:4], a["gray"][:4]))
    assert D.stereo_drive("sgm")["sg"] == dict(p1=100, p2=600, paths=8) and c["sg"] is None and c["speckle"] == (16, 100)
    mp = c["mp"]
    assert (mp["dmin"], mp["dmax"], mp["A"], mp["uniq"], mp["lr_max"], mp["max_raw"], mp["baseline"]) == (4, 51, 2, 10, 1, 5000, 0.5)
    assert all(x.shape == (120, 160) and x.dtype == np.float32 for x in c["left"] + c["right"])


@pytest.mark.parametrize("front", D.FRONTS)
def test_drives_track(drives, front):
    c, m = drives[front]
    e = errors(c, m)
    for (k, et, er), r in zip(e, [r for r in m["frames"][1:] if r["status"] == 0]):
        print(f"{front} frame {k}: {et * 1e3:.2f} mm {er:.3f} deg, pairs {r['pairs']:.0f}, hits {r['hits']}, steps {r['iterations']}, d {r['d']}, off {r['off']}")
    kt, worst_t = max(((k, et) for k, et, _ in e), key=lambda x: x[1])
    kr, worst_r = max(((k, er) for k, _, er in e), key=lambda x: x[1])
    print(f"{front}: largest {worst_t * 1e3:.3f} mm (frame {kt}) {worst_r:.4f} deg (frame {kr}); {m['shifts']} shifts, the window ends at {m['off']}; "
          f"the front end's models took {c['seconds']:.1f} s, the closed loop {m['seconds']:.1f} s")
    sighted = [k for k in range(D.N_FRAMES) if k not in D.BLIND]
    assert [k for k, _, _ in e] == sighted[1:] and all(m["frames"][k]["status"] == 0 for k in sighted)
    assert m["shifts"] >= 4 and m["shifts"] == sum(r["d"] != (0, 0, 0) for r in m["frames"])
    assert m["frames"][-1]["fused"] == len(sighted) and m["points"]["dropped"] == 0
    assert worst_t <= 2 * MEASURED[front][0] and worst_r <= 2 * MEASURED[front][1]
    assert c["seconds"] + m["seconds"] <= MODEL_SECONDS


@pytest.mark.parametrize("front", D.FRONTS)
def test_blind_frame_is_refused_and_changes_nothing(drives, front):
    c, m = drives[front]
    (b,) = D.BLIND
    assert b == 4 and all(np.ptp(a) == 0 and a[0, 0] == 90.0 for a in (c["left"][b], c["right"][b]))
    s = c["frames"][b]["stats"]
    print(front, "blind frame:", s)
    assert not c["frames"][b]["fdepth"].any() and not c["frames"][b]["depth"].any() and not c["depth"][b].any() and s["matched"] == 0
    # the two rules reject it for different reasons: not unique (box); matched at dmin and then out of range (semi-global)
    assert s["interior"] == 15840 and ((s["rej_unique"], s["rej_range"]) == ((15840, 0) if front == "box" else (220, 15620)))
    before, blind, after = m["frames"][b - 1], m["frames"][b], m["frames"][b + 1]
    assert blind["status"] == 1 and blind["pairs"] == 0 and np.isnan(blind["pose"]).all() and blind["hits"] > 0
    assert blind["off"] == before["off"] and blind["fused"] == before["fused"] and blind["d"] == (0, 0, 0)
    assert np.array_equal(bits(blind["good"]), bits(before["good"])) and np.array_equal(bits(before["good"]), bits(before["pose"]))
    assert after["status"] == 0 and after["fused"] == before["fused"] + 1


@pytest.mark.parametrize("front", D.FRONTS)
def test_matcher_and_filter_have_work_on_every_sighted_frame(drives, front):
    c, _ = drives[front]
    for k, fr in enumerate(c["frames"]):
        if k in D.BLIND:
            continue
        share, s = fr["stats"]["matched"] / fr["q"].size, fr["M"]["stats"]
        print(f"{front} frame {k}: {100 * share:.1f} % matched, the filter removes {s['removed_pixels']} pixels in {s['removed_components']} components")
        assert 0.35 <= share <= 0.65 and s["removed_pixels"] > 0 and s["guard"] == 0 and s["pixels"] == fr["stats"]["matched"]
        if front == "sgm":
            assert fr["S"].shape == (120, 160, 48)


def test_the_front_ends_end_in_different_pose_bits(drives):
    (cb, mb), (cs, ms) = drives["box"], drives["sgm"]
    assert not np.array_equal(bits(mb["frames"][-1]["pose"]), bits(ms["frames"][-1]["pose"]))
    differ = [k for k in range(D.N_FRAMES) if not np.array_equal(cb["frames"][k]["fdepth"], cs["frames"][k]["fdepth"])]
    poses = [k for k in range(1, D.N_FRAMES) if k not in D.BLIND and not np.array_equal(bits(mb["frames"][k]["pose"]), bits(ms["frames"][k]["pose"]))]
    print("depth frames differ on frames", differ, "poses on frames", poses)
    assert differ == [k for k in range(D.N_FRAMES) if k not in D.BLIND] and poses == differ[1:]
    assert not np.array_equal(mb["q"], ms["q"])
