"""The closed loop of the TSDF volume without a GPU: the composed model of tests/volume_follow_track_cases.py on its two drives. What the
drives are there for holds on the model: both track, drive A's window leaves the box it started in by more than its own depth, its
blind frame is refused and changes nothing and the frame behind it recovers, drive B's window returns to where it started and the
re-entry store changes what its return leg tracks against, the kernels' order of the sums stays within the bound of any order on every
frame, and the same corridor in 2.5 cm voxels shows what a closed loop needs min_eig_ratio for.

The model is the yardstick of tests/test_gpu_volume_follow_track.py, which asks the GPU for the same bits."""
import time

import numpy as np
import pytest

import volume_follow_track_cases as F
from test_volume_cpu import bits
from test_volume_icp_cpu import REFUSAL_RATIO, pose_error

f32 = np.float32

# Measured with this model (test_both_drives_track prints them): the largest errors against the true poses over a drive, every frame
# started from the pose the model returned for the frame before it. The assertions here and in tests/test_gpu_volume_follow_track.py
# are twice these.
MEASURED_A_T_M = 0.004885         # frame 13
MEASURED_A_R_DEG = 0.08190        # frame 17
MEASURED_B_T_M = 0.003734         # frame 1
MEASURED_B_R_DEG = 0.05190        # frame 14
MEASURED_B_REENTRY_T_M = 0.004132      # frame 18
MEASURED_B_REENTRY_R_DEG = 0.06256     # frame 18
MEASURED = {("A", False): (MEASURED_A_T_M, MEASURED_A_R_DEG), ("B", False): (MEASURED_B_T_M, MEASURED_B_R_DEG),
            ("B", True): (MEASURED_B_REENTRY_T_M, MEASURED_B_REENTRY_R_DEG)}
MODEL_SECONDS = 60.0              # a guard against a model that got slow, not a measurement: the runs take 3 to 5 s


def errors(name, m):
    """Per tracked frame with status 0: (k, translation error in metres, rotation error in degrees) against the true pose."""
    c = F.drive(name)
    return [(k,) + pose_error(r["pose"], c["poses"][k]) for k, r in enumerate(m["frames"]) if k > 0 and r["status"] == 0]


def timed(name, **kw):
    t = time.time()
    m = F.model(name, **kw)
    return m, time.time() - t


@pytest.fixture(scope="module")
def models():
    """(name, reentry) -> (model, seconds). The point store is on in all three, as in the GPU tests."""
    return {("A", False): timed("A", spill=True), ("B", False): timed("B", spill=True), ("B", True): timed("B", reentry=True, spill=True)}


def test_both_drives_track(models):
    for key, (m, seconds) in models.items():
        e = errors(key[0], m)
        for (k, et, er), r in zip(e, [r for r in m["frames"][1:] if r["status"] == 0]):
            print(f"{key} frame {k}: {et * 1e3:.2f} mm {er:.3f} deg, pairs {r['pairs']:.0f}, hits {r['hits']}, ratio "
                  f"{r['eig_min'] / r['eig_max']:.2e}, steps {r['iterations']}, d {r['d']}, off {r['off']}")
        kt, worst_t = max(((k, et) for k, et, _ in e), key=lambda x: x[1])
        kr, worst_r = max(((k, er) for k, _, er in e), key=lambda x: x[1])
        print(f"{key}: largest {worst_t * 1e3:.3f} mm (frame {kt}) {worst_r:.4f} deg (frame {kr}); {m['shifts']} shifts, the window ends at "
              f"{m['off']}; the model took {seconds:.1f} s")
        assert len(e) == len(m["frames"]) - 1 - len(F.drive(key[0])["blind"])
        assert worst_t <= 2 * MEASURED[key][0] and worst_r <= 2 * MEASURED[key][1]
        assert seconds <= MODEL_SECONDS


def test_drive_a_leaves_its_window_behind(models):
    m = models[("A", False)][0]
    p = F.drive("A")["p"]
    assert m["shifts"] >= 20 and m["shifts"] == sum(r["d"] != (0, 0, 0) for r in m["frames"])
    assert m["off"][2] >= p["dims"][2], m["off"]                     # every voxel of the first window has left
    assert len(m["points"]["xyz0"]) > 0 and m["points"]["dropped"] == 0
    assert m["frames"][-1]["fused"] == len(m["frames"]) - 1


def test_drive_a_blind_frame_is_refused_and_changes_nothing(models):
    m = models[("A", False)][0]
    (b,) = F.drive("A")["blind"]
    before, blind, after = m["frames"][b - 1], m["frames"][b], m["frames"][b + 1]
    assert blind["status"] == 1 and blind["iterations"] == 1 and blind["pairs"] == 0 and np.isnan(blind["pose"]).all()
    assert blind["hits"] > 0                                           # the model frame was there: the sensor's frame was not
    assert blind["off"] == before["off"] and blind["fused"] == before["fused"] and blind["d"] == (0, 0, 0)
    assert np.array_equal(bits(blind["good"]), bits(before["good"]))
    assert all(np.array_equal(x, y) for x, y in zip(blind["grid"], before["grid"]))
    assert after["status"] == 0 and after["fused"] == before["fused"] + 1
    assert not all(np.array_equal(x, y) for x, y in zip(after["grid"], before["grid"]))


@pytest.mark.parametrize("reentry", [False, True])
def test_drive_b_returns_to_where_it_started(models, reentry):
    m = models[("B", reentry)][0]
    assert m["off"] == (0, 0, 0) and m["shifts"] >= 10
    assert max(r["off"][2] for r in m["frames"]) >= 20
    if reentry:
        s = m["reentry"]
        print({k: s[k] for k in ("live", "saved", "restored", "dropped")})
        assert s["restored"] > 0 and s["dropped"] == 0 and s["live"] < F.REENTRY_CAPACITY


def test_reentry_changes_what_the_return_leg_tracks_against(models):
    """The voxels that a shift brings back are what the next ray-cast tracks against: on the return leg the model with the re-entry
    store hits more pixels and pairs more of them than the model without, and the poses differ from the first such frame on."""
    plain, store = models[("B", False)][0]["frames"], models[("B", True)][0]["frames"]
    turn = F.DRIVES["B"]["n"]                                          # the first frame of the return leg
    first = None
    for k, (a, b) in enumerate(zip(plain, store)):
        same = np.array_equal(bits(a["pose"]), bits(b["pose"]))
        print(f"frame {k}: hits {a['hits']} / {b['hits']}, pairs {a.get('pairs', 0):.0f} / {b.get('pairs', 0):.0f}, poses "
              f"{'equal' if same else 'differ'}")
        if first is None and not same:
            first = k
    # up to the turn nothing has come back, and the first shift back restores voxels that the ray-cast of the frame behind it sees
    assert first is not None and first > turn
    assert all(a["hits"] == b["hits"] and a["off"] == b["off"] for a, b in zip(plain[:first], store[:first]))
    more = [k for k in range(turn, len(plain)) if store[k]["hits"] > plain[k]["hits"] and store[k]["pairs"] > plain[k]["pairs"]]
    assert more and more[0] == first, (first, more)
    assert len(more) >= (len(plain) - first) // 2


def test_kernel_order_sums_stay_within_the_bound_of_any_order(models):
    """Every evaluation of every frame: the kernels' order against fp64 pairwise sums of the same exact terms, as a fraction of
    n 2^-52 sum |terms| (the bound of tests/test_gpu_volume_icp.py)."""
    for key, (m, _) in models.items():
        ratios = [r["sum_ratio"] for r in m["frames"][1:]]
        print(key, "largest |kernel order - pairwise| / bound per frame:", " ".join(f"{x:.3f}" for x in ratios))
        assert all(x <= 1.0 for x in ratios)
        assert sum(x > 0 for x in ratios) >= len(ratios) - 1          # (the orders do differ; the blind frame has no terms)


def test_pairwise_sums_track_the_same(models):
    """The same loop with fp64 pairwise sums over drive B's way out: the same shifts and pairs, and poses whose entries lie within
    1e-5 of those of the kernels' order. The two differ in the last bits of fp64 sums alone, which the step rounds to fp32: 1e-5 is
    forty ulp of a translation of 3 m, and four hundred times below the tracking error (pose_error's angle cannot show it: its arccos
    has a floor of 0.007 degrees on fp32 rotations)."""
    n = F.DRIVES["B"]["n"]
    other = F.drive_model("B", sums="pairwise", frames=n)["frames"]
    for k, (a, b) in list(enumerate(zip(models[("B", False)][0]["frames"][:n], other)))[1:]:
        apart = float(np.abs(a["pose"].astype(np.float64) - b["pose"]).max())
        print(f"frame {k}: the poses' entries differ by at most {apart:.2e}")
        assert a["off"] == b["off"] and a["status"] == b["status"] == 0 and a["pairs"] == b["pairs"]
        assert apart <= 1e-5


def test_fine_voxels_slide_where_the_refusal_ratio_says_so():
    """The same corridor and drive in 2.5 cm voxels: five frames track, then the model slides along the
    corridor by 0.19 m at frame 6 and does not come back. The alignments that slide are the ones whose eig_min / eig_max lies below
    REFUSAL_RATIO: with min_eig_ratio set to it they are refused (the rule of icp_align_model), and the frames before them are not.
    Measured with this model: errors of 2.6 to 22 mm and ratios of 4.3e-3 to 6.4e-3 over frames 1 to 5; 190 mm at 1.34e-3 and 355 mm
    at 9.8e-4 for frames 6 and 7."""
    t = time.time()
    m = F.model("fine")
    seconds = time.time() - t
    rows = []
    for k, et, er in errors("fine", m):
        r = m["frames"][k]
        refused = r["eig_min"] < float(f32(REFUSAL_RATIO)) * r["eig_max"]
        print(f"frame {k}: {et * 1e3:.1f} mm {er:.3f} deg, ratio {r['eig_min'] / r['eig_max']:.2e}, pairs {r['pairs']:.0f}, off {r['off']}"
              f"{', refused under REFUSAL_RATIO' if refused else ''}")
        rows.append((k, et, refused))
    print(f"the model took {seconds:.1f} s")
    assert [k for k, _, refused in rows if refused] == [6, 7]
    # tracked: within two of these voxels; slid: by more than the follow rule's threshold of four
    assert all(et < 0.05 for k, et, _ in rows if k < 6) and all(et > 0.1 for k, et, _ in rows if k >= 6)
    assert seconds <= MODEL_SECONDS
