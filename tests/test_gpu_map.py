"""The keyframe point-cloud map on the GPU (odo_map_*, api.PointMap) against a numpy reference of its spec (include/odometry_hip.h):
candidates, back-projection, world points, the voxel filter's first-occurrence rule, the capacity clamp and the counters, bit for
bit; the world/camera convention against ground-truth depth; and the tracker's own insertions against standalone ones."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROWS, COLS = 376, 1241
K = (718.856, 607.1928, 185.2157)


# ---- numpy reference of the spec ------------------------------------------------------------------------------------------
def ref_candidates(val, dep):
    d = dep.astype(np.float32).reshape(-1)
    ok = ~(np.abs(d - np.float32(0)) < np.float32(0.01)) & (d > 0)
    if val is not None:
        ok &= val.reshape(-1) != 0
    return np.nonzero(ok)[0]


def ref_world(pix, dep, A, cols=COLS, k=K):
    f0, cx, cy = (np.float32(v) for v in k)
    x = (pix % cols).astype(np.float32)
    y = (pix // cols).astype(np.float32)
    z = np.float32(1) / dep.reshape(-1)[pix].astype(np.float32)
    X = (z * (x - cx)) / f0
    Y = (z * (y - cy)) / f0
    a = np.asarray(A, np.float32).T.reshape(16)   # column-major
    return [((a[r] * X + a[4 + r] * Y) + a[8 + r] * z) + a[12 + r] for r in range(3)]


class RefMap:
    def __init__(self, capacity, voxel, cols=COLS, k=K):
        self.cap, self.voxel = capacity, np.float32(voxel)
        self.cols, self.k = cols, k
        self.xyzi, self.kp = np.zeros((0, 4), np.float32), np.zeros((0, 2), np.int32)
        self.keys = np.zeros(0, np.int64)
        self.st = dict(size=0, insertions=0, candidates=0, dropped_voxel=0, dropped_range=0, dropped_capacity=0)

    def insert(self, val, dep, img, A):
        ins = self.st["insertions"]
        self.st["insertions"] += 1
        if self.st["size"] >= self.cap:
            return
        pix = ref_candidates(val, dep)
        w = ref_world(pix, dep, A, self.cols, self.k)
        self.st["candidates"] += len(pix)
        keep = np.ones(len(pix), bool)
        if self.voxel > 0:
            q = [np.floor(c / self.voxel) for c in w]
            inr = np.all([np.abs(c) < np.float32(2 ** 20) for c in q], axis=0)
            self.st["dropped_range"] += int((~inr).sum())
            kk = [np.where(inr, c, 0).astype(np.int64) + 2 ** 20 for c in q]
            key = kk[0] | (kk[1] << 21) | (kk[2] << 42)
            first = np.zeros(len(pix), bool)
            _, idx = np.unique(np.where(inr, key, -1), return_index=True)
            first[idx] = True
            keep = inr & first & ~np.isin(key, self.keys)
            self.keys = np.concatenate([self.keys, key[keep]])
            self.st["dropped_voxel"] += int(inr.sum() - keep.sum())
        sel = np.nonzero(keep)[0]
        room = self.cap - self.st["size"]
        self.st["dropped_capacity"] += max(0, len(sel) - room)
        sel = sel[:room]
        I = np.zeros(len(sel), np.float32) if img is None else img.reshape(-1)[pix[sel]].astype(np.float32)
        rec = np.stack([w[0][sel], w[1][sel], w[2][sel], I], axis=1).astype(np.float32)
        self.xyzi = np.concatenate([self.xyzi, rec])
        self.kp = np.concatenate([self.kp, np.stack([np.full(len(sel), ins), pix[sel]], axis=1).astype(np.int32)])
        self.st["size"] += len(sel)


def assert_same(m, ref):
    xyzi, kp = m.points()
    assert xyzi.shape == ref.xyzi.shape, (xyzi.shape, ref.xyzi.shape)
    assert np.array_equal(kp, ref.kp), "keyframe / pixel records differ"
    assert np.array_equal(xyzi.view(np.uint32), ref.xyzi.view(np.uint32)), "point records differ"
    assert m.stats() == ref.st, (m.stats(), ref.st)


@pytest.fixture(scope="module")
def seq5():
    from odometry_amd import synth
    seq = synth.make_sequence(5, with_depth=True)
    seq["inv"] = [synth.semi_dense_inverse_depth(Z, L) for Z, L in zip(seq["depth"], seq["left"])]
    return seq


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def test_one_insertion_without_the_filter_equals_the_reference(ctx, seq5):
    from odometry_amd import api
    inv, img = seq5["inv"][0], seq5["left"][0]
    val = (np.random.default_rng(3).random((ROWS, COLS)) < 0.8).astype(np.uint8)
    A = seq5["poses"][2].astype(np.float32)
    m = api.PointMap(ctx, ROWS, COLS, 1_000_000, 0.0)
    m.insert(val, inv, img, K, A)
    ref = RefMap(1_000_000, 0.0)
    ref.insert(val, inv, img, A)
    assert ref.st["size"] > 10_000
    assert_same(m, ref)
    assert np.array_equal(m.keyframe_pose(0), A)
    m.close()


def test_five_keyframes_with_the_voxel_filter_equal_the_reference(ctx, seq5):
    from odometry_amd import api
    m = api.PointMap(ctx, ROWS, COLS, 2_000_000, 0.1)
    ref = RefMap(2_000_000, 0.1)
    for k in range(5):
        A = seq5["poses"][k].astype(np.float32)
        m.insert(None, seq5["inv"][k], seq5["left"][k], K, A)
        ref.insert(None, seq5["inv"][k], seq5["left"][k], A)
    assert ref.st["dropped_voxel"] > 0 and ref.st["size"] > 10_000
    assert_same(m, ref)
    for k in range(5):
        assert np.array_equal(m.keyframe_pose(k), seq5["poses"][k].astype(np.float32))
    # convention: the map's world points moved into frame 0's camera land on frame 0's ground-truth depth
    xyzi, _ = m.points()
    T0 = np.linalg.inv(seq5["poses"][0])
    P = (T0[:3, :3] @ xyzi[:, :3].T.astype(np.float64) + T0[:3, 3:4]).T
    P = P[P[:, 2] > 0.5]
    u = np.floor(K[0] * P[:, 0] / P[:, 2] + K[1] + 0.5).astype(int)
    v = np.floor(K[0] * P[:, 1] / P[:, 2] + K[2] + 0.5).astype(int)
    inside = (u >= 0) & (u < COLS) & (v >= 0) & (v < ROWS)
    assert inside.sum() > 5_000
    Zgt = seq5["depth"][0][v[inside], u[inside]]
    rel = np.abs(P[inside, 2] - Zgt) / P[inside, 2]
    assert np.median(rel) < 1e-2, np.median(rel)
    m.close()


def test_capacity_clamps_then_insertions_are_no_ops_and_clear_restarts(ctx, seq5):
    from odometry_amd import api
    big = RefMap(10 ** 7, 0.1)
    for k in range(2):
        big.insert(None, seq5["inv"][k], seq5["left"][k], seq5["poses"][k])
    cap = big.st["size"] - 1234
    assert cap > big.kp[:, 0].tolist().count(0)   # the clamp falls inside the second insertion
    m = api.PointMap(ctx, ROWS, COLS, cap, 0.1)
    ref = RefMap(cap, 0.1)
    for k in range(4):
        A = seq5["poses"][k].astype(np.float32)
        m.insert(None, seq5["inv"][k], seq5["left"][k], K, A)
        ref.insert(None, seq5["inv"][k], seq5["left"][k], A)
    assert ref.st["dropped_capacity"] == 1234 and ref.st["insertions"] == 4
    assert np.array_equal(ref.xyzi, big.xyzi[:cap])
    assert_same(m, ref)
    m.clear()
    assert m.stats() == dict(size=0, insertions=0, candidates=0, dropped_voxel=0, dropped_range=0, dropped_capacity=0)
    ref = RefMap(cap, 0.1)
    A = seq5["poses"][3].astype(np.float32)
    m.insert(None, seq5["inv"][3], seq5["left"][3], K, A)
    ref.insert(None, seq5["inv"][3], seq5["left"][3], A)
    assert_same(m, ref)
    m.close()


def test_points_beyond_the_key_range_are_dropped_and_counted(ctx, seq5):
    from odometry_amd import api
    m = api.PointMap(ctx, ROWS, COLS, 1_000_000, 0.1)
    ref = RefMap(1_000_000, 0.1)
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 1e6
    for A in (seq5["poses"][1].astype(np.float32), far):
        m.insert(None, seq5["inv"][1], None, None, A)
        ref.insert(None, seq5["inv"][1], None, A)
    st = m.stats()
    assert st["dropped_range"] == len(ref_candidates(None, seq5["inv"][1])) > 0
    assert_same(m, ref)
    assert np.all(m.points()[0][:, 3] == 0)   # no image: intensity 0
    m.close()


# ---- the tracker's insertions ------------------------------------------------------------------------------------------------
N_TRACK = 60


@pytest.fixture(scope="module")
def natural():
    import bench
    return bench.render_sequence(N_TRACK, 0, min(8, os.cpu_count() or 1), drive="natural")


def _run(seq, hints, with_map, record=False):
    """Tracks the first N_TRACK frames; returns the poses, and (with_map) the map, or (record) the keyframes' inputs."""
    from odometry_amd import api
    trk = api.Tracker(0)
    dev = [(trk.upload_frame(l), trk.upload_frame(r)) for l, r in zip(seq["left"][:N_TRACK], seq["right"][:N_TRACK])]
    m = None
    if with_map:
        m = api.PointMap(trk, ROWS, COLS, 3_000_000, 0.05)
        trk.attach_map(m)
    kfs = []

    def keep(frame, pose):
        if record:
            val, _, dep = trk.outputs(ROWS, COLS)
            kfs.append((frame, val, dep, pose))

    trk.init(*dev[0])
    keep(0, np.eye(4, dtype=np.float32))
    poses = []
    for k in range(1, N_TRACK):
        if hints and k + 1 < N_TRACK:
            trk.hint_next(*dev[k + 1])
        g = trk.track(*dev[k])
        poses.append((g["pose_to_keyframe"], g["abs_pose"]))
        if g["new_keyframe"]:
            keep(k, g["abs_pose"])
    n_kf = trk.stats()["n_keyframes"]
    return trk, m, poses, kfs, n_kf


@pytest.mark.parametrize("hints", [True, False])
def test_the_tracker_inserts_every_keyframe_and_changes_no_pose(natural, hints):
    from odometry_amd import api
    trk0, _, poses0, kfs, n_kf0 = _run(natural, hints, False, record=True)
    trk, m, poses, _, n_kf = _run(natural, hints, True)
    assert n_kf == n_kf0 == len(kfs) >= 3
    for (a, b), (c, d) in zip(poses0, poses):
        assert np.array_equal(a, c) and np.array_equal(b, d), "the map changed a pose"
    st = m.stats()
    assert st["insertions"] == n_kf
    # the same keyframes inserted by hand: mask, inverse depth, level-0 pyramid image, abs_pose
    m2 = api.PointMap(trk0, ROWS, COLS, 3_000_000, 0.05)
    ref = RefMap(3_000_000, 0.05)
    for i, (fr, val, dep, pose) in enumerate(kfs):
        img = api.ImagePyramid(4, natural["left"][fr], True).GetPyramidImage(0)
        m2.insert(val, dep, img, None, pose)
        ref.insert(val, dep, img, pose)
        assert np.array_equal(m.keyframe_pose(i), pose.astype(np.float32))
    assert_same(m2, ref)
    assert_same(m, ref)
    trk.attach_map(None)
    m.close(); m2.close()
    trk.close(); trk0.close()


def test_reinit_continues_the_numbering_detach_stops_and_destroy_refuses_while_attached(natural):
    from odometry_amd import api, _lib
    trk = api.Tracker(0)
    dev = [(trk.upload_frame(l), trk.upload_frame(r)) for l, r in zip(natural["left"][:12], natural["right"][:12])]
    m = api.PointMap(trk, ROWS, COLS, 3_000_000, 0.0)
    trk.attach_map(m)
    trk.init(*dev[0])
    for k in range(1, 6):
        trk.track(*dev[k])
    n1 = m.stats()["insertions"]
    assert n1 == trk.stats()["n_keyframes"]
    assert trk.lib.odo_map_destroy(m.h) == -1 and "attached" in _lib.last_error()
    trk.init(*dev[6])
    st = m.stats()
    assert st["insertions"] == n1 + 1
    _, kp = m.points()
    assert kp[-1, 0] == n1 and kp[0, 0] == 0      # frame 6 is keyframe n1 of the map
    trk.attach_map(None)
    for k in range(7, 12):
        trk.track(*dev[k])
    assert m.stats() == st                        # detached: nothing more goes in
    trk.close()
    assert trk.lib.odo_map_destroy(m.h) == 0
    m.h = None
