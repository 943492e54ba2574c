"""Frame-to-model tracking of the TSDF volume on the GPU (odo_volume_icp_eval_dev, odo_volume_icp_align_dev, odo_volume_track_dev,
api.TsdfVolume.icp_eval / align / track) against the numpy model and the host build of tests/test_volume_icp_cpu.py: the rows bit for
bit across frame sizes round the launch tile and every branch row, the sums within the bound of any summation order and bit-identical
from call to call, every step of an alignment against the host build's step, the ground truth and the refusal of the CPU test, the
early stop, track against ray-cast + align, the volume's state, the ordering between integrations and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import se3_log_norm
from test_gpu_volume import _grid_equal, _volume
from test_volume_cpu import _pose, bits, empty_grid, integrate_model
from test_volume_icp_cpu import (MEASURED_R_DEG, MEASURED_T_M, NACC, REFUSAL_RATIO, ROOT, bad_params, branch_rows, build_host_library,
                                 corridor_sequence, host_step, icp, icp_acc, icp_acc_kernel_order, icp_align_model, icp_frame, icp_rows_model, pose_error,
                                 random_frames, ribbed_sequence, rows_equal)

pytestmark = pytest.mark.gpu
f32 = np.float32


def _constant(name):
    src = open(os.path.join(ROOT, "odometry_amd", "csrc", "volume_icp.hip.h")).read()
    return int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))


TILE, BLOCK = _constant("kIcpTile"), _constant("kIcpBlock")       # a block is TILE x TILE lattice points, a wave TILE x (64 / TILE)
assert TILE * TILE == BLOCK and 64 % TILE == 0
SIZES = [(1, 1), (64 // TILE, TILE), (TILE, TILE), (TILE + 1, TILE), (TILE, TILE + 1), (17, 23), (64, 1), (1, 64), (65, 33), (120, 160)]
CASES = [(size, s) for size in SIZES for s in (1, 2, 4)]
CASES += [((r * s + dr, c * s + dc), s) for s in (2, 4) for r, c in [(TILE, TILE)] for dr, dc in ((0, 0), (1, 0), (0, 1))]   # the same seams on the stride's lattice


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_library(tmp_path_factory.mktemp("icp_host"))


def _check_eval(vol, p, raw, depth, nrmw, P_m, Cm, stride, dist_max, huber, tag):
    """rows_dev (into a buffer pre-filled with 0xAB) against the model bit for bit, acc within the bound of any summation order of
    the model's exact terms, two calls bit-identical. Returns the number of pairs."""
    M = icp_frame(P_m, P_m)[0]
    want, mask = icp_rows_model(raw, depth, nrmw, M, Cm, p, stride, dist_max, huber)
    acc, got = vol.icp_eval(raw, depth, nrmw, P_m, Cm, stride=stride, dist_max=dist_max, huber_delta=huber, rows=True)
    rows_equal(got, want, tag)
    s, mag = icp_acc(want, mask)
    n = int(mask.sum())
    assert acc[28] == n, (tag, acc[28], n)
    bound = n * 2.0 ** -52 * mag
    print(f"{tag}: {n} pairs, largest |acc - sum| / bound {np.max(np.abs(acc - s)[bound > 0] / bound[bound > 0]) if (bound > 0).any() else 0:.3f}")
    assert (np.abs(acc - s) <= bound).all(), (tag, acc - s, bound)
    order = icp_acc_kernel_order(want, mask, stride)
    assert np.array_equal(acc.view(np.uint64), order.view(np.uint64)), (tag, acc - order)
    again = vol.icp_eval(raw, depth, nrmw, P_m, Cm, stride=stride, dist_max=dist_max, huber_delta=huber)
    assert np.array_equal(acc.view(np.uint64), again.view(np.uint64)), tag
    return n


@pytest.mark.parametrize("size,stride", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_rows_and_sums_across_frame_sizes(ctx, size, stride):
    rows, cols = size
    K = (1.3 * max(rows, cols, 8), (cols - 1) / 2, (rows - 1) / 2)
    pairs = 0
    # a frame one pixel high or wide keeps its pairs only under a motion along its long side
    motion = ((0, 0, 0), (0.004, 0.0, 0.01)) if rows == 1 else ((0, 0, 0), (0.0, 0.004, 0.01)) if cols == 1 else None
    for seed in range(2):
        p, raw, depth, nrmw, P_m, P_init = random_frames(seed, size, K, *([motion] if motion else []))
        vol = _volume(ctx, p)
        pairs += _check_eval(vol, p, raw, depth, nrmw, P_m, icp_frame(P_m, P_init)[1], stride, 0.3, 0.02 * seed, f"{size} stride {stride}")
        vol.close()
    assert pairs > 0 or rows * cols == 1


@pytest.mark.parametrize("row", branch_rows(), ids=lambda r: r[0])
def test_every_branch_row(ctx, row):
    name, p, raw, depth, nrmw, M, Cm, stride, dist_max, huber, _ = row
    assert np.array_equal(M, np.eye(4))
    vol = _volume(ctx, p)
    _check_eval(vol, p, raw, depth, nrmw, np.eye(4), Cm, stride, dist_max, huber, name)
    vol.close()


# ---- the alignment ---------------------------------------------------------------------------------------------------------------
def _c_params(ic):
    from odometry_amd import _lib as L
    cp = L.IcpParams()
    cp.levels = len(ic["strides"])
    for i, (s, n) in enumerate(zip(ic["strides"], ic["iters"])):
        cp.stride[i], cp.iters[i] = s, n
    cp.dist_max, cp.huber_delta, cp.eps_t, cp.eps_r = ic["dist_max"], ic["huber_delta"], ic["eps_t"], ic["eps_r"]
    cp.min_pairs, cp.min_eig_ratio = ic["min_pairs"], ic["min_eig_ratio"]
    return cp


def _fused(ctx, seq, n):
    """A volume with frames 0 .. n - 1 of the sequence fused at their true poses."""
    vol = _volume(ctx, seq["p"])
    for k in range(n):
        vol.integrate(seq["depth"][k], seq["poses"][k])
    return vol


@pytest.fixture(scope="module")
def ribbed():
    return ribbed_sequence()


def _check_trace(vol, host, raw, depth, nrmw, P_m, P_init, ic, res, trace):
    """Every step: acc is icp_eval at the C before it, delta and C are the host build's icp_step on that acc, all bit for bit."""
    step = host_step(host)
    Cm = icp_frame(P_m, P_init)[1]
    for t in trace:
        acc = vol.icp_eval(raw, depth, nrmw, P_m, Cm, stride=ic["strides"][t["level"]], dist_max=ic["dist_max"], huber_delta=ic["huber_delta"])
        assert np.array_equal(acc.view(np.uint64), t["acc"].view(np.uint64)), t["iteration"]
        failed, _, delta, Cm = step(acc, Cm, ic["min_pairs"], ic["eps_t"], ic["eps_r"])
        assert np.array_equal(bits(delta), bits(t["delta"])) and np.array_equal(bits(Cm), bits(t["C"])), t["iteration"]
        assert bool(failed) == (res["status"] == 1 and t is trace[-1])
    assert np.array_equal(bits(res["C"]), bits(Cm)) and res["iterations"] == len(trace)


def test_align_step_by_step_and_against_the_model(ctx, host, ribbed):
    """Frame 3 of the ribbed corridor against the volume of frames 0 .. 2, with and without the Huber weight."""
    p, k = ribbed["p"], 3
    vol = _fused(ctx, ribbed, k)
    P_m = ribbed["poses"][k - 1]
    depth, nrmw = vol.raycast(P_m)
    raw = ribbed["depth"][k]
    for huber in (0.0, 0.01):
        ic = icp(p=p, huber_delta=huber)
        pose, res, trace = vol.align(raw, depth, nrmw, P_m, P_m, trace=True, params=_c_params(ic))
        assert res["status"] == 0 and 10 <= len(trace) <= sum(ic["iters"])
        _check_trace(vol, host, raw, depth, nrmw, P_m, P_m, ic, res, trace)
        want = icp_align_model(raw, depth, nrmw, P_m, P_m, p, ic, step=host_step(host))
        d = se3_log_norm(want["abs_pose"], pose)
        print(f"huber {huber}: {len(trace)} steps, ||log|| against the model's loop {d:.2e}, pairs {res['pairs']:.0f}")
        assert want["status"] == 0 and d < 1e-5
        assert res["pairs"] == want["pairs"] and abs(res["eig_min"] - want["eig_min"]) <= 1e-9 * want["eig_max"]
        assert abs(res["eig_max"] - want["eig_max"]) <= 1e-9 * want["eig_max"]
        assert pose.dtype == f32 and pose.shape == (4, 4)
    vol.close()


def test_ribbed_corridor_stays_inside_the_cpu_tests_bounds(ctx, ribbed):
    """The CPU test's procedure on the GPU: frames 0 .. k - 1 fused at their true poses, frame k tracked from pose k - 1, k = 1 .. 6."""
    vol = _volume(ctx, ribbed["p"])
    for k in range(1, 7):
        vol.integrate(ribbed["depth"][k - 1], ribbed["poses"][k - 1])
        pose, res = vol.track(ribbed["depth"][k], ribbed["poses"][k - 1])
        et, er = pose_error(pose, ribbed["poses"][k])
        print(f"frame {k}: {et * 1e3:.2f} mm {er:.3f} deg, pairs {res['pairs']:.0f}, ratio {res['eig_min'] / res['eig_max']:.2e}, "
              f"steps {res['iterations']}")
        assert res["status"] == 0
        assert et <= 2 * MEASURED_T_M and er <= 2 * MEASURED_R_DEG
        assert res["eig_min"] >= REFUSAL_RATIO * res["eig_max"]
    vol.close()


def test_pinned_corridor_is_refused_with_a_nan_pose_that_integrate_refuses(ctx):
    from odometry_amd import _lib as L
    seq = corridor_sequence(5)
    vol = _volume(ctx, seq["p"])
    for k in range(1, 5):
        vol.integrate(seq["depth"][k - 1], seq["poses"][k - 1])
        before = vol.stats()
        pose, res = vol.track(seq["depth"][k], seq["poses"][k - 1], params=vol.icp_params(min_eig_ratio=REFUSAL_RATIO))
        print(f"frame {k}: status {res['status']}, ratio {res['eig_min'] / res['eig_max']:.2e}, pairs {res['pairs']:.0f}")
        assert res["status"] == 2 and np.isnan(pose).all() and np.isfinite(res["C"]).all()
        with pytest.raises(L.OdoError):
            vol.integrate(seq["depth"][k], pose)
        pose2, res2 = vol.track(seq["depth"][k], seq["poses"][k - 1], integrate=True, params=vol.icp_params(min_eig_ratio=REFUSAL_RATIO))
        assert res2["status"] == 2 and vol.stats() == before                # integrate=True fuses nothing after a refusal
    vol.close()


def test_early_stop(ctx, host, ribbed):
    """The trace ends at convergence while the remaining launches leave the state unchanged; a failure ends it at once."""
    p, k = ribbed["p"], 5
    vol = _fused(ctx, ribbed, k)
    P_m = ribbed["poses"][k - 1]
    depth, nrmw = vol.raycast(P_m)
    raw = ribbed["depth"][k]
    ic = icp(p=p, iters=(20, 20, 24), eps_t=1e-4, eps_r=1e-4)
    pose, res, trace = vol.align(raw, depth, nrmw, P_m, P_m, trace=True, params=_c_params(ic))
    levels = [t["level"] for t in trace]
    print("steps per level:", [levels.count(l) for l in range(3)], "of", ic["iters"])
    assert res["status"] == 0 and levels == sorted(levels) and set(levels) == {0, 1, 2}
    assert all(levels.count(l) < ic["iters"][l] for l in range(3))          # every level stopped before its budget
    for l in range(3):
        last = [t for t in trace if t["level"] == l][-1]["delta"]
        assert np.linalg.norm(last[:3]) < 1e-4 and np.linalg.norm(last[3:]) < 1e-4
    _check_trace(vol, host, raw, depth, nrmw, P_m, P_m, ic, res, trace)      # the result's C is the last step's: nothing ran after it
    short = vol.align(raw, depth, nrmw, P_m, P_m, trace=True, params=_c_params(icp(p=p, iters=(2, 0, 1))))
    assert [t["level"] for t in short[2]] == [0, 0, 2] and short[1]["iterations"] == 3
    for t, u in zip(short[2][:2], trace[:2]):
        assert np.array_equal(t["acc"].view(np.uint64), u["acc"].view(np.uint64)) and np.array_equal(bits(t["C"]), bits(u["C"]))
    blind = np.zeros_like(raw)                                              # no pair: the first step fails, nothing follows it
    pose, res, trace = vol.align(blind, depth, nrmw, P_m, P_m, trace=True, params=_c_params(ic))
    assert res["status"] == 1 and res["iterations"] == 1 and len(trace) == 1 and res["pairs"] == 0 and np.isnan(pose).all()
    assert not trace[0]["delta"].any() and np.array_equal(bits(trace[0]["C"]), bits(icp_frame(P_m, P_m)[1]))
    vol.close()


def test_track_equals_raycast_plus_align_and_changes_nothing(ctx, ribbed):
    p, k = ribbed["p"], 2
    vol = _fused(ctx, ribbed, k)
    vol.enable_colour(3, False, 255)
    q, w = vol.grid()
    col, stats = vol.colour_grid(), vol.stats()
    P_m = ribbed["poses"][k - 1]
    depth, nrmw = vol.raycast(P_m)
    a_pose, a_res = vol.align(ribbed["depth"][k], depth, nrmw, P_m, P_m)
    t_pose, t_res = vol.track(ribbed["depth"][k], P_m)
    assert a_res["status"] == 0 and np.array_equal(bits(a_pose), bits(t_pose))
    for key in ("status", "iterations", "pairs", "cost", "eig_min", "eig_max"):
        assert a_res[key] == t_res[key], key
    assert np.array_equal(bits(a_res["C"]), bits(t_res["C"]))
    vol.icp_eval(ribbed["depth"][k], depth, nrmw, P_m, np.eye(4), stride=2)
    _grid_equal(vol, q, w, "after eval, align and track")
    assert np.array_equal(vol.colour_grid(), col) and vol.stats() == stats
    vol.close()


def test_the_timing_call_gives_two_figures_and_changes_nothing(ctx, ribbed):
    """icp_time (tools/volume_cost.py icp): two finite figures >= 0, and the grid, the counters and the sums of an evaluation read the
    same afterwards."""
    k = 2
    vol = _fused(ctx, ribbed, k)
    q, w = vol.grid()
    stats = vol.stats()
    P_m = ribbed["poses"][k - 1]
    depth, nrmw = vol.raycast(P_m)
    acc = vol.icp_eval(ribbed["depth"][k], depth, nrmw, P_m, np.eye(4), stride=2)
    us = vol.icp_time(ribbed["depth"][k], depth, nrmw, P_m, np.eye(4), stride=2, reps=3)
    assert len(us) == 2 and all(np.isfinite(u) and u >= 0 for u in us), us
    _grid_equal(vol, q, w, "after the timing call")
    assert vol.stats() == stats
    again = vol.icp_eval(ribbed["depth"][k], depth, nrmw, P_m, np.eye(4), stride=2)
    assert acc[28] > 0 and np.array_equal(acc.view(np.uint64), again.view(np.uint64))
    vol.close()


def test_integrate_track_integrate_without_a_host_wait(ctx, ribbed):
    """An integration on the context's stream, a track on the volume's and a second integration, device frames, nothing waited for in
    between: the track sees the first integration and not the second, and the second is not lost."""
    p = ribbed["p"]
    dev = [ctx.upload(np.ascontiguousarray(ribbed["depth"][k])) for k in range(3)]
    ref = _fused(ctx, ribbed, 1)
    want_pose, want_res = ref.track(ribbed["depth"][1], ribbed["poses"][0])
    ref.close()
    vol = _volume(ctx, p)
    vol.integrate(dev[0], ribbed["poses"][0])
    pose, res = vol.track(dev[1], ribbed["poses"][0])
    vol.integrate(dev[1], pose)
    assert res["status"] == 0 and np.array_equal(bits(pose), bits(want_pose)) and res["pairs"] == want_res["pairs"]
    q, w = empty_grid(p)
    q, w, _, _ = integrate_model(q, w, ribbed["depth"][0], ribbed["poses"][0], p)
    q, w, _, _ = integrate_model(q, w, ribbed["depth"][1], pose, p)
    _grid_equal(vol, q, w, "integrate, track, integrate")
    assert vol.stats()["frames"] == 2
    pose2, res2 = vol.track(dev[2], pose, integrate=True)                   # the same through integrate=True
    assert res2["status"] == 0 and vol.stats()["frames"] == 3
    q, w, _, _ = integrate_model(q, w, ribbed["depth"][2], pose2, p)
    _grid_equal(vol, q, w, "track with integrate=True")
    vol.close()
    for h in dev:
        ctx.free(h)


def test_refusals_enqueue_nothing(ctx, ribbed):
    from odometry_amd import _lib as L
    vol = _fused(ctx, ribbed, 1)
    q, w = vol.grid()
    stats = vol.stats()
    P_m = ribbed["poses"][0]
    depth, nrmw = vol.raycast(P_m)
    raw = ribbed["depth"][1]
    for kw, cp in bad_params():
        with pytest.raises(L.OdoError):
            vol.align(raw, depth, nrmw, P_m, P_m, params=cp)
        with pytest.raises(L.OdoError):
            vol.track(raw, P_m, params=cp)
    bad = np.eye(4, dtype=f32)
    bad[1, 3] = np.nan
    for args in ((bad, P_m), (P_m, bad)):
        with pytest.raises(L.OdoError):
            vol.align(raw, depth, nrmw, *args)
    with pytest.raises(L.OdoError):
        vol.track(raw, bad)
    with pytest.raises(L.OdoError):
        vol.icp_eval(raw, depth, nrmw, P_m, bad)
    with pytest.raises(L.OdoError):
        vol.icp_eval(raw, depth, nrmw, P_m, np.eye(4), stride=17)
    with pytest.raises(ValueError):
        vol.align(raw[:-1], depth, nrmw, P_m, P_m)
    _grid_equal(vol, q, w, "after the refusals")
    assert vol.stats() == stats
    pose, res = vol.track(raw, P_m)                                         # and the volume still works
    assert res["status"] == 0
    vol.close()
