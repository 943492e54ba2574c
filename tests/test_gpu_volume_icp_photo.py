"""The photometric term of frame-to-model tracking on the GPU (odo_volume_icp_photo_eval_dev, odo_volume_icp_photo_align_dev,
odo_volume_track_photo_dev, api.TsdfVolume.icp_eval / align / track with grey=) against the numpy model of
tests/volume_icp_photo_cases.py and the host build of tests/test_volume_icp_cpu.py: the sixteen floats of every pixel bit for bit
across frame sizes round the launch tile, the pinned cases and every branch row, the 31 sums within the bound of any summation order
and bit-identical from call to call, every step of an alignment against the host build's step, the ground truth of the CPU test, the
early stop, track against coloured ray-cast + align, the volume's state and the refusals."""
import numpy as np
import pytest

import volume_icp_photo_cases as pc
from conftest import se3_log_norm
from test_gpu_volume import _grid_equal, _volume
from test_gpu_volume_icp import BLOCK, TILE, _c_params
from test_volume_cpu import bits
from test_volume_icp_cpu import bad_params, build_host_library, host_step, icp, icp_frame, pose_error, rows_equal
from test_volume_icp_photo_cpu import (MEASURED_CORRIDOR_R_DEG, MEASURED_CORRIDOR_T_M, MEASURED_RIBBED_R_DEG, MEASURED_RIBBED_T_M)

pytestmark = pytest.mark.gpu
f32 = np.float32

assert TILE * TILE == BLOCK
SIZES = [(1, 1), (2, 2), (64 // TILE, TILE), (TILE, TILE), (TILE + 1, TILE), (TILE, TILE + 1), (17, 23), (64, 1), (1, 64), (65, 33)]
SIZES_S1 = [(120, 160)]                                            # 80 blocks: the step kernel's unrolled fold runs a whole body
CASES = [(size, s) for size in SIZES for s in (1, 2, 4)] + [(size, 1) for size in SIZES_S1]
CASES += [((TILE * s + dr, TILE * s + dc), s) for s in (2, 4) for dr, dc in ((0, 0), (1, 0), (0, 1))]   # the same seams on the stride's lattice
WORST = [0.0]                                                      # the largest |acc - sum| / bound met by this module


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()
    print(f"largest |acc - fp64 sum| as a fraction of the bound over the module: {WORST[0]:.3f}")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_library(tmp_path_factory.mktemp("icp_host"))


@pytest.fixture(scope="module")
def sequences():
    return dict(corridor=pc.corridor_photo_sequence(), ribbed=pc.ribbed_photo_sequence())


def _photo(weight, huber):
    from odometry_amd import _lib as L
    return L.IcpPhotoParams(weight, huber)


def _check_eval(vol, p, raw, grey, depth, nrmw, rgba, P_m, Cm, stride, dist_max, huber, weight, ph, tag):
    """rows_dev (into a buffer pre-filled with 0xAB) against the model bit for bit; acc within n_rows 2^-52 sum |terms| of the fp64 sum
    of the model's exact products, the counts exact; two calls bit-identical. Returns the numbers of geometric and photometric pairs."""
    M = icp_frame(P_m, P_m)[0]
    want, mg, mp = pc.icp_photo_rows_model(raw, grey, depth, nrmw, rgba, M, Cm, p, stride, dist_max, huber, weight, ph)
    kw = dict(stride=stride, dist_max=dist_max, huber_delta=huber, grey=grey, model_rgba=rgba, photo=_photo(weight, ph))
    acc, got = vol.icp_eval(raw, depth, nrmw, P_m, Cm, rows=True, **kw)
    assert acc.shape == (pc.NACC,) and got.shape == p["size"] + (16,)
    rows_equal(got, want, tag)
    s, mag, n = pc.icp_photo_acc(want, mg, mp)
    assert acc[28] == mg.sum() and acc[29] == mp.sum(), (tag, acc[28:30], mg.sum(), mp.sum())
    bound = n * 2.0 ** -52 * mag
    frac = float(np.max(np.abs(acc - s)[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    WORST[0] = max(WORST[0], frac)
    print(f"{tag}: {int(mg.sum())} + {int(mp.sum())} pairs, largest |acc - sum| / bound {frac:.3f}")
    assert (np.abs(acc - s) <= bound).all(), (tag, acc - s, bound)
    order = pc.icp_photo_acc_kernel_order(want, mg, mp, stride)
    assert np.array_equal(acc.view(np.uint64), order.view(np.uint64)), (tag, acc - order)
    again = vol.icp_eval(raw, depth, nrmw, P_m, Cm, **kw)
    assert np.array_equal(acc.view(np.uint64), again.view(np.uint64)), tag
    return int(mg.sum()), int(mp.sum())


@pytest.mark.parametrize("size,stride", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"s{v}")
def test_rows_and_sums_across_frame_sizes(ctx, size, stride):
    rows, cols = size
    K = (1.3 * max(rows, cols, 8), (cols - 1) / 2, (rows - 1) / 2)
    motion = ((0, 0, 0), (0.004, 0.0, 0.01)) if rows == 1 else ((0, 0, 0), (0.0, 0.004, 0.01)) if cols == 1 else None
    geo = photo = 0
    for seed in range(2):
        p, raw, grey, depth, nrmw, rgba, P_m, P_init = pc.random_photo_frames(seed, size, K, *([motion] if motion else []))
        vol = _volume(ctx, p)
        g, n = _check_eval(vol, p, raw, grey, depth, nrmw, rgba, P_m, icp_frame(P_m, P_init)[1], stride, 0.3, 0.02 * seed, 0.01, 6.0 * seed,
                           f"{size} stride {stride}")
        geo, photo = geo + g, photo + n
        vol.close()
    assert geo > 0 or rows * cols == 1
    assert photo > 0 or min(rows, cols) < TILE, (size, stride)
    assert photo == 0 or min(rows, cols) > 1                        # a frame one pixel high or wide has no four taps


def _coloured(ctx, seq, n):
    """A volume with colour and frames 0 .. n - 1 of the sequence fused, grey replicated into R, G and B, at their true poses."""
    vol = _volume(ctx, seq["p"])
    vol.enable_colour()
    for k in range(n):
        vol.integrate(seq["depth"][k], seq["poses"][k], colour=pc._grey_colour(seq["gray"][k]))
    return vol


@pytest.mark.parametrize("name", ["corridor", "ribbed"])
def test_rows_and_sums_on_the_pinned_cases(ctx, sequences, name):
    seq, k = sequences[name], 2
    vol = _coloured(ctx, seq, k)
    P_m = seq["poses"][k - 1]
    depth, nrmw, rgba = vol.raycast(P_m, colour=True)
    assert (rgba[..., 3] != 0).any()
    for stride in (1, 2, 4):
        g, n = _check_eval(vol, seq["p"], seq["depth"][k], seq["gray"][k], depth, nrmw, rgba, P_m, np.eye(4, dtype=f32), stride,
                           2 * float(f32(seq["p"]["mu"])), 0.0, 0.01, 4.0, f"{name} stride {stride}")
        assert g > 100 and n > 100
    vol.close()


@pytest.mark.parametrize("row", pc.photo_branch_rows(), ids=lambda r: r[0])
def test_every_branch_row(ctx, row):
    name, p, raw, grey, depth, nrmw, rgba, M, Cm, stride, dist_max, huber, weight, ph, _ = row
    assert np.array_equal(M, np.eye(4))
    vol = _volume(ctx, p)
    _check_eval(vol, p, raw, grey, depth, nrmw, rgba, np.eye(4), Cm, stride, dist_max, huber, weight, ph, name)
    vol.close()


# ---- the alignment ---------------------------------------------------------------------------------------------------------------
def _check_trace(vol, host, frames, P_m, P_init, ic, ph, res, trace):
    """Every step: acc is icp_eval at the C before it, delta and C are the host build's icp_step on its first 29, all bit for bit."""
    raw, grey, depth, nrmw, rgba = frames
    step = host_step(host)
    Cm = icp_frame(P_m, P_init)[1]
    for t in trace:
        acc = vol.icp_eval(raw, depth, nrmw, P_m, Cm, stride=ic["strides"][t["level"]], dist_max=ic["dist_max"], huber_delta=ic["huber_delta"],
                           grey=grey, model_rgba=rgba, photo=_photo(ph["weight"], ph["huber_delta"]))
        assert t["acc"].shape == (pc.NACC,) and np.array_equal(acc.view(np.uint64), t["acc"].view(np.uint64)), t["iteration"]
        failed, _, delta, Cm = step(acc[:29], Cm, ic["min_pairs"], ic["eps_t"], ic["eps_r"])
        assert np.array_equal(bits(delta), bits(t["delta"])) and np.array_equal(bits(Cm), bits(t["C"])), t["iteration"]
        assert bool(failed) == (res["status"] == 1 and t is trace[-1])
    assert np.array_equal(bits(res["C"]), bits(Cm)) and res["iterations"] == len(trace)


def test_align_step_by_step_and_against_the_model(ctx, host, sequences):
    """Frame 3 of the pinned corridor against the coloured volume of frames 0 .. 2, at the defaults and without the Huber weight."""
    seq, k = sequences["corridor"], 3
    p = seq["p"]
    vol = _coloured(ctx, seq, k)
    P_m = seq["poses"][k - 1]
    depth, nrmw, rgba = vol.raycast(P_m, colour=True)
    frames = (seq["depth"][k], seq["gray"][k], depth, nrmw, rgba)
    ic = icp(p=p)
    for ph in (pc.photo(), pc.photo(0.003, 0.0)):
        pose, res, trace = vol.align(frames[0], depth, nrmw, P_m, P_m, trace=True, params=_c_params(ic), grey=frames[1], model_rgba=rgba,
                                     photo=_photo(ph["weight"], ph["huber_delta"]))
        assert res["status"] == 0 and 10 <= len(trace) <= sum(ic["iters"])
        _check_trace(vol, host, frames, P_m, P_m, ic, ph, res, trace)
        want = pc.icp_photo_align_model(frames[0], frames[1], depth, nrmw, rgba, P_m, P_m, p, ic, ph, step=host_step(host))
        d = se3_log_norm(want["abs_pose"], pose)
        print(f"{ph}: {len(trace)} steps, ||log|| against the model's loop {d:.2e}, pairs {res['pairs']:.0f} + {res['photo_pairs']:.0f}")
        assert want["status"] == 0 and d < 1e-5
        assert res["pairs"] == want["pairs"] and res["photo_pairs"] == want["photo_pairs"]
        assert abs(res["photo_cost"] - want["photo_cost"]) <= 1e-9 * want["cost"] and abs(res["cost"] - want["cost"]) <= 1e-9 * want["cost"]
        assert abs(res["eig_min"] - want["eig_min"]) <= 1e-9 * want["eig_max"] and abs(res["eig_max"] - want["eig_max"]) <= 1e-9 * want["eig_max"]
        assert pose.dtype == f32 and pose.shape == (4, 4)
    vol.close()


@pytest.mark.parametrize("name", ["corridor", "ribbed"])
def test_pinned_cases_stay_inside_the_cpu_tests_bounds(ctx, sequences, name):
    """The CPU test's procedure on the GPU: frames 0 .. k - 1 fused with their colour at their true poses, frame k tracked from pose
    k - 1 with its grey frame, k = 1 .. 6; on the corridor every frame ends at most half as far from the truth as the geometric track."""
    seq = sequences[name]
    bound_t, bound_r = dict(corridor=(MEASURED_CORRIDOR_T_M, MEASURED_CORRIDOR_R_DEG), ribbed=(MEASURED_RIBBED_T_M, MEASURED_RIBBED_R_DEG))[name]
    vol = _volume(ctx, seq["p"])
    vol.enable_colour()
    for k in range(1, 7):
        vol.integrate(seq["depth"][k - 1], seq["poses"][k - 1], colour=pc._grey_colour(seq["gray"][k - 1]))
        pose, res = vol.track(seq["depth"][k], seq["poses"][k - 1], grey=seq["gray"][k])
        g_pose, g_res = vol.track(seq["depth"][k], seq["poses"][k - 1])
        et, er = pose_error(pose, seq["poses"][k])
        gt, gr = pose_error(g_pose, seq["poses"][k])
        print(f"{name} frame {k}: {et * 1e3:.2f} mm {er:.3f} deg (geometric only {gt * 1e3:.2f} mm {gr:.3f} deg), pairs {res['pairs']:.0f} + "
              f"{res['photo_pairs']:.0f}, steps {res['iterations']}")
        assert res["status"] == 0 and g_res["status"] == 0
        assert et <= 2 * bound_t and er <= 2 * bound_r
        if name == "corridor":
            assert et <= 0.5 * gt, (k, et, gt)
    vol.close()


def test_early_stop(ctx, host, sequences):
    """The trace ends at convergence while the remaining launches leave the state unchanged; a failure ends it at once."""
    seq, k = sequences["ribbed"], 5
    p = seq["p"]
    vol = _coloured(ctx, seq, k)
    P_m = seq["poses"][k - 1]
    depth, nrmw, rgba = vol.raycast(P_m, colour=True)
    frames = (seq["depth"][k], seq["gray"][k], depth, nrmw, rgba)
    ph = pc.photo()
    ic = icp(p=p, iters=(20, 20, 24), eps_t=1e-3, eps_r=1e-3)
    kw = dict(grey=frames[1], model_rgba=rgba, photo=_photo(ph["weight"], ph["huber_delta"]))
    pose, res, trace = vol.align(frames[0], depth, nrmw, P_m, P_m, trace=True, params=_c_params(ic), **kw)
    levels = [t["level"] for t in trace]
    print("steps per level:", [levels.count(l) for l in range(3)], "of", ic["iters"])
    assert res["status"] == 0 and levels == sorted(levels) and set(levels) == {0, 1, 2}
    assert all(levels.count(l) < ic["iters"][l] for l in range(3))         # every level stopped before its budget (the model: 12, 6, 5)
    _check_trace(vol, host, frames, P_m, P_m, ic, ph, res, trace)          # the result's C is the last step's: nothing ran after it
    blind = np.zeros_like(frames[0])                                       # no pair: the first step fails, nothing follows it
    pose, res, trace = vol.align(blind, depth, nrmw, P_m, P_m, trace=True, params=_c_params(ic), **kw)
    assert res["status"] == 1 and res["iterations"] == 1 and len(trace) == 1 and res["pairs"] == 0 and res["photo_pairs"] == 0
    assert np.isnan(pose).all() and not trace[0]["delta"].any() and np.array_equal(bits(trace[0]["C"]), bits(icp_frame(P_m, P_m)[1]))
    bare = nrmw.copy()                                                     # texture without a model surface is not an alignment
    bare[..., :3] = 0
    pose, res = vol.align(frames[0], depth, bare, P_m, P_m, params=_c_params(ic), **kw)
    assert res["status"] == 1 and res["pairs"] == 0 and res["photo_pairs"] > 100 and np.isnan(pose).all()
    vol.close()


def test_track_equals_coloured_raycast_plus_align_and_changes_nothing(ctx, sequences):
    seq, k = sequences["ribbed"], 2
    vol = _coloured(ctx, seq, k)
    q, w = vol.grid()
    col, stats = vol.colour_grid(), vol.stats()
    P_m = seq["poses"][k - 1]
    raw, grey = seq["depth"][k], seq["gray"][k]
    depth, nrmw, rgba = vol.raycast(P_m, colour=True)
    a_pose, a_res = vol.align(raw, depth, nrmw, P_m, P_m, grey=grey, model_rgba=rgba)
    t_pose, t_res = vol.track(raw, P_m, grey=grey)
    assert a_res["status"] == 0 and np.array_equal(bits(a_pose), bits(t_pose))
    for key in ("status", "iterations", "pairs", "cost", "eig_min", "eig_max", "photo_pairs", "photo_cost"):
        assert a_res[key] == t_res[key], key
    assert np.array_equal(bits(a_res["C"]), bits(t_res["C"])) and t_res["photo_pairs"] > 0
    g_pose, g_res = vol.align(raw, depth, nrmw, P_m, P_m)                   # without grey: the geometric path, as before
    p_pose, p_res = vol.track(raw, P_m)
    assert "photo_pairs" not in p_res and np.array_equal(bits(g_pose), bits(p_pose)) and g_res["cost"] == p_res["cost"]
    assert not np.array_equal(bits(g_pose), bits(t_pose))
    vol.icp_eval(raw, depth, nrmw, P_m, np.eye(4), stride=2, grey=grey, model_rgba=rgba)
    _grid_equal(vol, q, w, "after eval, align and track")
    assert np.array_equal(vol.colour_grid(), col) and vol.stats() == stats
    pose, res = vol.track(raw, P_m, integrate=True, grey=grey, colour=pc._grey_colour(grey))   # fuses the coloured frame at the pose
    assert res["status"] == 0 and np.array_equal(bits(pose), bits(t_pose)) and vol.stats()["frames"] == stats["frames"] + 1
    assert not np.array_equal(vol.colour_grid(), col)
    vol.close()


def test_refusals_enqueue_nothing(ctx, sequences):
    from odometry_amd import _lib as L
    seq = sequences["ribbed"]
    P_m, raw, grey = seq["poses"][0], seq["depth"][1], seq["gray"][1]
    plain = _volume(ctx, seq["p"])                                          # no colour grid: track(grey=) is refused, align is not
    plain.integrate(seq["depth"][0], P_m)
    with pytest.raises(L.OdoError, match="colour"):
        plain.track(raw, P_m, grey=grey)
    with pytest.raises(L.OdoError, match="colour"):
        plain.track(raw, P_m, grey=grey, integrate=True, colour=pc._grey_colour(grey))
    plain.close()
    vol = _coloured(ctx, seq, 1)
    q, w = vol.grid()
    col, stats = vol.colour_grid(), vol.stats()
    depth, nrmw, rgba = vol.raycast(P_m, colour=True)
    kw = dict(grey=grey, model_rgba=rgba)
    for _, cp in bad_params():
        with pytest.raises(L.OdoError):
            vol.align(raw, depth, nrmw, P_m, P_m, params=cp, **kw)
        with pytest.raises(L.OdoError):
            vol.track(raw, P_m, params=cp, grey=grey)
    for weight, huber in ((0.0, 0.0), (-0.01, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.01, -1.0), (0.01, float("nan"))):
        with pytest.raises(L.OdoError):
            vol.align(raw, depth, nrmw, P_m, P_m, photo=_photo(weight, huber), **kw)
        with pytest.raises(L.OdoError):
            vol.track(raw, P_m, grey=grey, photo=_photo(weight, huber))
        with pytest.raises(L.OdoError):
            vol.icp_eval(raw, depth, nrmw, P_m, np.eye(4), photo=_photo(weight, huber), **kw)
    bad = np.eye(4, dtype=f32)
    bad[1, 3] = np.nan
    for args in ((bad, P_m), (P_m, bad)):
        with pytest.raises(L.OdoError):
            vol.align(raw, depth, nrmw, *args, **kw)
    with pytest.raises(L.OdoError):
        vol.track(raw, bad, grey=grey)
    with pytest.raises(L.OdoError):
        vol.icp_eval(raw, depth, nrmw, P_m, bad, **kw)
    with pytest.raises(L.OdoError):
        vol.icp_eval(raw, depth, nrmw, P_m, np.eye(4), stride=17, **kw)
    with pytest.raises(ValueError):
        vol.align(raw, depth, nrmw, P_m, P_m, grey=grey[:-1], model_rgba=rgba)
    with pytest.raises(ValueError):
        vol.align(raw, depth, nrmw, P_m, P_m, grey=grey)                  # grey without the model's colours
    with pytest.raises(ValueError):
        vol.track(raw, P_m, colour=pc._grey_colour(grey))                 # colour without grey
    _grid_equal(vol, q, w, "after the refusals")
    assert np.array_equal(vol.colour_grid(), col) and vol.stats() == stats
    pose, res = vol.track(raw, P_m, grey=grey)                             # and the volume still works
    assert res["status"] == 0
    vol.close()
