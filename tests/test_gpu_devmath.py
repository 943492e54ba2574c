"""The device builds of the arithmetic that decides the pose, held to the oracle call by call.

tests/test_hostemu_parity.py and tests/test_devmath_cpu.py prove odo_math.h bit-exact against the oracle as g++ compiles it for the
host. The product only runs it as hipcc compiles it for gfx950, and its hot kernels run hand-written wave-wide and block-wide variants
(sincos_pair_lanes, se3_exp_wave, lm_apply_step_wave, solve_damped_wave_regs, lm_state_machine, lm_state_machine_hot,
point_residual_g, the shared-reciprocal divisions of dense.hip.h). Here every one of them runs on the device through
tests/devmath_harness.hip — built with the product's flags under both machine schedulers the library uses — on the input classes of
tests/devmath_cases.py, and must equal the host build (hence the oracle) BY BIT PATTERN. NaNs compare as NaNs; there is no tolerance
anywhere in this file except where a sum over a level is compared with the oracle's sum in another order (the library-level test)."""
import functools
import os

import numpy as np
import pytest

import devmath as D
import devmath_cases as Cs

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def host():
    return D.load_host()


@pytest.fixture(scope="module", params=D.UNITS)
def dev(request):
    """One build of the harness: under the main unit's scheduler, then under the LM chain unit's."""
    return D.load_device(request.param)


def bits_equal(a, b, what=""):
    eq = D.same_bits(a, b)
    assert eq.all(), "%s: %d of %d differ, first at %s" % (what, int((~eq).sum()), eq.size, tuple(np.argwhere(~eq)[0]))


# ---- one case per thread and one case per wavefront -------------------------------------------------------------------------------
def test_level_intrinsics(dev, host):
    args = Cs.level_cases()
    for a, b in zip(dev.level_k(*args), host.level_k(*args)):
        bits_equal(a, b, "make_level_k / cx_level")


def test_sincos(dev, host):
    """sincos_f per thread, and sincos_pair_lanes per wavefront with the class as its first and (shuffled) as its second argument: all
    four quadrants of its swap / XOR table for both signs, either side of every multiple of pi / 4, large arguments up to 2^62, zeros,
    denormals, infinities and NaN."""
    rng = np.random.default_rng(11)
    for name, x in Cs.sincos_classes().items():
        s, c = host.sincos(x)
        sd, cd = dev.sincos(x)
        bits_equal(sd, s, "sincos_f sin, class " + name)
        bits_equal(cd, c, "sincos_f cos, class " + name)
        if name == "grid":
            x = x[::8]
            s, c = s[::8], c[::8]
        perm = rng.permutation(len(x))
        out, off = dev.sincos_pair_wave(x, x[perm])
        assert not off.any(), "sincos_pair_lanes: lanes disagree, class " + name
        for col, ref in enumerate((s, c, s[perm], c[perm])):
            bits_equal(out[:, col], ref, "sincos_pair_lanes output %d, class %s" % (col, name))


def test_se3_exp(dev, host):
    for name, a in Cs.se3_exp_classes().items():
        q, M = host.se3_exp(a)
        qd, Md = dev.se3_exp(a)
        bits_equal(qd, q, "se3_exp quaternion / translation, class " + name)
        bits_equal(Md, M, "se3_exp matrix, class " + name)
        qw, Mw, off = dev.se3_exp_wave(a)
        assert not off.any(), "se3_exp_wave: lanes disagree, class " + name
        bits_equal(qw, qd, "se3_exp_wave against se3_exp on the device, class " + name)
        bits_equal(qw, q, "se3_exp_wave, class " + name)
        bits_equal(Mw, M, "se3_exp_wave matrix, class " + name)


def test_se3_matrix_round_trip_and_left_update(dev, host):
    for name, Min in Cs.pose_matrices().items():
        q, M = host.se3_roundtrip(Min)
        qd, Md = dev.se3_roundtrip(Min)
        bits_equal(qd, q, "se3_from_colmajor, class " + name)
        bits_equal(Md, M, "se3_to_colmajor, class " + name)
    d6, cur = Cs.compose_cases()
    q, M = host.se3_left_update(d6, cur, 0)
    for variant, what in ((0, "se3_left_update"), (1, "se3_left_update_mat")):
        qd, Md = dev.se3_left_update(d6, cur, variant)
        bits_equal(qd, q, what)
        bits_equal(Md, M, what + " matrix")


def test_solve_damped(dev, host):
    acc, lam, kind = Cs.solver_cases()
    d = host.solve_damped(acc, lam)
    dd = dev.solve_damped(acc, lam)
    bits_equal(dd, d, "solve_damped")
    dw, off = dev.solve_damped_wave(acc, lam)
    assert not off.any(), "solve_damped_wave_regs: lanes disagree"
    bits_equal(dw, dd, "solve_damped_wave_regs against solve_damped on the device")
    bits_equal(dw, d, "solve_damped_wave_regs")


def test_robust_weight_and_depth_lm_driver(dev, host):
    args = Cs.robust_cases()
    bits_equal(dev.robust_weight(*args), host.robust_weight(*args), "robust_weight")
    args = Cs.depth_schedule_cases()
    for a, b in zip(dev.depth_schedule(*args), host.depth_schedule(*args)):
        assert np.array_equal(a, b), "depth_lm_begin / decide / advance"


def test_apply_step(dev, host):
    st = Cs.apply_step_states(D.LM_STATE)
    ref = host.apply_step(st)
    out = dev.apply_step(st)
    eq = D.same_states(out, ref)
    assert eq.all(), "lm_apply_step: state %d dword %d" % tuple(np.argwhere(~eq)[0])
    outw, off = dev.apply_step_wave(st)
    assert not off.any(), "lm_apply_step_wave: lanes disagree"
    eq = D.same_states(outw, out) & D.same_states(outw, ref)
    assert eq.all(), "lm_apply_step_wave: state %d dword %d" % tuple(np.argwhere(~eq)[0])


# ---- the LM state machines over scripts -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scripts():
    return Cs.lm_scripts(D.LM_SCRIPT)


@pytest.mark.parametrize("form,block", [(0, 0), (1, 64), (1, -1), (2, 64), (2, -1)])
def test_lm_scripts(dev, host, form, block):
    """The 64-dword state after EVERY evaluation of every script equals emu_lm_script's: lm_consume one script per thread (form 0),
    lm_state_machine (1) and lm_state_machine_hot (2) one script per block of 64 threads and of the coarse kernel's own block size
    (-1). No field is masked: the hot form does not carry `last`, but lm_hot_store writes cur into it and cur == last holds after
    every path of the rule, so even that dword must agree."""
    sc, acc, kinds = _scripts()
    ref, count = host.lm_script(sc, acc)
    out, cnt = dev.lm_script(sc, acc, form, dev.coarse_block if block < 0 else block)
    assert np.array_equal(cnt, count), "evaluations consumed differ, first script %d" % int(np.argmax(cnt != count))
    eq = D.same_states(out, ref)
    if not eq.all():
        e, w = np.argwhere(~eq)[0]
        i = int(np.searchsorted(sc["acc_first"], e, side="right") - 1)
        raise AssertionError("script %d (%s): evaluation %d, dword %d differs (%d dwords in all)" %
                             (i, kinds[i], e - sc["acc_first"][i], w, int((~eq).sum())))
    assert count.sum() >= 2000


# ---- the per-pixel chain ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def levels(kitti_seq, small_seq):
    return Cs.pixel_levels(kitti_seq, small_seq)


def _k(host, lv, bilinear=0):
    fl, cxy = host.level_k([lv["K"]["f0"]], [lv["K"]["cx0"]], [lv["K"]["cy0"]], [lv["level"]])
    return float(fl[0]), float(cxy[0, 0]), float(cxy[0, 1]), bilinear


@pytest.mark.parametrize("bilinear", [0, 1])
def test_pixel_chain(dev, host, O, levels, bilinear):
    """make_point + point_residual<true> (floor and bilinear sampling), point_residual<false>, point_residual_g<false> and
    point_residual_only per pixel: the hit mask equals the host build's, the hit count equals the oracle's N, and r, w, J of the hits in
    scan order equal the oracle's dump by bit pattern. point_residual_g's J[0] and J[1] are compared with == : it drops the products by
    the Jacobian's structural zeros, whose only effect is the documented -0 -> +0."""
    O.set_sampling(bool(bilinear))
    try:
        for lv in levels:
            k = _k(host, lv, bilinear)
            rows, cols = lv["I1"].shape
            for name, T in Cs.level_poses(lv["K"], lv["level"], rows, cols, lv["motion"]).items():
                what = "%s, pose %s" % (lv["name"], name)
                hit_h = host.pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 0)[0]
                hit, r, w, J = dev.pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 0)
                assert np.array_equal(hit, hit_h), "hit mask, " + what
                n = int(hit.sum())
                ref = O.lm_accumulate(lv["I1"], lv["I2"], lv["D1"], lv["level"], T, robust=1, K=lv["K"], dump=max(n, 1))
                assert int(ref["acc"][28]) == n, "hit count against the oracle's N, " + what
                m = hit.astype(bool)
                bits_equal(r[m], ref["r"][:n], "r, " + what)
                bits_equal(w[m], ref["w"][:n], "w, " + what)
                bits_equal(J[m], ref["J"][:n], "J, " + what)
                if bilinear:
                    continue
                h1, r1, w1, J1 = dev.pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 1)
                assert np.array_equal(h1, hit)
                bits_equal(r1, r, "point_residual<false> r, " + what)
                bits_equal(J1, J, "point_residual<false> J, " + what)
                h3, r3, w3, _ = dev.pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 3)
                assert np.array_equal(h3, hit)
                bits_equal(r3, r, "point_residual_only r, " + what)
                bits_equal(w3, w, "point_residual_only w, " + what)
                h2, r2, w2, J2 = dev.pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 2)
                assert np.array_equal(h2, hit), "point_residual_g hit mask, " + what
                bits_equal(r2, r, "point_residual_g r, " + what)
                bits_equal(w2, w, "point_residual_g w, " + what)
                bits_equal(J2[..., 2:], J[..., 2:], "point_residual_g J[2..5], " + what)
                assert ((J2[..., :2] == J[..., :2]) | (np.isnan(J2[..., :2]) & np.isnan(J[..., :2]))).all(), "point_residual_g J[0..1], " + what
    finally:
        O.set_sampling(False)


def _row_products(r, w, J):
    """The 29 products odo::accumulate_row adds for one row, formed exactly: fl32(J w) and fl32(r w) in float32, every product of two
    float32 values exact in float64; + 0.0 because the device adds them to an accumulator that starts at +0."""
    jw = (J * w[:, None]).astype(f32).astype(np.float64)
    Jd, rd = J.astype(np.float64), r.astype(np.float64)
    out = np.zeros((len(r), 29))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            out[:, k] = jw[:, a] * Jd[:, b]
            k += 1
    out[:, 21:27] = jw * rd[:, None]
    out[:, 27] = (r * w).astype(f32).astype(np.float64) * rd
    out[:, 28] = 1.0
    return out + 0.0


@pytest.mark.parametrize("bilinear", [0, 1])
def test_dense_stages(dev, host, O, levels, bilinear):
    """dense_stage_a + dense_stage_b per pixel with the plain divisions (fast = 0) and with the shared-reciprocal forms (fast = 1):
    hit mask = the host build's, hit count = the oracle's N, each pixel's 29 products = those formed exactly in fp64 from the oracle's
    dump, and fast = 1 equal to fast = 0 on every guarded pixel (dense_fast_ok intrinsics, |T[i]| <= 2^20, |d| <= 4096)."""
    O.set_sampling(bool(bilinear))
    guarded_levels = 0
    try:
        for lv in levels:
            if bilinear and lv["name"] == "kitti_l0":
                continue
            k = _k(host, lv, bilinear)
            rows, cols = lv["I1"].shape
            fast_ok = dev.dense_fast_ok(k[0], k[1], k[2], rows, cols)
            guarded_levels += fast_ok
            poses = Cs.level_poses(lv["K"], lv["level"], rows, cols, lv["motion"])
            for name, T in poses.items():
                if lv["name"] == "kitti_l0" and name not in ("motion", "behind_and_off"):
                    continue                                # (466 k pixels x 29 doubles per call: two poses of the largest level)
                what = "%s, pose %s" % (lv["name"], name)
                hit_h = host.pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 0)[0]
                n = int(hit_h.sum())
                ref = O.lm_accumulate(lv["I1"], lv["I2"], lv["D1"], lv["level"], T, robust=1, K=lv["K"], dump=max(n, 1))
                expect = _row_products(ref["r"][:n], ref["w"][:n], ref["J"][:n])
                hit0, acc0 = dev.dense_pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 0)
                assert np.array_equal(hit0, hit_h), "dense stages (plain divisions) hit mask, " + what
                assert int(ref["acc"][28]) == n
                bits_equal(acc0[hit0.astype(bool)], expect, "dense stages (plain divisions) products, " + what)
                assert not acc0[~hit0.astype(bool)].any()
                if not (fast_ok and np.isfinite(T).all() and (np.abs(T) <= 2.0 ** 20).all()):
                    continue
                hit1, acc1 = dev.dense_pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 1)
                g = ~(np.abs(lv["D1"]) > 4096.0)             # the per-lane part of the guard
                assert np.array_equal(hit1[g], hit0[g]), "dense stages (shared reciprocals) hit mask, " + what
                bits_equal(acc1[g], acc0[g], "dense stages: shared reciprocals against plain divisions, " + what)
    finally:
        O.set_sampling(False)
    assert guarded_levels >= 8


# ---- the shared-reciprocal divisions, operand by operand --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _div32(name):
    return Cs.div32_operands(name)


@pytest.mark.parametrize("name", sorted(Cs.DIV32_FORMS))
def test_div_shared_fp32(dev, name):
    """rcp_refined + div_shared / div_shared_z / recip_shared against the device's own `/` on 2^24 operand pairs drawn from the interval the call site
    can produce inside dense_fast_ok's guard (interval ends included): no mismatch; and both against numpy's IEEE float32 division on
    the first 2^20."""
    form, a, b = _div32(name)
    assert len(b) >= 1 << 24
    n_out = 1 << 20
    n_bad, first, qs, qp = dev.div32(a, b, form, n_out)
    assert n_bad == 0, "%s: %d mismatches, first operands %s" % (name, n_bad, [(float(a[i]), float(b[i])) for i in first[:4]])
    with np.errstate(all="ignore"):
        ref = (a[:n_out] if form != 1 else f32(1.0)) / b[:n_out]
    bits_equal(qp, ref.astype(f32), name + ": the device's / against numpy")
    bits_equal(qs, ref.astype(f32), name + ": the shared form against numpy")


def test_div_shared_fp64(dev):
    a, b = _div64()
    n_out = 1 << 20
    n_bad, first, qs, qp = dev.div64(a, b, n_out)
    assert len(b) >= 1 << 24
    assert n_bad == 0, "%d mismatches, first operands %s" % (n_bad, [(float(a[i]), float(b[i])) for i in first[:4]])
    bits_equal(qp, a[:n_out] / b[:n_out], "the device's fp64 / against numpy")
    bits_equal(qs, a[:n_out] / b[:n_out], "rcp_refined_d + div_shared_d against numpy")


@functools.lru_cache(maxsize=None)
def _div64():
    return Cs.div64_operands()


def test_call_sites_inside_the_guard(dev):
    """point_xyz_shared / point_jacobian_shared / warp_uv_shared against point_xyz / point_jacobian / warp_point_uv with the guard's
    corners as inputs: fl in {1, 65536}, a principal point at an integer and 2^-8 from one, x == cx, x = 65530, |d| = 0.01 and 4096,
    a pose entry of 2^20."""
    from test_devmath_cpu import Cs_dense_fast_ok
    x, y, d, fl, cx, cy, T = Cs.callsite_cases()
    for i in range(0, len(x), 4099):
        assert dev.dense_fast_ok(fl[i], cx[i], cy[i], 1080, 1920) == 1 == Cs_dense_fast_ok(fl[i], cx[i], cy[i])
    n_bad, first = dev.callsites(x, y, d, fl, cx, cy, T)
    report = ["%s: %d mismatches, first cases %s" % (site, nb, [(int(x[i]), int(y[i]), float(d[i]), float(fl[i]), float(cx[i])) for i in fi[:4]])
              for site, nb, fi in zip(("point_xyz", "point_jacobian", "warp"), n_bad, first) if nb]
    assert not report, "; ".join(report)
    assert ((x.astype(f32) == cx) & (d < 0)).sum() > 100 and ((x.astype(f32) == cx) & (d > 0)).sum() > 100    # zero numerators of either sign
    xo, yo, do, flo, cxo, cyo, To = Cs.callsite_cases(1 << 16, outside=True)
    assert dev.dense_fast_ok(flo[0], cxo[0], cyo[0], 1080, 1920) == 0        # outside, the forms may differ: the library falls back (below)
    dev.callsites(xo, yo, do, flo, cxo, cyo, To)                           # (runs; nothing about its counts is asserted)


# ---- through the real library: the guard's fall-back ------------------------------------------------------------------------------
LIB_K = (300.0, 132.0, 36.0)
LIB_ROWS, LIB_COLS = 72, 264      # interior 64 x 256: four 64-pixel strips per row


def _lib_scene():
    rng = np.random.default_rng(77)
    t = rng.uniform(0, 255, (LIB_ROWS, LIB_COLS))
    for _ in range(2):
        t = (t + np.roll(t, 1, 0) + np.roll(t, 1, 1) + np.roll(t, (1, 1), (0, 1))) / 4
    I1 = t.astype(f32)
    I2 = np.roll(I1, 1, 1)
    inv = rng.uniform(0.05, 2.0, (LIB_ROWS, LIB_COLS)).astype(f32)
    maps = {"nothing": inv}
    one = inv.copy()
    one[20, 4 + 64 + 17] = 5000.0                       # a single lane of one wave
    maps["single_lane"] = one
    wave = inv.copy()
    wave[30, 4 + 128: 4 + 192] = 4096.5                 # a whole wave: strip 2 of row 30
    wave[31, 4: 4 + 64] = -6000.0
    maps["whole_wave"] = wave
    M = np.eye(4, dtype=f32)
    M[0, 3], M[2, 3] = 0.01, -0.02
    far = np.eye(4, dtype=f32)
    far[2, 3] = np.nextafter(f32(2.0 ** 20), f32(np.inf))          # a pose entry just above the guard's 2^20
    return I1, I2, maps, {"motion": M, "entry_above_2^20": far}


def test_dense_guard_falls_back_in_the_library(O):
    """lm.accumulate on a small all-dense level (every level through the dense kernel): depth maps in which nothing, a single lane of a
    wave and a whole wave exceed |d| = 4096, and a pose entry just above 2^20 — N equal to the oracle's, the sums as the existing dense
    tests compare them, and every sum BIT-identical to the ODO_DENSE_PLAIN_DIV=1 build of the same call (same association order, so any
    difference would be a per-pixel one)."""
    from odometry_amd import api
    api.default_context()
    I1, I2, maps, poses = _lib_scene()
    KD = dict(f0=LIB_K[0], cx0=LIB_K[1], cy0=LIB_K[2])
    for mname, inv in maps.items():
        res = {}
        for plain in (0, 1):
            if plain:
                os.environ["ODO_DENSE_PLAIN_DIV"] = "1"
            try:
                lm = api.LevenbergMarquardtOptimizer(0.01, 0.995, [10, 10], np.eye(4), None, 1, 28.0, intrinsics=LIB_K)
            finally:
                os.environ.pop("ODO_DENSE_PLAIN_DIV", None)
            lm.set_mode(1)                               # every level on the dense scan
            p0, d0, p1 = api.ImagePyramid(2, I1, False), api.DepthPyramid(2, inv, False), api.ImagePyramid(2, I2, False)
            res[plain] = {(pn, lvl): lm.accumulate(p0, d0, p1, lvl, T) for pn, T in poses.items() for lvl in (0, 1)}
            lm.close()
            for o in (p0, d0, p1):
                o.close()
        i0, i1, dd = O.image_pyramid(I1, 2, False), O.image_pyramid(I2, 2, False), O.depth_pyramid(inv, 2)
        for (pn, lvl), (st, acc) in res[0].items():
            what = "depth map %s, pose %s, level %d" % (mname, pn, lvl)
            ref = O.lm_accumulate(i0[lvl], i1[lvl], dd[lvl], lvl, poses[pn], robust=1, huber_delta=28.0, K=KD)
            assert st == ref["status"] and acc[28] == ref["acc"][28], what
            np.testing.assert_allclose(acc, ref["acc"], rtol=1e-11, atol=1e-6, err_msg=what)
            assert np.array_equal(acc, res[1][(pn, lvl)][1]), what + ": differs from the plain-division build"
        assert res[0][("motion", 0)][1][28] > 10000
