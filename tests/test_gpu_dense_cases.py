"""The dense levels' scan and scale kernels held to models at small sizes (tests/dense_cases.py).

The per-pixel arithmetic of a dense level is pinned call by call (tests/test_gpu_devmath.py: dm_dense_pixels against the host build and
the oracle). Here: WHICH pixels a block of lm_dense_eval_kernel / lm_dense_eval_batch_kernel visits and how its sums are joined, at
frames whose interior is below, at and above one and two strips and one, two and eight row groups, with grid caps that give a tiny frame
the multi-unit runs the product builds above 1024 units; and the t-distribution scale kernels (list order, strided order, the
product's launch sequence with the multi-workgroup kernel) at every edge of the residual count, bit for bit against an exact model.
Sums of exact fp64 terms are held to the bound of ANY summation order, n 2^-52 sum |terms|; each test prints its largest observed
ratio to that bound. Nothing here is a timing claim."""
import functools
import math

import numpy as np
import pytest

import dense_cases as Dc
import devmath as D

pytestmark = pytest.mark.gpu
f32 = np.float32
HUBER, SCALE_SQR = 28.0, 30.25
FILL = np.uint64(0xABABABABABABABAB)
ROBUST = (0, 1, 2)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module", params=D.UNITS)
def dev(request):
    """One build of the harness: under the main unit's scheduler, then under the LM chain unit's."""
    d = D.load_device(request.param)
    d.unit = request.param
    return d


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


@functools.lru_cache(maxsize=None)
def _inputs(rows, cols):
    return Dc.case_inputs(rows, cols)


_PIXELS = {}


def _pixels(dev, rows, cols, robust):
    """Per-pixel hit and exact 29 terms of a frame (dm_dense_pixels with the plain divisions: what every guarded and unguarded pixel of
    the scan must produce), computed once per harness build, frame and weight and shared by every cap of the frame."""
    key = (dev.unit, rows, cols, robust)
    if key not in _PIXELS:
        I1, I2, D1, k, T = _inputs(rows, cols)
        hit, acc = dev.dense_pixels(I1, I2, D1, k, T, 0, robust, HUBER, SCALE_SQR)
        hit.setflags(write=False)
        acc.setflags(write=False)
        _PIXELS[key] = (hit.reshape(-1), acc.reshape(-1, 29))
    return _PIXELS[key]


def _check_partials(P, hit, acc, blocks, what):
    """Every block's row of partial sums against the pixels the model gives the block. Returns the largest |error| / bound."""
    worst = 0.0
    for b, px in enumerate(blocks):
        h = hit[px]
        assert P[b, 28] == float(h.sum()), "%s, block %d: %r residuals, the model's pixels give %d" % (what, b, P[b, 28], int(h.sum()))
        terms = acc[px]
        assert not terms[h == 0].any()
        for q in range(28):
            exact = math.fsum(terms[:, q])
            bound = Dc.sum_bound(terms[:, q], len(px))
            err = abs(P[b, q] - exact)
            assert err <= bound, "%s, block %d, sum %d: %r against %r, bound %r" % (what, b, q, P[b, q], exact, bound)
            if bound > 0:
                worst = max(worst, err / bound)
    return worst


# ---- A. the dense scan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", Dc.CASES, ids=Dc.case_id)
def test_dense_runs_equal_model(dev, case):
    """dense_level_geometry and dense_block_run as the device computes them: every block's {strip, rg, rg0, rg1, count}."""
    rows, cols, cap = case
    want = Dc.geometry(rows, cols, cap)
    geom, runs = dev.dense_runs(rows, cols, cap, want[2])
    assert geom == want
    assert np.array_equal(runs, Dc.runs(rows, cols, cap)), "first differing block %d" % int(np.argmax((runs != Dc.runs(rows, cols, cap)).any(1)))


@pytest.mark.parametrize("case", Dc.CASES, ids=Dc.case_id)
def test_dense_eval_partials_equal_model(dev, case):
    """lm_dense_eval_kernel launched as the product launches it, for L2, Huber and t-distribution weights: block b's residual count is
    exactly the number of hits among the pixels the model gives block b, each of its 28 sums is within the any-order bound of the exact
    sum of those pixels' terms, no byte of the 0xAB fill is left in the level's rows and none is touched behind them, two launches
    agree bit for bit, and so does the plain-division build of the kernel."""
    rows, cols, cap = case
    I1, I2, D1, k, T = _inputs(rows, cols)
    nblk = Dc.geometry(rows, cols, cap)[2]
    blocks = Dc.block_pixels(rows, cols, cap)
    worst = 0.0
    for robust in ROBUST:
        what = "%s, robust %d" % (Dc.case_id(case), robust)
        hit, acc = _pixels(dev, rows, cols, robust)
        P = dev.dense_eval(I1, I2, D1, k, T, cap, nblk + 1, robust, HUBER, SCALE_SQR)
        assert not (_bits(P[:nblk]) == FILL).any(), what + ": a partial sum was never written"
        assert (_bits(P[nblk:]) == FILL).all(), what + ": written behind the level's rows"
        worst = max(worst, _check_partials(P, hit, acc, blocks, what))
        again = dev.dense_eval(I1, I2, D1, k, T, cap, nblk + 1, robust, HUBER, SCALE_SQR)
        assert np.array_equal(_bits(again), _bits(P)), what + ": two launches differ"
        plain = dev.dense_eval(I1, I2, D1, k, T, cap, nblk + 1, robust, HUBER, SCALE_SQR, plain_div=1)
        assert np.array_equal(_bits(plain), _bits(P)), what + ": the plain-division kernel differs"
    print("dense partials %s [%s]: largest error / bound = %.3f" % (Dc.case_id(case), dev.unit, worst))


BATCH = (dict(frame=(89, 137), cap=17, robust=1, active=1),       # the widest grid: 17 blocks -> 24 columns of the launch
         dict(frame=(9, 9), cap=Dc.GRID_CAP, robust=0, active=1),  # nblk == 1: blocks 1 .. 23 of its row leave at once
         dict(frame=(41, 137), cap=9, robust=2, active=1),         # nblk not a multiple of 8
         dict(frame=(40, 73), cap=5, robust=1, active=0))          # a stream whose Solve is over: its rows stay as they were


@pytest.mark.parametrize("plain_div", [0, 1])
def test_dense_eval_batch_equals_single_launches(dev, plain_div):
    """lm_dense_eval_batch_kernel over four items of different sizes in one launch: every active stream's partial rows equal its own
    single launch bit for bit (and the model, within the bound), the inactive stream's rows and the spare row behind every stream
    keep their fill."""
    items, nblks = [], []
    for it in BATCH:
        rows, cols = it["frame"]
        I1, I2, D1, k, T = _inputs(rows, cols)
        nblks.append(Dc.geometry(rows, cols, it["cap"])[2])
        items.append(dict(I1=I1, I2=I2, D1=D1, k=k, T=T, cap=it["cap"], n_rows=nblks[-1] + 1, robust=it["robust"], huber_delta=HUBER,
                          scale_sqr=SCALE_SQR, active=it["active"]))
    assert 1 in nblks and len(set(nblks)) == len(nblks) and max(nblks) % 8
    out = dev.dense_eval_batch(items, plain_div)
    worst = 0.0
    for it, a, P, nblk in zip(BATCH, items, out, nblks):
        what = "stream %dx%d" % it["frame"]
        if not it["active"]:
            assert (_bits(P) == FILL).all(), what + ": an inactive stream's rows were written"
            continue
        single = dev.dense_eval(a["I1"], a["I2"], a["D1"], a["k"], a["T"], a["cap"], nblk + 1, a["robust"], HUBER, SCALE_SQR, plain_div)
        assert np.array_equal(_bits(P), _bits(single)), what + ": differs from its single launch"
        assert (_bits(P[nblk:]) == FILL).all() and not (_bits(P[:nblk]) == FILL).any()
        hit, acc = _pixels(dev, *it["frame"], it["robust"])
        worst = max(worst, _check_partials(P, hit, acc, Dc.block_pixels(*it["frame"], it["cap"]), what))
    print("dense batch [%s, plain_div %d]: largest error / bound = %.3f" % (dev.unit, plain_div, worst))


# ---- B. the t-distribution scale ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", Dc.scale_cases(), ids=lambda v: str(v))
def test_tdist_scale_equals_model(dev, n, kind):
    """sigma^2 of every order that admits the size — the single-workgroup kernel in list order (n <= 40960) and in strided order, and
    the product's launch sequence twice in a row on one exchange buffer (pass parity, epoch reuse) — equals the exact model's bit for
    bit (tests/test_dense_cases_cpu.py: one admissible float at every pass). A multi-workgroup launch that gave up (a busy card) is
    printed; its fall-back's result is held to the same model."""
    res = Dc.residuals(n, kind)
    want, passes, single = Dc.scale_expected(n, kind)
    assert single
    want_bits = _bits(np.array([want], f32))[0]
    if n <= Dc.SINGLE_LIST_MAX:
        s2, info = dev.tdist_scale(res, Dc.ORDER_LIST)
        assert _bits(s2)[0] == want_bits, "list order: %r, model %r (%d passes)" % (s2[0], want, passes)
        assert info[0, 2] == Dc.WROTE_LIST
    s2, info = dev.tdist_scale(res, Dc.ORDER_STRIDED)
    assert _bits(s2)[0] == want_bits, "strided order: %r, model %r (%d passes)" % (s2[0], want, passes)
    assert info[0, 2] == Dc.WROTE_STRIDED
    s2, info = dev.tdist_scale(res, Dc.ORDER_PRODUCT, reps=2)
    lst, G, fits, _ = Dc.scale_plan(n)
    for rep in range(2):
        assert _bits(s2)[rep] == want_bits, "product launch %d: %r, model %r (%d passes), info %s" % (rep, s2[rep], want, passes, info[rep])
        if lst or not fits:
            assert tuple(info[rep, :3]) == (0, 0, Dc.product_writer(n))
        else:
            assert info[rep, 0] == G
            if info[rep, 1]:
                print("tdist scale n = %d, %s [%s]: multi-workgroup launch %d GAVE UP, the fall-back wrote sigma" % (n, kind, dev.unit, rep))
            else:
                assert info[rep, 2] == Dc.WROTE_MULTI
    assert _bits(s2)[0] == _bits(s2)[1]


# ---- through the public API, with the product's own cap ---------------------------------------------------------------------------
def _api_level_check(O, api, rows, cols, levels, mode, robusts, what, inputs=None, prime=None, after=None):
    """lm.accumulate on every level against the oracle's accumulation: status and N exact; for L2 and Huber weights every sum within
    the any-order bound of the exact sum of accumulate_row's products over the oracle's dumped r, w, J; for t-distribution weights
    (sigma enters every weight) rtol 1e-11, atol 1e-9 against the oracle's sums, which a 1-ulp error of sigma cannot pass.
    Returns the largest error / bound. inputs: (I1, I2, inverse depth, K, T) in place of Dc.api_inputs(rows, cols); prime(lm) /
    after(lm): called on every optimiser before its first and after its last accumulation (tests/test_gpu_kf_list_cases.py)."""
    I1, I2, inv, K, T = inputs or Dc.api_inputs(rows, cols)
    KD = dict(f0=K[0], cx0=K[1], cy0=K[2])
    p0, d0, p1 = api.ImagePyramid(levels, I1, False), api.DepthPyramid(levels, inv, False), api.ImagePyramid(levels, I2, False)
    i0, i1, dd = O.image_pyramid(I1, levels, False), O.image_pyramid(I2, levels, False), O.depth_pyramid(inv, levels)
    worst, statuses = 0.0, {}
    try:
        for robust in robusts:
            lm = api.LevenbergMarquardtOptimizer(0.01, 0.995, [10] * levels, np.eye(4), None, robust, HUBER, intrinsics=K)
            lm.set_mode(mode)
            if prime:
                prime(lm)
            for level in range(levels):
                w = "%s, level %d, robust %d" % (what, level, robust)
                st, acc = lm.accumulate(p0, d0, p1, level, T)
                n_px = max(1, i0[level].size)
                ref = O.lm_accumulate(i0[level], i1[level], dd[level], level, T, robust=robust, huber_delta=HUBER, K=KD, dump=n_px)
                statuses[(robust, level)] = (st, ref["status"])
                assert st == ref["status"], w
                assert acc[28] == ref["acc"][28], w + ": number of residuals"
                n = int(ref["acc"][28])
                if robust == 2:
                    np.testing.assert_allclose(acc, ref["acc"], rtol=1e-11, atol=1e-9, err_msg=w)
                    continue
                terms = Dc.row_products(ref["r"][:n], ref["w"][:n], ref["J"][:n])
                for q in range(28):
                    exact, bound = math.fsum(terms[:, q]), Dc.sum_bound(terms[:, q], n)
                    err = abs(acc[q] - exact)
                    assert err <= bound, "%s, sum %d: %r against %r, bound %r" % (w, q, acc[q], exact, bound)
                    if bound > 0:
                        worst = max(worst, err / bound)
            if after:
                after(lm)
            lm.close()
    finally:
        for o in (p0, d0, p1):
            o.close()
    return worst, statuses


@pytest.mark.parametrize("frame", Dc.API_FRAMES, ids=lambda f: "%dx%d_%dlevels" % f)
def test_dense_accumulate_matches_oracle_at_small_frames(O, frame):
    """lm.accumulate with every level on the dense scan (set_mode(1)) and the product's grid cap."""
    from odometry_amd import api
    api.default_context()
    rows, cols, levels = frame
    worst, statuses = _api_level_check(O, api, rows, cols, levels, 1, ROBUST, "%dx%d" % (rows, cols))
    assert all(statuses[(r, 0)] == (0, 0) for r in ROBUST)
    if frame == (24, 40, 3):
        assert all(statuses[(r, 2)] == (-1, -1) for r in ROBUST)          # no interior on the coarsest level: fails like the oracle
    if frame == (4108, 72, 1):
        assert Dc.geometry(rows, cols, Dc.GRID_CAP) == (1, 1025, 1024)     # runs of two units under the product's own cap
    print("dense accumulate %dx%d: largest error / bound = %.3f" % (rows, cols, worst))


def test_list_level_scale_matches_oracle_above_the_list_order(O):
    """A 26 696-point list level with t-distribution weights: its scale runs on the multi-workgroup kernel (n > 16 384); the sums
    carry sigma in every weight and must equal the oracle's to rtol 1e-11."""
    from odometry_amd import api
    api.default_context()
    rows, cols = Dc.LIST_FRAME
    assert (rows - 8) * (cols - 8) > Dc.LIST_MAX
    I1, I2, inv, K, T = Dc.list_inputs()
    KD = dict(f0=K[0], cx0=K[1], cy0=K[2])
    p0, d0, p1 = api.ImagePyramid(1, I1, False), api.DepthPyramid(1, inv, False), api.ImagePyramid(1, I2, False)
    lm = api.LevenbergMarquardtOptimizer(0.01, 0.995, [10], np.eye(4), None, 2, HUBER, intrinsics=K)
    lm.set_mode(2)
    st, acc = lm.accumulate(p0, d0, p1, 0, T)
    assert lm.points() == ([(rows - 8) * (cols - 8)], [1])
    multi, fallbacks = lm.tdist_stats()
    ref = O.lm_accumulate(I1, I2, inv, 0, T, robust=2, huber_delta=HUBER, K=KD)
    assert st == 0 == ref["status"] and acc[28] == ref["acc"][28] > Dc.LIST_MAX
    assert multi == 1
    if fallbacks:
        print("list-level scale: the multi-workgroup launch GAVE UP, the fall-back wrote sigma")
    np.testing.assert_allclose(acc, ref["acc"], rtol=1e-11, atol=1e-9)
    lm.close()
    for o in (p0, d0, p1):
        o.close()


def test_batched_dense_solves_of_different_sizes_equal_separate_solves():
    """api.solve_batch accepts streams of different frame sizes (they do not share dense launches: the batched evaluation is taken for
    equal sizes only, the harness test above is the cover of its different-size grid): two small dense Solves equal the separate ones
    bit for bit."""
    from odometry_amd import api
    api.default_context()
    frames = ((41, 137, 2), (24, 72, 2))
    pyrs, Ks = [], []
    for rows, cols, levels in frames:
        I1, I2, inv, K, _ = Dc.api_inputs(rows, cols)
        inv = np.where(np.abs(inv) < 0.01, f32(0.3), np.minimum(np.abs(inv), f32(2.0))).astype(f32)
        pyrs.append((api.ImagePyramid(levels, I1, False), api.DepthPyramid(levels, inv, False), api.ImagePyramid(levels, I2, False)))
        Ks.append(K)

    def make(i):
        lm = api.LevenbergMarquardtOptimizer(0.01, 0.995, [10, 10], np.eye(4), None, 1, HUBER, intrinsics=Ks[i])
        lm.set_mode(1)
        return lm
    want = []
    for i, (p0, d0, p1) in enumerate(pyrs):
        lm = make(i)
        want.append((lm.Solve(p0, d0, p1), lm.last_status, lm.launch_stats()[0]))
        lm.close()
    lms = [make(i) for i in range(len(frames))]
    poses, status = api.solve_batch(lms, [p[0] for p in pyrs], [p[1] for p in pyrs], [p[2] for p in pyrs])
    for i, lm in enumerate(lms):
        assert status[i] == want[i][1]
        assert np.array_equal(_bits(np.asarray(poses[i], f32)), _bits(np.asarray(want[i][0], f32))), "stream %d" % i
        assert lm.launch_stats()[0] == want[i][2]
        lm.close()
    assert want[0][2] > 1 and want[1][2] > 1
    for p in pyrs:
        for o in p:
            o.close()
