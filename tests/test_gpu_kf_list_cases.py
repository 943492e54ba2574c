"""The keyframe point lists and the kernels that read them, held to exact models (tests/kf_list_cases.py).

A. kf_count_kernel / kf_fill_kernel launched as the product launches them, and the by-reference instantiation of their bodies (the
   batched tracker's) from a table in global memory: every byte of rowcnt, npts and the four arrays of every level against the model —
   make_point of the valid interior pixels in raster order, the 0xAB fill everywhere else — at the edges of the chunk loop, the
   row-offset prefix, the ballot prefix, levels without interior, all eight lists and both sides of the dense_above skip.
B. lm_residual_list_kernel and lm_residual_only_list_kernel on lists built by those kernels: block partials bit for bit against
   numpy float64 additions in the kernel's documented order, residuals bit for bit against the per-point chain, the stale-launch
   guard; then lm.accumulate with every level on its list and in the automatic mode, and the hand-over rule between
   kf_fill_kernel's skip and lm_take_counts end to end.
Nothing here is a timing claim."""
import numpy as np
import pytest

import dense_cases as Dc
import devmath as D
import kf_list_cases as Kc
from test_gpu_dense_cases import _api_level_check

pytestmark = pytest.mark.gpu
f32 = np.float32
FILL64 = np.uint64(0xABABABABABABABAB)
ROBUST = (0, 1, 2)


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
    d = D.load_device(request.param)
    d.unit = request.param
    return d


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- A. the lists ----------------------------------------------------------------------------------------------------------------------
def _check_build(got, want, run, what):
    """One run of one set against the model: rowcnt and npts exact (their spare entries keep the fill), every list entry bit for bit
    with NaNs as NaNs — the model holds the fill behind npts and over the whole of a skipped level's list."""
    assert np.array_equal(got["rowcnt"][run], want["rowcnt"]), what + ": rowcnt"
    assert np.array_equal(got["npts"][run], want["npts"]), what + ": npts %s, the model's %s" % (got["npts"][run], want["npts"])
    for l in range(Kc.MAX_LEVELS):
        a, b = got["lists"][l][run], want["lists"][l]
        same = D.same_bits(a, b)
        assert same.all(), "%s: level %d, first differing entry %d of %d (npts %d)" % (what, l, int(np.argmax(~same.all(1))), len(a), want["npts"][l])


def _same_bytes(a, b):
    return (np.array_equal(a["rowcnt"], b["rowcnt"]) and np.array_equal(a["npts"], b["npts"]) and
            all(np.array_equal(_u32(x), _u32(y)) for x, y in zip(a["lists"], b["lists"])))


@pytest.mark.parametrize("case", Kc.CASES, ids=lambda c: c["id"])
def test_point_lists_equal_model(dev, host, case):
    sets = [Kc.contents(case["id"], seed) for seed in (0, 1)]
    want = []
    for levels in sets:
        points = [host.make_points(I1, D1, Kc.K, l) for l, (I1, D1) in enumerate(levels)]
        for l, (I1, D1) in enumerate(levels):                                       # make_point itself: the device build against the host build
            same = D.same_bits(dev.make_points(I1, D1, Kc.K, l), points[l])
            assert same.all(), "%s: make_point of level %d differs from the host build at %d values" % (case["id"], l, int((~same).sum()))
        want.append(Kc.expected(levels, points, case["dense_above"]))
    by_value = dev.kf_lists(sets, Kc.K, case["dense_above"], Kc.SPARE, by_ref=False)
    by_ref = dev.kf_lists(sets, Kc.K, case["dense_above"], Kc.SPARE, by_ref=True)
    for i in range(2):
        what = "%s [%s], contents %d" % (case["id"], dev.unit, i)
        _check_build(by_value[i], want[i], 0, what)
        for got, name in ((by_value[i], "by value"), (by_ref[i], "by reference")):
            second = dict(rowcnt=got["rowcnt"][1], npts=got["npts"][1], lists=[v[1] for v in got["lists"]])
            first = dict(rowcnt=got["rowcnt"][0], npts=got["npts"][0], lists=[v[0] for v in got["lists"]])
            assert _same_bytes(first, second), "%s, %s: a second build into the same buffers gives other bytes" % (what, name)
        assert _same_bytes(by_ref[i], by_value[i]), what + ": the by-reference bodies give other bytes than the by-value kernels"
        for l, skip in enumerate(want[i]["skipped"]):
            if skip:
                assert (_u32(by_value[i]["lists"][l]) == Kc.FILL32).all() and by_value[i]["npts"][0][l] > 0


# ---- B. what reads the lists -------------------------------------------------------------------------------------------------------------
_PIX = {}


def _pix(dev, n, robust, mode):
    key = (dev.unit, n, robust, mode)
    if key not in _PIX:
        I1, I2, D1, k, T = Kc.list_inputs(n)
        _PIX[key] = dev.pixels(I1, I2, D1, k, T, mode, robust, Kc.HUBER, Kc.SCALE_SQR)
    return _PIX[key]


@pytest.mark.parametrize("n,nblk", Kc.LIST_EVALS, ids=lambda v: str(v))
def test_list_kernels_equal_model_bit_for_bit(dev, n, nblk):
    """The level's list from kf_count_kernel / kf_fill_kernel, then both list kernels on nblk blocks, for L2, Huber and t-distribution
    weights: every block's 29 partial sums equal numpy float64 additions of the points' exact terms in the kernel's order BIT FOR BIT,
    the residual count with them; res[idx] equals the per-point residual (NaN: none) bit for bit; the spare partial row and the entry
    behind the last residual keep their fill; two launches agree."""
    I1, I2, D1, k, T = Kc.list_inputs(n)
    for robust in ROBUST:
        what = "n = %d on %d blocks, robust %d [%s]" % (n, nblk, robust, dev.unit)
        found, P, res = dev.list_eval(I1, I2, D1, k, T, nblk, n + 1, robust, Kc.HUBER, Kc.SCALE_SQR)
        assert found == n, what
        want, hit = Kc.list_model(_pix(dev, n, robust, 0), D1, nblk)
        assert np.array_equal(P[0, :nblk, 28], want[:, 28]), what + ": residual counts"
        diff = _u64(P[0, :nblk]) != _u64(want)
        assert not diff.any(), "%s: %d of %d partial sums differ, first at block %d sum %d: %r, the model's %r" % (
            what, int(diff.sum()), diff.size, *np.argwhere(diff)[0], P[0, :nblk][diff][0], want[diff][0])
        assert (_u64(P[:, nblk]) == FILL64).all(), what + ": written behind the last block's row"
        assert np.array_equal(_u64(P[0]), _u64(P[1])), what + ": two launches differ"
        hit3, r3 = Kc.list_points(D1, *_pix(dev, n, robust, 3)[:2])
        assert np.array_equal(hit3 != 0, hit)
        want_res = np.where(hit, r3, f32(np.nan)).astype(f32)
        assert D.same_bits(res[0, :n], want_res).all(), what + ": residuals"
        assert np.isnan(res[0, :n]).sum() == n - hit.sum()
        assert (_u32(res[:, n:]) == Kc.FILL32).all(), what + ": written behind the last residual"
        assert np.array_equal(_u32(res[0]), _u32(res[1]))


@pytest.mark.parametrize("active,level_ok", [(0, 1), (1, 0), (0, 0)])
def test_stale_list_launches_write_nothing(dev, active, level_ok):
    """A state whose level's loop has stopped, or that sits on another level than the launch expects: neither kernel writes a byte."""
    n, nblk = 513, 3
    I1, I2, D1, k, T = Kc.list_inputs(n)
    found, P, res = dev.list_eval(I1, I2, D1, k, T, nblk, n + 1, 1, Kc.HUBER, Kc.SCALE_SQR, active=active, level_ok=level_ok)
    assert found == n
    assert (_u64(P) == FILL64).all() and (_u32(res) == Kc.FILL32).all()


# ---- through the library -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 0], ids=["lists", "auto"])
@pytest.mark.parametrize("frame", Dc.API_FRAMES, ids=lambda f: "%dx%d_%dlevels" % f)
def test_list_accumulate_matches_oracle_at_small_frames(O, frame, mode):
    """lm.accumulate with every level on its point list (set_mode(2)) and with the automatic choice (set_mode(0)): the whole
    kf_fill -> PointList -> load_point route under the product's own launches."""
    from odometry_amd import api
    api.default_context()
    rows, cols, levels = frame
    worst, statuses = _api_level_check(O, api, rows, cols, levels, mode, ROBUST, "%dx%d, mode %d" % (rows, cols, mode))
    assert all(statuses[(r, 0)] == (0, 0) for r in ROBUST)
    if frame == (24, 40, 3):
        assert all(statuses[(r, 2)] == (-1, -1) for r in ROBUST)          # no interior on the coarsest level: fails like the oracle
    print("list accumulate %dx%d, mode %d: largest error / bound = %.3f" % (rows, cols, mode, worst))


@pytest.mark.parametrize("total,fuse", Kc.HANDOVER, ids=lambda v: str(v))
def test_skipped_lists_are_exactly_the_lists_never_read(O, monkeypatch, total, fuse):
    """kf_fill_kernel's skip against lm_take_counts on a 12 x 72 level (interior 256) with 128 / 129 points and ODO_FUSE_DENSE_MAX 128 /
    129, automatic mode. The optimiser first accumulates against ANOTHER keyframe of the same size with 100 points, so a list that is
    skipped and then read holds plausible stale points, not zeros: points() reports the flag lm_take_counts computes, and the sums
    match the oracle in all four combinations."""
    from odometry_amd import api
    api.default_context()
    monkeypatch.setenv("ODO_FUSE_DENSE_MAX", str(fuse))
    I1, I2, D1, K, T = Kc.handover_inputs(total)
    other = Kc.handover_inputs(100, seed=1)[2]
    seen = []

    def prime(lm):
        p0, d0, p1 = api.ImagePyramid(1, I1, False), api.DepthPyramid(1, other, False), api.ImagePyramid(1, I2, False)
        st, acc = lm.accumulate(p0, d0, p1, 0, T)
        assert st == 0 and lm.points() == ([100], [1])
        for o in (p0, d0, p1):
            o.close()

    def after(lm):
        seen.append(lm.points())

    worst, statuses = _api_level_check(O, api, 12, 72, 1, 0, ROBUST, "%d points, ODO_FUSE_DENSE_MAX %d" % (total, fuse),
                                       inputs=(I1, I2, D1, K, T), prime=prime, after=after)
    use = int(Kc.host_use_list(total, 256, fuse))
    assert seen == [([total], [use])] * len(ROBUST)
    assert all(statuses[(r, 0)] == (0, 0) for r in ROBUST)
