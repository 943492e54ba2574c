"""The depth estimator's selection and scan kernels on the tied and edge inputs of tests/depth_cases.py (the CPU half,
tests/test_depth_cases_cpu.py, shows that each row reaches the branch it is in the table for).

Stage 1 (DisparityDepthEstimate) of every row against the oracle, bit for bit, and against the rows' closed forms. Stage 2 (the whole
ComputeDepth) of every row with the persistent depth-LM launch against the same call on the step launches, bit for bit — an identity
the project claims for any input, rows with no matched point or with all depths equal included. Stage 2 of these rows against an
independent answer is tests/test_gpu_depth_lm_cases.py's: on every row each evaluation's error sum is one float whatever the order it is
added in (tests/test_depth_lm_cases_cpu.py shows it), so no accept / reject decision can flip with the summation order, and both launches
are held bit for bit to an exact-sum model that equals the oracle. The started-ahead and prepared entry points, and the batched kernels (TrackerBatch.init), on a few of the rows."""
import ctypes as C
import struct

import numpy as np
import pytest

import depth_cases as D

pytestmark = pytest.mark.gpu
ROWS = [r["name"] for r in D.TABLE]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def api():
    from odometry_amd import api
    api.default_context()  # raises if the HIP library or the device is missing: no silent fallback
    return api


def _estimator(api, O, prm):
    """The oracle's depth_params defaults (the runner's), the row's selection / scan parameters."""
    return api.DepthEstimator(prm["grad_th"], prm["ssd_th"], 15.0, 0.1, 30.0, 0.01, 28.0, 0.995, 50, prm["boundary"], None, None,
                              O.KITTI_BASELINE, 80000, max_disparity=prm["max_disparity"], any_size=True)


def _bufs(shape):
    return np.zeros(shape, np.uint8), np.zeros(shape, np.float32), np.zeros(shape, np.float32)


def _same_report(a, b):
    """report() dictionaries equal, the cost by its bits (a row whose points all fail has a NaN cost on both sides)."""
    bits = lambda v: struct.pack("f", v)   # noqa: E731
    return {k: v for k, v in a.items() if k != "cost"} == {k: v for k, v in b.items() if k != "cost"} and bits(a["cost"]) == bits(b["cost"])


@pytest.mark.parametrize("name", ROWS)
def test_row_stage_1_matches_the_oracle_bit_for_bit(api, O, name):
    r = D.BY_NAME[name]
    L, R, prm, ref = D.reference(r)
    de = _estimator(api, O, prm)
    val, disp, dep = _bufs(L.shape)
    assert de.DisparityDepthEstimate(L, R, val, disp, dep) == 0
    rep = de.report()
    de.close()
    print(f"{name}: mask differs at {int((val != ref['val']).sum())} pixels, disparity at {int((disp != ref['disp']).sum())}, inverse depth at "
          f"{int((dep != ref['dep']).sum())}; selected {rep['n_selected']} / {ref['n_selected']}, matched {rep['n_matched']} / {ref['n_matched']}")
    assert np.array_equal(val, ref["val"]), "selection mask differs"
    assert np.array_equal(disp, ref["disp"]), "disparity (the scan's first minimum) differs"
    assert np.array_equal(dep, ref["dep"])
    assert rep["n_selected"] == ref["n_selected"] and rep["n_matched"] == ref["n_matched"]
    A = dict(size=L.shape, bnd=prm["boundary"], params=prm)
    out = dict(val=val, disp=disp, dep=dep, n_selected=rep["n_selected"], n_matched=rep["n_matched"])
    D.closed_generic(A, out)
    if r["closed"]:
        r["closed"](A, out)


@pytest.mark.parametrize("name", ROWS)
def test_row_stage_2_is_the_same_on_the_persistent_launch_and_on_the_step_launches(api, O, name, monkeypatch):
    L, R, prm, _ = D.reference(D.BY_NAME[name])

    def run():
        de = _estimator(api, O, prm)   # a fresh estimator: ODO_DEPTH_NO_PERSIST is read at create
        val, disp, dep = _bufs(L.shape)
        st = de.ComputeDepth(L, R, val, disp, dep)
        rep, ps = de.report(), de.persistent_stats()
        de.close()
        return st, val, disp, dep, rep, ps

    st, val, disp, dep, rep, ps = run()
    monkeypatch.setenv("ODO_DEPTH_NO_PERSIST", "1")
    st2, val2, disp2, dep2, rep2, ps2 = run()
    monkeypatch.delenv("ODO_DEPTH_NO_PERSIST")
    print(f"{name}: status {st} / {st2}, report {rep} / {rep2}, mask differs at {int((val != val2).sum())} pixels, inverse depth at "
          f"{int((dep.view(np.uint32) != dep2.view(np.uint32)).sum())}")
    assert ps == (1, 0) and ps2 == (0, 0)            # one persistent launch that never gave up; the step launches
    assert st == st2 and st in (0, -1)
    assert np.array_equal(val, val2) and np.array_equal(disp, disp2)
    assert np.array_equal(dep.view(np.uint32), dep2.view(np.uint32))
    assert _same_report(rep, rep2)
    assert rep["n_valid"] == int(val.sum()) and (st == 0) == (rep["n_valid"] >= 500)


@pytest.mark.parametrize("name", D.AHEAD_ROWS)
def test_started_ahead_and_prepared_calls_equal_the_plain_call(api, O, name):
    """odo_depth_compute_begin_dev / _end_dev on a second context, and odo_depth_prepare_left_dev + odo_depth_compute_dev_stamped (the
    selection run ahead, with val == NULL), against odo_depth_compute_dev: status, mask, disparities, inverse depths and report."""
    L, R, prm, _ = D.reference(D.BY_NAME[name])
    ctx, side = api.default_context(), api.Context(0)
    rows, cols = L.shape
    n = rows * cols
    de = _estimator(api, O, prm)
    l, r = ctx.upload(L), ctx.upload(R)
    held = [l, r]

    def outs():
        o = (ctx.alloc(n), ctx.alloc(4 * n), ctx.alloc(4 * n))
        held.extend(o)
        return o

    def get(o):
        return (ctx.download(o[0], (rows, cols), np.uint8), ctx.download(o[1], (rows, cols), np.float32),
                ctx.download(o[2], (rows, cols), np.float32))

    o = outs()
    st = de.compute_dev(l, r, rows, cols, *o)
    want, want_rep = get(o), de.report()
    assert st in (0, -1) and want_rep["n_selected"] > 0

    def check(o, got_st, tag):
        got = get(o)
        assert got_st == st, tag
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), tag
        assert _same_report(de.report(), want_rep), tag

    o = outs()
    assert de.compute_begin_dev(side, l, r, rows, cols, *o, 11, 21) == 0 and de.early_pending()
    check(o, de.compute_end_dev(l, r, rows, cols, *o, 11, 21), "started ahead")
    assert not de.early_pending()
    o = outs()
    lib = ctx.lib
    assert lib.odo_depth_prepare_left_dev(de.h, side.h, l, rows, cols, C.c_ulonglong(77)) == 0
    check(o, lib.odo_depth_compute_dev_stamped(de.h, l, r, rows, cols, *o, C.c_ulonglong(77)), "prepared left half")
    assert de.persistent_stats() == (1, 0)
    de.close()
    ctx.synchronize()
    for p in held:
        ctx.free(p)
    side.close()


def test_batched_kernels_equal_the_single_ones_on_tied_rows(api, O):
    """TrackerBatch(2).init (depth_select_batch_kernel, depth_disparity_batch_kernel) on a periodic pair and a tied-median pair against
    two Tracker.init calls: masks, disparities and inverse depths bit for bit."""
    args = D.batch_tracker_args()
    rows, cols = D.BATCH["size"]
    pairs = [D.pair(D.BY_NAME[name], D.BATCH["size"]) for name in D.BATCH["rows"]]
    singles = []
    for Lh, Rh in pairs:
        trk = api.Tracker(0, **args)
        trk.init(trk.upload_frame(Lh), trk.upload_frame(Rh))
        singles.append(trk.outputs(rows, cols))
        trk.close()
    tb = api.TrackerBatch(2, 0, **args)
    tb.init([tb.upload_frame(p[0]) for p in pairs], [tb.upload_frame(p[1]) for p in pairs])
    for i, name in enumerate(D.BATCH["rows"]):
        got = tb.outputs(i, rows, cols)
        print(f"{name}: {int(got[0].sum())} valid depths; differs from the single tracker at "
              f"{[int((a.view(np.uint8) != b.view(np.uint8)).sum()) for a, b in zip(got, singles[i])]} bytes of mask / disparity / inverse depth")
        assert int(singles[i][0].sum()) >= 500
        for a, b in zip(got, singles[i]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    tb.close()
