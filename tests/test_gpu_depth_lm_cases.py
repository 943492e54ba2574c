"""The three builds of the inverse-depth LM — depth_lm_persistent_kernel, depth_lm_step_kernel + depth_finalize_kernel, and their
batched twins — against the exact-sum model of tests/depth_lm_cases.py, bit for bit: mask, inverse depths, iteration count, cost,
counts and status. The model does not share a line with odo_math.h; tests/test_depth_lm_cases_cpu.py shows that on every case each
evaluation's error is one float whatever the order it is summed in, and that the model equals the pinned oracle. No tolerance
anywhere: every comparison is by bits."""
import struct

import numpy as np
import pytest

import depth_cases as D
import depth_lm_cases as M

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in M.CASES]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def api():
    from odometry_amd import api
    api.default_context()  # raises if the HIP library or the device is missing: no silent fallback
    return api


def _bits(v):
    return struct.unpack("I", struct.pack("f", v))[0]


def _run(api, O, L, R, prm, lm):
    """A whole ComputeDepth on a fresh estimator (ODO_DEPTH_NO_PERSIST is read at create)."""
    de = api.DepthEstimator(prm["grad_th"], prm["ssd_th"], lm["photo_th"], lm["min_depth"], lm["max_depth"], lm["lam"], lm["huber_delta"],
                            lm["precision"], lm["max_iters"], prm["boundary"], None, None, O.KITTI_BASELINE, 80000,
                            max_disparity=prm["max_disparity"], any_size=True)
    val, disp, dep = np.zeros(L.shape, np.uint8), np.zeros(L.shape, np.float32), np.zeros(L.shape, np.float32)
    st = de.ComputeDepth(L, R, val, disp, dep)
    rep, ps = de.report(), de.persistent_stats()
    de.close()
    return dict(status=st, val=val, disp=disp, dep=dep, rep=rep, ps=ps)


def _hold(tag, got, m):
    rep = got["rep"]
    print(f"{tag}: mask differs at {int((got['val'] != m['val']).sum())} pixels, inverse depth at "
          f"{int((got['dep'].view(np.uint32) != m['dep'].view(np.uint32)).sum())}, disparity at {int((got['disp'] != m['disp']).sum())}; status "
          f"{got['status']} / {m['status']}, iters {rep['iters']} / {m['iters']}, cost bits {_bits(rep['cost']):08x} / {m['cost_bits']:08x}, valid "
          f"{rep['n_valid']} / {m['n_valid']}, selected {rep['n_selected']} / {m['n_selected']}, matched {rep['n_matched']} / {m['n_matched']}, "
          f"persistent_stats {got['ps']}")
    assert np.array_equal(got["val"], m["val"]), f"{tag}: mask"
    assert np.array_equal(got["dep"].view(np.uint32), m["dep"].view(np.uint32)), f"{tag}: inverse depth"
    assert np.array_equal(got["disp"], m["disp"]), f"{tag}: disparity"
    assert (rep["iters"], rep["n_valid"], rep["n_selected"], rep["n_matched"]) == (m["iters"], m["n_valid"], m["n_selected"], m["n_matched"]), tag
    assert _bits(rep["cost"]) == m["cost_bits"], f"{tag}: cost"
    assert got["status"] == m["status"], tag


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_model_on_the_persistent_launch_and_on_the_step_launches(api, O, name, monkeypatch):
    c = M.BY_NAME[name]
    L, R, prm, _, lm = M.resolve(c)
    m = M.run_model(c)
    monkeypatch.delenv("ODO_DEPTH_NO_PERSIST", raising=False)
    one = _run(api, O, L, R, prm, lm)
    monkeypatch.setenv("ODO_DEPTH_NO_PERSIST", "1")
    steps = _run(api, O, L, R, prm, lm)
    monkeypatch.delenv("ODO_DEPTH_NO_PERSIST")
    print(f"{name} {c['lm'] and lm}: the model runs {len(m['evals'])} evaluations, modes {''.join(str(e['mode']) for e in m['evals'])}")
    persistent = lm["max_iters"] <= M.PERSIST_MAX_ITERS
    _hold(f"{name} [{'persistent launch' if persistent else 'step launches: max_iters above the persistent launch'}]", one, m)
    _hold(f"{name} [step launches]", steps, m)
    # one persistent launch that never gave up (above kDpMaxIters: the step launches without being told to); the step launches
    assert one["ps"] == ((1, 0) if persistent else (0, 0)) and steps["ps"] == (0, 0)


def test_batched_kernels_equal_the_model(api, O, monkeypatch):
    """TrackerBatch(2).init (depth_lm_persistent_batch_kernel; with ODO_BATCH_DEPTH_PERSIST=0 depth_lm_step_batch_kernel +
    depth_finalize_batch_kernel) and two Tracker.init calls on depth_cases.BATCH's pairs: outputs and depth statistics against the
    model under batch_tracker_args() / BATCH_BASELINE."""
    args = D.batch_tracker_args()
    rows, cols = D.BATCH["size"]
    models = M.batch_models()

    def hold(tag, out, stats, m):
        print(f"{tag}: {int(out[0].sum())} valid depths; differs from the model at {int((out[0] != m['val']).sum())} pixels of the mask, "
              f"{int((out[1] != m['disp']).sum())} of the disparity, {int((out[2].view(np.uint32) != m['dep'].view(np.uint32)).sum())} of the inverse "
              f"depth; depth_iters {stats['depth_iters']} / {m['iters']}, n_valid_depth {stats['n_valid_depth']} / {m['n_valid']}")
        assert np.array_equal(out[0], m["val"]), tag
        assert np.array_equal(out[1], m["disp"]), tag
        assert np.array_equal(out[2].view(np.uint32), m["dep"].view(np.uint32)), tag
        assert (stats["depth_iters"], stats["n_valid_depth"]) == (m["iters"], m["n_valid"]), tag

    monkeypatch.delenv("ODO_BATCH_DEPTH_PERSIST", raising=False)
    for name, m in models:
        assert m["n_valid"] >= 500 and {0, 1} <= {e["mode"] for e in m["evals"]}
        trk = api.Tracker(0, **args)
        trk.init(trk.upload_frame(m["pair"][0]), trk.upload_frame(m["pair"][1]))
        hold(f"{name} [Tracker.init]", trk.outputs(rows, cols), trk.stats(), m)
        trk.close()
    for env, want in ((None, (1, 0)), ("0", (0, 0))):
        if env is not None:
            monkeypatch.setenv("ODO_BATCH_DEPTH_PERSIST", env)   # read when the tracker is made
            # ... and really off: a persistent launch made all the same would lose a pair (the estimators' test hook), give up inside
            # its wait bound and be redone on the step launches — chains_redone would be 1
            monkeypatch.setenv("ODO_DEPTH_PERSIST_FAULT", "1")
            monkeypatch.setenv("ODO_DEPTH_WAIT_US", "300")
        tb = api.TrackerBatch(2, 0, **args)
        tb.init([tb.upload_frame(m["pair"][0]) for _, m in models], [tb.upload_frame(m["pair"][1]) for _, m in models])
        stats, ps = tb.stats(), tb.depth_persistent_stats()
        for i, (name, m) in enumerate(models):
            hold(f"{name} [TrackerBatch(2).init, ODO_BATCH_DEPTH_PERSIST={env}]", tb.outputs(i, rows, cols), stats[i], m)
        tb.close()
        assert ps == want
    monkeypatch.delenv("ODO_BATCH_DEPTH_PERSIST")
