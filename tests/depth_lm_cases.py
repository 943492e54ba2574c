"""The inverse-depth LM (DepthOptimization, ref: src/depth_estimate.cpp:80-242) as an exact-sum model, and the cases its three
builds — depth_lm_step_kernel + depth_finalize_kernel, depth_lm_persistent_kernel, the batched twins — are held to
(tests/test_depth_lm_cases_cpu.py, tests/test_gpu_depth_lm_cases.py). Nothing here imports the GPU library.

The model is numpy float32 with one rounding per operation and the kernels' association; every evaluation's error sum is taken
EXACTLY (math.fsum of the float32 terms) and rounded once. The kernels add the same terms in fp64 in some fixed order: any order of n
non-negative terms stays within n 2^-52 S of their exact sum S, so where every float64 of [S - n 2^-52 S, S + n 2^-52 S] rounds to the
same float32, (float)fe, err_now and the accept / reject decision that follows are known bit for bit WHATEVER the order (`decidable`).
Where that interval straddles a float32 boundary a second argument is tried: if every term is a multiple of one power of two 2^q and
S < 2^53 2^q, every partial sum of every order is exactly representable and the sum is S itself.

The driver and the write-back filters are restated from the reference's lines (:141-168, :176-191), not from odo_math.h.

CASES = every row of depth_cases.TABLE at the runner's defaults + the parameter variants that reach what the defaults do not (a
lambda break, a rejected first evaluation, equality on the depth window, max_iters of 0, 1 and above the persistent launch's 250).
Each case carries floors on the branch counts of the model's own run, in the style of depth_cases.py: (floor, count measured when the
case was written)."""
import math

import numpy as np

import depth_cases as D

f32 = np.float32
PERSIST_MAX_ITERS = 250       # kDpMaxIters: above it ComputeDepth runs the step launches (checked against kernels.hip.h by the CPU test)
LM_DEFAULTS = dict(photo_th=15.0, min_depth=0.1, max_depth=30.0, lam=0.01, huber_delta=28.0, precision=0.995, max_iters=50)
COUNTS = ("points", "evaluations", "mode0", "mode1", "mode2", "mode3", "first_rejected", "budget_exhausted", "fn_zero", "out_left",
          "out_right", "nan_trial", "wf_eq_2", "wf_eq_cols_m2", "r_eq_huber", "res_eq_photo", "res_over_photo", "res_sentinel",
          "over_max_depth", "under_min_depth", "eq_max_depth", "eq_min_depth", "cur_le_0", "d0_zero")


def one_float(S, n):
    """Does every float64 within n 2^-52 S of S round to the same float32? (The bound is widened by a float64 step on each side for
    its own rounding.)"""
    if S == 0.0 or not math.isfinite(S):
        return True
    e = n * 2.0 ** -52 * S
    lo, hi = np.nextafter(S - e, -np.inf), np.nextafter(S + e, np.inf)
    with np.errstate(over="ignore"):
        return bool(f32(lo) == f32(hi))


def every_order_exact(terms, S):
    """Every term a multiple of 2^q (q = the lowest set bit over the terms) and S < 2^53 2^q: every partial sum of non-negative terms
    is a multiple of 2^q no larger than S, so it is a float64, and no addition of any order rounds."""
    t = terms[terms != 0.0]
    if not len(t):
        return True
    m, e = np.frexp(t)
    M = (m * 2.0 ** 53).astype(np.int64)                      # exact: m has at most 24 significant bits
    q = int((e.astype(np.int64) - 53 + np.log2((M & -M).astype(np.float64)).astype(np.int64)).min())
    return S < 2.0 ** (53 + q)


def model(L, R, val1, dep1, params):
    """DepthOptimization on the points of val1 == 1 (raster order), started from dep1. params: baseline, f0 and the keys of LM_DEFAULTS.
    Returns dict(val, dep, iters, cost (a float32), cost_bits, n_valid, status, evals = [dict(mode, decidable, how, S, n, err_now)],
    counts)."""
    p = {k: (v if k == "max_iters" else f32(v)) for k, v in params.items()}
    rows, cols = L.shape
    ys, xs = np.nonzero(val1 == 1)
    n = len(xs)
    d0 = dep1[ys, xs].astype(f32)
    left = L[ys, xs]
    Rr = R[ys]                                                 # a row of the right image per point
    ar = np.arange(n)
    xf = xs.astype(f32)
    txfx = p["baseline"] * p["f0"]                             # tx * fx (:217, :229)
    half = txfx * f32(0.5)
    hd = p["huber_delta"]
    c = dict.fromkeys(COUNTS, 0)
    c["points"], c["d0_zero"] = n, int((d0 == 0).sum())
    cur, pre, tmp, res = d0.copy(), np.zeros(n, f32), d0.copy(), np.zeros(n, f32)
    jt, bb = np.ones(n, f32), np.zeros(n, f32)
    lam, err_last, err_now, it = p["lam"], f32(1e10), f32(0.0), 0
    evals = []
    with np.errstate(all="ignore"):
        while p["max_iters"] > it:                             # :141
            # ---- ComputeResidualJacobian at tmp (:200-242) ----
            wf = np.floor(xf - txfx * tmp)                     # :217
            inr = (wf >= f32(2.0)) & (wf <= f32(cols - 2))     # :219, a NaN is out of range
            wx = np.where(inr, wf, f32(2.0)).astype(np.int64)
            r = left - Rr[ar, wx]                              # :226
            a = np.abs(r)
            w = np.where(a <= hd, f32(1.0), hd / a)            # :228
            rd = half * (Rr[ar, wx + 1] - Rr[ar, wx - 1])      # :229
            term = ((r * r) * w)[inr]                          # :233
            jt = np.where(inr, (rd * rd) * w, f32(0.0))        # :234, :220
            bb = np.where(inr, ((-rd) * w) * r, f32(0.0))      # :235, :221
            res = np.where(inr, a, f32(-1000.0))               # :231, :222
            fn = int(inr.sum())
            t64 = term.astype(np.float64)
            S = math.fsum(t64.tolist())
            err_now = (f32(1.0) / f32(fn)) * f32(S)            # :239
            how = "interval" if one_float(S, fn) else ("exact" if every_order_exact(t64, S) else None)
            c["evaluations"] += 1
            c["fn_zero"] += fn == 0
            c["out_left"] += int((wf < f32(2.0)).sum())
            c["out_right"] += int((wf > f32(cols - 2)).sum())
            c["nan_trial"] += int(np.isnan(tmp).sum())
            c["wf_eq_2"] += int((wf == f32(2.0)).sum())
            c["wf_eq_cols_m2"] += int((wf == f32(cols - 2)).sum())
            c["r_eq_huber"] += int((a[inr] == hd).sum())
            # ---- the driver (:150-161) ----
            if err_now > err_last:                             # :150
                lam = lam * f32(10.0)                          # :151
                mode = 2 if lam > f32(1e5) else 0              # :152
                if mode == 0:
                    cur = pre.copy()                           # :153
            else:
                cur = tmp.copy()                               # :155
                pre = cur.copy()                               # :156
                mode = 3 if err_now / err_last > p["precision"] else 1   # :157-158
                if mode == 1:
                    err_last = err_now                         # :159
                    lam = max(lam / f32(10.0), f32(1e-7))      # :160
            evals.append(dict(mode=mode, decidable=how is not None, how=how, S=S, n=fn, err_now=err_now))
            c[f"mode{mode}"] += 1
            c["first_rejected"] += len(evals) == 1 and mode in (0, 2)
            if mode >= 2:
                break
            A = jt + lam * jt                                  # :164
            tmp = (f32(1.0) / A) * bb + cur                    # :165-166
            it += 1                                            # :167
        c["budget_exhausted"] = int(p["max_iters"] > 0 and it == p["max_iters"])
        # ---- write-back and filters (:176-191) ----
        photo_bad = (res > p["photo_th"]) | (res == f32(-1000.0))          # :178
        inv = f32(1.0) / cur
        window_bad = (inv > p["max_depth"]) | (inv < p["min_depth"])       # :183
        good = ~photo_bad & ~window_bad
    c["res_eq_photo"] = int((res == p["photo_th"]).sum())
    c["res_over_photo"] = int((res > p["photo_th"]).sum())
    c["res_sentinel"] = int((res == f32(-1000.0)).sum())
    c["over_max_depth"] = int((~photo_bad & (inv > p["max_depth"])).sum())
    c["under_min_depth"] = int((~photo_bad & (inv < p["min_depth"])).sum())
    c["eq_max_depth"] = int((~photo_bad & (inv == p["max_depth"])).sum())
    c["eq_min_depth"] = int((~photo_bad & (inv == p["min_depth"])).sum())
    c["cur_le_0"] = int((cur <= 0).sum())
    val, dep = np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), f32)
    val[ys[good], xs[good]] = 1
    dep[ys[good], xs[good]] = cur[good]
    n_valid = int(good.sum())
    return dict(val=val, dep=dep, iters=it, cost=f32(err_now), cost_bits=int(np.asarray(err_now, f32).view(np.uint32)), n_valid=n_valid,
                status=-1 if n_valid < 500 else 0, evals=evals, counts={k: int(v) for k, v in c.items()})


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def case(row, name=None, floors=None, why="", **lm):
    return dict(name=name or row, row=row, lm=lm, floors=floors or {}, why=why)


COMMONEST = "the commonest 1 / d0 of the oracle's stage 1"
# floors of table rows at the defaults: the rows that reach most of the branches, and the rows that run out of budget; every other
# row is held to the floor every case has (it has points, and evaluations unless max_iters is 0). EXACT counts must be equal.
EXACT = ("evaluations",)
ROW_FLOORS = {
    "trip-edges": dict(points=(40960, 40960), out_left=(500, 1069), out_right=(80, 173), nan_trial=(10000, 21530), wf_eq_2=(100, 264),
                       wf_eq_cols_m2=(1, 8), r_eq_huber=(1000, 2630), res_eq_photo=(50, 190), over_max_depth=(4000, 8478),
                       under_min_depth=(1000, 2648), cur_le_0=(4000, 8173), d0_zero=(8000, 16008), mode3=(1, 1)),
    "tap-edges-b2-c1": dict(out_left=(300, 600), out_right=(1, 5), nan_trial=(10000, 27377), wf_eq_2=(1000, 2511), wf_eq_cols_m2=(1, 2),
                            r_eq_huber=(300, 646), res_eq_photo=(5, 18), mode0=(10, 25), mode1=(10, 22), mode3=(1, 1)),
    "periodic-p16-d11-md0": dict(mode0=(10, 22), mode1=(10, 22), out_right=(1, 2), res_eq_photo=(1, 1), under_min_depth=(50, 103)),
    "periodic-p5-d3-md0": dict(points=(7296, 7296), mode0=(5, 11)),
    "never-below-start": dict(d0_zero=(17000, 17401), out_left=(1000, 2398), out_right=(1000, 2102), wf_eq_cols_m2=(50, 104),
                              cur_le_0=(3000, 6720), res_sentinel=(2500, 5041)),
    "on-ssd-threshold": dict(res_eq_photo=(10, 36), r_eq_huber=(100, 237), mode0=(4, 8), wf_eq_cols_m2=(1, 2), out_right=(10, 38)),
    "radix-pass": dict(points=(40960, 40960), mode0=(2, 5)),
    "cap": dict(budget_exhausted=(1, 1), evaluations=(50, 50)),
    "flat-and-textured": dict(budget_exhausted=(1, 1), evaluations=(50, 50), mode0=(1, 2)),
    "all-tie-md0": dict(budget_exhausted=(1, 1), fn_zero=(40, 49), res_sentinel=(8814, 8814)),
    "all-tie-md128": dict(budget_exhausted=(1, 1), fn_zero=(40, 49)),
}
VARIANTS = [
    case("tap-edges-b2-c1", "tap-edges-b2-c1/precision-1-iters-250", dict(mode2=(1, 1), evaluations=(148, 148), mode0=(50, 76), mode1=(50, 71)),
         "ends in a lambda break after 147 iterations, on the persistent launch", precision=1.0, max_iters=250),
    case("tap-edges-b2-c1", "tap-edges-b2-c1/precision-1-iters-251", dict(mode2=(1, 1), evaluations=(148, 148)),
         "the same trajectory above kDpMaxIters: step launches only", precision=1.0, max_iters=251),
    case("tap-edges-b2-c1", "tap-edges-b2-c1/iters-0", dict(evaluations=(0, 0), cur_le_0=(1000, 1838)),
         "no evaluation: cost 0, the scan's depths filtered", max_iters=0),
    case("tap-edges-b2-c1", "tap-edges-b2-c1/iters-1", dict(evaluations=(1, 1), budget_exhausted=(1, 1), res_eq_photo=(5, 14)), "one evaluation",
         max_iters=1),
    case("tap-edges-b2-c1", "tap-edges-b2-c1/iters-0-on-max-depth", dict(evaluations=(0, 0), eq_max_depth=(10000, 12988), over_max_depth=(1850, 1860)),
         "1 / cur == max_depth stays valid, the 22 points farther away drop", max_iters=0, max_depth=COMMONEST),
    case("tap-edges-b2-c1", "tap-edges-b2-c1/iters-0-on-min-depth", dict(evaluations=(0, 0), eq_min_depth=(10000, 12988)),
         "1 / cur == min_depth stays valid", max_iters=0, min_depth=COMMONEST),
    case("never-below-start", "never-below-start/huber-1e9", dict(first_rejected=(1, 1), mode0=(5, 7), mode2=(1, 1), cur_le_0=(17401, 17401)),
         "err_now of 5.1e10 > 1e10: the first evaluation is rejected, current falls back to the zero pre vector", huber_delta=1e9),
    case("never-below-start", "never-below-start/huber-1e9-lambda-1e5", dict(first_rejected=(1, 1), mode2=(1, 1), evaluations=(1, 1)),
         "lambda break at evaluation 0: iters == 0", huber_delta=1e9, lam=1e5),
    case("periodic-p16-d11-md0", "periodic-p16-d11-md0/lambda-100", dict(mode0=(10, 20), mode1=(10, 20), evaluations=(41, 41)),
         "a long run that mixes rejections and acceptances from a high damping", lam=100.0),
]
CASES = [case(r["name"], floors=ROW_FLOORS.get(r["name"])) for r in D.TABLE] + VARIANTS
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES) and not set(ROW_FLOORS) - set(D.BY_NAME)
# A case is in the list or it is not; nothing is skipped at run time. NOT_DECIDABLE names the table rows (never a variant) whose
# evaluations no argument above decides, with the reason — see the CPU test.
NOT_DECIDABLE = {}


_resolved, _models = {}, {}


def resolve(c):
    """(L, R, stage-1 parameters, the oracle's stage-1 result, the LM's parameters as numbers) of the case."""
    if c["name"] not in _resolved:
        L, R, prm, ref = D.reference(D.BY_NAME[c["row"]])
        lm = dict(LM_DEFAULTS, **c["lm"])
        for k, v in lm.items():
            if v == COMMONEST:
                with np.errstate(divide="ignore"):
                    inv = f32(1.0) / ref["dep"][ref["val"] == 1]
                vals, cnt = np.unique(inv[np.isfinite(inv)], return_counts=True)
                lm[k] = float(vals[np.argmax(cnt)])
        _resolved[c["name"]] = (L, R, prm, ref, lm)
    return _resolved[c["name"]]


def run_model(c):
    from oracle import oracle as O
    if c["name"] not in _models:
        L, R, prm, ref, lm = resolve(c)
        m = model(L, R, ref["val"], ref["dep"], dict(lm, baseline=O.KITTI_BASELINE, f0=718.856))
        for a in (m["val"], m["dep"]):
            a.setflags(write=False)
        m["n_selected"], m["n_matched"], m["disp"] = ref["n_selected"], ref["n_matched"], ref["disp"]
        _models[c["name"]] = m
    return _models[c["name"]]


def batch_models():
    """The model of depth_cases.BATCH's pairs under batch_tracker_args() / BATCH_BASELINE (the tracker's depth LM defaults are the
    runner's): [(name, model)]."""
    from oracle import oracle as O
    if "batch" not in _models:
        out = []
        for name in D.BATCH["rows"]:
            L, R = D.pair(D.BY_NAME[name], D.BATCH["size"])
            a = D.batch_tracker_args()
            assert a["baseline"] == D.BATCH_BASELINE
            bp = dict({k: a[k] for k in ("grad_th", "ssd_th", "boundary", "max_disparity", "photo_th", "min_depth", "max_depth")},
                      f0=a["K"][0], baseline=a["baseline"], **{k: LM_DEFAULTS[k] for k in ("lam", "huber_delta", "precision", "max_iters")})
            ref = O.compute_depth(L, R, O.depth_params(any_size=1, **bp), stage=1)
            m = model(L, R, ref["val"], ref["dep"], {k: bp[k] for k in (*LM_DEFAULTS, "baseline", "f0")})
            m["disp"], m["oracle_params"], m["pair"] = ref["disp"], bp, (L, R)
            out.append((name, m))
        _models["batch"] = out
    return _models["batch"]
