"""The tables, the plan mirror and the child process of tests/test_gpu_batch_chain_cases.py (and of its CPU companion,
tests/test_batch_chain_cases_cpu.py): the batched pose-LM kernels — lm_coarse_kernel_batch, lm_coarse_full_kernel_batch,
lm_fine_kernel_batch, lm_fine_trace_kernel_batch, lm_step_kernel_batch — held to each sequence's own single Solve.

A SEQUENCE is (frames, initial pose, lambda0, max_iters per level, robust); a BATCH is a list of sequences issued as ONE
api.solve_batch. The sequences are the rows of state_machine_cases.CASES (every exit of the decision) and the poses of
residual_edge_cases.POSES (every edge of the residual) on their 32 x 40 two-level frames, a table MIXED of sequences whose plans
differ within one launch (other frame sizes: the same textures and inverse-depth checkerboard), and MANY: the exits table cycled
with distinct initial poses, for batches of up to 64 (and, not batchable, 65) sequences.

    python tests/batch_chain_cases.py OUT.npz ROUTE

runs every batch of ROUTE in every build (all recording / all lean / recording on every other sequence) in this process, whose
environment is the route's (ODO_COARSE_MAX and ODO_LM_BATCH_FINE_K are read once per process), next to each sequence's single Solve
on the step launches (ODO_LM_NO_FINE=1 ODO_LM_NO_COARSE=1 while the reference optimisers are created: the in-library reference that
tests/test_gpu_state_machine_branches.py and tests/test_gpu_residual_edges.py hold to the oracle), computed once per sequence, and
writes poses, statuses, evaluation counts, the plan report (odo_lm_last_plan), point counts and trace rows to OUT.npz.

Optimisers are made once per sequence and reused from batch to batch with Reset (pose, lambda), as a tracker reuses its own: tokens,
launch parities and exchange epochs of earlier batched Solves are part of what a batched Solve starts from.
"""
import os
import re
import sys

import numpy as np

import residual_edge_cases as base
import state_machine_cases as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_INT = base.TRACE_INT
PLAN = ("n", "min_level", "fine_lo", "workgroups", "launches", "redone")
BUILDS = ("rec", "lean", "mixed")
STEP_ENV = {"ODO_LM_NO_FINE": "1", "ODO_LM_NO_COARSE": "1"}
KNOBS = ("ODO_HOME_XCD", "ODO_NO_HOME_XCD", "ODO_LM_NO_FINE", "ODO_LM_FINE_K", "ODO_LM_NO_COARSE", "ODO_COARSE_MAX", "ODO_LM_BATCH_FINE_K",
         "ODO_LM_FINE_PASSES", "ODO_LM_FINE_FAULT", "ODO_LM_MODE", "ODO_LM_UNFUSED", "ODO_FUSE_DENSE_MAX", "ODO_NO_POLL")
# route -> the environment of its child process
ROUTES = {
    "b_default": {},
    "b_step": {"ODO_LM_NO_FINE": "1", "ODO_LM_NO_COARSE": "1"},
    "b_coarse": {"ODO_LM_NO_FINE": "1"},
    "b_fine": {"ODO_COARSE_MAX": "0"},
    "b_fine_k2": {"ODO_COARSE_MAX": "0", "ODO_LM_BATCH_FINE_K": "2"},
    "b_fine_k1": {"ODO_COARSE_MAX": "0", "ODO_LM_BATCH_FINE_K": "1"},
    "b_k2": {"ODO_LM_BATCH_FINE_K": "2"},      # (the MIXED tables only: the one route with a coarse, a persistent AND a step level in one sequence)
}
MIXED_ONLY = ("b_k2",)
MANY_ROUTES = ("b_default", "b_fine")
SMALL = (base.ROWS, base.COLS, base.LEVELS)     # 32 x 40, two levels: 768 and 96 points


# ---- the sequences -------------------------------------------------------------------------------------------------------------------
def _seq(name, size=SMALL, valid=None, kind="shifted", T=None, lam=0.01, iters=(6, 6), robust=sm.ROBUST):
    assert len(iters) == size[2]
    return dict(name=name, size=tuple(size), valid=valid, kind=kind, T=np.array(base._translation() if T is None else T, np.float32),
                lam=lam, iters=list(iters), robust=robust)


EXITS = [_seq("x_" + n, kind=c["kind"], T=c["T"], lam=c["lam"], iters=c["iters"]) for n, c in sm.CASES.items()]
EDGES = [_seq("e_" + n, T=T, iters=base.ITERS) for n, T in base.POSES.items()]
# odd sequences L2 weights, even ones Huber (a batched Solve never carries t-distribution weights)
EXITS_W = [dict(s, name="w_" + s["name"][2:], robust=(0 if i % 2 else 1)) for i, s in enumerate(EXITS)]
FAILING = ("no_residual", "all_out", "behind", "nan", "inf")        # status -1; every other sequence of EXITS and EDGES: 0

# Sequences whose plans differ within one launch. All sequences of a batch need the same number of levels, and a third level of the
# 32 x 40 frame (8 x 10) has no interior pixel, so no point list and no fused Solve (test_batch_chain_cases_cpu.py): two tables.
#   24 x 40:    512 and 48 points — the coarse launch takes both levels, the persistent launch carries the sequence's state
#   32 x 40:    768 and 96 — coarse + persistent
#   64 x 88:    4 480 and 864 — no level for the coarse launch beside a persistent launch (more than 512 points): in the batch's coarse
#               launch the sequence only initialises its state, begins its first level and publishes
#   56 x 72, inverse depth in a window only: 384, 96 and 24 points — all coarse with three levels
#   104 x 136:  12 288, 2 640 and 468 points (48, 11 and 2 virtual blocks)
#   88 x 120:   8 960, 1 872 and 308 points (35, 8 and 2 virtual blocks): with two workgroups per sequence the persistent launch
#               takes up to 8 virtual blocks — level 1 fits, level 0 goes to step launches behind it
MIXED2 = [
    _seq("m2_all_coarse", size=(24, 40, 2)),
    _seq("m2_persistent", T=base._translation(0.05, 0.025)),
    _seq("m2_budget_0", iters=(0, 0)),
    _seq("m2_long", T=base._translation(0.1, -0.05)),
    _seq("m2_no_coarse", size=(64, 88, 2)),
    _seq("m2_budget_1", iters=(1, 1)),
]
MIXED3 = [
    _seq("m3_all_coarse", size=(56, 72, 3), valid=(20, 36, 24, 48), iters=(6, 6, 6)),
    _seq("m3_two_pass", size=(104, 136, 3), iters=(6, 6, 6)),
    _seq("m3_budget_0", size=(88, 120, 3), iters=(0, 0, 0)),
    _seq("m3_step_behind", size=(88, 120, 3), iters=(6, 6, 6)),
    _seq("m3_budget_1", size=(104, 136, 3), iters=(1, 1, 1)),
]
EXPECTED_POINTS = {(32, 40, 2, None): [768, 96], (24, 40, 2, None): [512, 48], (64, 88, 2, None): [4480, 864], (56, 72, 3, (20, 36, 24, 48)): [384, 96, 24],
                   (104, 136, 3, None): [12288, 2640, 468], (88, 120, 3, None): [8960, 1872, 308]}

# The exits table cycled, every copy with its own initial pose (equal rows would hide a mix-up between sequences)
N_MAX = 64
MANY_ORDER = (9, 64, 8, 33, 1, 17, 16)      # the context's argument table grows twice (9, 64) and is reused at smaller n


def _many(j):
    s = EXITS[j % len(EXITS)]
    T = s["T"].copy()
    T[2, 3] += np.float32(0.002) * (j // len(EXITS))
    return dict(s, name="n_%02d" % j, T=T)


MANY = [_many(j) for j in range(N_MAX + 1)]
SEQUENCES = {s["name"]: s for s in EXITS + EDGES + EXITS_W + MIXED2 + MIXED3 + MANY}

# batch name -> names of its sequences, in the order issued
BATCHES = {
    "exits": [s["name"] for s in EXITS],
    "edges": [s["name"] for s in EDGES],
    "all": [s["name"] for s in EXITS + EDGES],
    "weights": [s["name"] for s in EXITS_W],
    "mixed2": [s["name"] for s in MIXED2],
    "mixed3": [s["name"] for s in MIXED3],
}
for _b in ("exits", "edges", "all"):
    BATCHES[_b + "_rev"] = BATCHES[_b][::-1]
MANY_BATCHES = {"many_%d" % n: [s["name"] for s in MANY[:n]] for n in MANY_ORDER}
NOT_BATCHED = {"many_65": [s["name"] for s in MANY[:N_MAX + 1]],        # more sequences than a batched Solve takes
               "tdist": [s["name"] for s in EXITS[:3]]}                 # its second optimiser carries t-distribution weights


def batches_of(route):
    """The batches a route's child issues (every one of them in every build)."""
    return {k: v for k, v in BATCHES.items() if route not in MIXED_ONLY or k.startswith("mixed")}


def frame_key(s):
    return s["size"] + (s["valid"], s["kind"])


def intrinsics(s):
    """(f0, cx0, cy0) — residual_edge_cases.K for the 32 x 40 frame, the same rule at the other sizes."""
    rows, cols, _ = s["size"]
    return dict(f0=float(cols), cx0=cols / 2.0, cy0=rows / 2.0)


def frames(s):
    rows, cols, _ = s["size"]
    if s["size"] == SMALL and s["valid"] is None:
        return sm.frames(s["kind"])
    assert s["kind"] == "shifted"
    return base.frames(rows, cols, s["valid"])


def interior_points(s):
    return EXPECTED_POINTS[s["size"] + (s["valid"],)]


# ---- the plan: a mirror of lm_plan_levels and of lm_batch_begin's choice of K ------------------------------------------------------------
def constant(name):
    src = open(os.path.join(ROOT, "odometry_amd", "csrc", "kernels.hip.h")).read()
    m = re.search(r"^constexpr\s+int\s+" + name + r"\s*=\s*(\w+)\s*;", src, re.M)
    v = m.group(1)
    return int(v) if v.isdigit() else int(re.search(r"^#define\s+" + v + r"\s+(\d+)", src, re.M).group(1))


LM_BLOCK, COARSE_BLOCK, COARSE_MAX_POINTS = constant("kLmBlock"), constant("kCoarseBlock"), constant("kCoarseMaxPoints")
FINE_K_MAX, FINE_ROWS_MAX = constant("kFineKMax"), constant("kFineRowsMax")
FINE_PASSES = 2     # odo_lm_create's default (ODO_LM_FINE_PASSES unset)
BATCH_MAX = 64


def list_blocks(npts):
    return min(max((npts + LM_BLOCK - 1) // LM_BLOCK, 1), FINE_ROWS_MAX)


def plan_levels(npts, fine_k, coarse_env=-1, coarse_on=True, stop=0):
    """lm_plan_levels: (min_level, fine_lo) — the coarse launch takes the levels >= min_level, the persistent launch [fine_lo, min_level),
    step launches the rest. npts per level, finest first."""
    n_levels = len(npts)

    def fits(l):
        nblk = list_blocks(npts[l])
        return nblk <= 2 * fine_k * FINE_PASSES and nblk <= FINE_ROWS_MAX and npts[l] <= nblk * LM_BLOCK
    min_level = fine_lo = n_levels
    for p in range(2):
        want_fine = fine_k > 0 and p == 0
        coarse_max = min(coarse_env, COARSE_MAX_POINTS) if coarse_env >= 0 else (COARSE_BLOCK if want_fine else COARSE_MAX_POINTS)
        min_level = n_levels
        while min_level > stop and npts[min_level - 1] <= coarse_max:
            min_level -= 1
        if not coarse_on:
            min_level = n_levels
        fine_lo = min_level
        if not want_fine:
            break
        while fine_lo > stop and fits(fine_lo - 1):
            fine_lo -= 1
        if fine_lo < min_level:
            break
    return min_level, fine_lo


def batch_k(n, env):
    """lm_batch_begin: (workgroups per sequence of the batched persistent launch — 0: none —, sequences per XCD)."""
    per_xcd = (n + 7) // 8
    fine_env = int(env.get("ODO_LM_BATCH_FINE_K", -1))
    k = fine_env if fine_env >= 0 else (FINE_K_MAX if n <= 4 else FINE_K_MAX // 2 if n <= 8 else FINE_K_MAX // 4)
    if k * per_xcd > FINE_K_MAX:
        k = FINE_K_MAX // per_xcd
    if "ODO_LM_NO_FINE" in env:
        k = 0
    return k, per_xcd


def batch_plan(names, route):
    """What odo_lm_last_plan must report for every sequence of a batch: [(n, min_level, fine_lo, workgroups)], and the batch's K."""
    env = ROUTES[route]
    n = len(names)
    k, _ = batch_k(n, env)
    plans = [plan_levels(interior_points(SEQUENCES[s]), k, int(env.get("ODO_COARSE_MAX", -1)), "ODO_LM_NO_COARSE" not in env) for s in names]
    issued = k if any(fl < ml for ml, fl in plans) else 0
    return [(n, ml, fl, issued) for ml, fl in plans], k


def passes(npts, k):
    """Passes per evaluation a level of npts points takes inside a persistent launch of k workgroups (2 k virtual blocks per pass)."""
    return (list_blocks(npts) + 2 * k - 1) // (2 * k)


def kind_of(s, plan):
    """Which launches a sequence's levels with a budget go to, e.g. 'coarse+persistent+step'; '' for a budget of 0 on every level."""
    _, ml, fl, _ = plan
    n_levels = s["size"][2]
    parts = []
    if any(s["iters"][l] > 0 for l in range(ml, n_levels)):
        parts.append("coarse")
    if any(s["iters"][l] > 0 for l in range(fl, ml)):
        parts.append("persistent")
    if any(s["iters"][l] > 0 for l in range(0, fl)):
        parts.append("step")
    return "+".join(parts)


def records(build, i):
    return build == "rec" or (build == "mixed" and i % 2 == 0)


# ---- the child process -----------------------------------------------------------------------------------------------------------------
class _Child:
    def __init__(self, api):
        self.api, self.pyr, self.lms, self.refs, self.res = api, {}, {}, {}, {}
        self.child_env = {k: os.environ[k] for k in KNOBS if k in os.environ}

    def pyramids(self, s):
        key = frame_key(s)
        if key not in self.pyr:
            img0, inv, img1 = frames(s)
            n = s["size"][2]
            self.pyr[key] = (self.api.ImagePyramid(n, img0, True), self.api.DepthPyramid(n, inv, False), self.api.ImagePyramid(n, img1, True))
        return self.pyr[key]

    def _make(self, s, robust=None):
        K = intrinsics(s)
        return self.api.LevenbergMarquardtOptimizer(s["lam"], sm.PRECISION, s["iters"], s["T"], None, s["robust"] if robust is None else robust,
                                                    sm.HUBER, intrinsics=(K["f0"], K["cx0"], K["cy0"]))

    def batch_lm(self, s, robust=None):
        """The sequence's own optimiser (made under the child's environment), back at its initial pose and lambda."""
        key = (s["name"], robust)
        if key not in self.lms:
            self.lms[key] = self._make(s, robust)
        self.lms[key].Reset(s["T"], s["lam"])
        return self.lms[key]

    def ref_lm(self, s):
        """An optimiser on the step launches for the sequence's frame size, budget and weights, at its initial pose and lambda."""
        key = (s["size"], tuple(s["iters"]), s["robust"])
        if key not in self.refs:
            os.environ.update(STEP_ENV)
            self.refs[key] = self._make(s)
            for k in STEP_ENV:
                os.environ.pop(k, None)
            os.environ.update(self.child_env)
        self.refs[key].Reset(s["T"], s["lam"])
        return self.refs[key]

    def _store(self, key, lm, T, with_trace):
        plan = lm.last_plan()
        self.res[key + ".pose"] = np.asarray(T, np.float32)
        self.res[key + ".meta"] = np.array([lm.last_status, lm.launch_stats()[0]] + [plan[f] for f in PLAN], np.int64)
        if with_trace:
            rows = lm.trace()
            self.res[key + ".trace_i"] = np.array([[r[f] for f in TRACE_INT] for r in rows], np.int64).reshape(-1, len(TRACE_INT))
            self.res[key + ".trace_f"] = np.array([[r["err"], r["lambda_after"], *r["delta"]] for r in rows], np.float32).reshape(-1, 8)

    def single(self, s, second):
        """The sequence's single Solve on the step launches (recording), once; second: also the Solve after Reset(its result, 0.01)."""
        key = "single." + s["name"]
        if key + ".pose" not in self.res:
            lm = self.ref_lm(s)
            lm.set_record(True)
            T = lm.Solve(*self.pyramids(s))
            self._store(key, lm, T, True)
            self.res[key + ".points"] = np.array(lm.points()[0], np.int64)
        if second and key + ".second.pose" not in self.res:
            lm = self.ref_lm(s)
            lm.set_record(True)
            T = lm.Solve(*self.pyramids(s))
            lm.Reset(T, 0.01)
            T2 = lm.Solve(*self.pyramids(s))
            self._store(key + ".second", lm, T2, True)

    def batch(self, name, names, build, second=False, robust_of=None):
        seqs = [SEQUENCES[n] for n in names]
        for s in seqs:
            self.single(s, second)
        lms = [self.batch_lm(s, None if robust_of is None else robust_of(i, s)) for i, s in enumerate(seqs)]
        for i, lm in enumerate(lms):
            lm.set_record(records(build, i))
        pyr = [self.pyramids(s) for s in seqs]
        poses, _ = self.api.solve_batch(lms, [p[0] for p in pyr], [p[1] for p in pyr], [p[2] for p in pyr])
        for i, lm in enumerate(lms):
            self._store(f"{name}.{build}.{i}", lm, poses[i], records(build, i))
            self.res[f"{name}.{build}.{i}.points"] = np.array(lm.points()[0], np.int64)
        if second:
            for i, lm in enumerate(lms):
                lm.Reset(poses[i], 0.01)
            poses2, _ = self.api.solve_batch(lms, [p[0] for p in pyr], [p[1] for p in pyr], [p[2] for p in pyr])
            for i, lm in enumerate(lms):
                self._store(f"{name}.{build}.{i}.second", lm, poses2[i], records(build, i))

    def close(self):
        for lm in list(self.lms.values()) + list(self.refs.values()):
            lm.close()
        for objs in self.pyr.values():
            for o in objs:
                o.close()


def main(out, route):
    sys.path.insert(0, ROOT)
    from odometry_amd import api
    api.default_context()
    child = _Child(api)
    if route in MANY_ROUTES:
        # first, in a context that has not issued a batched Solve yet: its argument table is allocated for 9 entries, grows to 64 (a
        # sync and a reallocation between two batched Solves) and is reused at every smaller n
        for build in ("mixed", "lean"):
            for name, names in MANY_BATCHES.items():
                child.batch(name, names, build, second=True)
        child.batch("many_65", NOT_BATCHED["many_65"], "mixed", second=True)
        child.batch("tdist", NOT_BATCHED["tdist"], "mixed", robust_of=lambda i, s: 2 if i == 1 else None)
        # ... whose second sequence's single Solve carries the same weights (the persistent and coarse launches' t-distribution builds
        # sum the scale in another order than the step launches' pipeline: the reference here is the optimiser's own kind of Solve)
        s = SEQUENCES[NOT_BATCHED["tdist"][1]]
        lm = child._make(s, 2)
        lm.set_record(True)
        child._store("single_tdist", lm, lm.Solve(*child.pyramids(s)), True)
        lm.close()
    for build in BUILDS:
        for name, names in batches_of(route).items():
            child.batch(name, names, build)
    child.close()
    np.savez(out, **child.res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
