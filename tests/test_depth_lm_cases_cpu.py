"""The exact-sum model of the inverse-depth LM (tests/depth_lm_cases.py) shown sound with the oracle alone: on every case the error
sum of EVERY evaluation is known to the last bit whatever the order it is added in, the model equals oracle.compute_depth(stage=2) bit
for bit — mask, inverse depths, iteration count, cost, valid count, status — and the model's own run reaches the branches the case is
in the list for. tests/test_gpu_depth_lm_cases.py holds the kernels to the same model."""
import os
import re
import struct

import numpy as np
import pytest

import depth_cases as D
import depth_lm_cases as M

f32 = np.float32
NAMES = [c["name"] for c in M.CASES]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_the_case_list_is_the_table_plus_the_variants(O):
    assert [c["name"] for c in M.CASES[:len(D.TABLE)]] == [r["name"] for r in D.TABLE]
    assert all(not c["lm"] for c in M.CASES[:len(D.TABLE)]) and all(c["lm"] for c in M.VARIANTS)
    assert M.CASES[len(D.TABLE):] == M.VARIANTS and len(M.VARIANTS) == 9
    # the one row that may be left out of the decidability claim, and only with a reason; never a variant
    assert set(M.NOT_DECIDABLE) <= {"radix-pass"} and all(M.NOT_DECIDABLE.values())
    src = open(os.path.join(D.ROOT, "odometry_amd", "csrc", "kernels.hip.h")).read()
    assert int(re.search(r"^constexpr\s+int\s+kDpMaxIters\s*=\s*(\d+)\s*;", src, re.M).group(1)) == M.PERSIST_MAX_ITERS
    iters = sorted(c["lm"]["max_iters"] for c in M.VARIANTS if "max_iters" in c["lm"])
    assert iters == [0, 0, 0, 1, M.PERSIST_MAX_ITERS, M.PERSIST_MAX_ITERS + 1]
    p = O.depth_params()   # the runner's defaults, as the oracle holds them
    assert {k: f32(getattr(p, k)) for k in M.LM_DEFAULTS} == {k: f32(v) for k, v in M.LM_DEFAULTS.items()}
    assert (f32(p.baseline), f32(p.f0)) == (f32(O.KITTI_BASELINE), f32(718.856))


def test_the_two_arguments_tell_a_decided_sum_from_an_undecided_one():
    one = float(f32(1.0))
    mid = one + 2.0 ** -24                     # half way between 1 and the next float32
    assert M.one_float(one, 40960) and not M.one_float(mid, 1) and not M.one_float(mid * (1 - 2.0 ** -40), 40960)
    assert M.one_float(mid * (1 - 2.0 ** -30), 40960)          # 40960 2^-52 = 2^-36.7: well inside one float32
    assert M.one_float(0.0, 0) and M.one_float(float("inf"), 3)
    # multiples of 2^-20 that sum below 2^33: exact in every order, and shown so by adding them in a few orders
    rng = np.random.default_rng(0)
    t = (rng.integers(0, 1 << 24, 40960).astype(np.float64) * 2.0 ** -20)
    S = float(t.sum())
    assert M.every_order_exact(t, S)
    for _ in range(4):
        acc = 0.0
        for v in rng.permutation(t).tolist():
            acc += v
        assert acc == S
    assert not M.every_order_exact(np.array([2.0 ** 60, 2.0 ** -20]), 2.0 ** 60)


@pytest.mark.parametrize("name", NAMES)
def test_case_is_decidable_equals_the_oracle_and_reaches_its_branches(O, name):
    c = M.BY_NAME[name]
    L, R, prm, ref, lm = M.resolve(c)
    m = M.run_model(c)
    modes = "".join(str(e["mode"]) for e in m["evals"])
    print(f"{name} {L.shape[0]}x{L.shape[1]} {c['lm'] and lm}: {len(m['evals'])} evaluations, modes {modes}, iters {m['iters']}, cost "
          f"{float(m['cost'])!r} ({m['cost_bits']:08x}), {m['n_valid']} valid of {m['counts']['points']} points, status {m['status']}; decided by the "
          f"interval {sum(e['how'] == 'interval' for e in m['evals'])}, by exactness {sum(e['how'] == 'exact' for e in m['evals'])}, undecided "
          f"{[i for i, e in enumerate(m['evals']) if not e['decidable']]}")
    print("    counts: " + ", ".join(f"{k} {v}" for k, v in m["counts"].items() if v))
    # ---- every evaluation's sum is one float whatever the order ----
    if name not in M.NOT_DECIDABLE:
        assert all(e["decidable"] for e in m["evals"]), [(i, e["S"], e["n"]) for i, e in enumerate(m["evals"]) if not e["decidable"]]
    # ---- the model is the pinned oracle, bit for bit ----
    o = O.compute_depth(L, R, O.depth_params(**dict(prm, **lm)), stage=2)
    cost_bits = struct.unpack("I", struct.pack("f", o["cost"]))[0]
    print(f"    against the oracle: mask differs at {int((m['val'] != o['val']).sum())} pixels, inverse depth at "
          f"{int((m['dep'].view(np.uint32) != o['dep'].view(np.uint32)).sum())}; iters {o['iters']}, cost bits {cost_bits:08x}, valid {o['n_valid']}, "
          f"status {o['status']}")
    assert np.array_equal(m["val"], o["val"])
    assert np.array_equal(m["dep"].view(np.uint32), o["dep"].view(np.uint32))
    assert np.array_equal(m["disp"], o["disp"])       # stage 2 leaves the disparities as the scan wrote them
    assert (m["iters"], m["cost_bits"], m["n_valid"], m["status"]) == (o["iters"], cost_bits, o["n_valid"], o["status"])
    assert (m["n_selected"], m["n_matched"]) == (o["n_selected"], o["n_matched"])
    # ---- the branches the case is here for ----
    cnt = m["counts"]
    assert cnt["points"] > 0 and (cnt["evaluations"] > 0) == (lm["max_iters"] > 0)
    assert cnt["evaluations"] == len(m["evals"]) == sum(cnt[f"mode{k}"] for k in range(4))
    for k, (floor, measured) in c["floors"].items():
        if k in M.EXACT:
            assert cnt[k] == floor, f"{name}: {k} = {cnt[k]}, must be {floor}"
        else:
            assert cnt[k] >= floor, f"{name}: {k} = {cnt[k]} < floor {floor} (written down: {measured})"


def test_the_cases_reach_every_branch_between_them():
    tot = {k: sum(M.run_model(c)["counts"][k] for c in M.CASES) for k in M.COUNTS}
    n_exact = sum(e["how"] == "exact" for c in M.CASES for e in M.run_model(c)["evals"])
    print(f"{len(M.CASES)} cases, {tot['evaluations']} evaluations, {n_exact} of them decided by exactness alone; totals: {tot}")
    for k in M.COUNTS:   # every counter of the list: modes 0 .. 3, a rejected first evaluation, iters == max_iters, fn == 0, ...
        assert tot[k] > 0, k
    held = {k for c in M.CASES for k, (floor, _) in c["floors"].items() if floor > 0}
    assert held >= set(M.COUNTS) - {"res_over_photo"}, set(M.COUNTS) - held    # ... and each is some case's floor
    sizes = {M.run_model(c)["counts"]["points"] for c in M.CASES}
    assert max(sizes) == 512 * D.CAP and min(sizes) < 8000                     # a full slot table and a sparse one
    firsts = [M.run_model(c)["evals"][0]["mode"] for c in M.CASES if M.run_model(c)["evals"]]
    assert 0 in firsts and 2 in firsts and 1 in firsts                         # a first evaluation rejected, with and without the break
    nan_cost = [c["name"] for c in M.CASES if np.isnan(M.run_model(c)["cost"])]
    assert nan_cost == ["all-tie-md0", "all-tie-md128"]


def test_the_batched_pairs_are_decidable_and_equal_the_oracle(O):
    for name, m in M.batch_models():
        L, R = m["pair"]
        o = O.compute_depth(L, R, O.depth_params(any_size=1, **m["oracle_params"]), stage=2)
        print(f"{name} at {L.shape}: {len(m['evals'])} evaluations, modes {''.join(str(e['mode']) for e in m['evals'])}, {m['n_valid']} valid")
        assert all(e["decidable"] for e in m["evals"])
        assert np.array_equal(m["val"], o["val"]) and np.array_equal(m["dep"].view(np.uint32), o["dep"].view(np.uint32))
        assert (m["iters"], m["n_valid"], m["status"]) == (o["iters"], o["n_valid"], 0)
