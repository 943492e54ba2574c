"""The tables of tests/batch_chain_cases.py do what tests/test_gpu_batch_chain_cases.py has them for — shown without a GPU, with the
oracle and integers only: the exits batch is a mix of long and short Solves and of both statuses; the Python mirror of lm_plan_levels
and of lm_batch_begin's choice of K gives, for every batch and route, the plan the GPU tests then demand from odo_lm_last_plan; every
kind of sequence the table MIXED is there for occurs under the route it is meant for; and the point counts the mirror plans with are
the oracle's."""
import re
import os

import numpy as np
import pytest

import batch_chain_cases as bc
import state_machine_cases as sm
from test_gpu_state_machine_branches import oracle_reference


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _plans(batch, route):
    names = {**bc.BATCHES, **bc.MANY_BATCHES}[batch]
    plans, k = bc.batch_plan(names, route)
    return {n: p for n, p in zip(names, plans)}, k


def test_the_constants_are_the_headers():
    src = open(os.path.join(bc.ROOT, "odometry_amd", "csrc", "odometry_hip.hip")).read()
    assert (bc.LM_BLOCK, bc.COARSE_BLOCK, bc.COARSE_MAX_POINTS, bc.FINE_K_MAX, bc.FINE_ROWS_MAX) == (256, 512, 1024, 32, 160)
    # the host's cap of a list level's blocks is the persistent launch's row count, the batch bound and the default passes are the mirror's
    assert int(re.search(r"constexpr int kLmListMaxBlocks = (\d+);", src).group(1)) == bc.FINE_ROWS_MAX
    assert re.search(r"bool batchable = n <= (\d+);", src).group(1) == str(bc.BATCH_MAX) == str(bc.N_MAX)
    assert int(re.search(r'getenv\("ODO_LM_FINE_PASSES"\) \? atoi\(getenv\("ODO_LM_FINE_PASSES"\)\) : (\d+);', src).group(1)) == bc.FINE_PASSES
    assert set(bc.MANY_ORDER) == {1, 8, 9, 16, 17, 33, 64} and bc.MANY_ORDER[:2] == (9, 64)


def test_the_exits_batch_is_a_mix_of_lengths_and_statuses(O):
    pyr = {}
    evals, status = {}, {}
    for name, c in sm.CASES.items():
        solve, _ = oracle_reference(O, pyr, c)
        evals[name], status[name] = solve["n_evals"], solve["status"]
    print(evals, status)
    ran = [v for k, v in evals.items() if status[k] == 0]
    assert len(set(ran)) > 2 and max(ran) >= 2 * min(ran) and min(ran) >= 1
    for name in sm.CASES:
        assert status[name] == (-1 if name in bc.FAILING else 0), name
    assert sum(1 for n in sm.CASES if n in bc.FAILING) == 1


def test_the_edges_batch_has_the_failing_statuses(O):
    from test_gpu_residual_edges import cases as edge
    flat = lambda levels: np.concatenate([l.ravel() for l in levels])
    img0, inv, img1 = edge.frames()
    r0, r1, rd = O.image_pyramid(img0, edge.LEVELS, True), O.image_pyramid(img1, edge.LEVELS, True), O.depth_pyramid(inv, edge.LEVELS)
    params = O.lm_params(max_iters=tuple(edge.ITERS), robust=edge.ROBUST, huber_delta=edge.HUBER, K=edge.K)
    for name, T in edge.POSES.items():
        st = O.lm_solve(flat(r0), flat(rd), flat(r1), edge.ROWS, edge.COLS, params, init=T)["status"]
        assert (st != 0) == (name in bc.FAILING), name
    assert [s["name"] for s in bc.EDGES] == ["e_" + n for n in edge.POSES] and len(bc.EDGES) == 9 and len(bc.EXITS) == 12


def test_the_point_counts_are_the_oracles(O):
    """Interior pixels (four from each border) with an inverse depth, per level: the oracle's N of an evaluation at the identity
    against the keyframe's own image, where every keyframe point lands on itself."""
    seen = set()
    for s in bc.SEQUENCES.values():
        key = s["size"] + (s["valid"],)
        if key in seen:
            continue
        seen.add(key)
        rows, cols, levels = s["size"]
        img0, inv, _ = bc.frames(dict(s, kind="shifted"))
        ip, dp = O.image_pyramid(img0, levels, True), O.depth_pyramid(inv, levels)
        got = [int(O.lm_accumulate(ip[l], ip[l], dp[l], l, np.eye(4), K=bc.intrinsics(s))["acc"][28]) for l in range(levels)]
        assert got == bc.interior_points(s), key
        if s["valid"] is None:
            assert got == [((rows >> l) - 8) * ((cols >> l) - 8) for l in range(levels)], key
    assert seen == set(bc.EXPECTED_POINTS)
    assert bc.intrinsics(bc.EXITS[0]) == sm.K


def test_a_third_level_of_the_small_frame_has_no_point(O):
    """... so it would be a dense level on top of the pyramid, which no fused (and no batched) Solve starts with: MIXED is two tables."""
    img0, inv, _ = sm.frames("shifted")
    ip, dp = O.image_pyramid(img0, 3, True), O.depth_pyramid(inv, 3)
    assert ip[2].shape == (8, 10)
    assert int(O.lm_accumulate(ip[2], ip[2], dp[2], 2, np.eye(4), K=sm.K)["acc"][28]) == 0
    for table, levels in ((bc.MIXED2, 2), (bc.MIXED3, 3)):
        assert {s["size"][2] for s in table} == {levels}
        assert [s["name"][3:] for s in table][0] == "all_coarse" and table[-1]["name"].endswith("budget_1")
        assert any(s["name"].endswith("budget_0") and not any(s["iters"]) for s in table)
        assert max(sum(s["iters"]) for s in table) >= 6 * sum(table[-1]["iters"])       # a much smaller budget than its neighbours'
        assert len(table) >= 5      # five to eight sequences: 16 workgroups each by default
        assert max(s["size"][0] for s in table) <= 104 and max(s["size"][1] for s in table) <= 136


@pytest.mark.parametrize("route", list(bc.ROUTES))
def test_the_small_frame_goes_where_the_route_says(route):
    for batch in ("exits", "edges", "all", "weights", "exits_rev"):
        plans, k = _plans(batch, route)
        n = len(plans)
        want = {"b_default": (1, 0), "b_step": (2, 2), "b_coarse": (0, 0), "b_fine": (2, 0), "b_fine_k2": (2, 0), "b_fine_k1": (2, 0),
                "b_k2": (1, 0)}[route]
        want_k = {"b_default": 8, "b_step": 0, "b_coarse": 0, "b_fine": 8, "b_fine_k2": 2, "b_fine_k1": 1, "b_k2": 2}[route]
        if n == 9 and route in ("b_default", "b_fine"):
            assert bc.batch_k(n, bc.ROUTES[route]) == (8, 2)
        assert k == want_k, (batch, route)
        for name, p in plans.items():
            assert p == (n, want[0], want[1], want_k if want[1] < want[0] else 0), (batch, route, name)
    # two sequences share an XCD in every batch of the exits, and three in the batch of all 21
    assert bc.batch_k(12, {})[1] == 2 and bc.batch_k(21, {})[1] == 3
    # one workgroup holds two virtual blocks per pass: the 768-point level (three) takes two passes inside b_fine_k1's launch
    if route == "b_fine_k1":
        assert bc.passes(768, 1) == 2 and bc.passes(96, 1) == 1
    if route == "b_fine_k2":
        assert bc.passes(768, 2) == 1


def test_the_number_of_workgroups_follows_n():
    assert [bc.batch_k(n, {}) for n in (1, 4, 5, 8, 9, 16, 17, 33, 64)] == \
        [(32, 1), (32, 1), (16, 1), (16, 1), (8, 2), (8, 2), (8, 3), (6, 5), (4, 8)]
    assert bc.batch_k(64, bc.ROUTES["b_fine"]) == (4, 8) and bc.batch_k(9, {})[1] == 2
    assert bc.batch_k(64, {"ODO_LM_BATCH_FINE_K": "32"}) == (4, 8) and bc.batch_k(8, bc.ROUTES["b_fine_k2"]) == (2, 1)
    for n in bc.MANY_ORDER:
        for route in bc.MANY_ROUTES:
            plans, k = _plans("many_%d" % n, route)
            assert len(plans) == n and k * ((n + 7) // 8) <= bc.FINE_K_MAX
            # every sequence of it is in the persistent launch
            assert all(p == (n, 1 if route == "b_default" else 2, 0, k) for p in plans.values()), (n, route)
    assert len(bc.NOT_BATCHED["many_65"]) == bc.BATCH_MAX + 1
    # distinct initial poses
    poses = {bc.SEQUENCES[s]["T"].tobytes() + bytes(str((bc.SEQUENCES[s]["kind"], bc.SEQUENCES[s]["lam"], bc.SEQUENCES[s]["iters"])), "ascii")
             for s in bc.NOT_BATCHED["many_65"]}
    assert len(poses) == bc.BATCH_MAX + 1


def test_every_kind_of_mixed_occurs_under_its_route():
    kinds = {}
    for batch in ("mixed2", "mixed3"):
        for route in bc.ROUTES:
            plans, k = _plans(batch, route)
            for name, p in plans.items():
                kinds[(route, name)] = (bc.kind_of(bc.SEQUENCES[name], p), p, k)
                print(route, name, kinds[(route, name)])
    # five sequences: 16 workgroups each, a level of up to 64 virtual blocks in two passes
    assert kinds[("b_default", "m2_all_coarse")] == ("coarse", (6, 0, 0, 16), 16)          # fine_lo >= min_level: its state is carried
    assert kinds[("b_default", "m2_persistent")] == ("coarse+persistent", (6, 1, 0, 16), 16)
    # no level for the batch's coarse launch (min_level == the number of levels): there it only initialises and publishes
    assert kinds[("b_default", "m2_no_coarse")] == ("persistent", (6, 2, 0, 16), 16)
    assert kinds[("b_k2", "m2_no_coarse")] == ("persistent+step", (6, 2, 1, 2), 2) and kinds[("b_coarse", "m2_no_coarse")][0] == "coarse+step"
    assert kinds[("b_default", "m2_budget_0")][0] == "" and kinds[("b_default", "m2_budget_1")][0] == "coarse+persistent"
    assert kinds[("b_default", "m3_all_coarse")] == ("coarse", (5, 0, 0, 16), 16)
    assert kinds[("b_default", "m3_two_pass")] == ("coarse+persistent", (5, 2, 0, 16), 16)
    assert bc.passes(12288, 16) == 2 and bc.passes(2640, 16) == 1 and bc.list_blocks(12288) == 48 and bc.list_blocks(2640) == 11
    assert kinds[("b_default", "m3_step_behind")][0] == "coarse+persistent" and bc.passes(8960, 16) == 2
    assert kinds[("b_default", "m3_budget_0")][0] == ""
    # two workgroups per sequence hold up to 8 virtual blocks: the 11 of 104 x 136's level 1 do not fit, so levels 1 and 0 go to step
    # launches behind the persistent launch; 88 x 120's level 1 (8 blocks) fits and only its level 0 does
    assert kinds[("b_fine_k2", "m3_two_pass")] == ("persistent+step", (5, 3, 2, 2), 2)
    assert kinds[("b_fine_k2", "m3_step_behind")] == ("persistent+step", (5, 3, 1, 2), 2) and bc.list_blocks(1872) == 8
    assert kinds[("b_fine_k2", "m3_all_coarse")] == ("persistent", (5, 3, 0, 2), 2)
    assert kinds[("b_fine_k1", "m3_step_behind")] == ("persistent+step", (5, 3, 2, 1), 1)
    # all three kinds of launch for one sequence: the coarse launch's level, the persistent launch's, a step launch's
    assert kinds[("b_coarse", "m3_two_pass")] == ("coarse+step", (5, 2, 2, 0), 0)
    assert kinds[("b_step", "m3_two_pass")] == ("step", (5, 3, 3, 0), 0)
    assert kinds[("b_k2", "m3_step_behind")] == ("coarse+persistent+step", (5, 2, 1, 2), 2)
    assert kinds[("b_k2", "m3_two_pass")] == ("coarse+step", (5, 2, 2, 2), 2) and kinds[("b_k2", "m2_persistent")][0] == "coarse+persistent"
    assert set(bc.batches_of("b_k2")) == {"mixed2", "mixed3"} and set(bc.batches_of("b_default")) == set(bc.BATCHES)
    # the step grid of a batch is its largest sequence's: the small ones' surplus blocks have nothing to do
    for route in ("b_step", "b_coarse", "b_fine_k2"):
        stepping = [bc.list_blocks(bc.interior_points(bc.SEQUENCES[n])[0]) for n in bc.BATCHES["mixed3"] if "step" in kinds[(route, n)][0]]
        assert len(set(stepping)) > 1 or route == "b_coarse", route
