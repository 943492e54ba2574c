"""The batched pose-LM kernels — lm_coarse_kernel_batch / lm_coarse_full_kernel_batch, lm_fine_kernel_batch / lm_fine_trace_kernel_batch,
lm_step_kernel_batch — on the exits table of tests/state_machine_cases.py and the edges table of tests/residual_edge_cases.py, with each
row ONE SEQUENCE of a batched Solve (tests/batch_chain_cases.py): sequences that stop on lambda next to sequences without any residual
and sequences with a budget of 0, in every order, recording, lean and mixed, Huber next to L2 weights, on seven routes through the
kernels; sequences of other frame sizes whose plans differ within one launch (MIXED); batches of 1 to 64 sequences that grow and reuse
the context's argument table; and calls that cannot be batched (65 sequences, t-distribution weights).

Asserted for every sequence of every batch, build and route: pose, status, evaluation count and every recorded row equal the
sequence's own single Solve on the step launches bit for bit (the in-library reference tests/test_gpu_state_machine_branches.py and
tests/test_gpu_residual_edges.py hold to the oracle) — a sequence's bits depend neither on its place nor on its neighbours; the
recorded rows of the default route against the oracle at test_gpu_state_machine_branches.py's bounds; every exits row takes the exit it
is named for; and, from odo_lm_last_plan, that the call was batched with the n issued, that every sequence's levels went where the
Python mirror of lm_plan_levels and lm_batch_begin (checked without a GPU in tests/test_batch_chain_cases_cpu.py) says, and that no
persistent launch gave up."""
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_chain_cases as bc
import state_machine_cases as sm
from test_gpu_state_machine_branches import assert_rows_are_the_oracles, oracle_reference

pytestmark = pytest.mark.gpu

ROOT = bc.ROOT
STATUS, EVALS, PLAN0 = 0, 1, 2      # columns of a stored `meta` row: status, evaluations, the six words of odo_lm_last_plan


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every Solve of this module: one child process per route, one after the other (a persistent launch needs its CUs to itself)."""
    tmp = tmp_path_factory.mktemp("batch_chain")
    out = {}
    for route, env in bc.ROUTES.items():
        path = os.path.join(str(tmp), route + ".npz")
        e = {k: v for k, v in os.environ.items() if k not in bc.KNOBS}
        e.update(env)
        subprocess.run([sys.executable, os.path.join(ROOT, "tests", "batch_chain_cases.py"), path, route], check=True, env=e, timeout=300)
        out[route] = dict(np.load(path))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _plan(meta):
    return dict(zip(bc.PLAN, (int(v) for v in meta[PLAN0:PLAN0 + 6])))


def _same_solve(r, key, ref, recorded):
    """r[key ...] (one sequence of a batched Solve) is r[ref ...] (its single Solve): pose bits, status, evaluations, trace rows."""
    assert np.array_equal(_bits(r[key + ".pose"]), _bits(r[ref + ".pose"])), key
    assert int(r[key + ".meta"][STATUS]) == int(r[ref + ".meta"][STATUS]), key
    assert int(r[key + ".meta"][EVALS]) == int(r[ref + ".meta"][EVALS]), key
    if recorded:
        ti, tf = r[key + ".trace_i"], r[key + ".trace_f"]
        assert ti.shape == r[ref + ".trace_i"].shape and np.array_equal(ti, r[ref + ".trace_i"]), key
        assert np.array_equal(_bits(tf), _bits(r[ref + ".trace_f"])), key


_ROUTE_BATCH = [(route, batch) for route in bc.ROUTES for batch in bc.batches_of(route)]


@pytest.mark.parametrize("route,batch", _ROUTE_BATCH)
def test_the_batch_ran_batched_on_the_route_meant(runs, route, batch):
    r, names = runs[route], bc.BATCHES[batch]
    want, k = bc.batch_plan(names, route)
    for build in bc.BUILDS:
        for i, name in enumerate(names):
            key = f"{batch}.{build}.{i}"
            plan = _plan(r[key + ".meta"])
            print(route, key, name, plan, bc.kind_of(bc.SEQUENCES[name], want[i]))
            assert (plan["n"], plan["min_level"], plan["fine_lo"], plan["workgroups"]) == want[i], key
            assert plan["redone"] == 0, f"{key}: the persistent launch of n = {len(names)}, K = {k}, grid {8 * k * ((len(names) + 7) // 8)} gave up"
            assert plan["launches"] >= (1 if any(bc.kind_of(bc.SEQUENCES[n], w) for n, w in zip(names, want)) else 0), key
            assert list(r[key + ".points"]) == bc.interior_points(bc.SEQUENCES[name]) == list(r[f"single.{name}.points"]), key
    # the single Solves are Solves of their own, on the step launches
    for name in names:
        plan = _plan(r[f"single.{name}.meta"])
        n_levels = bc.SEQUENCES[name]["size"][2]
        assert (plan["n"], plan["min_level"], plan["fine_lo"], plan["workgroups"], plan["redone"]) == (0, n_levels, n_levels, 0, 0), name


@pytest.mark.parametrize("route,batch", _ROUTE_BATCH)
def test_every_sequence_equals_its_single_solve(runs, route, batch):
    r, names = runs[route], bc.BATCHES[batch]
    for build in bc.BUILDS:
        for i, name in enumerate(names):
            _same_solve(r, f"{batch}.{build}.{i}", "single." + name, bc.records(build, i))
    # the statuses are a mix, and a failing sequence's neighbours are none the worse for it (their bits: above)
    if batch in ("exits", "edges", "all", "exits_rev", "edges_rev", "all_rev"):
        for build in bc.BUILDS:
            for i, name in enumerate(names):
                assert int(r[f"{batch}.{build}.{i}.meta"][STATUS]) == (-1 if name[2:] in bc.FAILING else 0), (build, name)
    if batch.startswith("mixed"):
        evals = {name: int(r[f"single.{name}.meta"][EVALS]) for name in names}
        budget_0, budget_1 = [n for n in names if n.endswith("budget_0")][0], [n for n in names if n.endswith("budget_1")][0]
        assert evals[budget_0] == 0 and evals[budget_1] == bc.SEQUENCES[budget_1]["size"][2] and max(evals.values()) >= 4 * evals[budget_1]
        # a budget of 0 on every level: no evaluation, status 0 (and the pose of its single Solve: above)
        assert int(r[f"single.{budget_0}.meta"][STATUS]) == 0 and len(r[f"single.{budget_0}.trace_i"]) == 0


@pytest.mark.parametrize("route", [rt for rt in bc.ROUTES if rt not in bc.MIXED_ONLY])
def test_each_exits_row_takes_its_exit_inside_a_batch(runs, route):
    r = runs[route]
    for batch in ("exits", "exits_rev", "all", "all_rev"):
        at = {name[2:]: i for i, name in enumerate(bc.BATCHES[batch]) if name.startswith("x_")}
        assert set(at) == set(sm.CASES)
        sm.check_exits({c: r[f"{batch}.rec.{i}.trace_i"] for c, i in at.items()}, {c: r[f"{batch}.rec.{i}.trace_f"] for c, i in at.items()})


@pytest.mark.parametrize("batch", ["exits", "edges", "all", "all_rev", "weights"])
def test_the_recorded_rows_of_the_default_route_are_the_oracles(runs, O, batch):
    r, pyr = runs["b_default"], {}
    for i, name in enumerate(bc.BATCHES[batch]):
        s = bc.SEQUENCES[name]
        solve, conds = oracle_reference(O, pyr, s, robust=s["robust"])
        for build in ("rec", "mixed"):
            if not bc.records(build, i):
                continue
            key = f"{batch}.{build}.{i}"
            ti, tf = r[key + ".trace_i"], r[key + ".trace_f"]
            assert int(r[key + ".meta"][STATUS]) == solve["status"], key
            if name[2:] in bc.FAILING:
                # the reference fails in its first evaluation (N == 0) and records nothing; what the device recorded of it holds N == 0
                assert solve["n_evals"] == 0 and len(ti) <= 1 and (ti[:, 2] == 0).all(), key
                continue
            assert int(r[key + ".meta"][EVALS]) == solve["n_evals"] == len(ti), key
            assert_rows_are_the_oracles(key, ti, tf, solve, conds)


@pytest.mark.parametrize("route", bc.MANY_ROUTES)
@pytest.mark.parametrize("n", sorted(bc.MANY_ORDER))
def test_one_to_sixty_four_sequences(runs, route, n):
    """More than eight sequences share XCDs with fewer workgroups each; the batches are issued in the order 9, 64, 8, 33, 1, 17, 16 in
    a fresh context, so its argument table is allocated, grows once more and is reused at every smaller n. After each batched Solve the
    optimisers are Reset to their results and solved again, as a tracker does."""
    r, batch = runs[route], "many_%d" % n
    names = bc.MANY_BATCHES[batch]
    want, k = bc.batch_plan(names, route)
    assert len(names) == n
    for build in ("mixed", "lean"):
        for i, name in enumerate(names):
            for which in ("", ".second"):
                key = f"{batch}.{build}.{i}{which}"
                plan = _plan(r[key + ".meta"])
                assert (plan["n"], plan["min_level"], plan["fine_lo"], plan["workgroups"]) == want[i], key
                assert plan["redone"] == 0, f"{key}: the persistent launch of n = {n}, K = {k}, grid {8 * k * ((n + 7) // 8)} gave up"
                _same_solve(r, key, f"single.{name}{which}", bc.records(build, i))
    print(route, batch, "K", k, "launches", _plan(r[f"{batch}.lean.0.meta"])["launches"])


@pytest.mark.parametrize("route", bc.MANY_ROUTES)
def test_a_call_that_cannot_be_batched_says_so_and_gives_the_single_results(runs, route):
    r = runs[route]
    names = bc.NOT_BATCHED["many_65"]
    for i, name in enumerate(names):
        for which in ("", ".second"):
            key = f"many_65.mixed.{i}{which}"
            assert _plan(r[key + ".meta"])["n"] == 0 and _plan(r[key + ".meta"])["redone"] == 0, key
            _same_solve(r, key, f"single.{name}{which}", bc.records("mixed", i))
    # one optimiser with t-distribution weights: every sequence is solved on its own, the one with those weights as its own Solve does
    for i, name in enumerate(bc.NOT_BATCHED["tdist"]):
        key = f"tdist.mixed.{i}"
        assert _plan(r[key + ".meta"])["n"] == 0, key
        _same_solve(r, key, "single_tdist" if i == 1 else "single." + name, bc.records("mixed", i))
    assert not np.array_equal(_bits(r["single_tdist.pose"]), _bits(r["single." + bc.NOT_BATCHED["tdist"][1] + ".pose"]))
