"""The moving volume's three stores used together, without a GPU (DESIGN.md sections 9.9, 9.13, 9.14): the composed model of
tests/volume_stores_cases.py with one store equals that store's own model bit for bit, every row's predicate holds, every switch of
the composition changes exactly the rows placed for it, and every row is small enough for the GPU side to run in seconds."""
import itertools

import numpy as np
import pytest

import volume_reentry_cases as R
import volume_spill_mesh_cases as M
import volume_stores_cases as V
from test_volume_shift_cpu import offset_model, shift_model, spill_model, window

NAMES = [r["name"] for r in V.rows()]


def _alone(r, store, off):
    """The row's walk with `store` alone, its capacity and colour flag as the row has them."""
    p, q, w, col = V.grid(r["grid"])
    caps = {s: r["capacities"][s] if s == store else None for s in V.STORES}
    return (p, q, w, col), caps, V.stores_walk_model(p, q, w, col, r["shifts"], caps, r["colour_flags"], off=off)


@pytest.mark.parametrize("off", [(0, 0, 0), (1, 0, 0)])
@pytest.mark.parametrize("name", NAMES)
def test_one_store_of_the_composed_model_is_that_stores_own_model(name, off):
    """Points: spill_model shift by shift on shift_model's grids with the clamp; mesh: run_shifts; re-entry: walk_model. Also in the
    window (1, 0, 0), where the GPU tests' volumes start."""
    r = V.row(name)
    for store in r["stores"]:
        (p, q, w, col), caps, st = _alone(r, store, off)
        flag = r["colour_flags"][store]
        if store == "points":
            m, o, parts = (q, w, col), off, []
            for d in r["shifts"]:
                parts.append(spill_model(m[0], m[1], m[2] if flag else None, window(p, o), d))
                m, o = shift_model(*m, d), offset_model(o, d)
            cat = [np.concatenate([x[i] for x in parts]) for i in range(3 if flag else 2)]
            n = min(len(cat[0]), caps["points"])
            want = dict(xyz0=cat[0][:n], nrmw=cat[1][:n], rgba=cat[2][:n] if flag else None, dropped=len(cat[0]) - n)
            assert V.points_equal(st[-1]["points"], want), (name, store)
            assert V.grids_equal(st[-1], dict(q=m[0], w=m[1], col=m[2], off=o))
        elif store == "mesh":
            want = M.run_shifts(p, q, w, col if flag else None, r["shifts"], caps["mesh"], off=off)
            assert V.mesh_equal(st[-1]["mesh"], want["store"]) and [s["app"]["mesh"][4] for s in st[1:]] == want["taken"], (name, store)
            assert np.array_equal(st[-1]["q"], want["q"]) and np.array_equal(st[-1]["w"], want["w"]) and st[-1]["off"] == want["off"]
        else:
            want = R.walk_model(q, w, col, r["shifts"], caps["reentry"], store_colour=flag, off=off)
            assert len(want) == len(st)
            for a, b in zip(st, want):
                assert V.grids_equal(a, dict(q=b[0], w=b[1], col=b[2], off=tuple(b[3]))) and R.stores_equal(a["reentry"], b[4]), (name, store)
                assert R.invariant_holds(a["reentry"], a["off"], p["dims"])


@pytest.mark.parametrize("name", NAMES)
def test_every_rows_predicate_holds(name):
    """No row is excused: a row whose predicate fails is a failure."""
    r = V.row(name)
    st = V.row_states(name)
    assert r["holds"](r, st), (name, r["reason"], V.counts(st))
    # the predicate does not depend on where the window starts (the GPU tests start at (1, 0, 0))
    moved = V.row_states(name, off=(1, 0, 0))
    assert [s["spill"] for s in moved[1:]] == [s["spill"] for s in st[1:]] and V.counts(moved) == V.counts(st)


def test_no_row_passes_on_empty_stores():
    """Every store that a row has sees items: points, vertices and triangles, voxels saved and restored."""
    for r in V.rows():
        c = V.counts(V.row_states(r["name"]))
        print(r["name"], c)
        for store, keys in (("points", ["points"]), ("mesh", ["vertices", "triangles"]), ("reentry", ["saved", "restored"])):
            assert (store not in r["stores"]) or all(c[k] > 0 for k in keys), (r["name"], c)


@pytest.mark.parametrize("variant", sorted(V.MUTANT_ROWS))
def test_every_switch_changes_exactly_its_rows(variant):
    placed = [r["name"] for r in V.rows() if V.MUTANT_ROWS[variant](r)]
    changed = [n for n in NAMES if not V.states_equal(V.row_states(n), V.row_states(n, variant))]
    assert len(placed) > 0 and changed == placed, (variant, changed, placed)
    # and the GPU side would see it at the end of the walk too, where the back-to-back run compares
    for n in placed:
        assert not V.states_equal(V.row_states(n)[-1:], V.row_states(n, variant)[-1:]), (variant, n)


def test_the_table_has_the_rows_it_is_there_for():
    rows = V.rows()
    assert len({r["name"] for r in rows}) == len(rows)
    assert sum(r["holds"] is V._twice for r in rows) == 2 and V.row("twice, whole window")["shifts"][0][0] == V.grid()[0]["dims"][0]
    assert sorted(r["short"] for r in rows if "short" in r) == sorted(c for n in range(4) for c in itertools.combinations(V.STORES, n))
    assert sorted(r["stores"] for r in rows if r["holds"] is V._subset) == sorted(V._subsets()) and len(V._subsets()) == 7
    assert V.row("closed walk")["shifts"] == R.CLOSED_WALK
    # one item short: with one more the walk fits
    short = V.short_capacities()
    p, q, w, col = V.grid()
    for caps in (dict(V.AMPLE, points=short["points"] + 1), dict(V.AMPLE, mesh=(short["mesh"][0] + 1, short["mesh"][1])),
                 dict(V.AMPLE, reentry=short["reentry"] + 1)):
        st = V.stores_walk_model(p, q, w, col, V.OVERFLOW[:2], caps, V.ALL_COLOUR)
        assert st[-1]["points"]["dropped"] == 0 and st[-1]["mesh"]["dropped"] == (0, 0) and st[-1]["reentry"]["dropped"] == 0


def test_every_row_stays_small():
    for r in V.rows():
        p = V.grid(r["grid"])[0]
        assert int(np.prod(p["dims"])) <= 4096 and len(r["shifts"]) <= 8, r["name"]
