"""Proves the table of tests/pyramid_cases.py without a GPU: every row reaches the cases it is there for (predicates on models alone);
the oracle's P1 equals an exact integer model on levels 0 - 2 and a stepwise float32 numpy restatement on every row and level; the
replay of image_pyramid_fused_kernel_body's index arithmetic finds every LDS index inside what its phase wrote, and reports each of
seven mutated launch constants on at least one size of the table. tests/test_gpu_pyramid_cases.py then holds the kernels to the oracle
on the same rows."""
import os

import numpy as np
import pytest

import pyramid_cases as PC
from pyramid_cases import K, bits

SWEEP_AXIS = sorted({n for r in PC.TABLE if r["group"].startswith("sweep") for n in r["size"]})


def test_constants_are_the_kernels_own():
    assert (K["kPT"], K["kPIn"], K["kPInS"], K["kPL1"], K["kPL2"]) == (32, 53, 54, 25, 11)
    assert (K["origin"], K["l1lo"], K["l1hi"], K["l2lo"], K["l2hi"]) == (-14, -6, 18, -2, 8)
    assert (K["grid_x"], K["grid_y"], K["wide_from"], K["fused_max_levels"], K["max_levels"]) == (64, 4, 1024, 4, 8)
    # the halos are exactly what the level below needs: 5 taps at stride 2
    assert K["kPL1"] == K["l1hi"] - K["l1lo"] + 1 and K["kPL2"] == K["l2hi"] - K["l2lo"] + 1
    assert K["kPIn"] == 2 * (K["kPL1"] - 1) + 5 and K["origin"] == 2 * K["l1lo"] - 2


def test_each_axis_sees_every_size_and_every_residue():
    for tag in "abc":
        rows = PC.group_rows(f"sweep-{tag}")
        assert sorted(r["size"][0] for r in rows) == PC.SWEEP == sorted(r["size"][1] for r in rows)
        assert sum(r["size"][0] == r["size"][1] for r in rows) < 4                   # not a square-only table
        for axis in (0, 1):
            assert {r["size"][axis] % K["kPT"] for r in rows if r["size"][axis] >= 72} == set(range(32))
            assert {r["size"][axis] % K["kPT"] for r in rows} == set(range(32))
    assert PC.SWEEP[0] == 8 and PC.SWEEP[-1] == 103
    shapes = {(r["kind"], r["size"], r["levels"]) for r in PC.TABLE}
    for size in ((1, 1), (1, 9), (9, 1), (2, 2), (3, 2), (4, 5), (7, 7), (33, 65)):
        for levels in (1, 2, 3):
            assert (("image", size, levels) in shapes) == PC.legal(size[0], size[1], levels)
    assert {("image", (130, 257), 5), ("image", (130, 257), 8), ("depth", (130, 257), 5), ("depth", (130, 257), 8)} <= shapes
    assert PC.level_dims(130, 257, 8)[-1] == (1, 2)
    for kind in ("image", "depth"):
        assert {(kind, (r, c), 2) for r in (3, 4, 5) for c in (63, 64, 65)} <= shapes
    assert PC.n_tiles(992, 1056) == K["wide_from"] - 1 and PC.n_tiles(1024, 1024) == K["wide_from"]
    assert sum(r["size"][0] * r["size"][1] > 200 * 300 for r in PC.TABLE) == 2           # the only large rows


@pytest.mark.parametrize("group", PC.GROUPS)
def test_every_row_reaches_the_cases_it_is_there_for(group):
    for r in PC.group_rows(group):
        assert r["cases"] or r["group"] in ("constant",) or r["size"] == (1, 1), r["name"]
        for case in r["cases"]:
            assert PC.PREDICATES[case](r, PC.image(r)), (r["name"], case)


def test_every_case_is_reached_and_the_sweep_ranges_are_the_replays():
    reached = {c for r in PC.TABLE for c in r["cases"]}
    assert reached == set(PC.PREDICATES), set(PC.PREDICATES) ^ reached
    # the ranges the sweep was laid out by (sweep_cases) against the replayed arithmetic, both ways, for every size of the sweep
    for n in PC.SWEEP:
        f = PC.replay_axis(n, 4)[1]
        assert (f["tiles"] == 1) == (n <= 32)
        assert (PC.pyramid_trips(n, 4) >= 2) == (n <= 11) and (n >> 3 == 1) == (n <= 15)
        assert any(t < f["tiles"] - 1 for t in f["l1_far_clipped"]) == (33 <= n <= 37 or 65 <= n <= 69 or 97 <= n <= 101)
        assert bool(f["full_halo_tiles"]) == (n >= 71), n              # below, a halo of the second tile is clipped or reflected
        assert (f["last_tile_width"] == 1) == (n % 32 == 1)
        assert f["last_tile_width"] == (n - 1) % 32 + 1
    assert {PC.replay_axis(n, 4)[1]["last_tile_width"] for n in range(33, 72)} == set(range(1, 33))
    for r in PC.TABLE:
        if r["group"].startswith("sweep"):
            have = {c for c in PC.PREDICATES if c in ("single_tile", "several_tiles", "reflects_twice", "one_pixel_level", "l1_far_clip_before_last",
                                                      "interior_full_halo", "last_tile_one_row", "last_tile_one_col") and PC.PREDICATES[c](r, None)}
            assert have == set(r["cases"]) - {"integer"}, r["name"]


# ---- the oracle against the definition -------------------------------------------------------------------------------------------
INTEGER_ROWS = [r for r in PC.TABLE if "integer" in r["cases"]]


@pytest.mark.parametrize("group", sorted({r["group"] for r in INTEGER_ROWS}))
def test_exact_integer_model(group):
    """Integer content: the oracle's blurred level 0, level 1 and level 2 are the int64 sums over reflect-101 indices divided by 16,
    256 and 65 536, bit for bit — the definition, whatever the association order. Level 3 is not exact in float32 (the oracle is
    1.3e-5 off the rational value on a 72 x 72 image): the stepwise restatement below holds it."""
    n = 0
    for r in INTEGER_ROWS:
        if r["group"] != group:
            continue
        model = PC.integer_model(PC.image(r), r["levels"])
        smoothed, plain = PC.reference(r, True), PC.reference(r, False)
        assert np.array_equal(bits(smoothed[0]), bits(model[0])), r["name"]
        assert np.array_equal(bits(plain[0]), bits(PC.image(r))), r["name"]
        for l in range(1, min(r["levels"], 3)):
            assert np.array_equal(bits(smoothed[l]), bits(model[l])) and np.array_equal(bits(plain[l]), bits(model[l])), (r["name"], l)
        n += 1
    assert n > 0


def test_integer_model_closed_forms():
    """The model itself on the two contents with a closed form: a constant stays the constant on every level; one 255 at (0, 0) of a
    zero image weighs 4, 2, 2, 1 (of 16) in the blur and 36, 6, 6, 1 (of 256) at level 1: reflect-101 never reads the edge pixel twice."""
    r = PC.BY_NAME["constant-72x103"]
    for a in PC.integer_model(PC.image(r), 4):
        assert (a == 255).all()
    for smooth in PC.SMOOTH:
        for a in PC.reference(r, smooth):
            assert (bits(a) == bits(PC.f32(255))).all()                     # level 3 too: a constant is exact on every level
    m = PC.integer_model(PC.image(PC.BY_NAME["impulse-40x72-at-0-0"]), 4)
    assert m[0][0, 0] == 255 * 4 / 16 and m[0][0, 1] == m[0][1, 0] == 255 * 2 / 16 and m[0][1, 1] == 255 / 16 and m[0][2, 2] == 0
    assert m[1][0, 0] == 255 * 36 / 256 and m[1][0, 1] == m[1][1, 0] == 255 * 6 / 256 and m[1][1, 1] == 255 / 256
    corner = PC.integer_model(PC.image(PC.BY_NAME["impulse-40x72-at-39-71"]), 4)
    assert corner[0][39, 71] == 255 * 4 / 16 and corner[0][38, 70] == 255 / 16 and corner[1][19, 35] == 255 * 16 / 256


@pytest.mark.parametrize("group", PC.GROUPS)
def test_stepwise_restatement_is_the_oracle(group):
    """Blur, pyrDown, decimation and the median restated in numpy, float32 step by step in the oracle's association: the same bits on
    every row, level and smoothing."""
    for r in PC.group_rows(group):
        for smooth in PC.SMOOTH:
            want = PC.np_pyramid("image" if r["kind"] == "image" else "depth", PC.image(r), r["levels"], smooth)
            got = PC.reference(r, smooth)
            assert len(got) == len(want) == r["levels"]
            for l, (g, w) in enumerate(zip(got, want)):
                assert g.shape == w.shape == PC.level_dims(r["size"][0], r["size"][1], r["levels"])[l], (r["name"], l)
                assert np.array_equal(bits(g), bits(w)), (r["name"], smooth, l, int((bits(g) != bits(w)).sum()))


def test_median_closed_forms():
    n = 0
    for r in PC.TABLE:
        if r["closed"] is not None:
            med = PC.reference(r, True)[0]
            assert np.array_equal(bits(med[1:-1, 1:-1]), bits(r["closed"](PC.image(r)))), r["name"]
            n += 1
    assert n >= 6
    # the two patterns differ by one class of pixels and give different answers everywhere inside
    a, b = PC.BY_NAME["median-four-zeros-13x67"], PC.BY_NAME["median-five-zeros-13x67"]
    assert (PC.reference(a, True)[0][1:-1, 1:-1] > 0).all() and not PC.reference(b, True)[0][1:-1, 1:-1].any()


def test_depth_levels_are_the_odd_pixels_of_level_0():
    for r in PC.TABLE:
        if r["kind"] != "image":
            for smooth in PC.SMOOTH:
                lv = PC.reference(r, smooth)
                for l in range(1, r["levels"]):
                    m = (1 << l) - 1
                    rr, cc = lv[l].shape
                    assert np.array_equal(bits(lv[l]), bits(lv[0][m::1 << l, m::1 << l][:rr, :cc])), (r["name"], l)


# ---- the replay of the fused kernel's indices ------------------------------------------------------------------------------------
def test_replay_is_clean():
    """Every LDS index inside what its phase wrote, every halo width in 1 ... kPL1 / kPL2, every pixel of every level owned by exactly
    one tile: sizes 1 ... 399 at every number of levels the size allows, smoothed and not."""
    n_checked = 0
    for n in range(1, 400):
        for levels in range(1, K["fused_max_levels"] + 1):
            if PC.legal(n, n, levels):
                for smooth in PC.SMOOTH:
                    bad, facts = PC.replay_axis(n, levels, smooth)
                    assert not bad, bad[:4]
                    assert all(1 <= w <= K["kPL1"] for w in facts["n1"]) and all(1 <= w <= K["kPL2"] for w in facts["n2"])
                n_checked += 1
    assert n_checked > 1500
    for n in (992, 1024, 1056):
        assert not PC.replay_axis(n, 4)[0]


MUTANTS = {
    "kPIn-52": dict(kPIn=52),
    "origin-13": dict(origin=-13),
    "l1-halo-from-5": dict(l1lo=-5),
    "l1-halo-to-17": dict(l1hi=17),
    "l2-halo-from-1": dict(l2lo=-1),
    "l2-halo-to-7": dict(l2hi=7),
    "kPL1-24": dict(kPL1=24),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_replay_reports_mutant(name):
    """The replay has power: each mutated constant is reported on at least one size of the table's sweep."""
    caught = [n for n in SWEEP_AXIS if PC.replay_axis(n, 4, **MUTANTS[name])[0]]
    assert caught, name
    if name == "kPL1-24":        # needs an interior tile with a full level-1 halo: only the top of the sweep has one
        assert min(caught) >= 70 and set(range(72, 104)) <= set(caught)
    else:
        assert min(caught) <= 40


def test_child_script_judges_nothing():
    src = open(os.path.join(PC.ROOT, "tests", "pyramid_child.py")).read()
    assert "assert" not in src and "oracle" not in src.split('"""')[2]
