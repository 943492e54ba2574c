"""The table of tests/volume_shift_cases.py without a GPU: the launch constants, every row's predicate, the replay of the shift kernel's
walk against shift_model, each of the replay's switches against the rows of its class, what the earlier rows of the suite did not
reach, the spill's partition of the extraction on the large grids, and the chain's counts."""
import numpy as np

import volume_shift_cases as V
from test_volume_cpu import bits, extract_model, params
from test_volume_shift_cpu import grids, origin_model, rows, shift_model, spill_mask, spill_model, window


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def test_launch_constants_are_read_from_the_sources():
    assert len(V.plane_cap_matches()) == 1
    k = V.constants()
    assert k["plane_cap"] == 65535 and k["kVolShiftLanes"] == 64 and k["kVolShiftRows"] == 4, k
    assert k["kVolShiftLanes"] % 64 == 0


def test_every_row_is_in_the_table_for_a_reason_that_holds():
    for r in V.SHIFT:
        print(f"{r['name']}: {r['why']}")
        for d in r["shifts"]:
            print(f"    d {d}: " + V.paths_line(r["dims"][0], d[0]) + (", second-trip planes inside / outside %d / %d" %
                                                                     V.second_trip_planes(r["dims"][2], d[2]) if r["cls"] == "tall" else ""))
        assert r["holds"](r), r["name"]
        assert r["colour"] and int(np.prod(r["dims"])) <= 1025 * 32 * 32, r["name"]
    held = V.class_holds()
    assert all(held.values()), held
    assert len(set(V.names())) == len(V.SHIFT) and all(n in V.names() for n in V.NO_COLOUR)


def test_quad_paths_on_hand_counted_rows():
    p = V.quad_paths(8, 4)          # quad 0 reads words 4 .. 7 at once, quad 1 would read 8 .. 11
    assert (p["build"], p["trips"], p["vload"], p["dword_all"], p["partly"], p["none"]) == ("vector", 1, 1, 0, 0, 1)
    p = V.quad_paths(8, 1)          # 1 .. 4 and 5 .. 8
    assert (p["vload"], p["dword_all"], p["partly"], p["none"]) == (0, 1, 1, 0)
    p = V.quad_paths(8, 0)
    assert p["vload"] == 2
    p = V.quad_paths(259, -1)       # 65 quads: two trips; the tail quad holds words 256 .. 258 and, behind the end, 259 <- 258
    assert (p["build"], p["qpr"], p["trips"], p["tail_guarded"]) == ("dword", 65, 2, True)
    assert p["tail"] == dict(trip=1, valid=3, valid_inside=3, guarded_inside=1)
    assert p["per_trip"][1] == dict(vload=0, dword_all=0, partly=1, none=0) and p["partly"] == 2     # (quad 0 reads -1)
    p = V.quad_paths(259, 1)
    assert p["tail"] == dict(trip=1, valid=3, valid_inside=2, guarded_inside=0)
    p = V.quad_paths(516, -256)
    assert p["trips"] == 3 and p["per_trip"][0]["none"] == 64 and p["per_trip"][1]["vload"] == 64 and p["per_trip"][2]["vload"] == 1


def test_replay_equals_the_model_on_every_row_and_each_switch_fails_exactly_its_class():
    """With no switch the replay is shift_model bit for bit and reads every word that stays exactly once. A switch changes the grids
    (or, the tail switch, the words read: the dword build's store has a guard of its own, so an unguarded read is never written) on
    the rows and shifts of its class and on no other."""
    met = dict(vload_ignores_dx=0, one_quad_trip=0, one_plane_trip=0, tail_unguarded_read=0, none=0)
    k = V.constants()
    for r in V.SHIFT:
        p, q, w, col = V.inputs(r["name"])
        for d in r["shifts"]:
            want = shift_model(q, w, col, d)
            info = {}
            assert _same(V.shift_replay(q, w, col, d, info=info), want), (r["name"], d)
            assert info["loaded"] == V.stays(r["dims"], d), (r["name"], d)
            paths = V.quad_paths(r["dims"][0], d[0])
            moves = V.stays(r["dims"], d) > 0                                    # (a shift that empties the grid loads nothing at all)
            row_stays = abs(d[1]) < r["dims"][1] and abs(d[2]) < r["dims"][2]   # some row of the new grid has its source row inside
            cls = dict(vload_ignores_dx=paths["vload"] > 0 and d[0] != 0 and row_stays,
                       one_quad_trip=paths["trips"] >= 2,
                       one_plane_trip=r["dims"][2] > k["plane_cap"],
                       tail_unguarded_read=paths["tail_guarded"] and paths["tail"]["guarded_inside"] > 0 and row_stays)
            for switch, in_class in cls.items():
                info = {}
                got = V.shift_replay(q, w, col, d, info=info, **{switch: True})
                differs = not _same(got, want) or info["loaded"] != V.stays(r["dims"], d)
                assert differs == in_class, (r["name"], d, switch, differs, in_class)
                if switch == "tail_unguarded_read":
                    assert _same(got, want), (r["name"], d)
                    assert info["loaded"] - V.stays(r["dims"], d) == \
                        (paths["tail"]["guarded_inside"] * max(0, r["dims"][1] - abs(d[1])) * max(0, r["dims"][2] - abs(d[2]))
                         if in_class else 0)
                met[switch] += int(in_class)
            met["none"] += int(not any(cls.values()) and moves)
    print(met)
    assert all(v > 0 for v in met.values()), met


def test_the_replay_without_colour_and_on_the_earlier_rows():
    for name in V.NO_COLOUR:
        p, q, w, col = V.inputs(name)
        for d in V.find(name)["shifts"]:
            assert _same(V.shift_replay(q, w, None, d), shift_model(q, w, None, d)), (name, d)
    for name, p, q, w, col, d in rows():
        assert _same(V.shift_replay(q, w, col, d), shift_model(q, w, col, d)), (name, d)


def test_the_earlier_rows_reach_none_of_the_three_launch_paths():
    """The gap this table closes, written down: over every row the suite held the shift to before (the grids of
    test_volume_shift_cpu.rows() under shifts_for, and the two launch-geometry grids under their two shifts) no row takes the 16-byte
    load with dx != 0, none runs the dword build's quad loop twice, and none has more planes than gridDim.y holds."""
    k = V.constants()
    earlier = [(p["dims"], d) for _, p, _, _, _, d in rows()] + V.EARLIER_GEOMETRY_ROWS
    assert len(earlier) == 7 * 14 + 4
    for dims, d in earlier:
        paths = V.quad_paths(dims[0], d[0])
        assert not (paths["vload"] > 0 and d[0] != 0), (dims, d)
        assert not (paths["build"] == "dword" and paths["trips"] >= 2), (dims, d)
        assert dims[2] <= k["plane_cap"], dims
    # and this table reaches each of them
    new = [(r["dims"], d) for r in V.SHIFT for d in r["shifts"]]
    assert any(V.quad_paths(n[0], d[0])["vload"] > 0 and d[0] != 0 for n, d in new)
    assert any(V.quad_paths(n[0], d[0])["build"] == "dword" and V.quad_paths(n[0], d[0])["trips"] >= 3 for n, d in new)
    assert any(n[2] > k["plane_cap"] for n, d in new)


def test_the_rows_spill_is_spill_model():
    """volume_shift_cases.spill computes a row's points once and masks them per shift: the same arrays as spill_model."""
    for name in ("vload 8x4x3", "trips-dword 259x3x3", "short 2x3x5"):
        p, q, w, col = V.inputs(name)
        for d in V.find(name)["shifts"]:
            for a, b in zip(V.spill(name, d), spill_model(q, w, col, window(p, V.OFF0), d)):
                assert a.shape == b.shape and a.tobytes() == b.tobytes(), (name, d)
    p, q, w, col = V.inputs("short 2x3x5")
    assert V.spill("short 2x3x5", (1, 0, 0), colour=False)[2] is None


def test_spill_and_what_stays_partition_the_extraction_on_the_large_grids():
    """test_volume_shift_cpu.test_spill_and_what_stays_partition_the_extraction on a grid of 65 537 planes and on the two grids whose
    extraction blocks end with a chunk of the scan and one over it, in a dyadic window: spill + extraction after = extraction
    before, as multisets of the (x, y, z, w) bit patterns."""
    def rec(P, N):
        a = np.concatenate([bits(P[:, :3]), bits(N[:, 3:4])], 1)
        return a[np.lexsort(a.T[::-1])]

    n_rows = 0
    for name in ("tall 2x2x65537", "scan 1024x32x32", "scan 1025x32x32"):
        row = V.find(name)
        _, q, w, _ = V.inputs(name)
        p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=row["dims"], vs=2.0 ** -4, origin=(-0.5, 3.0 / 16, 1.25))
        cen = origin_model(p["origin"], (0, 0, 0), p["vs"]).astype(np.float64)
        Pb, Nb = extract_model(q, w, p)
        before = rec(Pb, Nb)
        for d in row["shifts"]:
            pw = window(p, d)
            assert np.array_equal(np.asarray(pw["origin"], np.float64), cen + np.array(d) / 16.0)     # exact
            q2, w2, _ = shift_model(q, w, None, d)
            m = spill_mask(q, w, d)[0]
            Pa, Na = extract_model(q2, w2, pw)
            assert len(Pa) + int(m.sum()) == len(Pb), (name, d)
            assert np.array_equal(rec(np.concatenate([Pb[m], Pa]), np.concatenate([Nb[m], Na])), before), (name, d)
            n_rows += 1
    assert n_rows == 6 + 2 + 2


def test_the_chain_spills_at_every_shift_and_its_capacities_cut_where_they_should():
    c = V.chain()
    assert len(V.CHAIN) == 27 and V.CHAIN[:24] == [(1, 0, 0)] * 24 and V.CHAIN[24:] == [(0, 1, 0)] * 3
    assert grids()["random 64x4x4"][0] is c["p"]
    print("points per spill", c["counts"], "capacities", c["capacities"])
    assert all(n > 0 for n in c["counts"]), c["counts"]
    total = sum(c["counts"])
    more, at, inside = c["capacities"]
    ends = np.cumsum(c["counts"])
    assert more > total
    assert at == ends[11] and at in ends and at < total                          # fills at the end of the 12th spill
    assert ends[11] < inside < ends[12] and inside - ends[11] == c["counts"][12] // 2 + 1   # fills inside the 13th
    assert c["off"] == (24, 3, 0) and c["w"].any()
