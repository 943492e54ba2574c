"""The map's voxel-hash rows (tests/map_hash_cases.py) without a GPU: the mirror against plain integers, the table model against RefMap
and against the sequential simulation, linear probing's order independence on every row, each row's predicate, the four switches on
exactly their rows, how far the existing small MAP rows of tests/geometry_cases.py reach into the table, and the refusals of the
test-only read-out on a NULL handle."""
import ctypes as C

import numpy as np
import pytest

import map_hash_cases as H

u64 = np.uint64
f32 = np.float32
EXTREME = [-2 ** 20 + 1, -2 ** 20 + 2, -1, 0, 1, 2 ** 20 - 2, 2 ** 20 - 1]


def test_the_constants_and_the_slot_rule_are_read_from_the_sources():
    k = H.constants()
    assert k["kMapBlock"] == 256 and k["kMapEmpty"] == 2 ** 64 - 1 and k["slot_factor"] == 2
    for cap, n in ((256, 256), (512, 256), (16, 768), (64, 3), (1 << 17, 240 * 424), (1, 1), (255, 257), (256, 257)):
        s = H.n_slots(cap, n)
        assert s & (s - 1) == 0 and s >= 2 * (cap + n) and (s == 1 or s // 2 < 2 * (cap + n))
    assert H.n_slots(256, 256) == 1024 and H.n_slots(256, 257) == 2048 and H.n_slots(1 << 17, 240 * 424) == 1 << 19


def test_the_hash_and_the_packing_equal_plain_integer_arithmetic():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 2 ** 63, 10_000, dtype=np.int64).astype(u64)
    fields = [(a, b, c) for a in EXTREME for b in EXTREME for c in EXTREME]
    packed = H.pack(*np.array(fields, np.int64).T)
    for (a, b, c), p in zip(fields, packed.tolist()):
        assert p == (a + 2 ** 20) | ((b + 2 ** 20) << 21) | ((c + 2 ** 20) << 42) < 2 ** 63
    assert len(set(packed.tolist())) == len(fields) and H.EMPTY not in packed.tolist()
    allk = np.concatenate([keys, packed, np.array([0, 1, 2 ** 63 - 1, 2 ** 64 - 2], u64)])
    got = H.mix(allk)
    assert got.dtype == u64 and [H.mix_int(int(k)) for k in allk.tolist()] == got.tolist()
    assert np.array_equal(H.home(allk, 1024), got & u64(1023))
    # the switched packing does let a field's top bit run into its neighbour
    assert H.pack(0, 0, 0, shift_20=True) == H.pack(0, 1, 0, shift_20=True) and H.pack(0, 0, 0) != H.pack(0, 1, 0)


def _entries(tab):
    return np.array(sorted(tab.values()), np.int32).reshape(-1, 2)


@pytest.mark.parametrize("name", H.NAMES)
def test_the_table_model_is_refmap_and_the_simulation(name):
    c, trail, sims = H.case(name), H.ref_trail(name), H.sim(name)
    assert len(trail) == len(sims) == len(c["inputs"])
    for i, ((st, xyzi, kp), snap) in enumerate(zip(trail, sims)):
        tab = H.table_model(c, i + 1)
        # the model's entries, in (insertion, pixel) order and cut at capacity, are RefMap's points
        assert np.array_equal(_entries(tab)[:c["capacity"]], kp), (name, i)
        assert st["size"] == snap["size"] == min(len(tab), c["capacity"])
        # the sequential simulation's table is the model's, and its survivors of this insertion are the model's new entries
        occ = snap["keys"] != u64(H.EMPTY)
        assert {int(k): (int(p) >> 32, int(p) & 0xffffffff) for k, p in zip(snap["keys"][occ], snap["payload"][occ])} == tab
        assert np.all(snap["payload"][~occ] == u64(H.EMPTY))
        assert snap["survivors"] == sorted(p for ins, p in tab.values() if ins == i) and snap["stuck"] == 0


@pytest.mark.parametrize("name", H.NAMES)
def test_designed_rows_got_the_keys_and_homes_they_were_designed_for(name):
    c = H.case(name)
    if "designed" not in c:
        return
    slots, seen = H.case_slots(c), set()
    for (val, dep, img, A), want in zip(c["inputs"], c["designed"]):
        pix, inr, key, _, _ = H.frame_keys(c, val, dep, A)
        new = [k for k in key.tolist() if k not in seen]
        assert inr.all() and new == want and len(set(want)) == len(want), name       # distinct, and what the pixels really produce
        seen.update(want)
        if "homed" in c:
            assert c["homed"](H.home(np.array(want, u64), slots).astype(np.int64), slots).all(), name


@pytest.mark.parametrize("name", H.NAMES)
def test_occupied_slots_and_carries_do_not_depend_on_the_order(name):
    c, snap = H.case(name), H.sim(name)[-1]
    slots = H.case_slots(c)
    keys = np.sort(H.table_keys(snap))
    rng = np.random.default_rng(17)
    orders = [keys, keys[::-1], rng.permutation(keys), rng.permutation(keys)]
    reps = [H.probe_replay(o, slots) for o in orders]
    want_occ = snap["keys"] != u64(H.EMPTY)
    for r in reps:
        assert np.array_equal(r["occupied"], want_occ) and np.array_equal(r["over"], reps[0]["over"])
        assert r["carried"] == r["below_home"] == reps[0]["carried"] and len(r["slot"]) == len(keys)
        # a table filled in this order, with the model's payloads, passes the checks the device's table is put through
        pay = {int(k): p for k, p in zip(snap["keys"][want_occ].tolist(), snap["payload"][want_occ].tolist())}
        p = np.array([pay[int(k)] if int(k) != H.EMPTY else H.EMPTY for k in r["table"].tolist()], u64)
        got = H.check_table(r["table"], p, snap, slots)
        assert got["carried"] == r["carried"] and got["n_keys"] == len(keys)


def test_the_table_checks_are_not_blind():
    c, snap = H.case("wrap"), H.sim("wrap")[-1]
    slots = H.case_slots(c)
    H.check_table(snap["keys"], snap["payload"], snap, slots)
    at = np.nonzero(snap["keys"] != u64(H.EMPTY))[0]
    a, b, free = int(at[3]), int(at[100]), 600
    assert snap["keys"][free] == u64(H.EMPTY) and snap["keys"][free - 1] == u64(H.EMPTY)

    def broken(edit):
        k, p = snap["keys"].copy(), snap["payload"].copy()
        edit(k, p)
        with pytest.raises(AssertionError):
            H.check_table(k, p, snap, slots)

    def swap_payloads(k, p):
        p[a], p[b] = p[b], p[a]

    def move_out_of_the_run(k, p):
        k[free], p[free], k[a], p[a] = k[a], p[a], u64(H.EMPTY), u64(H.EMPTY)

    def second_copy(k, p):
        k[free], p[free] = k[a], p[a]

    def payload_left_behind(k, p):
        p[free] = u64(5)

    def last_pixel_wins(k, p):
        p[a] = p[a] + u64(1)

    for edit in (swap_payloads, move_out_of_the_run, second_copy, payload_left_behind, last_pixel_wins):
        broken(edit)


def _over_end(name, upto):
    c = H.case(name)
    return H.probe_replay(np.sort(H.table_keys(H.sim(name)[upto])), H.case_slots(c))


def test_row_wrap():
    c, r = H.case("wrap"), _over_end("wrap", 0)
    assert H.case_slots(c) == 1024 and len(r["slot"]) == 256 and r["carried"] >= 252
    assert H.runs(r["occupied"])[1] >= 256


def test_row_one_home():
    c, r = H.case("one_home"), _over_end("one_home", 0)
    slots = H.case_slots(c)
    keys = H.table_keys(H.sim("one_home")[0])
    assert len(keys) == 256 and np.all(H.home(keys, slots) == u64(slots // 2)) and r["carried"] == 0
    # the occupied slots are home .. home + 255 whatever the order, so whichever key came last lies 255 slots from home
    assert np.array_equal(np.nonzero(r["occupied"])[0], slots // 2 + np.arange(256))


def test_row_ends_at_the_end():
    c = H.case("ends_at_the_end")
    slots = H.case_slots(c)
    r0, r1 = _over_end("ends_at_the_end", 0), _over_end("ends_at_the_end", 1)
    assert np.array_equal(np.nonzero(r0["occupied"])[0], np.arange(slots - 128, slots)) and r0["carried"] == 0
    assert r1["carried"] == 1 and np.array_equal(np.nonzero(r1["occupied"])[0], np.concatenate([[0], np.arange(slots - 128, slots)]))
    # on the device the old keys are all there before the new one claims: it is the one in slot 0
    snap = H.sim("ends_at_the_end")[1]
    assert int(snap["keys"][0]) == c["designed"][1][0] and int(snap["payload"][0]) == (1 << 32) | 77


def test_row_repeat_and_extend():
    c, trail, sims = H.case("repeat_and_extend"), H.ref_trail("repeat_and_extend"), H.sim("repeat_and_extend")
    slots = H.case_slots(c)
    assert slots == 2048
    assert trail[0][0]["dropped_voxel"] == 0 and trail[1][0]["dropped_voxel"] == 128 and trail[1][0]["size"] == 384
    old, new = c["designed"]
    repeats = old[0::2]
    assert sims[1]["survivors"] == list(range(1, 256, 2))
    for order in (sorted(old), sorted(old, reverse=True)):
        r = H.probe_replay(order + new, slots)
        assert r["carried"] >= 380
        assert sum(r["slot"][k] < slots - 4 for k in repeats) >= 124            # the repeats are found behind the wrap
        assert min(r["slot"][k] for k in new) == 252 and max(r["slot"][k] for k in new) == 379   # behind every old key
        assert sorted(r["slot"][k] for k in old) == list(range(252)) + list(range(slots - 4, slots))


def test_row_one_voxel():
    c, trail, sims = H.case("one_voxel"), H.ref_trail("one_voxel"), H.sim("one_voxel")
    assert H.constants()["kMapBlock"] * 3 == c["size"][0] * c["size"][1]
    val, dep, _, A = c["inputs"][0]
    pix, inr, key, _, _ = H.frame_keys(c, val, dep, A)
    assert inr.all() and len(pix) > 350 and len(set(key.tolist())) == 1 and key[0] == H.pack(0, 0, 0)
    assert pix[0] == H.ONE_VOXEL_FIRST and 256 <= pix[0] < 512 and (pix >= 512).sum() > 100
    flat = dep.reshape(-1)
    assert (flat[300:] <= 0).sum() >= 10 and ((np.abs(flat[300:]) < f32(0.01)) & (flat[300:] > 0)).sum() >= 10
    assert trail[0][2].tolist() == [[0, H.ONE_VOXEL_FIRST]] and trail[0][0]["dropped_voxel"] == len(pix) - 1
    assert trail[1][0]["size"] == 1 and trail[1][0]["dropped_voxel"] == 2 * len(pix) - 1 and trail[1][0]["candidates"] == 2 * len(pix)
    assert sims[1]["survivors"] == [] and len(H.table_keys(sims[1])) == 1


def test_row_field_edges():
    c, trail = H.case("field_edges"), H.ref_trail("field_edges")
    prev = dict(trail[0][0], dropped_range=0, size=0, dropped_voxel=0)
    top, outside = 2 ** 20, {}
    for i, (val, dep, img, A) in enumerate(c["inputs"]):
        axis, t = i // 4, H.EDGE_T[i % 4]
        pix, inr, key, k, w = H.frame_keys(c, val, dep, A)
        assert len(pix) == 3
        # every world coordinate is exact in fp32: the fp64 evaluation of the same sums gives the same numbers
        P = np.stack([pix.astype(np.float64) - 1.0, np.zeros(3), np.ones(3)])
        exact = A[:3, :3].astype(np.float64) @ P + A[:3, 3:4].astype(np.float64)
        assert np.array_equal(np.stack(w).astype(np.float64), exact)
        q = np.floor(exact[axis]).astype(np.int64)
        want_in = np.abs(q) < top
        assert np.array_equal(inr, want_in) and np.array_equal(k[axis][inr], q[want_in])
        st = trail[i][0]
        assert st["dropped_range"] - prev["dropped_range"] == int((~want_in).sum())
        sign = 1 if t > 0 else -1
        assert sign * (top - 1) in q[want_in].tolist()                  # the last voxel inside the field is kept ...
        outside.setdefault((axis, sign), []).extend(q[~want_in].tolist())
        prev = st
    assert sorted(outside) == [(a, s) for a in range(3) for s in (-1, 1)]
    assert all(s * top in v for (a, s), v in outside.items())           # ... and the first one outside is counted, per axis and sign
    assert trail[-1][0]["dropped_range"] == sum(len(v) for v in outside.values()) == 12
    tab = H.table_model(c)
    fields = {((k >> (21 * a)) & (2 ** 21 - 1)) for k in tab for a in range(3)}
    assert {1, 2 ** 21 - 1} <= fields and 0 not in fields


def test_row_field_neighbours():
    c, trail = H.case("field_neighbours"), H.ref_trail("field_neighbours")
    tab = H.table_model(c)
    assert sorted(tab) == sorted(H.pack(*np.array(H.NEIGHBOURS, np.int64).T).tolist()) and len(tab) == len(H.NEIGHBOURS)
    assert sorted(tab.values()) == [(i, 1) for i in range(len(H.NEIGHBOURS))]
    st = trail[-1][0]
    assert st["size"] == st["candidates"] == len(H.NEIGHBOURS) and st["dropped_voxel"] == st["dropped_range"] == 0
    for (a, b, cc), (val, dep, img, A) in zip(H.NEIGHBOURS, c["inputs"]):
        _, inr, _, k, w = H.frame_keys(c, val, dep, A)
        assert inr.all() and [int(v[0]) for v in k] == [a, b, cc]
        assert [float(v[0]) for v in w] == [a + 0.5, b + 0.5, cc + 0.5]


def test_row_fullest_table():
    c, trail, sims = H.case("fullest_table"), H.ref_trail("fullest_table"), H.sim("fullest_table")
    slots = H.case_slots(c)
    n = c["size"][0] * c["size"][1]
    assert slots == 1024 == 2 * (c["capacity"] + n) and len(H.table_keys(sims[1])) == 511 == c["capacity"] - 1 + n
    assert [t[0]["size"] for t in trail] == [255, 256, 256] and [t[0]["dropped_capacity"] for t in trail] == [0, 255, 255]
    assert trail[2][0] == dict(trail[1][0], insertions=3)
    assert np.array_equal(sims[2]["keys"], sims[1]["keys"]) and np.array_equal(sims[2]["payload"], sims[1]["payload"])
    assert len(sims[1]["survivors"]) == 256


def test_row_not_a_number():
    c, trail, sims = H.case("not_a_number"), H.ref_trail("not_a_number"), H.sim("not_a_number")
    kinds = set()
    for i, (val, dep, img, A) in enumerate(c["inputs"]):
        pix, inr, _, _, w = H.frame_keys(c, val, dep, A)
        assert len(pix) > 100 and not inr.any()
        kinds |= {"nan"} if np.isnan(np.stack(w)).any() else set()
        kinds |= {"+inf"} if np.isposinf(np.stack(w)).any() else set()
        kinds |= {"-inf"} if np.isneginf(np.stack(w)).any() else set()
        st = trail[i][0]
        assert st["dropped_range"] == st["candidates"] == (i + 1) * len(pix) and st["size"] == 0
        assert len(H.table_keys(sims[i])) == 0
    assert kinds == {"nan", "+inf", "-inf"}


def row_figures(name):
    """(keys, load, longest run, carried over the end, most keys on one home) of a row's final table."""
    c, snap = H.case(name), H.sim(name)[-1]
    slots = H.case_slots(c)
    keys = H.table_keys(snap)
    load, run = H.runs(snap["keys"] != u64(H.EMPTY))
    share, carried = H.home_stats(keys.tolist(), slots)
    return len(keys), slots, round(load, 4), run, carried, share


# per row: keys, slots, load, longest run of occupied slots, keys carried over the table's end, most keys that share a home
FIGURES = {
    "wrap": (256, 1024, 0.25, 256, 252, 68),
    "one_home": (256, 1024, 0.25, 256, 0, 256),
    "ends_at_the_end": (129, 1024, 0.126, 129, 1, 129),
    "repeat_and_extend": (384, 2048, 0.1875, 384, 380, 104),
    "one_voxel": (1, 2048, 0.0005, 1, 0, 1),
    "field_edges": (15, 256, 0.0586, 1, 0, 1),
    "field_neighbours": (16, 4096, 0.0039, 1, 0, 1),
    "fullest_table": (511, 1024, 0.499, 18, 0, 3),
    "not_a_number": (0, 1024, 0.0, 0, 0, 0),
}


@pytest.mark.parametrize("name", H.NAMES)
def test_row_figures(name):
    got = row_figures(name)
    print(f"{name}: keys {got[0]} slots {got[1]} load {got[2]} longest run {got[3]} carried {got[4]} share a home {got[5]}")
    if name == "natural":      # a rendering: printed (DESIGN.md section 9.1 has the figures), held only to the sizing rule's bound
        assert got[1] == 1 << 19 and 0 < got[0] < got[1] // 2 and got[5] <= got[3]
    else:
        assert got == FIGURES[name]


def _observed(name, switch):
    """What a switch is judged by. The probe's switches: the occupied slots, the survivors and the keys never placed. The packing's:
    the survivors and the number of keys (its keys and homes differ on every row by construction, its voxels only where two fall
    together). The payload's: the survivors and the payloads."""
    sims = H.sim(name, switch)
    base = H.sim(name)
    out = []
    for which in (sims, base):
        surv = [s["survivors"] for s in which]
        if switch in ("no_wrap", "stop_at_foreign_key"):
            out.append((surv, [np.nonzero(s["keys"] != u64(H.EMPTY))[0].tolist() for s in which], which[-1]["stuck"]))
        elif switch == "shift_20":
            out.append((surv, [len(H.table_keys(s)) for s in which]))
        else:
            out.append((surv, [np.sort(s["payload"]).tolist() for s in which]))
    return out


@pytest.mark.parametrize("switch", H.SWITCHES)
def test_each_switch_shows_on_exactly_its_rows(switch):
    shows = {name for name in H.NAMES if _observed(name, switch)[0] != _observed(name, switch)[1]}
    assert shows == {name for name in H.NAMES if switch in H.case(name)["classes"]}
    assert len(shows) >= 2


# The small MAP rows of tests/geometry_cases.py with their existing inputs, capacity and voxel: (keys, slots, most keys that share a
# home, keys carried over the table's end, longest run). What the suite reached of the table before these rows.
COVERAGE = {"1x1": (2, 16384, 1, 0, 1), "1x63": (118, 16384, 2, 0, 2), "3x85": (429, 16384, 2, 0, 3), "16x16": (417, 16384, 2, 0, 2),
            "1x257": (446, 16384, 2, 0, 3)}


def test_how_far_the_existing_small_rows_reach_into_the_table():
    import geometry_cases as G
    got = {}
    for r in G.MAP:
        if r["size"][0] * r["size"][1] >= G.MAP_RANDOM_BELOW:
            continue
        c = H.geometry_case(r["size"])
        snap = H.simulate(c)[-1]
        keys = H.table_keys(snap)
        share, carried = H.home_stats(keys.tolist(), H.case_slots(c))
        got[r["name"]] = (len(keys), H.case_slots(c), share, carried, H.runs(snap["keys"] != u64(H.EMPTY))[1])
    print(got)
    assert got == COVERAGE
    assert max(v[3] for v in got.values()) == 0      # none of them carries a key over the table's end


def test_the_read_out_refuses_null():
    from odometry_amd import _lib
    lib = _lib.load()
    restype, argtypes = _lib.SIGNATURES["odo_debug_map_table"]
    assert restype is C.c_int and len(argtypes) == 5
    keys, pay, n = (C.c_ulonglong * 4)(*[7] * 4), (C.c_ulonglong * 4)(*[7] * 4), C.c_ulonglong(7)
    assert lib.odo_debug_map_table(None, 4, keys, pay, C.byref(n)) == -1 and "odo_debug_map_table" in _lib.last_error()
    assert list(keys) == [7] * 4 and list(pay) == [7] * 4 and n.value == 7
    hdr = open(_lib.__file__.replace("odometry_amd/_lib.py", "include/odometry_hip.h")).read()
    assert "TEST ONLY" in hdr[:hdr.index("int odo_debug_map_table(")].rsplit("/*", 1)[1]
    assert "odo_debug_map_table" not in open(_lib.__file__.replace("odometry_amd/_lib.py", "INTEGRATION.md")).read()
