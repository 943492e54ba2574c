"""The map's voxel hash on the device, slot by slot (tests/map_hash_cases.py has the rows, the models and the checks): every row goes
through api.PointMap, and after every insertion the points, records and statistics are RefMap's bit for bit and the table read out by
odo_debug_map_table has the mirror's slot count, the model's keys, every key's first claimant as payload, all ones in every empty
slot, no empty slot between a key's home and its place, the replay's occupied slots and the replay's number of keys below their home.
No tolerance anywhere. Every table here is at most half full (odo_map_create's sizing rule), so every probe ends."""
import ctypes as C

import numpy as np
import pytest

import map_hash_cases as H
from test_gpu_map import assert_same

pytestmark = pytest.mark.gpu
u64 = np.uint64
FILL = 0x0707070707070707


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_ulonglong))


def read_table(m, room):
    """(return code, slot count stored, keys, payload) of odo_debug_map_table with buffers of `room` slots filled with FILL."""
    keys, pay, n = np.full(room, FILL, u64), np.full(room, FILL, u64), C.c_ulonglong(FILL)
    rc = m.lib.odo_debug_map_table(m.h, room, _ptr(keys), _ptr(pay), C.byref(n))
    return rc, n.value, keys, pay


def new_map(ctx, c):
    from odometry_amd import api
    return api.PointMap(ctx, c["size"][0], c["size"][1], c["capacity"], c["voxel"])


def run_row(ctx, name, m=None):
    """Every insertion of a row with every check after each; returns the tables [(keys, payload)] and the map."""
    c, trail, sims = H.case(name), H.ref_trail(name), H.sim(name)
    slots = H.case_slots(c)
    m = m or new_map(ctx, c)
    tables = []
    for i, (val, dep, img, A) in enumerate(c["inputs"]):
        m.insert(val, dep, img, c["K"], A)
        assert_same(m, H.Snapshot(*trail[i]))                                     # 1
        rc, n, keys, pay = read_table(m, slots)
        assert rc == 0 and n == slots                                             # 2
        got = H.check_table(keys, pay, sims[i], slots)                            # 3 .. 7
        load, run = H.runs(keys != u64(H.EMPTY))
        print(f"{name}[{i}]: keys {got['n_keys']} of {slots} slots, load {load:.4f}, longest run {run}, below home {got['carried']}, "
              f"farthest from home {got['longest_probe']}")
        tables.append((keys, pay))
    return tables, m


@pytest.mark.parametrize("name", H.NAMES)
def test_the_table_is_the_models_after_every_insertion(ctx, name):
    tables, m = run_row(ctx, name)
    keys, pay = tables[-1]
    c = H.case(name)
    if name == "one_home":       # all 256 claimants walked the same run: the last of them lies 255 slots from home
        at = np.nonzero(keys != u64(H.EMPTY))[0]
        assert int(((at - H.home(keys[at], len(keys)).astype(np.int64)) & (len(keys) - 1)).max()) == 255
    if name == "ends_at_the_end":
        assert int(keys[0]) == c["designed"][1][0] and int(pay[0]) == (1 << 32) | 77 and np.all(tables[0][0][:512] == u64(H.EMPTY))
    if name == "repeat_and_extend":
        new = np.isin(keys, np.array(c["designed"][1], u64))
        assert np.array_equal(np.nonzero(new)[0], np.arange(252, 380))            # behind every old key
        assert np.array_equal(tables[1][0][~new], tables[0][0][~new]) and np.array_equal(tables[1][1][~new], tables[0][1][~new])
    if name == "fullest_table":  # the third insertion meets a full map
        assert np.array_equal(tables[2][0], tables[1][0]) and np.array_equal(tables[2][1], tables[1][1])
        assert int((keys != u64(H.EMPTY)).sum()) == 511
    if name == "not_a_number":
        assert np.all(keys == u64(H.EMPTY)) and np.all(pay == u64(H.EMPTY))
    m.close()


def test_a_full_map_leaves_the_table_alone_and_clear_empties_it(ctx):
    c, other = H.case("wrap"), H.case("one_home")
    assert (c["size"], c["capacity"], c["voxel"]) == (other["size"], other["capacity"], other["voxel"])
    slots = H.case_slots(c)
    tables, m = run_row(ctx, "wrap")
    st = m.stats()
    assert st["size"] == c["capacity"]
    val, dep, img, A = other["inputs"][0]
    m.insert(val, dep, img, other["K"], A)                       # keys the table does not hold, into a full map
    rc, n, keys, pay = read_table(m, slots)
    assert rc == 0 and np.array_equal(keys, tables[0][0]) and np.array_equal(pay, tables[0][1])
    assert m.stats() == dict(st, insertions=2)
    m.clear()
    rc, n, keys, pay = read_table(m, slots)
    assert rc == 0 and n == slots and np.all(keys == u64(H.EMPTY)) and np.all(pay == u64(H.EMPTY))
    again, _ = run_row(ctx, "one_home", m)                       # the cleared map is a fresh one
    fresh, m2 = run_row(ctx, "one_home")
    for (k0, p0), (k1, p1) in zip(again, fresh):
        assert np.array_equal(k0 != u64(H.EMPTY), k1 != u64(H.EMPTY))
        o0, o1 = np.argsort(k0), np.argsort(k1)                  # which key of a run sits where is the claims' order; the pairs are not
        assert np.array_equal(k0[o0], k1[o1]) and np.array_equal(p0[o0], p1[o1])
    m.close()
    m2.close()


def test_the_read_out_refuses_a_map_without_a_filter_and_a_short_buffer(ctx):
    from odometry_amd import _lib, api
    c = H.case("wrap")
    slots = H.case_slots(c)
    m = new_map(ctx, c)
    val, dep, img, A = c["inputs"][0]
    m.insert(val, dep, img, c["K"], A)
    rc, n, keys, pay = read_table(m, slots - 1)
    assert rc == -1 and "odo_debug_map_table" in _lib.last_error() and n == slots
    assert np.all(keys == u64(FILL)) and np.all(pay == u64(FILL))
    rc, n, keys, pay = read_table(m, slots + 3)                  # more room than slots: the rest stays as it was
    assert rc == 0 and n == slots and np.all(keys[slots:] == u64(FILL)) and np.all(pay[slots:] == u64(FILL))
    H.check_table(keys[:slots], pay[:slots], H.sim("wrap")[0], slots)
    m.close()
    m = api.PointMap(ctx, 16, 16, 256, 0.0)
    m.insert(val, dep, img, c["K"], A)
    rc, n, keys, pay = read_table(m, slots)
    assert rc == -1 and "voxel" in _lib.last_error()
    assert np.all(keys == u64(FILL)) and np.all(pay == u64(FILL))
    assert m.stats()["size"] == 256
    m.close()
