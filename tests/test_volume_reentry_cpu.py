"""The re-entry store of the moving TSDF volume (odo_volume_enable_reentry, _reentry_voxels, _reentry_stats; api.TsdfVolume.
enable_reentry / stored_voxels / reentry_stats) without a GPU: the ABI and the refusals, the numpy model of the specification
(include/odometry_hip.h) pinned to the prose by a plain-loop version, its properties (round trip, closed
walk, invariant, the non-zero-bit predicate, the capacity cuts), the shared header as a stand-alone program under sanitizers, and the
kernels' code-object metadata. The model is the yardstick of tests/test_gpu_volume_reentry.py, which asks the GPU for the same bits."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import volume_reentry_cases as R
from test_volume_cpu import words
from test_volume_shift_cpu import MAX_OFF, leaves_model, shift_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["odo_volume_enable_reentry", "odo_volume_reentry_voxels", "odo_volume_reentry_stats", "odo_volume_reentry_time",
               "odo_debug_volume_reentry_guard"]
REENTRY_KERNELS = ["volume_reentry_save_count_kernel", "volume_reentry_save_scan_kernel", "volume_reentry_save_scatter_kernel",
                   "volume_reentry_store_count_kernel", "volume_reentry_store_scan_kernel", "volume_reentry_compact_kernel",
                   "volume_reentry_advance_kernel"]
BIG = 1 << 20


def _grids_equal(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and tuple(a[3]) == tuple(b[3])


# ---- ABI and refusals ------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from odometry_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "odometry_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} not declared"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert hasattr(lib, name), f"{name} not exported"
    for name in ("enable_reentry", "stored_voxels", "reentry_stats", "reentry_time"):
        assert callable(getattr(api.TsdfVolume, name))
    assert "volume_reentry_kernels.hip" in [os.path.basename(s) for s, _ in __import__("odometry_amd.build", fromlist=["x"]).UNITS]


def test_bad_arguments_are_refused_before_touching_a_device():
    """Every case below is refused by the validation alone: the volume's handle is a fake that is never dereferenced."""
    from odometry_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(8)
    d = (C.c_int * 3)(1, 0, 0)
    n = C.c_long(0)
    buf = np.zeros(8, np.uint32)
    up = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    ip = buf.ctypes.data_as(C.POINTER(C.c_int32))
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    for cap in (0, -1, (1 << 28) + 1):
        assert lib.odo_volume_enable_reentry(fake, cap) == -1 and "capacity" in L.last_error(), cap
        assert re.fullmatch(r"odo_volume_enable_reentry: capacity -?\d+ out of range \(1 \.\. 2\^28\)", L.last_error())
    assert lib.odo_volume_enable_reentry(None, 16) == -1 and L.last_error() == "odo_volume_enable_reentry: NULL volume"
    assert lib.odo_volume_reentry_voxels(None, 1, ip, up, None, C.byref(n), 0) == -1
    assert lib.odo_volume_reentry_voxels(fake, 1, ip, up, None, None, 0) == -1             # no n
    assert lib.odo_volume_reentry_voxels(fake, -1, ip, up, None, C.byref(n), 0) == -1
    assert lib.odo_volume_reentry_voxels(fake, (1 << 28) + 1, ip, up, None, C.byref(n), 0) == -1
    assert lib.odo_volume_reentry_voxels(fake, 2, None, up, None, C.byref(n), 0) == -1      # a capacity without its buffers
    assert lib.odo_volume_reentry_voxels(fake, 2, ip, None, None, C.byref(n), 0) == -1
    assert "odo_volume_reentry_voxels" in L.last_error()
    assert lib.odo_volume_reentry_stats(None, (C.c_long * 4)()) == -1 and lib.odo_volume_reentry_stats(fake, None) == -1
    assert lib.odo_volume_reentry_time(None, d, 1, fp) == -1 and lib.odo_volume_reentry_time(fake, None, 1, fp) == -1
    assert lib.odo_volume_reentry_time(fake, d, 1, None) == -1
    for reps in (0, -1, 10001):
        assert lib.odo_volume_reentry_time(fake, d, reps, fp) == -1 and "reps" in L.last_error(), reps
    assert lib.odo_debug_volume_reentry_guard(None, C.byref(n), C.byref(n)) == -1
    assert lib.odo_debug_volume_reentry_guard(fake, None, C.byref(n)) == -1 and lib.odo_debug_volume_reentry_guard(fake, C.byref(n), None) == -1
    assert tuple(d) == (1, 0, 0)


# ---- the model against the prose ---------------------------------------------------------------------------------------------------
def test_vectorised_model_equals_the_loop_model_bit_for_bit():
    """7 grids x 14 shifts, each a closed walk d, e, -d, -e, with and without colour: grid, colour grid, window, store in order and
    counters after every shift; the invariant after every shift; and the walk ends where it began with an empty store."""
    met = dict(rows=0, restores=0, keeps=0, all_three=0, nothing_stays=0, saved_for_bits=0)
    for name, n, p, q, w, col, shifts in R.rows():
        for colour in (True, False):
            c = col if colour else None
            got = R.walk_model(q, w, c, shifts, BIG)
            ref = R.walk_model(q, w, c, shifts, BIG, step=R.reentry_loop)
            before = got[0]
            for d, a, b in zip(shifts, got[1:], ref[1:]):
                assert _grids_equal(a, b) and R.stores_equal(a[4], b[4]), (name, n, colour, d)
                assert R.invariant_holds(a[4], a[3], p["dims"]), (name, n, d)
                res, kept = a[4]["restored"] - before[4]["restored"], before[4]["live"] - (a[4]["restored"] - before[4]["restored"])
                sav = a[4]["saved"] - before[4]["saved"]
                met["restores"] += int(res > 0)
                met["keeps"] += int(kept > 0)
                met["all_three"] += int(res > 0 and kept > 0 and sav > 0)
                met["nothing_stays"] += int(any(abs(x) >= m for x, m in zip(d, p["dims"])))
                assert a[4]["live"] == a[4]["saved"] - a[4]["restored"] and a[4]["dropped"] == 0
                before = a
            end = got[-1]
            assert _grids_equal(end, got[0]) and end[4]["live"] == 0 and end[3] == (0, 0, 0), (name, n, colour)
            # the predicate tests bits, not the weight
            W = words(q, w)
            met["saved_for_bits"] += int(((w.reshape(-1) == 0) & (W != 0)).sum())
            met["rows"] += 1
    print(met)
    assert met["rows"] == 7 * 14 * 2 and all(v > 0 for v in met.values()), met


def test_without_the_store_the_same_calls_leave_zeros_in_the_slabs():
    """What the feature changes: d then -d with shift_model alone loses the slab, with the store it does not."""
    p, q, w, col = R.grids()["random 64x4x4"]
    d = (3, 0, 0)
    q1, w1, c1 = shift_model(*shift_model(q, w, col, d), R.neg(d))
    assert not np.array_equal(w1, w) and not w1[:, :, :3].any() and not c1[:, :, :3].any()
    end = R.walk_model(q, w, col, [d, R.neg(d)], BIG)[-1]
    assert _grids_equal(end, (q, w, col, (0, 0, 0))) and end[4]["live"] == 0 and end[4]["saved"] == end[4]["restored"] > 0


def test_a_closed_walk_restores_every_bit_and_empties_the_store():
    """Seven shifts that mix axes and signs, one of them by a whole grid height (nothing stays), back at off = 0."""
    for name in ("random 64x4x4", "random 65x5x4"):
        p, q, w, col = R.grids()[name]
        assert any(abs(d[1]) >= p["dims"][1] for d in R.CLOSED_WALK) or name != "random 64x4x4"
        st = R.walk_model(q, w, col, R.CLOSED_WALK, BIG)
        for s in st[1:]:
            assert R.invariant_holds(s[4], s[3], p["dims"])
        assert max(s[4]["live"] for s in st) > 0
        end = st[-1]
        assert _grids_equal(end, st[0]) and end[4]["live"] == 0 and end[4]["dropped"] == 0, name
        # and the long chain out and back
        ch = R.walk_model(q, w, col, R.CHAIN, BIG)
        assert _grids_equal(ch[-1], ch[0]) and ch[-1][4]["live"] == 0 and ch[24][3] == (24, 0, 0)


def test_a_voxel_is_saved_for_any_non_zero_bit_and_not_when_all_zero():
    p, q, w, col = R.grids()["random 2x2x2"]
    q, w, col = np.zeros_like(q), np.zeros_like(w), np.zeros_like(col)
    q[0, 0, 0] = -7                      # w = 0, q != 0
    col[0, 1, 0, 2] = 9                  # only a colour bit
    w[1, 0, 0] = 3                       # observed, q = 0
    d = (2, 0, 0)                        # every voxel leaves
    s = R.reentry_model(q, w, col, (0, 0, 0), R.empty_store(True), d, 64)[4]
    assert s["g"].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 1]] and s["vox"].tolist() == [0xFFF9, 0, 3 << 16]
    assert s["col"].tolist() == [0, 9 << 16, 0] and s["live"] == s["saved"] == 3
    # without a colour grid the colour-only voxel is all zero
    s = R.reentry_model(q, w, None, (0, 0, 0), R.empty_store(False), d, 64)[4]
    assert s["g"].tolist() == [[0, 0, 0], [0, 0, 1]] and s["col"] is None
    # and the round trip gives the uploaded bits back
    end = R.walk_model(q, w, col, [d, R.neg(d)], 64)[-1]
    assert _grids_equal(end, (q, w, col, (0, 0, 0)))


def test_capacity_cuts_only_the_tail_of_the_newly_saved_entries():
    p, q, w, col = R.grids()["random 64x4x4"]
    shifts, n1, n2, caps = R.capacity_rows()
    full = R.walk_model(q, w, col, shifts, BIG)[-1][4]
    want_dropped = [0, 0, 1, n1 + n2 - 1, n2 - n2 // 2]
    for cap, dropped in zip(caps, want_dropped):
        st = R.walk_model(q, w, col, shifts, cap)
        s = st[-1][4]
        m = min(cap, n1 + n2)
        assert s["live"] == m and s["dropped"] == dropped and s["saved"] == m, (cap, s["live"], s["dropped"])
        assert np.array_equal(s["g"], full["g"][:m]) and np.array_equal(s["vox"], full["vox"][:m]) and np.array_equal(s["col"], full["col"][:m])
        ref = R.walk_model(q, w, col, shifts, cap, step=R.reentry_loop)[-1][4]
        assert R.stores_equal(s, ref), cap
        assert R.invariant_holds(s, st[-1][3], p["dims"])
    # inside the second shift: the first shift's entries are all kept
    s = R.walk_model(q, w, col, shifts, caps[4])
    assert s[1][4]["dropped"] == 0 and s[2][4]["dropped"] > 0


def test_restore_keep_and_save_are_all_non_empty_in_one_shift():
    p, q, w, col = R.grids()["random 64x4x4"]
    st = R.walk_model(q, w, col, R.MIXED, BIG)
    a, b = st[2][4], st[3][4]
    restored, saved = b["restored"] - a["restored"], b["saved"] - a["saved"]
    kept = a["live"] - restored
    assert restored > 0 and kept > 0 and saved > 0, (restored, kept, saved)
    assert np.array_equal(b["g"][:kept], a["g"][~_inside(a["g"], st[3][3], p["dims"])])      # the kept entries, in their order
    ref = R.walk_model(q, w, col, R.MIXED, BIG, step=R.reentry_loop)
    assert all(_grids_equal(x, y) and R.stores_equal(x[4], y[4]) for x, y in zip(st, ref))


def _inside(g, off, dims):
    t = g - np.array(off, np.int64)
    return ((t >= 0) & (t < np.array(dims, np.int64))).all(1)


def test_a_store_without_colours_on_a_coloured_volume_gives_colour_word_zero_back():
    p, q, w, col = R.grids()["random 65x5x4"]
    d = (4, 0, -1)
    st = R.walk_model(q, w, col, [d, R.neg(d)], BIG, store_colour=False)
    ref = R.walk_model(q, w, col, [d, R.neg(d)], BIG, store_colour=False, step=R.reentry_loop)
    assert all(_grids_equal(x, y) and R.stores_equal(x[4], y[4]) for x, y in zip(st, ref))
    assert st[1][4]["col"] is None
    q2, w2, c2 = st[-1][:3]
    lv = leaves_model(q.shape, d)
    assert np.array_equal(q2, q) and np.array_equal(w2, w)
    assert np.array_equal(c2[~lv], col[~lv]) and not c2[lv].any() and col[lv].any()
    # a voxel with colour bits only is still saved (the predicate reads the volume's colour grid) and comes back all zero
    only = (words(q, w).reshape(q.shape) == 0) & col.any(-1) & lv
    assert only.any() and st[1][4]["live"] == int(((words(q, w).reshape(q.shape) != 0) | col.any(-1))[lv].sum())


# ---- the shared header under sanitizers ----------------------------------------------------------------------------------------------
def _step_blob(q, w, col, off, store, d, capacity):
    nz, ny, nx = q.shape
    m = len(store["g"])
    head = np.array([nx, ny, nz, *d, *off, capacity, m, int(col is not None), int(store["col"] is not None)], "<i4")
    return head.tobytes() + words(q, w).astype("<u4").tobytes() + (R.colour_words(col).astype("<u4").tobytes() if col is not None else b"") + \
        store["g"].astype("<i4").tobytes() + store["vox"].astype("<u4").tobytes() + \
        (store["col"].astype("<u4").tobytes() if store["col"] is not None else b"")


def _step_parse(blob, shape, colour, store):
    n = int(np.prod(shape))
    at = 4 * n
    W2 = np.frombuffer(blob[:at], "<u4")
    q2, w2 = R.unwords(W2, shape)
    c2 = None
    if colour:
        c2 = np.frombuffer(blob[at:at + 4 * n], np.uint8).reshape(shape + (4,))
        at += 4 * n
    m2, restored, saved, dropped = (int(x) for x in np.frombuffer(blob[at:at + 16], "<i4"))
    at += 16
    g = np.frombuffer(blob[at:at + 12 * m2], "<i4").reshape(-1, 3).astype(np.int64)
    at += 12 * m2
    vox = np.frombuffer(blob[at:at + 4 * m2], "<u4")
    at += 4 * m2
    cw = np.frombuffer(blob[at:at + 4 * m2], "<u4") if store["col"] is not None else None
    assert len(blob) == at + (4 * m2 if cw is not None else 0)
    return q2, w2, c2, dict(g=g, vox=vox, col=cw, live=m2, saved=store["saved"] + saved, restored=store["restored"] + restored,
                            dropped=store["dropped"] + dropped)


def test_shared_header_equals_the_loop_model_under_sanitizers(tmp_path):
    """odometry_amd/csrc/volume_shift_math.h — the lines the device and the library compile — as a stand-alone g++ program with
    AddressSanitizer and UBSan: every shift of every row's walk against the loop model, windows at +-2^24, a capacity cut, a store
    without colours, and the key arithmetic with off, g and the window at +-2^31 and +-2^24, all byte for byte."""
    exe = str(tmp_path / "volume_reentry_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "volume_reentry_harness.cpp"), "-o", exe])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")

    def run(mode, blob):
        open(src, "wb").write(blob)
        out = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout[-1500:] + out.stderr[-3000:]
        return open(dst, "rb").read()

    def walk(q, w, col, shifts, capacity, off, store_colour, tag):
        store = R.empty_store(store_colour)
        for d in shifts:
            want = R.reentry_loop(q, w, col, off, store, d, capacity)
            got = _step_parse(run("step", _step_blob(q, w, col, off, store, d, capacity)), q.shape, col is not None, store)
            assert _grids_equal(got[:3] + (want[3],), want) and R.stores_equal(got[3], want[4]), (tag, d)
            q, w, col, off, store = want

    n_rows = 0
    for name, n, p, q, w, col, shifts in R.rows():
        colour = n % 2 == 0
        walk(q, w, col if colour else None, shifts, BIG, (0, 0, 0), colour, (name, n))
        n_rows += 1
    assert n_rows == 98
    p, q, w, col = R.grids()["random 65x5x4"]
    for off in ((MAX_OFF - 5, -MAX_OFF, MAX_OFF - 1), (-MAX_OFF + 7, MAX_OFF - 2, -MAX_OFF)):
        first = tuple(-5 if o > 0 else 5 for o in off)      # away from the bound and back to it
        walk(q, w, col, [first, (first[0] // 5, first[1] // 5, 0), R.neg(first)], BIG, off, True, off)
    shifts, n1, n2, caps = R.capacity_rows()
    p, q, w, col = R.grids()["random 64x4x4"]
    for cap in caps:
        walk(q, w, col, shifts, cap, (0, 0, 0), True, cap)
    walk(q, w, col, R.MIXED, BIG, (0, 0, 0), False, "no colours in the store")
    walk(q, w, col, R.CLOSED_WALK, BIG, (3, -MAX_OFF + 9, 1), True, "closed walk")
    # the key arithmetic at the edges of int
    edge = [-2 ** 31, -2 ** 31 + 1, -MAX_OFF - 1, -MAX_OFF, -1, 0, 1, 63, MAX_OFF, MAX_OFF + 64, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1]
    rng = np.random.default_rng(3)
    recs = [(o, i, g, o2, n) for o in edge for i in (0, 1, 2 ** 30 - 1) for g in edge for o2 in (edge[0], edge[3], 0, edge[8], edge[-1])
            for n in (2, 65, 2 ** 30)]
    recs += [tuple(int(x) for x in rng.integers(-2 ** 31, 2 ** 31, 4)) + (int(rng.integers(2, 2 ** 30)),) for _ in range(2000)]
    arr = np.array(recs, "<i4")
    got = np.frombuffer(run("keys", np.array([len(arr)], "<i4").tobytes() + arr.tobytes()),
                        np.dtype([("glob", "<i8"), ("inside", "<i4"), ("t", "<i4")]))
    a = arr.astype(np.int64)
    t = a[:, 2] - a[:, 3]
    inside = (t >= 0) & (t < a[:, 4])
    assert np.array_equal(got["glob"], a[:, 0] + a[:, 1])
    assert np.array_equal(got["inside"], inside.astype(np.int32)) and np.array_equal(got["t"], np.where(inside, t, 0).astype(np.int32))
    assert inside.sum() > 20 and (~inside).sum() > 20 and (np.abs(got["glob"]) > 2 ** 31).any()


# ---- code object -------------------------------------------------------------------------------------------------------------------
def test_reentry_kernels_are_in_the_gfx950_code_object_without_spills_or_scratch():
    from odometry_amd import _lib
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools here")
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "lib.so")
        shutil.copy(_lib.LIB_PATH, so)
        subprocess.run([os.path.join(llvm, "llvm-objdump"), "--offloading", so], cwd=td, check=True, capture_output=True)
        notes = ""
        for f in sorted(os.listdir(td)):
            if "gfx950" in f:
                notes += subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", os.path.join(td, f)], check=True,
                                        capture_output=True, text=True).stdout
    found = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        for k in REENTRY_KERNELS:
            if k in name:
                found.setdefault(k, []).append((int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                                                int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))))
                print(name, "vgprs", re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1), "sgprs", re.search(r"\.sgpr_count:\s+(\d+)", blk).group(1))
    assert sorted(found) == sorted(REENTRY_KERNELS), found
    assert all(len(v) == 1 and v[0] == (0, 0) for v in found.values()), found
