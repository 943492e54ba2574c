"""The pyramid kernels on the GPU against the table of tests/pyramid_cases.py, bit for bit, on all three launch paths: the default one in
this process (the fused kernel, its wide build from 1 024 tiles, the level-by-level kernels above four levels) and, in two fresh child
processes (tests/pyramid_child.py), every row level by level (ODO_PYR_UNFUSED) and every row through the wide build (ODO_PYR_WIDE_FROM=1)
— the library reads the two switches once per process. Then the entry points no other test calls: a strided host image, the
device-buffer constructor, the rebuild of a handle, and the refusals. tests/test_pyramid_cases_cpu.py proves on the CPU that each row
reaches the case it is in the table for and that the oracle, the integer model and the stepwise restatement agree."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import pyramid_cases as PC
import pyramid_child
from pyramid_cases import bits, f32

pytestmark = pytest.mark.gpu
CHILD_TIME_LIMIT = 120       # seconds; a safety cap, not a measurement: the same table takes seconds in this process
_stopped = []                # why nothing more may be started on the GPU (a child faulted, aborted or ran into the cap)


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _stopped:
        pytest.skip(_stopped[0])


@pytest.fixture(scope="module")
def api():
    from odometry_amd import api
    api.default_context()
    return api


@pytest.fixture(scope="module")
def in_process(api):
    """Every level of every row on the default path."""
    t0 = time.perf_counter()
    out = pyramid_child.build_levels(api, PC.TABLE)
    dt = time.perf_counter() - t0
    print(f"\n{len(PC.TABLE)} rows, {len(out)} levels in this process: {dt:.2f} s")      # meant to take seconds
    return out


def _run_child(tmp, tag, switch):
    out = os.path.join(tmp, f"{tag}.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("ODO_PYR_UNFUSED", "ODO_PYR_WIDE_FROM")}
    env.update(switch)
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, os.path.join(PC.ROOT, "tests", "pyramid_child.py"), out], env=env, timeout=CHILD_TIME_LIMIT,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _stopped.append(f"the {tag} child did not finish in {CHILD_TIME_LIMIT} s")
        pytest.fail(_stopped[0])
    if p.returncode != 0:
        why = f"the {tag} child exited with status {p.returncode}"
        if p.returncode < 0 or p.returncode in (134, 139):
            _stopped.append(why)                              # a fault or an abort: nothing further is started
        pytest.fail(why + "\n" + p.stdout[-1500:] + p.stderr[-3000:])
    print(f"\n{tag} child: {time.perf_counter() - t0:.2f} s")
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def children(api, tmp_path_factory):
    """{"unfused": levels, "wide": levels}: the table in two fresh processes, one after the other; the second starts only after the
    first has exited with status 0."""
    tmp = str(tmp_path_factory.mktemp("pyramid_children"))
    unfused = _run_child(tmp, "unfused", {"ODO_PYR_UNFUSED": "1"})
    wide = _run_child(tmp, "wide", {"ODO_PYR_WIDE_FROM": "1"})
    return dict(unfused=unfused, wide=wide)


def differences(got, rows, want=None):
    """Every (row, smooth, level) of `rows` whose bits in `got` differ from the oracle's (or from `want`'s), with the first pixels."""
    out = []
    for r in rows:
        for smooth in PC.SMOOTH:
            ref = PC.reference(r, smooth)
            for l in range(r["levels"]):
                g = got[PC.key(r, smooth, l)]
                w = ref[l] if want is None else want[PC.key(r, smooth, l)]
                if g.shape != w.shape or g.dtype != f32:
                    out.append((r["name"], smooth, l, "shape", g.shape, w.shape))
                elif not np.array_equal(bits(g), bits(w)):
                    ys, xs = np.nonzero(bits(g) != bits(w))
                    out.append((r["name"], smooth, l, len(ys), list(zip(ys[:6].tolist(), xs[:6].tolist()))))
    return out


@pytest.mark.parametrize("group", PC.GROUPS)
def test_every_row_bit_for_bit(in_process, group):
    rows = PC.group_rows(group)
    assert rows
    bad = differences(in_process, rows)
    assert not bad, (len(bad), bad[:8])


def test_both_sides_of_the_wide_threshold(in_process):
    below, at = PC.BY_NAME["threshold-below-992x1056"], PC.BY_NAME["threshold-at-1024x1024"]
    assert PC.n_tiles(*below["size"]) == PC.K["wide_from"] - 1 and PC.n_tiles(*at["size"]) == PC.K["wide_from"]
    assert not differences(in_process, [below, at])
    model = PC.integer_model(PC.image(at), 4)                 # the wide build against the definition itself
    for l in range(3):
        assert np.array_equal(bits(in_process[PC.key(at, l == 0, l)]), bits(model[l])), l


@pytest.mark.parametrize("group", PC.GROUPS)
@pytest.mark.parametrize("path", ["unfused", "wide"])
def test_three_paths_one_set_of_bits(in_process, children, path, group):
    rows = PC.group_rows(group)
    got = children[path]
    bad = differences(got, rows)
    assert not bad, (path, len(bad), bad[:8])
    bad = differences(got, rows, want=in_process)
    assert not bad, (path, "against this process", len(bad), bad[:8])


def test_children_built_every_level(in_process, children):
    assert set(children["unfused"]) == set(children["wide"]) == set(in_process)
    assert len(in_process) == sum(2 * r["levels"] for r in PC.TABLE)


# ---- entry points ----------------------------------------------------------------------------------------------------------------
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _levels(ctx, h):
    n = ctx.lib.odo_pyramid_levels(h)
    out = []
    for l in range(n):
        r, c = C.c_int(0), C.c_int(0)
        assert ctx.lib.odo_pyramid_level_dims(h, l, C.byref(r), C.byref(c)) == 0
        a = np.full((r.value, c.value), 0xABABABAB, np.uint32).view(f32)
        assert ctx.lib.odo_pyramid_download(h, l, _fp(a)) == 0
        out.append(a)
    return out


def _same(got, want):
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (l, g.shape, w.shape)


def _kind(api, r):
    from odometry_amd import _lib
    return _lib.PYR_IMAGE if r["kind"] == "image" else _lib.PYR_DEPTH


ENTRY_ROWS = ("sweep-b-72x" + str(PC.partner(72, 37, 11)), "sweep-c-33x" + str(PC.partner(33, 13, 50)), "deep-b-130x257-l5", "grid-image-5x65",
              "depth-60-72x" + str(PC.partner(72, 37, 11)), "depth-deep-90-130x257-l5", "median-four-zeros-13x67", "grid-depth-3x63")


@pytest.mark.parametrize("name", ENTRY_ROWS)
def test_strided_host_image(api, name):
    """stride_bytes = 4 * (cols + 5), the padding full of 1e30: nothing of it reaches any level."""
    r = PC.BY_NAME[name]
    ctx, img = api.default_context(), PC.image(r)
    rows, cols = img.shape
    padded = np.full((rows, cols + 5), 1e30, f32)
    padded[:, :cols] = img
    for smooth in PC.SMOOTH:
        h = C.c_void_p()
        assert ctx.lib.odo_pyramid_create(ctx.h, _fp(padded), rows, cols, 4 * (cols + 5), r["levels"], int(smooth), _kind(api, r), C.byref(h)) == 0
        got = _levels(ctx, h)
        ctx.lib.odo_pyramid_destroy(h)
        h = C.c_void_p()
        assert ctx.lib.odo_pyramid_create(ctx.h, _fp(np.ascontiguousarray(img)), rows, cols, 4 * cols, r["levels"], int(smooth), _kind(api, r),
                                          C.byref(h)) == 0
        _same(got, _levels(ctx, h))
        ctx.lib.odo_pyramid_destroy(h)
        _same(got, PC.reference(r, smooth))
    assert (padded[:, cols:] == f32(1e30)).all()


@pytest.mark.parametrize("name", ENTRY_ROWS)
def test_device_buffer_constructor_leaves_its_source_alone(api, name):
    r = PC.BY_NAME[name]
    ctx, img = api.default_context(), PC.image(r)
    rows, cols = img.shape
    for smooth in PC.SMOOTH:
        d_src = ctx.upload(img)
        h = C.c_void_p()
        try:
            assert ctx.lib.odo_pyramid_create_dev(ctx.h, d_src, rows, cols, r["levels"], int(smooth), _kind(api, r), C.byref(h)) == 0
            _same(_levels(ctx, h), PC.reference(r, smooth))
            assert np.array_equal(ctx.download(d_src, img.shape, np.uint32), bits(img))
        finally:
            ctx.lib.odo_pyramid_destroy(h)
            ctx.free(d_src)


@pytest.mark.parametrize("name", ENTRY_ROWS)
def test_rebuild_with_a_second_image_and_the_smoothing_flipped(api, name):
    from oracle import oracle as O
    r = PC.BY_NAME[name]
    ctx, first = api.default_context(), PC.image(r)
    rows, cols = first.shape
    second = r["build"](np.random.default_rng(1000 + r["seed"]), rows, cols)
    assert (bits(second) != bits(first)).any()
    d_first, d_second = ctx.upload(first), ctx.upload(second)
    try:
        for smooth in PC.SMOOTH:
            if r["kind"] == "image":
                want = O.image_pyramid(second, r["levels"], not smooth)
            else:
                want = O.depth_pyramid(second, r["levels"], smooth=not smooth)
            h, fresh = C.c_void_p(), C.c_void_p()
            assert ctx.lib.odo_pyramid_create_dev(ctx.h, d_first, rows, cols, r["levels"], int(smooth), _kind(api, r), C.byref(h)) == 0
            _same(_levels(ctx, h), PC.reference(r, smooth))
            assert ctx.lib.odo_pyramid_rebuild_dev(h, d_second, int(not smooth)) == 0
            got = _levels(ctx, h)
            assert ctx.lib.odo_pyramid_create_dev(ctx.h, d_second, rows, cols, r["levels"], int(not smooth), _kind(api, r), C.byref(fresh)) == 0
            _same(got, _levels(ctx, fresh))
            _same(got, want)
            assert ctx.lib.odo_pyramid_rebuild_dev(h, d_first, int(smooth)) == 0          # and back again
            _same(_levels(ctx, h), PC.reference(r, smooth))
            ctx.lib.odo_pyramid_destroy(h)
            ctx.lib.odo_pyramid_destroy(fresh)
        assert np.array_equal(ctx.download(d_second, second.shape, np.uint32), bits(second))
    finally:
        ctx.free(d_first)
        ctx.free(d_second)


def test_refusals_return_minus_one_and_the_context_stays_usable(api):
    from odometry_amd import _lib
    from oracle import oracle as O
    ctx = api.default_context()
    lib = ctx.lib
    img = PC.mantissa(np.random.default_rng(5), 8, 8)
    d_img = ctx.upload(img)

    def works():
        h = C.c_void_p()
        assert lib.odo_pyramid_create(ctx.h, _fp(img), 8, 8, 0, 4, 1, _lib.PYR_IMAGE, C.byref(h)) == 0
        lv = _levels(ctx, h)
        assert [a.shape for a in lv] == [(8, 8), (4, 4), (2, 2), (1, 1)]              # a 1 x 1 last level is a level
        _same(lv, O.image_pyramid(img, 4, True))
        lib.odo_pyramid_destroy(h)

    def refused(text, rows, cols, stride, levels, kind=None):
        for dev in (False, True):
            if dev and stride:
                continue
            h = C.c_void_p()
            k = _lib.PYR_IMAGE if kind is None else kind
            if dev:
                rc = lib.odo_pyramid_create_dev(ctx.h, d_img, rows, cols, levels, 1, k, C.byref(h))
            else:
                rc = lib.odo_pyramid_create(ctx.h, _fp(img), rows, cols, stride, levels, 1, k, C.byref(h))
            assert rc == -1 and not h.value, (text, dev)
            assert text in _lib.last_error(), (text, _lib.last_error())
        works()

    try:
        works()
        refused("too small for 4 levels", 7, 8, 0, 4)                 # 7 -> 3 -> 1 -> 0: a 0-sized last level is not a level
        refused("too small for 4 levels", 8, 7, 0, 4)
        refused("levels 0 out of range", 8, 8, 0, 0)
        refused("levels 9 out of range", 8, 8, 0, 9)
        refused("bad size 0x8", 0, 8, 0, 1)
        refused("bad size 8x0", 8, 0, 0, 1)
        refused("stride smaller than a row", 8, 8, 4 * 8 - 4, 4)
        refused("bad kind", 8, 8, 0, 4, kind=7)
        # 7 x 8 at three levels ends in 1 x 2 and is accepted, on both kinds
        for kind, ref in ((_lib.PYR_IMAGE, O.image_pyramid(img[:7], 3, False)), (_lib.PYR_DEPTH, O.depth_pyramid(img[:7], 3))):
            h = C.c_void_p()
            assert lib.odo_pyramid_create(ctx.h, _fp(np.ascontiguousarray(img[:7])), 7, 8, 0, 3, 0, kind, C.byref(h)) == 0
            lv = _levels(ctx, h)
            assert lv[2].shape == (1, 2)
            _same(lv, ref)
            lib.odo_pyramid_destroy(h)
        assert lib.odo_pyramid_rebuild_dev(None, d_img, 1) == -1
    finally:
        ctx.free(d_img)
