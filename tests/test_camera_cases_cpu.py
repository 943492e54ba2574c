"""The camera model's map and remap (camera_math.h) without a GPU: every row of tests/camera_cases.py reaches
the case it is in the table for; the oracle, the plain-loop model and the vectorised model agree (bit for bit on the exact-grid and
non-representable rows, within derived bounds on the realistic ones); the oracle's maps against exact rational arithmetic; the shared
header odometry_amd/csrc/camera_math.h — the lines the device compiles — and the oracle's camera model as stand-alone programs under
AddressSanitizer and UBSan with float-cast-overflow; and mutants of the header, each caught by the row named for it.

The oracle and the models are the yardsticks of tests/test_gpu_camera_cases.py, which asks the GPU for the same bits."""
import os
import subprocess

import numpy as np
import pytest

import camera_cases as CC
from camera_cases import f32, f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "odometry_amd", "csrc", "camera_math.h")
SANITIZE = ["-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all"]
MAP_REC = np.dtype([("raw", "<f8", 5), ("dist", "<f8", 4), ("R", "<f8", 9), ("P", "<f8", 12), ("rows", "<i4"), ("cols", "<i4")])
REMAP_HEAD = np.dtype([("srows", "<i4"), ("scols", "<i4"), ("drows", "<i4"), ("dcols", "<i4"), ("border", "<f4")])
IDS = dict(ids=lambda r: r["name"])


def rows_of(*groups):
    return [r for r in CC.TABLE if r["group"] in groups]


# ---- the table reaches what it claims -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", CC.TABLE, **IDS)
def test_every_row_reaches_the_case_it_is_there_for(r):
    _, t = CC.loop_output(r)
    assert t["n"] == CC.pixels(r) == t["fits"] + t["nonrep"]
    assert r["predicate"](t), (r["name"], {k: v for k, v in t.items() if v})


def test_table_covers_the_issue_list():
    names = set(CC.BY_NAME)
    assert {(r["size"]) for r in rows_of("geom")} >= set(CC.GEOMETRY_SIZES)
    assert {r["source"][1:3] for r in rows_of("geom")} >= set(CC.GEOMETRY_SOURCES)
    for r in rows_of("exact"):
        assert r["border"] in (17.0, -7.0) and not (CC.source(r) == r["border"]).any() and CC.source(r).min() >= 1
        assert np.array_equal(CC.source(r), np.rint(CC.source(r)))
    for r in rows_of("nonrep"):
        assert f32(r["border"]) == f32(1.0) / f32(3.0)
    total = dict.fromkeys(CC.TALLIES, 0)
    for r in rows_of("nonrep"):
        for k, v in CC.loop_output(r)[1].items():
            total[k] += v
    for k in ("nan_x", "nan_y", "pinf_x", "ninf_x", "pinf_y", "ninf_y", "over_pos_x", "over_neg_x"):
        assert total[k] > 0, (k, total)
    assert {"euroc", "barrel", "rotated-2deg", "shift-right-up", "shift-left-down", "half-focal"} <= names
    sizes = {(r["source"][1] * r["source"][2] > CC.pixels(r)) - (r["source"][1] * r["source"][2] < CC.pixels(r)) for r in rows_of("real")}
    assert sizes == {-1, 0, 1}                                              # sources smaller than, equal to and larger than the view


def test_projective_maps_hold_every_class():
    """On the oracle's maps of the projective rows together: NaN, +inf and -inf in x and in y; each row's column 8 is at the horizon and
    its entry (8, 0) is NaN."""
    seen = {"x": set(), "y": set()}
    for name in ("projective", "projective-mirrored"):
        mx, my = CC.oracle_maps(CC.BY_NAME[name])
        assert np.isnan(mx[0, 8]) and np.isnan(my[0, 8])
        assert np.isinf(mx[1:, 8]).all() and np.isinf(my[1:, 8]).all()
        assert np.isfinite(np.delete(mx, 8, axis=1)).all() and np.isfinite(np.delete(my, 8, axis=1)).all()
        seen["x"] |= set(CC.classes(mx).ravel().tolist())
        seen["y"] |= set(CC.classes(my).ravel().tolist())
    assert seen["x"] == seen["y"] == {0, 1, 2, 3}
    mx, my = CC.oracle_maps(CC.BY_NAME["nan-y-only"])
    assert np.isnan(my[3]).all() and not np.isnan(mx).any() and CC.fits(mx).all()


@pytest.mark.parametrize("r", rows_of("exact", "geom"), **IDS)
def test_exact_grid_maps_are_the_closed_form(r):
    """map_x = (u - ox) * 64 / P fx and map_y = (v - oy) * 64 / P fy with no rounding anywhere: the oracle's fp32 maps equal the
    formula evaluated in float64 (dyadic numbers of a few bits)."""
    mx, my = CC.oracle_maps(r)
    cols, rows = r["size"]
    s = 64.0 / r["P"][0, 0]
    assert np.array_equal(mx.astype(f64), np.broadcast_to((np.arange(cols) - r["P"][0, 2]) * s, (rows, cols)))
    assert np.array_equal(my.astype(f64), np.broadcast_to(((np.arange(rows) - r["P"][1, 2]) * s)[:, None], (rows, cols)))


# ---- oracle = loop = model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", CC.TABLE, **IDS)
def test_oracle_equals_the_loop_and_the_models(r):
    """Bit for bit: the oracle against the plain loop and against the float64 model with fp32's roundings, on every row; against the
    float64 model WITHOUT intermediate roundings on every pixel of the exact-grid, geometry and non-representable rows whose value does
    not weigh the float32(1/3) border (whole-number sources, weights k / 1024: every product and sum is exact)."""
    src, (mx, my), want = CC.source(r), CC.oracle_maps(r), CC.oracle_output(r)
    loop, _ = CC.loop_output(r)
    assert CC.same_floats(loop, want), int((CC.bits(loop) != CC.bits(want)).sum())
    assert CC.same_floats(CC.remap_model(src, mx, my, r["border"], rounded=True), want)
    if r["group"] != "real":
        model = CC.remap_model(src, mx, my, r["border"])
        inexact = CC.border_weighted(src.shape, mx, my) if r["group"] == "nonrep" else np.zeros(mx.shape, bool)
        assert np.array_equal(CC.bits(model)[~inexact], CC.bits(want)[~inexact])
        if r["group"] == "nonrep":
            bad = ~(CC.fits(mx) & CC.fits(my))
            assert bad.any() and (CC.bits(want)[bad] == CC.bits(f32(r["border"]))).all()       # the border value itself
            assert not inexact[bad].any()


@pytest.mark.parametrize("r", rows_of("real"), **IDS)
def test_realistic_rows_lie_within_the_derived_bound_of_the_float64_model(r):
    """|fp32 chain - exact| <= 7 * 2^-24 * M, M = max(|src|, |border|). The weights are products of multiples of 1/32 below 1: exact in
    fp32, non-negative, summing to 1. Each of the four products s_i * w_i is rounded once: an error of at most 2^-24 * M * w_i,
    2^-24 * M together. Each of the three sums is rounded once; every partial sum of the computed products is at most M (1 + 2^-23) in
    magnitude: 3 * 2^-24 * M (1 + 2^-23). That is 4 * 2^-24 * M and second-order terms; 7 * 2^-24 * M with the float64 model's own
    2^-50 * M to spare. Not fitted: the measured worst case is printed."""
    src, (mx, my), want = CC.source(r), CC.oracle_maps(r), CC.oracle_output(r)
    model = CC.remap_model(src, mx, my, r["border"], out64=True)
    M = max(float(np.abs(src).max()), abs(r["border"]))
    err = float(np.abs(want.astype(f64) - model).max())
    print(f"{r['name']}: worst |oracle - float64 model| = {err:.3e} = {err / (2.0 ** -24 * M):.3f} * 2^-24 * max|src|, bound 7")
    assert err <= 7 * 2.0 ** -24 * M


# ---- the oracle's maps against exact arithmetic -----------------------------------------------------------------------------------------
EXACT_ROWS = [r for r in CC.TABLE if CC.pixels(r) <= CC.EXACT_LIMIT and np.isfinite(r["raw"]).all() and r["group"] != "geom"]


@pytest.mark.parametrize("r", EXACT_ROWS, **IDS)
def test_oracle_maps_against_exact_rational_arithmetic(r):
    """The bound is maps_exact's (derived there). Entries with |_w| < 0.5 are compared by class only."""
    mx, my = CC.oracle_maps(r)
    cols, rows = r["size"]
    ex, ey, bx, by, ws = CC.maps_exact(r["raw"], r["dist"], r["R"], r["P"], rows, cols)
    worst, equal, n = 0.0, 0, 0
    for v in range(rows):
        for u in range(cols):
            for got, q, b in ((mx[v, u], ex[v][u], bx[v][u]), (my[v, u], ey[v][u], by[v][u])):
                if q is None:
                    assert abs(ws[v][u]) < 0.5
                    if ws[v][u] == 0.0:
                        assert not np.isfinite(got), (u, v, got)
                    continue
                if abs(q) >= CC.Fr(2) ** 128:                                # beyond fp32: the class is +-inf
                    assert got == (np.inf if q > 0 else -np.inf), (u, v, got)
                    continue
                assert np.isfinite(got), (u, v, got)
                d = abs(CC.Fr(float(got)) - q)
                assert d <= b, (r["name"], u, v, float(got), float(q), float(d), float(b))
                worst = max(worst, float(d / CC.ulp32(q)))
                equal += int(f32(got).view(np.uint32) == CC.round32(q).view(np.uint32))
                n += 1
    print(f"{r['name']}: {n} entries, worst |oracle - exact| = {worst:.4f} ulp32, bit-equal to the rounded exact value: {equal} ({100.0 * equal / max(n, 1):.2f} %)")
    if r["group"] == "exact":
        assert worst == 0.0 and equal == n


# ---- the stand-alone programs ------------------------------------------------------------------------------------------------------------
def build_math_harness(exe, header=None, sanitize=SANITIZE):
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off"] + sanitize
    if header:
        cmd.append('-DCAMERA_MATH_H="%s"' % header)
    return subprocess.Popen(cmd + [os.path.join(ROOT, "tests", "camera_math_harness.cpp"), "-o", exe])


@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    """(the camera_math.h program, the oracle program), both with ASan + UBSan + float-cast-overflow."""
    d = tmp_path_factory.mktemp("camera_harness")
    a, b = str(d / "camera_math_harness"), str(d / "camera_oracle_harness")
    pa = build_math_harness(a)
    pb = subprocess.Popen(["gcc", "-O1", "-g", "-std=c99", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-fast-math"] + SANITIZE +
                          [os.path.join(ROOT, "tests", "camera_oracle_harness.c"), os.path.join(ROOT, "oracle", "odo_oracle.c"), "-o", b, "-lm"])
    assert pa.wait() == 0 and pb.wait() == 0
    return a, b, d


def run_maps(exe, d, rows):
    """[(status, mapx, mapy)] of the program for the rows; (returncode, text) on a failure."""
    rec = np.zeros(len(rows), MAP_REC)
    for i, r in enumerate(rows):
        rec["raw"][i], rec["dist"][i], rec["R"][i], rec["P"][i] = r["raw"], r["dist"], r["R"].reshape(9), r["P"].reshape(12)
        rec["rows"][i], rec["cols"][i] = r["size"][1], r["size"][0]
    src, dst = str(d / "maps_in.bin"), str(d / "maps_out.bin")
    rec.tofile(src)
    out = subprocess.run([exe, "maps", src, dst], capture_output=True, text=True, timeout=120)
    if out.returncode != 0 or not out.stdout.strip().endswith("OK"):
        return out.returncode, out.stdout[-500:] + out.stderr[-3000:]
    raw = np.fromfile(dst, np.uint8)
    res, at = [], 0
    for r in rows:
        st = int(raw[at:at + 4].view("<i4")[0])
        at += 4
        n = CC.pixels(r)
        if st == 0:
            m = raw[at:at + 8 * n].view("<f4").reshape(2, r["size"][1], r["size"][0])
            at += 8 * n
            res.append((st, m[0], m[1]))
        else:
            res.append((st, None, None))
    assert at == len(raw)
    return res


def run_remap(exe, d, jobs):
    """jobs: [(src, mapx, mapy, border)] -> [dst]; (returncode, text) on a failure."""
    src_path, dst_path = str(d / "remap_in.bin"), str(d / "remap_out.bin")
    with open(src_path, "wb") as f:
        for s, mx, my, border in jobs:
            h = np.zeros(1, REMAP_HEAD)
            h["srows"], h["scols"], h["drows"], h["dcols"], h["border"] = s.shape[0], s.shape[1], mx.shape[0], mx.shape[1], border
            f.write(h.tobytes() + np.ascontiguousarray(s, "<f4").tobytes() + np.ascontiguousarray(mx, "<f4").tobytes() +
                    np.ascontiguousarray(my, "<f4").tobytes())
    out = subprocess.run([exe, "remap", src_path, dst_path], capture_output=True, text=True, timeout=120)
    if out.returncode != 0 or not out.stdout.strip().endswith("OK"):
        return out.returncode, out.stdout[-500:] + out.stderr[-3000:]
    raw = np.fromfile(dst_path, "<f4")
    res, at = [], 0
    for _, mx, _, _ in jobs:
        res.append(raw[at:at + mx.size].reshape(mx.shape))
        at += mx.size
    assert at == len(raw)
    return res


def row_jobs(rows):
    return [(CC.source(r),) + CC.oracle_maps(r) + (r["border"],) for r in rows]


def test_shared_header_equals_the_oracle_on_every_row_under_sanitizers(harnesses):
    exe, _, d = harnesses
    maps = run_maps(exe, d, CC.TABLE)
    assert isinstance(maps, list), maps
    for r, (st, mx, my) in zip(CC.TABLE, maps):
        ox, oy = CC.oracle_maps(r)
        assert st == 0 and CC.same_floats(mx, ox) and CC.same_floats(my, oy), r["name"]
    outs = run_remap(exe, d, row_jobs(CC.TABLE))
    assert isinstance(outs, list), outs
    for r, got in zip(CC.TABLE, outs):
        assert CC.same_floats(got, CC.oracle_output(r)), r["name"]
    singular = dict(CC.BY_NAME["identity"], R=np.zeros((3, 3)))
    assert run_maps(exe, d, [singular]) == [(-1, None, None)]


def random_jobs(n_sources=20, per_source=1000, seed=7):
    """Random small sources (1 .. 6 rows and columns, full-mantissa values) with random map entries around and far outside them: NaN,
    +-inf, +-3e38, the values on both sides of |c * 32| = 2^31, ties and plain coordinates, each coordinate drawn on its own."""
    rng = np.random.default_rng(seed)
    special = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 67108864.0, -67108864.0, 67108860.0, -67108860.0, 1.0e9, -1.0e9, -0.0], f32)
    jobs = []
    for k in range(n_sources):
        rows, cols = int(rng.integers(1, 7)), int(rng.integers(1, 7))
        src = ((rng.random((rows, cols)) - 0.25) * 300.0).astype(f32)

        def coords(extent):
            c = rng.uniform(-1.5, extent + 1.5, per_source).astype(f32)
            tie = rng.uniform(size=per_source) < 0.15
            c[tie] = (np.rint(c[tie] * 32.0) + 0.5) / 32.0
            sp = rng.uniform(size=per_source) < 0.12
            c[sp] = rng.choice(special, int(sp.sum()))
            return c.reshape(1, per_source)
        jobs.append((src, coords(cols), coords(rows), float(f32(rng.uniform(-20, 20)))))
    return jobs


def test_shared_header_equals_the_oracle_on_random_entries_under_sanitizers(harnesses):
    """20 000 entries. The loader's bounds check and AddressSanitizer see every source read; UBSan every conversion."""
    from oracle import oracle as O
    exe, _, d = harnesses
    jobs = random_jobs()
    outs = run_remap(exe, d, jobs)
    assert isinstance(outs, list), outs
    n = nonrep = touched = 0
    for (src, mx, my, border), got in zip(jobs, outs):
        want = O.camera_remap(src, mx, my, border)
        assert CC.same_floats(got, want)
        assert CC.same_floats(got, CC.remap_model(src, mx, my, border, rounded=True))
        bad = ~(CC.fits(mx) & CC.fits(my))
        assert (CC.bits(got)[bad] == CC.bits(f32(border))).all()
        n, nonrep, touched = n + mx.size, nonrep + int(bad.sum()), touched + int((got != f32(border)).sum())
    print(f"{n} entries, {nonrep} that do not fit, {touched} that read the source")
    assert n == 20000 and nonrep > 3000 and touched > 5000


def test_oracle_camera_model_is_clean_under_sanitizers(harnesses):
    """orc_camera_init_maps / orc_camera_remap of odo_oracle.c as a program of their own on the non-representable rows: no report (before
    the rule, `(int)rintf(NaN)` was one) and the library oracle's bits."""
    _, exe, d = harnesses
    rows = rows_of("nonrep")
    maps = run_maps(exe, d, rows)
    assert isinstance(maps, list), maps
    for r, (st, mx, my) in zip(rows, maps):
        ox, oy = CC.oracle_maps(r)
        assert st == 0 and CC.same_floats(mx, ox) and CC.same_floats(my, oy), r["name"]
    outs = run_remap(exe, d, row_jobs(rows) + random_jobs(2, 500, seed=9))
    assert isinstance(outs, list), outs
    for r, got in zip(rows, outs):
        assert CC.same_floats(got, CC.oracle_output(r)), r["name"]


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
# (name, the text of camera_math.h that is replaced, its replacement, "remap" or "maps", the rows that must catch it)
MUTANTS = [
    ("sx / 32 for sx >> 5", "const int ix = sx >> 5", "const int ix = sx / 32", "remap", ("sx-m33", "half-top-left")),
    ("sx % 32 for sx & 31", "(float)(sx & 31)", "(float)(sx % 32)", "remap", ("ix-m1-axpos", "half-top-left")),
    ("roundf for rintf", "(int)rintf(fx)", "(int)roundf(fx)", "remap", ("tie-x-even", "tie-x-odd")),
    ("truncation for rintf", "(int)rintf(fx)", "(int)(fx)", "remap", ("tie-x-odd", "tie-x-even")),
    ("roundf for rintf in y", "sy = (int)rintf(fy)", "sy = (int)roundf(fy)", "remap", ("tie-y-even", "tie-y-odd")),
    ("the x1 test made on ix", "x1 = (unsigned)(ix + 1) < (unsigned)scols", "x1 = (unsigned)ix < (unsigned)scols", "remap", ("ix-m1-axpos", "ix-last")),
    ("ay and ax swapped in one weight", "w01 = (1.0f - ay) * ax", "w01 = (1.0f - ax) * ay", "remap", ("all-weight-pairs",)),
    ("the guard removed", "  if (!(remap_coord_fits(fx) && remap_coord_fits(fy))) return border_value;\n", "", "remap", ("finite-overflow", "projective", "nan-y-only")),
    ("2.0 * x2 dropped from the tangential term", "c.p2 * (r2 + 2.0 * x2)", "c.p2 * r2", "maps", ("barrel",)),
]


def test_every_mutant_is_caught_by_the_row_named_for_it(tmp_path):
    """Host builds only, in a temporary directory: a copy of camera_math.h with one expression replaced, the harness compiled against
    it (UBSan with float-cast-overflow, so that the mutant without the guard is a report on any host and not only a different number
    on some). Caught = the program's output for the row differs from the oracle's, or the program ends with a report. The unmutated
    copy, built the same way, is caught by no row."""
    text = open(HEADER).read()
    flags = ["-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all"]
    builds = []
    for k, (name, old, new, _, _) in enumerate([("control", "", "", "", ())] + MUTANTS):
        assert k == 0 or text.count(old) == 1, (name, text.count(old))
        hdr, exe = str(tmp_path / f"camera_math_{k}.h"), str(tmp_path / f"mutant_{k}")
        with open(hdr, "w") as f:
            f.write(text.replace(old, new) if k else text)
        builds.append((exe, build_math_harness(exe, hdr, flags)))
    for exe, p in builds:
        assert p.wait() == 0, exe

    def caught(exe, mode, r):
        if mode == "maps":
            got = run_maps(exe, tmp_path, [r])
            return not isinstance(got, list) or not (CC.same_floats(got[0][1], CC.oracle_maps(r)[0]) and CC.same_floats(got[0][2], CC.oracle_maps(r)[1]))
        got = run_remap(exe, tmp_path, row_jobs([r]))
        return not isinstance(got, list) or not CC.same_floats(got[0], CC.oracle_output(r))

    for r in CC.TABLE:
        assert not caught(builds[0][0], "maps", r) and not caught(builds[0][0], "remap", r), r["name"]
    for (exe, _), (name, _, _, mode, rows) in zip(builds[1:], MUTANTS):
        by = [r["name"] for r in CC.TABLE if caught(exe, mode, r)]
        print(f"{name}: caught by {len(by)} rows: {', '.join(by)}")
        for want in rows:
            assert want in by, (name, want, by)


# ---- the ABI's argument checks ---------------------------------------------------------------------------------------------------------
def test_accessors_and_refusals_that_touch_no_device():
    """A camera made over a context handle that is never dereferenced (and therefore never destroyed: a few hundred bytes): the raw
    calibration and the level count come back, and everything that needs maps is refused before a device is touched."""
    import ctypes as C
    from odometry_amd import _lib as L
    lib = L.load()
    raw, dist = CC.EUROC_RAW, CC.EUROC_DIST
    h = C.c_void_p()
    assert lib.odo_camera_create(C.c_void_p(8), 3, *raw, *dist, 6.0, 4.0, 94, 60, C.byref(h)) == 0
    raw5, dist4, sensor2, res2 = (C.c_double * 5)(), (C.c_double * 4)(), (C.c_double * 2)(), (C.c_int * 2)()
    assert lib.odo_camera_raw(h, raw5, dist4, sensor2, res2) == 0
    assert list(raw5) == list(raw) and list(dist4) == list(dist) and list(sensor2) == [6.0, 4.0] and list(res2) == [94, 60]
    assert lib.odo_camera_raw(h, None, None, None, None) == 0 and lib.odo_camera_raw(None, raw5, None, None, None) == -1
    assert lib.odo_camera_levels(h) == 3 and lib.odo_camera_levels(None) == -1
    rows, cols = C.c_int(-5), C.c_int(-5)
    assert lib.odo_camera_map_size(h, C.byref(rows), C.byref(cols)) == -1 and (rows.value, cols.value) == (-5, -5)
    src, dst = np.ones((3, 4), f32), np.full((3, 4), 7.0, f32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    fake = C.c_void_p(16)
    for args, why in (((h, fp(src), 3, 4, fp(dst)), "ConfigureCamera has not run"), ((h, None, 3, 4, fp(dst)), "NULL arg"),
                      ((h, fp(src), 3, 4, None), "NULL arg"), ((None, fp(src), 3, 4, fp(dst)), "NULL arg")):
        assert lib.odo_camera_undistort_rectify(*args, C.c_float(1.0)) == -1 and why in L.last_error(), why
    for args, why in (((h, fake, 3, 4, fake), "ConfigureCamera has not run"), ((h, None, 3, 4, fake), "NULL arg"), ((h, fake, 3, 4, None), "NULL arg")):
        assert lib.odo_camera_undistort_rectify_dev(*args, C.c_float(1.0)) == -1 and why in L.last_error(), why
    assert (dst == 7.0).all()
    dp = C.POINTER(C.c_double)
    P = np.ascontiguousarray(CC.EUROC_P)
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    assert lib.odo_camera_configure(h, singular.ctypes.data_as(dp), P.ctypes.data_as(dp), 4, 3) == -1 and "singular" in L.last_error()
    assert lib.odo_camera_configure(h, None, P.ctypes.data_as(dp), 4, 3) == -1 and lib.odo_camera_configure(h, singular.ctypes.data_as(dp), None, 4, 3) == -1
    assert lib.odo_camera_configure(h, np.eye(3).ctypes.data_as(dp), P.ctypes.data_as(dp), 0, 3) == -1 and "bad size" in L.last_error()
    assert lib.odo_camera_map_size(h, None, None) == -1                       # still not configured
