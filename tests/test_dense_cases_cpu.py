"""The models of tests/dense_cases.py held to themselves, without a GPU: the dense scan's decomposition visits every unit exactly once,
the case table of tests/test_gpu_dense_cases.py really contains the situations it is there for, and the exact model of the
t-distribution scale leaves one admissible float at every pass of every committed residual set."""
import numpy as np
import pytest

import dense_cases as Dc


def _partition(n_strips, n_rg, nblk):
    seen = np.zeros((n_strips, n_rg), np.int32)
    for b in range(nblk):
        for s, g in Dc.run_units(Dc.block_run(n_strips, n_rg, nblk, b)):
            assert 0 <= s < n_strips and 0 <= g < n_rg
            seen[s, g] += 1
    assert (seen == 1).all(), (n_strips, n_rg, nblk)


def test_every_unit_exactly_once_small_range():
    """n_strips <= 11, n_rg <= 39 (n_rg < G included), every cap of the list: the walk of every block stays inside the level and the
    blocks together visit each (strip, row group) once."""
    for n_strips in range(1, 12):
        for n_rg in range(1, 40):
            for cap in (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 16, 17, 64):
                _partition(n_strips, n_rg, max(1, min(n_strips * n_rg, cap)))


@pytest.mark.parametrize("n_strips,n_rg,nblk", [(1024, 2048, 1024)] + [(1024, 2048, n) for n in range(1, 10)] + [(1024, 3, 1024), (1024, 1, 8)])
def test_every_unit_exactly_once_product_extremes(n_strips, n_rg, nblk):
    """The largest level the 32-bit arithmetic is written for (65535 x 65535: 1024 strips x 2048 row groups) at the product's cap and
    at nblk = 1 .. 9, and n_rg < G at full width. Runs are intervals of the band's strip-major order, so it is enough that the
    intervals of a band's blocks tile [0, U) and that every run starts on the unit its interval starts on (block_run itself asserts that no
    intermediate leaves 32 bits)."""
    G = min(nblk, 8)
    total = 0
    for g in range(G):
        at = 0
        for b in range(g, nblk, G):
            strip, rg, rg0, rg1, count = Dc.block_run(n_strips, n_rg, nblk, b)
            assert (rg0, rg1) == (g * n_rg // G, (g + 1) * n_rg // G) and count >= 0
            nrg = rg1 - rg0
            if nrg:
                assert strip * nrg + (rg - rg0) == at and rg0 <= rg < rg1
            at += count
        assert at == (rg1 - rg0) * n_strips
        total += at
    assert total == n_strips * n_rg


def test_geometry_matches_the_header_rule():
    assert Dc.R == 4 and Dc.GRID_CAP == 1024
    assert Dc.geometry(8, 100, 1024) == (0, 0, 1) and Dc.geometry(100, 8, 1024) == (0, 0, 1)
    assert Dc.geometry(9, 9, 1024) == (1, 1, 1)
    assert Dc.geometry(4108, 72, 1024) == (1, 1025, 1024)            # the smallest frame at which the product builds multi-unit runs
    assert Dc.geometry(1080, 1920, 1024) == (30, 268, 1024)


def test_case_table_contains_every_situation():
    widths, heights = set(), set()
    nblks, counts = set(), set()
    empty_band = wrap = no_interior = 0
    for rows, cols, cap in Dc.CASES:
        assert rows >= 8 and cols >= 8
        n_strips, n_rg, nblk = Dc.geometry(rows, cols, cap)
        if rows == 8 or cols == 8:
            no_interior += 1
            assert nblk == 1 and Dc.block_run(n_strips, n_rg, nblk, 0)[4] == 0
            continue
        widths.add(cols - 8)
        heights.add(rows - 8)
        nblks.add(nblk)
        px = Dc.block_pixels(rows, cols, cap)
        allpx = np.concatenate(px)
        assert len(allpx) == (rows - 8) * (cols - 8) == len(np.unique(allpx))          # every interior pixel in exactly one block
        G = min(nblk, 8)
        empty_band += any(g * n_rg // G == (g + 1) * n_rg // G for g in range(G))
        for b in range(nblk):
            run = Dc.block_run(n_strips, n_rg, nblk, b)
            counts.add(run[4])
            wrap += Dc.wraps(run)
    assert widths >= set(Dc.WIDTHS) and heights >= set(Dc.HEIGHTS)
    assert {(r - 8, c - 8) for r, c, cap in Dc.CASES if cap == Dc.GRID_CAP} >= {(h, w) for h in Dc.HEIGHTS for w in Dc.WIDTHS}
    assert no_interior >= 2 and {(r == 8, c == 8) for r, c, _ in Dc.CASES} >= {(True, False), (False, True)}
    assert any(n < 8 for n in nblks) and 8 in nblks and any(n > 8 and n % 8 for n in nblks) and any(n > 8 and n % 8 == 0 for n in nblks)
    assert empty_band >= 3
    assert {0, 1, 2} <= counts and any(c >= 3 and c % 2 for c in counts) and any(c >= 4 and c % 2 == 0 for c in counts)
    assert wrap >= 10
    assert len(Dc.CASES) == len(set(Dc.CASES))


def test_case_inputs_reach_both_division_paths_and_the_image_edge():
    for rows, cols in ((41, 137), (12, 72), (17, 137)):
        I1, I2, D1, k, T = Dc.case_inputs(rows, cols)
        inner = D1[4:rows - 4, 4:cols - 4]
        assert (np.abs(inner) > 4096).any() and (inner == 0).any() and ((np.abs(inner) >= 0.01) & (np.abs(inner) <= 4096)).any()
        assert 4 <= k[1] < cols - 4 and k[1] == int(k[1]) and 4 <= k[2] < rows - 4 and k[2] == int(k[2])   # x == cx, y == cy occur
        assert not np.array_equal(T, np.eye(4, dtype=np.float32))


def test_case_frames_produce_residuals_and_misses():
    """The host build of the per-pixel chain on every frame of the table: a good part of the interior produces residuals (a frame
    whose pixels all miss would hold the scan to sums of nothing), and in the wide frames some valid pixels warp out."""
    import devmath as D
    host = D.load_host()
    for rows, cols in sorted({(r, c) for r, c, _ in Dc.CASES if r > 8 and c > 8}):
        I1, I2, D1, k, T = Dc.case_inputs(rows, cols)
        hit = host.pixels(I1, I2, D1, k, T, 0)[0]
        inner = D1[4:rows - 4, 4:cols - 4]
        valid = int((np.abs(inner) >= 0.01).sum())
        assert hit.sum() >= 0.4 * valid and (hit.sum() > 0 or valid == 0), (rows, cols, int(hit.sum()), valid)
        if cols - 8 >= 63 and rows - 8 >= 8:
            assert hit.sum() < valid
        assert not hit[:4].any() and not hit[:, :4].any() and not hit[rows - 4:].any() and not hit[:, cols - 4:].any()


def test_list_frame_sums_do_not_cancel():
    """The list-level frame of tests/test_gpu_dense_cases.py is compared with the oracle's sums at rtol 1e-11: that is a statement
    about sigma only if the oracle's own summation error is far below it. Every interior pixel is a point (above the list order's
    16 384), no sum cancels by more than a factor 16, and the oracle is within 1e-12 of the exact sum of its own dumped terms."""
    import math
    from oracle import oracle as O
    I1, I2, inv, K, T = Dc.list_inputs()
    rows, cols = Dc.LIST_FRAME
    ref = O.lm_accumulate(I1, I2, inv, 0, T, robust=2, huber_delta=28.0, K=dict(f0=K[0], cx0=K[1], cy0=K[2]), dump=rows * cols)
    n = int(ref["acc"][28])
    assert ref["status"] == 0 and n == (rows - 8) * (cols - 8) > Dc.LIST_MAX and n <= Dc.SINGLE_LIST_MAX
    terms = Dc.row_products(ref["r"][:n], ref["w"][:n], ref["J"][:n])
    for q in range(28):
        exact, total = math.fsum(terms[:, q]), math.fsum(np.abs(terms[:, q]))
        assert total <= 16 * abs(exact), q
        assert abs(ref["acc"][q] - exact) <= 1e-12 * abs(exact), q


def test_scale_plan_edges():
    """The sizes of the scale cases sit on the edges of tdist_scale_plan: (list, G, fits, single_order)."""
    assert Dc.LIST_MAX == 16384 and Dc.SINGLE_LIST_MAX == 40960 and Dc.FITS_MAX == 2097152
    assert Dc.scale_plan(16384)[0] == 1 and Dc.scale_plan(16385) == (0, 5, 1, 1)
    assert Dc.scale_plan(20480)[1] == 5 and Dc.scale_plan(20481)[1] == 6
    assert Dc.scale_plan(40960)[3] == 1 and Dc.scale_plan(40961)[3] == 0
    assert Dc.scale_plan(524288)[1] == 128 and Dc.scale_plan(524287)[1] == 128 and Dc.scale_plan(520192)[1] == 127
    assert Dc.scale_plan(2097152)[2] == 1 and Dc.scale_plan(2097153)[2] == 0
    assert [Dc.product_writer(n) for n in (0, 16384, 16385, 2097152, 2097153)] == \
        [Dc.WROTE_LIST, Dc.WROTE_LIST, Dc.WROTE_MULTI, Dc.WROTE_MULTI, Dc.WROTE_STRIDED]
    assert set(Dc.SCALE_SIZES) >= {0, 1, 63, 64, 65, 255, 256, 257, 16384, 16385, 20480, 20481, 40960, 40961, 524288, 524289, 2097152, 2097153}


def test_tdist_model_on_known_values():
    assert Dc.tdist_model(np.zeros(0, np.float32))[0] == np.float32(25.0)
    assert Dc.tdist_model(np.full(100, np.nan, np.float32))[:2] == (np.float32(25.0), 0)
    # one residual r: sigma' = sqrt(201 r^2 / (200 + r^2 / sigma^2)); the fixed point is sigma = |r|
    s2, passes, single = Dc.tdist_model(np.array([3.0], np.float32))
    assert single and passes > 2 and abs(float(s2) - 9.0) < 0.1
    # a term in float32, operation by operation
    e2 = np.float32(7.25) * np.float32(7.25)
    want = np.float32(np.float32(e2 * np.float32(201.0)) / np.float32(np.float32(200.0) + np.float32(e2 / np.float32(25.0))))
    assert Dc.tdist_terms(np.array([e2]), np.float32(5.0))[0] == want


@pytest.mark.parametrize("n", Dc.SCALE_SIZES)
def test_scale_cases_leave_one_admissible_float(n):
    """For every committed (n, residual set): at every pass the interval of sums any fp64 summation order can produce rounds to ONE
    float sigma, so the GPU tests may ask for the model's sigma^2 bit for bit. A case that fails gets another seed in
    dense_cases.SCALE_SEEDS."""
    for nn, kind in Dc.scale_cases():
        if nn != n:
            continue
        s2, passes, single = Dc.scale_expected(n, kind)
        assert single, "n = %d, %s: more than one admissible sigma at some pass" % (n, kind)
        assert passes < Dc.MAX_PASSES
        res = Dc.residuals(n, kind)
        if kind == "all_nan" or n == 0:
            assert s2 == np.float32(25.0) and passes == 0
        if kind == "nan_tail":
            first = 64 * ((n - 1) // 64)
            assert not np.isnan(res[:first]).any() and np.isnan(res[-1])
        if kind == "mixed" and n >= 255:
            assert 0.2 < np.isnan(res).mean() < 0.4
        if kind == "const":
            assert passes <= 12
