"""The models and cases of tests/kf_list_cases.py held to themselves, without a GPU: every row of the list table reaches the situation
it is listed for, the host build of make_point equals a numpy float32 restatement on the table's inputs, three deliberately wrong
list models are caught by the table (and only by the rows placed for them), and the summation model of lm_residual_list_kernel is
the order its docstring states."""
import math

import numpy as np
import pytest

import dense_cases as Dc
import devmath as D
import kf_list_cases as Kc

f32 = np.float32
BY_ID = {c["id"]: c for c in Kc.CASES}


@pytest.fixture(scope="module")
def host():
    return D.load_host()


def _sit(cid):
    return Kc.situations(BY_ID[cid], Kc.contents(cid))


def test_depth_validity_at_its_edges():
    """The code's rule, !(fabsf(d) < 0.01f): the threshold itself is valid, its lower float32 neighbour is not, zeros and denormals are
    not, infinities are — and so is NaN, which the lists therefore hold."""
    vals = np.array([v for v, _ in Kc.EDGE_DEPTHS], f32)
    assert [bool(v) for v in Kc.valid(vals)] == [ok for _, ok in Kc.EDGE_DEPTHS]
    assert Kc.LO < f32(0.01) < Kc.HI and f32(0.01) - Kc.LO <= f32(1e-9)
    kinds = {"nan": np.isnan(vals).any(), "inf": np.isposinf(vals).any() and np.isneginf(vals).any(),
             "denormal": ((vals != 0) & (np.abs(vals) < np.finfo(f32).tiny)).any(), "zeros": (np.signbit(vals) & (vals == 0)).any(),
             "far": (np.abs(vals[np.isfinite(vals)]) > 4096).any(), "negative": (vals < -0.01).any()}
    assert all(kinds.values()), kinds
    I1, D1 = Kc.contents("edge_depths")[0]
    inner = D1[4:-4, 4:-4]
    assert all((inner.view(np.uint32) == v.view(np.uint32)).any() for v in vals)                   # every value, bit for bit, is in the frame


def test_case_table_reaches_every_situation():
    assert len(BY_ID) == len(Kc.CASES)
    for c in Kc.CASES:
        assert 1 <= len(c["levels"]) <= Kc.MAX_LEVELS
        assert all(r <= 522 and co <= 521 for r, co, _ in c["levels"])                              # (522 rows: the prefix loop's third trip)
        assert sum(Kc.interior(r, co)[0] for r, co, _ in c["levels"]) > 0                          # the product launches nothing otherwise
    # widths: chunk trips, the loop ending exactly, a second chunk of one pixel, three chunks; the hand-over of base_sh carries points
    for iw, trips in zip(Kc.WIDTHS, (1, 1, 1, 1, 1, 1, 2, 3)):
        for pat in ("all", "random"):
            s = _sit("w%d_%s" % (iw, pat))
            assert s["chunk_trips"] == trips and s["exact_end"] == (iw == 256)
            assert (s["carries"] > 0) == (trips > 1)
    assert _sit("w257_all")["carries"] == 3 and _sit("w513_all")["carries"] == 6
    # heights: trips of the row-offset prefix; the rows behind row 256 hold points that a later row's offset must count
    for ih, trips in zip(Kc.HEIGHTS, (0, 1, 1, 2, 2, 3)):
        for iw, pat in ((1, "all"), (3, "random")):
            s = _sit("h%d_w%d_%s" % (ih, iw, pat))
            assert s["prefix_trips"] == trips
            assert (s["prefix_late"] > 0) == (trips > 1)
    # row patterns
    assert _sit("pat_lane0")["lane0_only"] == 3 * 9 and _sit("pat_lane0")["lane63_only"] == 0
    assert _sit("pat_lane63")["lane63_only"] == 3 * 8 and _sit("pat_lane63")["lane0_only"] == 0
    assert _sit("pat_lane63_w64")["lane63_only"] == 2
    assert _sit("pat_first_col")["lane0_only"] == 3 and _sit("pat_last_col")["lane0_only"] == 3      # x = cols - 5: lane 0 of the third chunk
    for cid, want in (("pat_all", 513 * 3), ("pat_none", 0), ("pat_first_col", 3), ("pat_last_col", 3), ("pat_last_chunk", 3), ("pat_alt", 770),
                      ("pat_empty_row", 513 * 2)):
        I1, D1 = Kc.contents(cid)[0]
        assert int(Kc.valid(D1[4:-4, 4:-4]).sum()) == want, cid
        assert _sit(cid)["border_depths"] == 0
    D1 = Kc.contents("pat_last_chunk")[0][1]
    assert not Kc.valid(D1[4:-4, 4:4 + 512]).any() and _sit("pat_last_chunk")["carries"] == 0
    assert not Kc.valid(Kc.contents("pat_empty_row")[0][1][5, 4:-4]).any()
    assert _sit("pat_border")["border_depths"] == 11 * 521 - 3 * 513 and _sit("pat_border")["levels_with_points"] == 1
    # levels
    assert _sit("levels4_last_rows8")["no_interior"] == 1 and BY_ID["levels4_last_rows8"]["levels"][3][0] <= 8
    assert _sit("levels3_mid_cols8")["no_interior"] == 1 and BY_ID["levels3_mid_cols8"]["levels"][1][1] <= 8
    assert _sit("levels3_first_rows5")["no_interior"] == 1
    assert len(BY_ID["levels8"]["levels"]) == 8 and _sit("levels8")["no_interior"] == 0 and _sit("levels8")["levels_with_points"] == 8
    # the skip: either side of both inequalities, total > dense_above and 2 total > interior (256)
    verdicts = {(t, a): _sit("skip_%d_above%d" % (t, a))["skipped"] for t, a in Kc.SKIP_POINTS}
    assert verdicts == {(128, 1): [False], (129, 128): [True], (129, 129): [False], (129, 0): [False], (256, 255): [True], (256, 256): [False]}
    assert _sit("skip_0_filled_1")["skipped"] == [True, False] and _sit("filled_0_skip_1")["skipped"] == [False, True]
    assert _sit("skip_tall")["skipped"] == [True] and _sit("skip_tall")["prefix_trips"] == 2
    assert _sit("skip_mixed_levels")["skipped"] == [True, True, False] and _sit("skip_mixed_levels")["no_interior"] == 1


def test_skip_rule_is_the_hosts_rule():
    """kf_fill_kernel_body skips a level's list exactly when lm_take_counts (mode 0) will not read it — for every count of a small
    interior and every threshold around it — apart from the levels the host reads although they were never worth skipping."""
    for n_int in (1, 2, 255, 256, 257):
        for above in range(0, n_int + 2):
            for total in range(0, n_int + 1):
                skip, use = Kc.skip_verdict(total, n_int, above), Kc.host_use_list(total, n_int, above)
                assert not (skip and use), (n_int, above, total)                                    # a skipped list is never read
                if above > 0 and total > 0:
                    assert skip == (not use), (n_int, above, total)


def test_host_make_point_equals_numpy_restatement(host):
    n = bad = 0
    for c in Kc.CASES:
        for seed in (0, 1):
            for l, (I1, D1) in enumerate(Kc.contents(c["id"], seed)):
                got, want = host.make_points(I1, D1, Kc.K, l), Kc.make_points_np(I1, D1, Kc.K, l)
                same = D.same_bits(got, want)
                bad += int((~same).sum())
                n += same.size
    assert bad == 0 and n > 13 * 100000, (bad, n)


def _model(cid, host, variant=None):
    c = BY_ID[cid]
    levels = Kc.contents(cid)
    points = [host.make_points(I1, D1, Kc.K, l) for l, (I1, D1) in enumerate(levels)]
    return Kc.expected(levels, points, c["dense_above"], variant=variant)


def test_model_fills_what_it_claims(host):
    for c in Kc.CASES:
        m = _model(c["id"], host)
        levels = Kc.contents(c["id"])
        for l in range(Kc.MAX_LEVELS):
            ih, iw = Kc.interior(*levels[l][1].shape) if l < len(levels) else (0, 0)
            lst = m["lists"][l].view(np.uint32)
            assert lst.shape == (ih * iw + Kc.SPARE, 13)
            n = 0 if (l >= len(levels) or ih == 0 or m["skipped"][l]) else int(m["npts"][l])
            assert (lst[n:] == Kc.FILL32).all()
            if ih:
                assert int(m["npts"][l]) == int(Kc.valid(levels[l][1][4:-4, 4:-4]).sum())
            else:
                assert m["npts"][l] == 0
        assert m["rowcnt"].view(np.uint32)[-1] == Kc.FILL32 and len(m["rowcnt"]) == sum(Kc.interior(r, co)[0] for r, co, _ in c["levels"]) + 1


@pytest.mark.parametrize("variant", Kc.VARIANTS)
def test_wrong_models_are_caught_only_by_their_rows(host, variant):
    """A compaction that restarts each chunk at the row's base differs exactly on the rows whose later chunk starts behind points of an
    earlier one; a row-offset prefix that stops after 256 rows exactly where rows from 256 on hold points above a later row; `>=` in
    the skip's first inequality exactly at total == dense_above with more than half the interior, in its second exactly at
    2 total == interior."""
    caught = {c["id"] for c in Kc.CASES if not Kc.same_build(_model(c["id"], host), _model(c["id"], host, variant))}
    if variant == "chunk_restart":
        built = {c["id"] for c in Kc.CASES if _sit(c["id"])["carries"] > 0 and not all(_sit(c["id"])["skipped"])}
        assert {"w257_all", "w257_random", "w513_all", "w513_random", "pat_all", "pat_alt", "pat_empty_row", "pat_border"} <= built
    elif variant == "prefix_256":
        built = {c["id"] for c in Kc.CASES if _sit(c["id"])["prefix_late"] > 0 and not all(_sit(c["id"])["skipped"])}
        assert built == {"h%d_w%d_%s" % (ih, iw, pat) for ih in (258, 513, 514) for iw, pat in ((1, "all"), (3, "random"))}
    elif variant == "skip_ge_total":
        built = {"skip_129_above129", "skip_256_above256"}
    else:
        built = {"skip_128_above1", "skip_0_filled_1", "filled_0_skip_1"}
    assert caught == built, (sorted(caught - built), sorted(built - caught))


# ---- B ---------------------------------------------------------------------------------------------------------------------------------
def test_list_eval_sizes_and_grids():
    assert Kc.LIST_MAX_BLOCKS == 160 and Kc.LM_BLOCK == 256
    assert [Kc.list_blocks(n) for n in (0, 1, 256, 257, 40960, 40961, 10 ** 6)] == [1, 1, 1, 2, 160, 160, 160]
    assert set(Kc.LIST_EVALS) >= {(1, 1), (255, 1), (256, 1), (257, 2), (512, 2), (513, 3), (1000, 1), (513, 2), (2049, 3), (40961, 160)}
    assert Kc.list_frame(40961) == (177, 264) and all(max(Kc.list_frame(n)) <= 521 for n, _ in Kc.LIST_EVALS)
    # grid-stride trips of a thread: one, and two to four where the grid is forced small or capped
    trips = {(n, b): -(-n // (b * Kc.LM_BLOCK)) for n, b in Kc.LIST_EVALS}
    assert trips[(1000, 1)] == 4 and trips[(513, 2)] == 2 and trips[(2049, 3)] == 3 and trips[(40961, 160)] == 2
    assert all(t == 1 for (n, b), t in trips.items() if b == Kc.list_blocks(n) and n <= 40960)


def test_list_inputs_give_hits_and_misses(host):
    """Every size has exactly n points; from 255 points on, points that give a residual and points that do not (warped out of the image,
    behind the camera), far points and negative depths are among them, under every weight the terms differ."""
    for n, nblk in Kc.LIST_EVALS:
        I1, I2, D1, k, T = Kc.list_inputs(n)
        inner = D1[4:-4, 4:-4]
        assert int(Kc.valid(inner).sum()) == n and D1.shape == Kc.list_frame(n)
        pix = host.pixels(I1, I2, D1, k, T, 0, 1, Kc.HUBER, Kc.SCALE_SQR)
        hit, r, w = Kc.list_points(D1, *pix[:3])
        assert len(hit) == n
        if n == 1:
            assert hit.sum() == 1, "the single point gives no residual: choose another seed (Kc.LIST_SEEDS)"
        if n >= 255:
            assert 0.4 * n < hit.sum() < n
            assert (inner < -0.01).any() and (np.abs(inner) > 4096).any()
            assert (w[hit != 0] < 1).any() and (w[hit != 0] == 1).any()                            # both branches of the Huber weight
        r3 = Kc.list_points(D1, host.pixels(I1, I2, D1, k, T, 3)[1])[0]
        assert np.array_equal(r3[hit != 0], r[hit != 0])


def test_partial_rows_is_the_stated_order():
    """partial_rows against a scalar restatement of the kernel's loops on a small random set, and within the any-order bound of the
    exact sums; an order that differs (a plain running sum) gives other bits, so the bit-for-bit check is a statement about order."""
    rng = np.random.default_rng(5)
    n, nblk = 1300, 2
    terms = (rng.standard_normal((n, Dc.NACC)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(f32).astype(np.float64)
    hit = rng.random(n) < 0.7
    got = Kc.partial_rows(terms, hit, nblk)
    want = np.zeros((nblk, Dc.NACC))
    for b in range(nblk):
        acc = np.zeros((256, Dc.NACC))
        for t in range(256):
            for idx in range(b * 256 + t, n, nblk * 256):
                if hit[idx]:
                    acc[t] = acc[t] + terms[idx]
        v = np.zeros((8, Dc.NACC))
        for s in range(8):
            for i in range(32):
                v[s] = v[s] + acc[8 * i + s]
        v = v + v[np.arange(8) ^ 4]
        v = v + v[np.arange(8) ^ 2]
        v = v + v[np.arange(8) ^ 1]
        want[b] = v[0]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    running = np.zeros((nblk, Dc.NACC))
    for b in range(nblk):
        for idx in range(n):
            if hit[idx] and (idx // 256) % nblk == b:
                running[b] = running[b] + terms[idx]
    assert (got != running).any()
    for b in range(nblk):
        mine = np.array([hit[i] and (i // 256) % nblk == b for i in range(n)])
        for q in range(Dc.NACC):
            assert abs(got[b, q] - math.fsum(terms[mine, q])) <= Dc.sum_bound(terms[mine, q], int(mine.sum()))


def test_handover_inputs_and_rule():
    for total, fuse in Kc.HANDOVER:
        for seed in (0, 1):
            D1 = Kc.handover_inputs(total, seed)[2]
            assert D1.shape == (12, 72) and int(Kc.valid(D1[4:-4, 4:-4]).sum()) == total and not Kc.valid(D1[:4]).any()
        assert not np.array_equal(Kc.handover_inputs(total, 0)[2], Kc.handover_inputs(total, 1)[2])
    want = {(t, f): Kc.host_use_list(t, 256, f) for t, f in Kc.HANDOVER}
    assert want == {(128, 128): True, (128, 129): True, (129, 128): False, (129, 129): True}
    assert {(t, f): Kc.skip_verdict(t, 256, f) for t, f in Kc.HANDOVER} == {k: not v for k, v in want.items()}
