"""Every row of tests/depth_cases.py's table is the input it claims to be, shown with the oracle alone: the pair reaches the branch of
depth_select_kernel_body / depth_disparity_kernel_body it is in the table for at least as often as its floor says, the closed forms
hold for the oracle's outputs, and an independent numpy restatement of the selection rule gives the oracle's mask. A floor is a
condition on the input, not on the code under test; tests/test_gpu_depth_cases.py holds the kernels to the same rows."""
import numpy as np
import pytest

import depth_cases as D

f32 = np.float32
ROWS = [r["name"] for r in D.TABLE]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def test_the_table_holds_the_rows_it_is_there_for():
    groups = {r["group"] for r in D.TABLE}
    assert groups == {"tied-median", "radix-pass", "flat-and-textured", "on-threshold", "cap", "tile-size", "all-tie", "periodic",
                      "trip-edges", "on-ssd-threshold", "never-below-start", "tap-edges"}
    keys = sorted(D.tile_dims(*r["size"], 4)[0] * D.tile_dims(*r["size"], 4)[1] for r in D.TABLE if r["group"] == "tile-size")
    assert keys == [512, 513, 1024, 1025, D.MAX_KEYS]
    assert (D.CAP, D.CHUNK, D.MAX_KEYS, D.MAIN_TRIP, D.PAIR_TRIP) == (80, 512, 4096, 256, 128)    # what the cap row's chunks and waves assume
    tap = [r for r in D.TABLE if r["group"] == "tap-edges"]
    assert {(r["params"]["boundary"], r["size"][1] % 4) for r in tap} == {(b, c) for b in (2, 4) for c in range(4)}
    for g in ("all-tie", "periodic"):
        assert {r["params"]["max_disparity"] for r in D.TABLE if r["group"] == g} == {0, 128}
    assert {r["period"] for r in D.TABLE if r["group"] == "periodic"} == {5, 16, 64, 256}
    for r in D.TABLE:   # scan rows keep their matches and stay below the 1e10 the minimum starts at
        assert isinstance(r["params"]["ssd_th"], str) or r["params"]["ssd_th"] < 1e10
        assert r["size"][1] <= 800 or r["group"] in ("tile-size", "radix-pass"), r["name"]


def test_scan_path_replays_the_three_loops():
    """scan_path against a literal transcription of the kernel's loop structure, for every candidate of every length up to 3 trips."""
    for n in list(range(1, 300)) + [511, 512, 513, 767, 768, 769]:
        got = [D.scan_path(n, o) for o in range(n)]
        want, base = {}, 0
        while base + 256 <= n:
            for lane in range(64):
                for u in range(4):
                    want[base + 4 * lane + u] = ("main", base // 256, lane, u)
            base += 256
        for lane in range(64):
            rx, trip = base + lane, 0
            while rx + 64 < n:
                for u in range(2):
                    want[rx + 64 * u] = ("pair", trip, lane, u)
                rx += 128
                trip += 1
            k = 0
            while rx < n:
                want[rx] = ("single", k, lane, 0)
                rx += 64
                k += 1
        assert got == [want[o] for o in range(n)], n


def select_model(O, L, bnd, grad_th):
    """DisparityDepthEstimate's point selection restated: |grad| of the blurred image in float32 (one rounding per operation), the
    tile's threshold = its sorted magnitudes' element bsz / 2 plus grad_th, strictly above, the first 80 in raster order."""
    Lb = O.blur3x3(L)
    rows, cols = Lb.shape
    gx = f32(0.5) * (Lb[:, 2:] - Lb[:, :-2])
    gy = f32(0.5) * (Lb[2:, :] - Lb[:-2, :])
    mag = np.zeros((rows, cols), f32)
    mag[1:-1, 1:-1] = np.sqrt(gx[1:-1] * gx[1:-1] + gy[:, 1:-1] * gy[:, 1:-1])
    bw, bh = (cols - 2 * bnd) // 32, (rows - 2 * bnd) // 16
    val = np.zeros((rows, cols), np.uint8)
    for b in range(512):
        sy, sx = bnd + (b // 32) * bh, bnd + (b % 32) * bw
        tile = mag[sy:sy + bh, sx:sx + bw]
        th = f32(np.sort(tile.ravel())[(bw * bh) // 2] + f32(grad_th))
        keep = np.flatnonzero(tile.ravel() > th)[:80]
        val[sy + keep // bw, sx + keep % bw] = 1
    return val


@pytest.mark.parametrize("name", ROWS)
def test_row_reaches_its_branch_and_its_closed_forms_hold(O, name):
    r = D.BY_NAME[name]
    A, c = D.analysis(r), D.counts(r)
    out = D.outputs_of(A["ref"])
    assert A["ref"]["status"] == 0 and out["n_selected"] == int(out["val"].sum()) > 0
    report = []
    for k, (floor, measured) in r["floors"].items():
        report.append(f"{k} {c[k]} (floor {floor}, written down {measured})")
        if k.endswith("_selected") or k == "chunks":
            assert c[k] == floor, f"{name}: {k} = {c[k]}, must be {floor}"
        else:
            assert c[k] >= floor, f"{name}: {k} = {c[k]} < floor {floor}"
    print(f"{name} [{r['group']}] {A['size'][0]}x{A['size'][1]}, {c['keys']} keys per tile, {out['n_selected']} selected, "
          f"{out['n_matched']} matched: " + "; ".join(report))
    D.closed_generic(A, out)
    if r["closed"]:
        r["closed"](A, out)
    assert np.array_equal(select_model(O, A["L"], A["bnd"], A["params"]["grad_th"]), out["val"]), "the restated selection differs from the oracle's"
    # the scan restated for a sample of the points: every candidate's SSD in float32, first strict minimum below the 1e10 start
    ys, xs = np.nonzero(out["val"])
    lo = D.scan_lo(xs, A["bnd"], A["params"]["max_disparity"])
    for i in np.linspace(0, len(xs) - 1, 60).astype(int):
        s = D.ssd_candidates(A["Lb"], A["Rb"], int(xs[i]), int(ys[i]), int(lo[i]))
        best, col = f32(1e10), -1
        if len(s) and s.min() < best:
            best, col = s.min(), int(lo[i]) + int(np.argmin(s))
        assert best == A["scan"]["best_ssd"][ys[i], xs[i]] and col == A["scan"]["best_col"][ys[i], xs[i]]
        want = 0.0 if best > f32(A["params"]["ssd_th"]) else float(xs[i] - col)
        assert out["disp"][ys[i], xs[i]] == want


def test_every_sub_bin_of_every_radix_pass_is_reached_over_the_table():
    """Wave 0 resolves four histogram bins per lane (c0 .. c3): the digit chosen in a pass is 4 * lane + q. Over the table every q is
    reached in every pass; the digits are those of the median's bit pattern, read from the sorted keys."""
    tot = np.zeros((4, 4), np.int64)
    for r in D.TABLE:
        c = D.counts(r)
        tot += np.array([[c[f"pass{p}_bin{q}"] for q in range(4)] for p in range(4)])
    print("tiles per (pass, digit % 4) over the table:", tot.tolist())
    assert (tot >= 500).all(), tot     # measured: the rarest is pass 0, digit % 4 == 2 (magnitudes of 32 .. 128), 523 tiles


def test_which_row_covers_which_branch():
    """The printed summary: branch -> rows that reach it. A builder that loses its branch fails its floor above; this one fails when a
    branch of the list is left with no row at all."""
    branches = ("tiles_tied", "tiles_inside_run", "tiles_share8", "tiles_share16", "tiles_share24", "tiles_flat_empty", "tiles_flat_capped",
                "on_threshold", "tiles_79", "tiles_80", "tiles_81", "tiles_first_in_later_chunk", "tiles_cap_in_later_chunk",
                "tiles_80_81_same_wave", "tiles_80_81_other_wave", "points_without_candidates", "points_all_tied", "tied_other_lane",
                "tied_other_row_of_16", "tied_same_lane_last_loops", "tied_same_lane_main_loop", "min_on_first", "min_on_last",
                "min_on_last_of_main_trip", "min_on_first_of_next_main_trip", "min_in_pair_loop", "min_in_single_loop",
                "best_on_threshold", "best_at_start", "points_top_row", "points_bottom_row", "points_first_column", "points_last_column")
    for b in branches:
        rows = [r["name"] for r in D.TABLE if b in r["floors"] and r["floors"][b][0] > 0 and D.counts(r)[b] >= r["floors"][b][0]]
        print(f"{b}: {', '.join(rows)}")
        assert rows, f"no row of the table is held to {b}"
    chunks = sorted({D.counts(r)["chunks"] for r in D.TABLE})
    print("chunks of 512 keys per tile:", chunks)
    assert chunks == [1, 2, 3, 8]


def test_the_on_ssd_threshold_row_takes_its_threshold_from_a_point(O):
    A = D.analysis(D.BY_NAME["on-ssd-threshold"])
    th = f32(A["params"]["ssd_th"])
    ys, xs = np.nonzero(A["ref"]["val"])
    best = A["scan"]["best_ssd"][ys, xs]
    assert float(th) == A["params"]["ssd_th"] and (best == th).sum() >= 1
    nxt = best[best > th].min()
    assert (A["ref"]["disp"][ys, xs][best == th] > 0).all(), "equality with ssd_th is a hit"
    assert not A["ref"]["disp"][ys, xs][best == nxt].any(), "the next larger SSD is a miss"


def test_negative_grad_th_is_accepted_by_the_oracle(O):
    """(odo_depth_create takes any grad_th as well: it checks the boundary only.)"""
    r = D.BY_NAME["flat-and-textured-negative"]
    assert r["params"]["grad_th"] < 0 and D.counts(r)["tiles_flat_capped"] == 256


def test_the_batched_rows_pass_stage_2_in_the_oracle(O):
    """What tests/test_gpu_depth_cases.py's batched test needs: a whole ComputeDepth of each pair succeeds (500 valid depths), or
    Tracker.init would refuse the frame."""
    for name in D.BATCH["rows"]:
        L, R = D.pair(D.BY_NAME[name], D.BATCH["size"])
        ref = O.compute_depth(L, R, O.depth_params(any_size=1, **D.batch_oracle_params()), stage=2)
        assert ref["status"] == 0 and ref["n_valid"] >= 500, name
        print(f"{name} at {D.BATCH['size']}: stage 2 status 0, {ref['n_valid']} valid depths of {ref['n_selected']} selected")


# ---- the rows tell a nearly correct rule from the correct one ---------------------------------------------------------------------
def _select_variant(A, strict=True, cap_per_chunk=False, rank_shift=0):
    """select_model on the row's magnitudes with one rule changed."""
    val = np.zeros(A["size"], np.uint8)
    for t in D.tiles(A):
        bsz = t["bw"] * t["bh"]
        th = f32(t["sorted"][bsz // 2 + rank_shift] + f32(A["params"]["grad_th"]))
        over = t["mag"] > th if strict else t["mag"] >= th
        if cap_per_chunk:
            keep = np.concatenate([np.flatnonzero(over[c:c + D.CHUNK])[:D.CAP] + c for c in range(0, bsz, D.CHUNK)])[:2 * D.CAP]
        else:
            keep = np.flatnonzero(over)[:D.CAP]
        val[t["sy"] + keep // t["bw"], t["sx"] + keep % t["bw"]] = 1
    return val


def _scan_variant(A, rule, n_points=300):
    """How many of n_points sampled points get another column than the oracle's when ties are resolved by `rule`:
    "lane" — the wave argmin compares (SSD, lane) instead of (SSD, column); "row" — the merge of the four rows of 16 lanes lets the
    later row win a tie; "last" — a lane keeps its LAST minimum (<= for <)."""
    ys, xs = np.nonzero(A["ref"]["val"])
    lo = D.scan_lo(xs, A["bnd"], A["params"]["max_disparity"])
    pick = np.flatnonzero(xs - lo > 1)
    differ = 0
    for i in pick[np.linspace(0, len(pick) - 1, n_points).astype(int)]:
        s = D.ssd_candidates(A["Lb"], A["Rb"], int(xs[i]), int(ys[i]), int(lo[i]))
        ties = np.flatnonzero(s == s.min())
        lanes = np.array([D.scan_path(len(s), int(o))[2] for o in ties])
        if rule == "lane":
            col = ties[np.lexsort((ties, lanes))[0]]
        elif rule == "row":
            col = ties[np.lexsort((ties, -(lanes // 16)))[0]]
        else:
            col = min(ties[lanes == l].max() for l in set(lanes.tolist()))
        differ += int(lo[i]) + int(col) != A["scan"]["best_col"][ys[i], xs[i]]
    return differ


def test_nearly_correct_rules_are_told_apart_by_their_rows(O):
    """Each restated rule with one change differs from the oracle on the row that is in the table for it (and the unchanged
    restatement does not: test_row_reaches_its_branch_and_its_closed_forms_hold)."""
    differs = lambda name, **kw: int((_select_variant(D.analysis(D.BY_NAME[name]), **kw) != D.analysis(D.BY_NAME[name])["ref"]["val"]).sum())  # noqa: E731
    got = dict(ge_on_threshold=differs("on-threshold", strict=False), ge_flat=differs("flat-and-textured", strict=False),
               cap_per_chunk=differs("cap", cap_per_chunk=True), rank_below=differs("tied-median-5-levels", rank_shift=-1),
               rank_above=differs("tied-median-5-levels", rank_shift=1),
               lane_order_p5=_scan_variant(D.analysis(D.BY_NAME["periodic-p5-d3-md0"]), "lane"),
               later_row_of_16_p16=_scan_variant(D.analysis(D.BY_NAME["periodic-p16-d11-md128"]), "row"),
               last_minimum_p64=_scan_variant(D.analysis(D.BY_NAME["periodic-p64-d3-md128"]), "last"),
               last_minimum_p256=_scan_variant(D.analysis(D.BY_NAME["periodic-p256-d3-md0"]), "last"),
               last_minimum_all_tie=_scan_variant(D.analysis(D.BY_NAME["all-tie-md0"]), "last"))
    print("pixels / sampled points (of 300) on which the changed rule differs from the oracle:", got)
    assert all(v > 0 for v in got.values()), got
    assert got["ge_flat"] >= 256 * D.CAP   # every flat tile would take its first 80 pixels
