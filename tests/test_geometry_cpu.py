"""The table of tests/geometry_cases.py without a GPU: every row reaches the branch it is in the table for under the launch constants
parsed from the kernels' headers (so a changed constant names the rows that no longer do their job), the unions of branches the
table covers, the volume's tile walk replayed with and without each carry, and every row shown to be a valid, non-trivial input by
the numpy models alone. tests/test_gpu_geometry.py holds the kernels to the same model results bit for bit."""
import numpy as np
import pytest

import geometry_cases as G


@pytest.fixture(scope="module")
def K():
    return G.constants()


def test_the_launch_constants_are_read_from_the_headers(K):
    for name in ("kVolBlock", "kVolExtBlock", "kVolTileX", "kVolTileY", "kVolMaxBlocks", "kVolScanThreads", "kMapBlock", "kMapScanThreads",
                 "kFeBlock", "kFeMaxSplat", "kFeRegBlocksMax", "kFeResBlocksMax"):
        assert K.get(name, 0) > 0, name
    # what the kernels themselves assume of them
    assert K["kVolTileX"] == 64 and K["kVolTileX"] * K["kVolTileY"] == K["kVolBlock"]
    assert K["kMapBlock"] % 64 == 0 and K["kFeBlock"] % 64 == 0 and K["kVolExtBlock"] % 64 == 0


# ---- every row does its job ---------------------------------------------------------------------------------------------------------
def _volume_geometry(r, K):
    return G.volume_geometry(r["dims"] or G.volume_inputs(r)[0]["dims"], K)


@pytest.mark.parametrize("name", [r["name"] for r in G.VOLUME])
def test_volume_row_reaches_its_branch(K, name):
    r = G.volume_row(name)
    g = _volume_geometry(r, K)
    assert r["holds"](g), f"{name} is in the table for: {r['why']}; its geometry is now {g}"


@pytest.mark.parametrize("name", [r["name"] for r in G.MAP])
def test_map_row_reaches_its_branch(K, name):
    r = G.map_row(name)
    g = G.map_geometry(r["size"], K)
    assert r["holds"](g), f"{name} is in the table for: {r['why']}; its geometry is now {g}"


@pytest.mark.parametrize("name", [r["name"] for r in G.FRONTEND])
def test_frontend_row_reaches_its_branch(K, name):
    r = G.frontend_row(name)
    g = G.frontend_geometry(r["depth_size"], r["size"], K)
    assert r["holds"](g), f"{name} is in the table for: {r['why']}; its geometry is now {g}"


def test_the_rows_between_them_cover_the_branches(K):
    vol = [_volume_geometry(r, K) for r in G.VOLUME]
    taken = [G.carries_taken(g) for g in vol]
    assert any(g["step_x"] != 0 for g in vol)
    assert any(x > 0 for x, _ in taken) and any(y > 0 for _, y in taken)
    assert any(g["tiles"] == g["nblk"] for g in vol) and any(g["tiles"] == g["nblk"] + 1 for g in vol)
    assert any(g["dims"][0] < g["tile"][0] and g["dims"][1] < g["tile"][1] for g in vol)                 # a grid below one tile
    assert any(g["tiles"] >= 20 * g["nblk"] for g in vol)
    ext = {g["ext_blocks"] for g in vol}
    assert 1 in ext and K["kVolScanThreads"] in ext and max(ext) > K["kVolScanThreads"]
    assert any(g["n"] < g["ext_block"] for g in vol)
    mp = [G.map_geometry(r["size"], K) for r in G.MAP]
    assert {min(g["per"], 3) for g in mp} == {1, 2, 3}
    assert any(g["n"] < 64 for g in mp) and any(g["n"] % 64 != 0 and g["n"] > 64 for g in mp) and any(g["n"] < g["block"] for g in mp)
    assert any(g["nblk"] == K["kMapScanThreads"] for g in mp)
    assert any(g["per"] == 2 and g["scan_busy"] < g["scan_threads"] for g in mp)
    fe = [G.frontend_geometry(r["depth_size"], r["size"], K) for r in G.FRONTEND]
    rb = {g["rb"] for g in fe}
    assert 1 in rb and K["kFeRegBlocksMax"] in rb and any(1 < v < K["kFeBlock"] for v in rb)
    assert any(g["nd"] % K["kFeBlock"] != 0 for g in fe) and any(g["nd"] % 64 != 0 for g in fe)
    assert any(g["nd"] == g["rb"] * K["kFeBlock"] and g["rb"] == K["kFeRegBlocksMax"] for g in fe)
    assert any(g["rb"] == K["kFeRegBlocksMax"] and g["nd"] > g["rb"] * K["kFeBlock"] for g in fe)       # a second pass
    assert any(g["sb"] == 1 for g in fe) and any(g["sb"] == K["kFeResBlocksMax"] for g in fe)
    assert {g["n"] % 4 for g in fe} >= {0, 2, 3}


# ---- the walk, replayed ---------------------------------------------------------------------------------------------------------------
def test_the_walk_visits_every_tile_exactly_once(K):
    grids = [_volume_geometry(r, K)["dims"] for r in G.VOLUME] + G.EARLIER_VOLUME_GRIDS + [(1024, 600, 2), (600, 300, 3), (63, 3, 2049)]
    for dims in grids:
        g = G.volume_geometry(dims, K)
        visits, stuck = G.walk(g)
        assert not stuck and (visits == 1).all(), (dims, int((visits != 1).sum()))
        assert (g["step_k"] * g["tiles_y"] + g["step_y"]) * g["tiles_x"] + g["step_x"] == g["nblk"]


@pytest.mark.parametrize("carry", ["x", "y"])
def test_a_walk_without_a_carry_is_wrong_on_the_rows_and_was_right_on_the_earlier_grids(K, carry):
    """The gap this table closes, written down: leave the x-carry out of vol_next_tile and the three grids the GPU suite compared
    with the model before still have every tile visited exactly once; none of the rows that are in the table for the carry has.
    The same for the y-carry on the one earlier grid whose step_y is zero."""
    off = {carry + "_carry": False}
    rows = [r for r in G.VOLUME if carry in r["carry"]]
    assert len(rows) >= 5
    for r in rows:
        wrong = G.wrong_tiles(G.volume_geometry(r["dims"], K), **off)
        print(f"{r['name']}: {len(wrong)} tiles not visited exactly once without the {carry}-carry")
        assert wrong, r["name"]
    earlier = [len(G.wrong_tiles(G.volume_geometry(d, K), **off)) for d in G.EARLIER_VOLUME_GRIDS]
    print(f"earlier grids {G.EARLIER_VOLUME_GRIDS}: {earlier}")
    if carry == "x":
        assert earlier == [0, 0, 0], earlier
    else:
        assert earlier[0] == 0 and earlier[1] > 0 and earlier[2] > 0, earlier   # the pinned grid alone never took it


# ---- the volume rows are valid, non-trivial inputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r["name"] for r in G.VOLUME])
def test_volume_row_is_a_valid_input(name):
    run = G.volume_run(name)
    r, g = run["row"], run["geometry"]
    n_points = len(run["points"][0])
    assert len(run["keys"]) == n_points                                    # edge_keys is extract_model's order
    print(f"{name}: updated / in band {run['counts']}, {n_points} points, mid-voxel capacity {run['mid']}")
    if r["kind"] == "rendered":
        assert n_points > 1000 and all(u > 10_000 and b > 0 for u, b in run["counts"])
    elif name == "tiny2":
        # tiny_cases()' non-rotation poses and a grid beside the image: the row exists for what is NOT updated
        assert n_points == 0 and all(u == 0 for u, _ in run["counts"])
    else:
        assert n_points > 0 and all(u > 0 for u, _ in run["counts"])
    if name == "321x77x41":
        assert run["first"][1][:, :, 320].any()                            # the one live lane of the last x tile writes
    if name == "65x5x2":
        assert run["first"][1][:, 4, 64].any() and run["first"][1][:, :4, 64].any() and run["first"][1][:, 4, :64].any()   # the spill
    # the condition on the carry rows: a walk without the carry differs from the model where the first frame writes
    tx, ty = g["tile"]
    w1 = run["first"][1]
    for carry in r["carry"]:
        wrong = G.wrong_tiles(g, **{carry + "_carry": False})
        hit = [t for t in wrong if w1[t[2], t[1] * ty:(t[1] + 1) * ty, t[0] * tx:(t[0] + 1) * tx].any()]
        print(f"{name}: without the {carry}-carry {len(wrong)} tiles are wrong, the first frame updates voxels in {len(hit)} of them")
        assert hit, (name, carry)
        if len(wrong) == 2:
            assert len(hit) == 2, (name, carry)


def test_the_volume_rows_between_them():
    runs = [G.volume_run(r["name"]) for r in G.VOLUME]
    zero = sum(int((x["points"][1][:, :3] == 0).all(1).sum()) for x in runs)
    total = sum(len(x["points"][0]) for x in runs)
    assert 0 < zero < total                                                # points with and without a normal
    assert any(x["p"]["max_weight"] < len(x["frames"]) and (x["last"][1] == x["p"]["max_weight"]).sum() > 1000 for x in runs)   # saturation
    # a capacity that cuts an extraction inside a voxel exists among the rendered and among the small rows
    for kind in ("rendered", "small", "tiny"):
        mids = [x for x in runs if x["row"]["kind"] == kind and x["mid"] is not None]
        assert mids, kind
        for x in mids:
            v = x["keys"] // 3
            assert v[x["mid"] - 1] == v[x["mid"]] and (x["mid"] < 2 or v[x["mid"] - 2] != v[x["mid"] - 1])
    assert G.volume_run("700x150x100")["mid"] is not None                  # the scan's chunk loop and the mid-voxel cut together


def test_the_tiny_rows_reach_every_skip_class():
    from test_volume_cpu import empty_grid, integrate_loop
    total = {}
    for r in G.VOLUME:
        if r["kind"] != "tiny":
            continue
        p, frames = G.volume_inputs(r)
        q, w = empty_grid(p)
        for raw, pose in frames:
            q, w, met = integrate_loop(q, w, raw, pose, p)
            for k, v in met.items():
                total[k] = total.get(k, 0) + v
        assert np.array_equal(q, G.volume_run(r["name"])["last"][0]) and np.array_equal(w, G.volume_run(r["name"])["last"][1])
    assert all(v > 0 for v in total.values()), total


# ---- the map rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r["name"] for r in G.MAP])
def test_map_row_is_a_valid_input(name):
    size = G.map_row(name)["size"]
    inputs = G.map_inputs(size)
    large = size[0] * size[1] >= G.MAP_RANDOM_BELOW
    for voxel in (0.0, G.MAP_VOXEL):
        trail, ref = G.map_model(size, G.map_capacity(size), voxel, inputs)
        st = ref.st
        print(f"{name} voxel {voxel}: {st}")
        assert st["insertions"] == 3 and st["dropped_capacity"] == 0
        assert st["candidates"] > 0 and st["size"] > 0
        if large:
            assert st["size"] > 10_000 and (voxel == 0.0 or st["dropped_voxel"] > 0)
    if size[0] * size[1] > 1 and not large:                               # masked, invalid and negative pixels all occur
        val, dep, _, _ = inputs[0]
        d = dep.reshape(-1)
        assert (val == 0).any() and (np.abs(d) < 0.01).any() and (d < -0.01).any() and (d > 0.01).any()


@pytest.mark.parametrize("size", G.MAP_SPECIAL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_contention_range_and_mask_rows(size):
    from test_gpu_map import ref_candidates
    inputs = G.map_inputs(size)
    # one voxel for (nearly) everything: the first insertion keeps the lowest-index pixel of each voxel, the second keeps nothing
    far = G.shifted(inputs[:2], 200.0)
    trail, ref = G.map_model(size, G.map_capacity(size), 1e4, far)
    n0 = len(ref_candidates(far[0][0], far[0][1]))
    assert 1 <= trail[0][1] <= 8 and trail[1][1] == trail[0][1], trail
    assert trail[0][0]["dropped_voxel"] > 0.9 * n0 and ref.st["dropped_voxel"] == ref.st["candidates"] - ref.st["size"]
    first = ref_candidates(far[0][0], far[0][1])[0]
    assert ref.kp[0].tolist() == [0, first]
    # a voxel so small that keys in and out of range mix in one insertion
    trail, ref = G.map_model(size, G.map_capacity(size), 1e-5, inputs)
    st0 = trail[0][0]
    assert 0 < st0["dropped_range"] < st0["candidates"], st0
    # mask and filter together
    masked = G.with_mask(inputs)
    trail, ref = G.map_model(size, G.map_capacity(size), G.MAP_VOXEL, masked)
    _, plain = G.map_model(size, G.map_capacity(size), G.MAP_VOXEL, [(None,) + x[1:] for x in masked])
    assert 0 < ref.st["candidates"] < plain.st["candidates"] and ref.st["size"] > 0


@pytest.mark.parametrize("size", G.MAP_SPECIAL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_capacity_cuts_fall_where_the_rows_say(K, size):
    cuts, (p0, p1) = G.capacity_cuts(size)
    inputs = G.map_inputs(size)
    assert len(p0) > 4 and len(p1) > 1
    block = K["kMapBlock"]
    cap = cuts["wave"][0]
    assert 0 < cap < len(p0) and p0[cap - 1] // 64 < p0[cap] // 64          # the next survivor sits in a later wave
    if G.map_geometry(size, K)["nblk"] > 1:
        assert p0[cap - 1] // block == p0[cap] // block                     # ... of the same block
        cap = cuts["block"][0]
        assert 0 < cap < len(p0) and p0[cap - 1] // block < p0[cap] // block
    else:
        assert cuts["block"][0] == len(p0)                                  # one block: its last survivor ends the insertion
    for name, (cap, n) in cuts.items():
        trail, ref = G.map_model(size, cap, G.MAP_VOXEL, inputs[:n])
        print(f"{size} {name}: capacity {cap}, {ref.st}")
        assert ref.st["size"] == cap
    trail, _ = G.map_model(size, cuts["one"][0], G.MAP_VOXEL, inputs)
    assert trail[0][0]["dropped_capacity"] == 0 and trail[1][1] == trail[0][1] + 1 and trail[1][0]["dropped_capacity"] == len(p1) - 1
    trail, _ = G.map_model(size, cuts["end"][0], G.MAP_VOXEL, inputs)
    assert trail[1][0]["dropped_capacity"] == 0 and trail[2][0] == dict(trail[1][0], insertions=3)   # a counted no-op


# ---- the front-end rows -----------------------------------------------------------------------------------------------------------------
def test_frontend_rows_are_valid_inputs():
    seen = dict(dropped_behind=0, dropped_range=0, dropped_splat=0)
    for name, variant in G.frontend_cases():
        x = G.frontend_inputs(name, variant)
        st = G.frontend_want(name, variant)[2]
        print(f"{name} {variant}: {st}")
        assert x["colour"].shape == x["rig"]["size"] + (4,) and x["raw"].shape == x["rig"]["depth_size"]
        assert st["n_depth"] == int((x["raw"] != 0).sum()) > 0
        if variant == "flipped":
            assert st["dropped_behind"] == st["n_depth"] and st["n_filled"] == 0
        else:
            assert st["n_filled"] > 0
        if G.frontend_row(name)["tiny"]:
            for k in seen:
                seen[k] += st[k]
            if variant in ("near_plane", "flipped"):
                assert st["dropped_behind"] > 0
            if variant == "scale_out":
                assert st["dropped_range"] > 0
            if variant == "magnify":
                assert 0 < st["dropped_splat"] < st["n_depth"]
        else:
            assert st["n_filled"] > x["rig"]["size"][0] * x["rig"]["size"][1] // 2
    assert all(v > 0 for v in seen.values()), seen
