"""The map, volume and RGB-D front-end kernels at the launch geometries of tests/geometry_cases.py: every row of the table against the
numpy model of its subsystem, bit for bit and with exact counters — the volume's grid, statistics and extracted surface (full, cut one
point short, cut exactly, cut inside a voxel), the map after every insertion (sizes around a wave, a block and the scan's thread count,
one voxel for a whole frame, keys in and out of range, capacity cuts on wave and block boundaries), the front end through both submit
paths with a partial last wave, fewer register rows than resolve threads and a second pass. tests/test_geometry_cpu.py shows with the
models alone that each row reaches the branch it is in the table for and is a valid input. There is no tolerance in this file."""
import numpy as np
import pytest

import geometry_cases as G
from test_gpu_map import assert_same
from test_gpu_rgbd_frontend import _both_paths, _check, _frontend
from test_gpu_volume import _grid_equal, _points_equal, _volume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


# ---- volume -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r["name"] for r in G.VOLUME])
def test_volume_row_matches_the_model_bit_for_bit(ctx, name):
    run = G.volume_run(name)
    p, frames, want = run["p"], run["frames"], run["points"]
    n_points = len(want[0])
    vol = _volume(ctx, p)
    try:
        assert vol.stats() == dict(frames=0, updated=0, in_band=0, cumulative=0)
        total = 0
        for n, (raw, A) in enumerate(frames):
            vol.integrate(raw, A)
            upd, band = run["counts"][n]
            total += upd
            st = vol.stats()
            print(f"{name} frame {n}: updated {st['updated']} in band {st['in_band']} (model {upd}, {band})")
            assert st == dict(frames=n + 1, updated=upd, in_band=band, cumulative=total), (name, n, st, upd, band, total)
            if n == 0:
                _grid_equal(vol, *run["first"], f"{name} after the first integration")
        _grid_equal(vol, *run["last"], f"{name} after {len(frames)} integrations")
        got = vol.extract(n_points + 1000, with_dropped=True)
        _points_equal(got, want, name)
        assert got[2] == 0
        caps = [("one short", n_points - 1), ("exact", n_points), ("inside a voxel", run["mid"])]
        for tag, cap in caps:
            if cap is None or cap < 0:
                continue
            part = vol.extract(cap, with_dropped=True)
            _points_equal(part, (want[0][:cap], want[1][:cap]), f"{name} capacity {cap} ({tag})")
            assert part[2] == n_points - cap, (name, tag, part[2], n_points - cap)
        _points_equal(vol.extract(n_points + 1000), want, f"{name} again")   # a pure function of the volume
        _grid_equal(vol, *run["last"], f"{name} after the extractions")
    finally:
        vol.close()


# ---- map ----------------------------------------------------------------------------------------------------------------------------
def _run_map(ctx, size, capacity, voxel, inputs, tag, then_clear=False):
    """The insertions into a map of the GPU's and into the model's, compared after each one; returns the model."""
    from odometry_amd import api
    m = api.PointMap(ctx, size[0], size[1], capacity, voxel)
    ref = G.ref_map(size, capacity, voxel)
    K = G.map_K(size)
    try:
        for n, (val, dep, img, A) in enumerate(inputs):
            m.insert(val, dep, img, K, A)
            ref.insert(val, dep, img, A)
            try:
                assert_same(m, ref)
            except AssertionError as e:
                raise AssertionError(f"{tag}, insertion {n}: {e}") from e
        if then_clear:
            m.clear()
            assert m.stats() == dict(size=0, insertions=0, candidates=0, dropped_voxel=0, dropped_range=0, dropped_capacity=0)
            again = G.ref_map(size, capacity, voxel)
            val, dep, img, A = inputs[-1]
            m.insert(val, dep, img, K, A)
            again.insert(val, dep, img, A)
            assert_same(m, again)
    finally:
        m.close()
    return ref


@pytest.mark.parametrize("voxel", [0.0, G.MAP_VOXEL])
@pytest.mark.parametrize("name", [r["name"] for r in G.MAP])
def test_map_row_matches_the_model_after_every_insertion(ctx, name, voxel):
    size = G.map_row(name)["size"]
    ends = name in (G.MAP[0]["name"], G.MAP[-1]["name"])                   # clear + one more insertion at the smallest and the largest
    ref = _run_map(ctx, size, G.map_capacity(size), voxel, G.map_inputs(size), f"{name} voxel {voxel}", then_clear=ends)
    print(f"{name} voxel {voxel}: {ref.st}")
    assert ref.st["size"] > 0


@pytest.mark.parametrize("size", G.MAP_SPECIAL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_one_voxel_for_a_whole_frame(ctx, size):
    """Every candidate of a frame claims the same hash slot: one CAS word and one atomicMin word under maximal contention. The
    lowest-index pixel of each voxel survives the first insertion, nothing survives the second."""
    far = G.shifted(G.map_inputs(size)[:2], 200.0)
    ref = _run_map(ctx, size, G.map_capacity(size), 1e4, far, f"{size} voxel 1e4")
    assert 1 <= ref.st["size"] <= 8 and ref.st["dropped_voxel"] == ref.st["candidates"] - ref.st["size"]


@pytest.mark.parametrize("size", G.MAP_SPECIAL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_keys_in_and_out_of_range_in_one_insertion(ctx, size):
    ref = _run_map(ctx, size, G.map_capacity(size), 1e-5, G.map_inputs(size), f"{size} voxel 1e-5")
    assert 0 < ref.st["dropped_range"] < ref.st["candidates"]


@pytest.mark.parametrize("size", G.MAP_SPECIAL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_mask_and_filter_together(ctx, size):
    ref = _run_map(ctx, size, G.map_capacity(size), G.MAP_VOXEL, G.with_mask(G.map_inputs(size)), f"{size} mask + filter")
    assert ref.st["size"] > 0


@pytest.mark.parametrize("cut", ["wave", "block", "one", "end", "single"])
@pytest.mark.parametrize("size", G.MAP_SPECIAL_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_capacity_cut(ctx, size, cut):
    """The capacity from the model's survivor list (geometry_cases.capacity_cuts): right after the last survivor of a wave / of a
    block, with room for exactly one point, exactly at the end of an insertion (the next one is a counted no-op), and 1."""
    cuts, _ = G.capacity_cuts(size)
    cap, n = cuts[cut]
    ref = _run_map(ctx, size, cap, G.MAP_VOXEL, G.map_inputs(size)[:n], f"{size} capacity {cap} ({cut})")
    print(f"{size} {cut}: capacity {cap}, {ref.st}")
    assert ref.st["size"] == cap and ref.st["insertions"] == n


# ---- front end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("name,variant", G.frontend_cases(), ids=lambda v: str(v))
def test_frontend_row_matches_the_model_through_both_paths(name, variant, channels):
    x = G.frontend_inputs(name, variant)
    colour = np.ascontiguousarray(x["colour"][..., :channels])
    _, _, st = _both_paths(x["rig"], colour, x["raw"], x["scale_in"], x["scale_out"], channels=channels)
    print(f"{name} {variant} {channels} channels: {st}")
    assert st == G.frontend_want(name, variant)[2]


def test_frontend_register_rows_are_rewritten_every_frame():
    """171 x 224 readings: 150 register blocks, fewer than the resolve kernel's last block has threads. The same frame six times round
    a three-slot ring, two in flight behind the one checked: a register row left over from an earlier frame would show as a count
    that is off."""
    from odometry_amd import api
    name = "171x224-480x640"
    x = G.frontend_inputs(name)
    want = G.frontend_want(name)
    colour = np.ascontiguousarray(x["colour"][..., :3])
    ctx = api.Context(0)
    fe = _frontend(ctx, x["rig"], slots=3)
    try:
        c, d = fe.upload(colour), fe.upload(x["raw"])
        slots = []
        for k in range(6):
            slots.append(fe.submit(c, d))
            if k >= 2:
                _check(fe, slots[k - 2], want, f"submit {k - 2}")
                assert fe.stats(slots[k - 2][0])["frame"] == k - 2
        _check(fe, slots[4], want, "submit 4")
        _check(fe, slots[5], want, "submit 5")
        assert len({s[0].value for s in slots}) == 3
    finally:
        fe.close()
        ctx.close()
