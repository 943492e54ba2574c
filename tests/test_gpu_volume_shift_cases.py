"""The moving TSDF volume's shift and spill on the GPU over the table of tests/volume_shift_cases.py, bit for bit against the models of
tests/test_volume_shift_cpu.py: the 16-byte load with dx != 0, rows of two and three trips of the quad loop in both builds with
guarded tails, more planes than the launch's y extent holds, the spill's scan at a chunk's end, the same without a colour grid and
with a store made before the colour grid, and a chain of 27 shifts enqueued back to back into stores that fill at and inside a
spill. No tolerance anywhere in this file."""
import numpy as np
import pytest

import volume_shift_cases as V
from test_gpu_volume_shift import _guard_intact, _prefill, _store_equals, _volume, _window_equals
from test_volume_cpu import bits, extract_model
from test_volume_colour_cpu import point_colours_model
from test_volume_shift_cpu import offset_model, shift_model, spill_model, window

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from odometry_amd import api
    c = api.Context(0)
    yield c
    c.close()


def _grids_equal(vol, q2, w2, c2, tag):
    gq, gw = vol.grid()
    assert np.array_equal(gw, w2) and np.array_equal(gq, q2), tag
    if c2 is not None:
        assert np.array_equal(vol.colour_grid(), c2), tag


def _extract_equals(vol, q2, w2, c2, pw, tag):
    """extract() of the shifted volume = extract_model of the shifted grid in the moved window."""
    P, N = extract_model(q2, w2, pw)
    got = vol.extract(len(P) + 16, with_dropped=True, colour=c2 is not None)
    assert len(got[0]) == len(P) and got[-1] == 0, (tag, len(got[0]), len(P))
    assert np.array_equal(bits(got[0]), bits(P)) and np.array_equal(bits(got[1]), bits(N)), tag
    if c2 is not None:
        assert np.array_equal(got[2], point_colours_model(q2, w2, c2)), tag


def _shift_row(ctx, name, colour=True, store_before_colour=False):
    """Every shift of the row in a fresh volume whose destination grids hold 0xAB, with a fresh 0xAB-filled store that has room for
    the model's spill; the first shift that leaves something in the grid is also extracted."""
    from odometry_amd import _lib as L
    row = V.find(name)
    p, q, w, col = V.inputs(name)
    col = col if colour else None
    spill_colour = colour and not store_before_colour
    extracted = False
    for d in row["shifts"]:
        tag = (name, d)
        P, N, rgba = V.spill(name, d, colour=spill_colour)
        capacity = len(P) + 64
        if store_before_colour:
            vol = _volume(ctx, p, spill=capacity)
            vol.enable_colour()
        else:
            vol = _volume(ctx, p, colour=colour)
        _prefill(vol, q, colour)           # (a store that is there already takes nothing from it: the 0xAB grid has no surface)
        off = V.OFF0
        if not store_before_colour:
            vol.enable_spill(capacity)
        vol.upload(q, w)
        if colour:
            vol.upload_colour(col)
        vol.shift(d)
        off = offset_model(off, d)
        q2, w2, c2 = shift_model(q, w, col, d)
        _grids_equal(vol, q2, w2, c2, tag)
        _window_equals(vol, p, off, tag)
        _store_equals(vol, P, N, rgba, tag)
        assert _guard_intact(vol), tag
        assert vol.stats()["frames"] == 0
        if store_before_colour:
            with pytest.raises(L.OdoError, match="no colours"):
                vol.spilled(colour=True)
        if not extracted and w2.any():
            _extract_equals(vol, q2, w2, c2, window(p, off), tag)
            extracted = True
        vol.close()
    assert extracted, name


@pytest.mark.parametrize("name", V.names())
def test_every_row_of_the_table_matches_the_model_bit_for_bit(ctx, name):
    assert V.find(name)["holds"](V.find(name)), name
    _shift_row(ctx, name)


@pytest.mark.parametrize("name", V.NO_COLOUR)
def test_rows_without_a_colour_grid(ctx, name):
    """src_col == nullptr: the shift moves one grid, the store has no colours."""
    _shift_row(ctx, name, colour=False)


@pytest.mark.parametrize("name", V.NO_COLOUR)
def test_rows_with_a_store_made_before_the_colour_grid(ctx, name):
    """The shift moves both grids, the points are spilled without colours and spilled(colour=True) is refused."""
    _shift_row(ctx, name, store_before_colour=True)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_chain_of_27_shifts_fills_the_store_at_and_inside_a_spill(ctx, which):
    """24 shifts by (1, 0, 0) and 3 by (0, 1, 0) with nothing between them, every one of which spills. The store holds the first
    min(capacity, total) points of the models' concatenation, the rest is counted as dropped, nothing is written behind the store's
    last point, and emptied it takes the next spill from its start."""
    c = V.chain()
    p, q, w, col = V.grids()["random 64x4x4"]
    capacity = c["capacities"][which]
    P, N, Cc = (np.concatenate([s[n] for s in c["spills"]]) for n in range(3))
    total = len(P)
    assert total == sum(c["counts"]) and all(n > 0 for n in c["counts"])
    vol = _volume(ctx, p, colour=True, spill=capacity)
    vol.upload(q, w)
    vol.upload_colour(col)
    for d in V.CHAIN:
        vol.shift(d)
    n = min(capacity, total)
    assert (n == total) == (which == 0)
    _store_equals(vol, P[:n], N[:n], Cc[:n], f"capacity {capacity}", dropped=total - n)
    assert _guard_intact(vol), capacity
    _grids_equal(vol, c["q"], c["w"], c["col"], capacity)
    _window_equals(vol, p, c["off"], capacity)
    # emptied, one more shift appends from the store's start
    d = (0, 0, 1)
    P1, N1, C1 = spill_model(c["q"], c["w"], c["col"], window(p, c["off"]), d)
    assert len(P1) > 0
    got = vol.spilled(clear=True, colour=True, with_dropped=True)
    assert len(got[0]) == n and got[-1] == total - n
    vol.shift(d)
    m = min(capacity, len(P1))
    _store_equals(vol, P1[:m], N1[:m], C1[:m], f"capacity {capacity}, after clear", dropped=len(P1) - m)
    _grids_equal(vol, *shift_model(c["q"], c["w"], c["col"], d), capacity)
    _window_equals(vol, p, offset_model(c["off"], d), capacity)
    vol.close()
