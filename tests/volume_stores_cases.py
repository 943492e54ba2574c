"""The three stores of the moving TSDF volume used together (the point store of DESIGN.md section 9.9, the mesh store of 9.13, the
re-entry store of 9.14): the composed model, the table of rows with what each is there for as a predicate on the model, and four
switches of the composition.

stores_walk_model re-implements nothing. A shift's point spill is test_volume_shift_cpu.spill_model, its mesh spill is
volume_spill_mesh_cases.spill_of_mesh appended with store_append, both on the grid as the previous shift's
volume_reentry_cases.reentry_model left it (restored voxels included), and the grid moves on by reentry_model (by shift_model
without a re-entry store). It is the yardstick of tests/test_gpu_volume_stores.py, which asks the GPU for the same bits.

A state is a dict: q, w, col, off, and per store that the volume has a dict (None without it):
  points   xyz0, nrmw, rgba (None: a store without colours), dropped
  mesh     volume_spill_mesh_cases' store
  reentry  volume_reentry_cases' store
and `app`, what the shift that led to the state appended: points = (first, count), mesh = (first vertex, vertices, first triangle,
triangles, taken), with the counts of the spill itself in `spill` (points, vertices, triangles) whatever the stores took of it."""
import functools
import itertools

import numpy as np

import volume_reentry_cases as R
import volume_spill_mesh_cases as M
from test_volume_cpu import bits
from test_volume_colour_cpu import mesh_colours_model
from test_volume_mesh_cpu import mesh_model
from test_volume_shift_cpu import offset_model, shift_model, spill_model, window

f32 = np.float32
STORES = ("points", "mesh", "reentry")
AMPLE = dict(points=1 << 14, mesh=(1 << 14, 1 << 14), reentry=1 << 16)
ALL_COLOUR = dict(points=True, mesh=True, reentry=True)
OFF0 = (0, 0, 0)


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def empty_points(colour):
    return dict(xyz0=np.zeros((0, 4), f32), nrmw=np.zeros((0, 4), f32), rgba=np.zeros((0, 4), np.uint8) if colour else None, dropped=0)


def points_append(store, spill, capacity):
    """The clamp of test_gpu_volume_shift.py::test_two_shifts_back_to_back_and_the_clamp_at_capacity: the store is the first
    `capacity` points of the spills' concatenation, and every point behind them is counted as dropped."""
    P, N, rgba = spill
    n = min(len(P), capacity - len(store["xyz0"]))
    return dict(xyz0=np.concatenate([store["xyz0"], P[:n]]), nrmw=np.concatenate([store["nrmw"], N[:n]]),
                rgba=np.concatenate([store["rgba"], rgba[:n]]) if store["rgba"] is not None else None,
                dropped=store["dropped"] + len(P) - n), n


def stores_walk_model(p, q, w, col, shifts, capacities, colour_flags, off=OFF0, variant=None):
    """Every state of a walk, in front of the first shift and behind each one. capacities: points (int), mesh ((vertices,
    triangles)), reentry (int), None or left out for a store the volume does not have. colour_flags: per store, whether it was made
    after the colour grid (without a colour grid no store has colours). Shifts are non-zero.

    variant (the switches, each a composition error the rows must catch):
      "stale"        the spills read the grid as it was in front of the previous shift's restore (a stale grid pointer)
      "no-offset"    after a refused append the mesh store's later appends are not offset by its fill
      "colour"       the re-entry store keeps and restores colours although it was made without them
      "save-behind"  the re-entry save runs behind the shift and reads the shifted grid"""
    cap = {s: capacities.get(s) for s in STORES}
    has = {s: col is not None and bool(colour_flags[s]) for s in STORES}
    if variant == "colour":
        has["reentry"] = col is not None
    st = dict(q=q, w=w, col=col, off=tuple(off), app=None, spill=None,
              points=empty_points(has["points"]) if cap["points"] else None,
              mesh=M.empty_store(has["mesh"]) if cap["mesh"] else None,
              reentry=R.empty_store(has["reentry"]) if cap["reentry"] else None)
    states, stale, refused = [st], (q, w, col), False
    for d in shifts:
        d = tuple(int(x) for x in d)
        assert d != (0, 0, 0)
        q, w, col, off = st["q"], st["w"], st["col"], st["off"]
        gq, gw, gc = stale if variant == "stale" else (q, w, col)      # what the two spills read
        pw, dims = window(p, off), p["dims"]
        nxt = dict(app={}, spill={})
        nxt["points"] = nxt["mesh"] = nxt["reentry"] = None
        # the point spill
        P = spill_model(gq, gw, gc if has["points"] else None, pw, d)
        nxt["spill"]["points"] = len(P[0])
        if cap["points"]:
            nxt["points"], n = points_append(st["points"], P, cap["points"])
            nxt["app"]["points"] = (len(st["points"]["xyz0"]), n)
        # the mesh spill
        mesh = mesh_model(gq, gw, pw, detail=True)
        colours = mesh_colours_model(gq, gw, gc) if has["mesh"] else None
        unoffset = "no-offset" if variant == "no-offset" and refused else None
        spill_fn = lambda fill: M.spill_of_mesh(mesh, colours, d, dims, fill, unoffset)
        whole = spill_fn((0, 0))
        nxt["spill"]["mesh"] = (len(whole[0]), len(whole[2]))
        if cap["mesh"]:
            nxt["mesh"], ok = M.store_append(st["mesh"], spill_fn, cap["mesh"])
            refused = refused or not ok
            nxt["app"]["mesh"] = (len(st["mesh"]["xyz0"]), len(whole[0]) if ok else 0, len(st["mesh"]["tri"]), len(whole[2]) if ok else 0, ok)
        # the shift, with the re-entry store's restore, keep and save round it
        stale = shift_model(q, w, col, d)
        if cap["reentry"]:
            q2, w2, c2, off2, store = R.reentry_model(q, w, col, off, st["reentry"], d, cap["reentry"])
            if variant == "save-behind":     # the same restore and keep; what is saved is read from the shifted grid
                store = R.reentry_model(*stale, off, st["reentry"], d, cap["reentry"])[4]
            nxt["reentry"] = store
        else:
            (q2, w2, c2), off2 = stale, offset_model(off, d)
        nxt.update(q=q2, w=w2, col=c2, off=off2)
        states.append(nxt)
        st = nxt
    return states


def points_equal(a, b):
    return (len(a["xyz0"]) == len(b["xyz0"]) and np.array_equal(bits(a["xyz0"]), bits(b["xyz0"])) and
            np.array_equal(bits(a["nrmw"]), bits(b["nrmw"])) and (a["rgba"] is None) == (b["rgba"] is None) and
            (a["rgba"] is None or np.array_equal(a["rgba"], b["rgba"])) and a["dropped"] == b["dropped"])


def mesh_equal(a, b):
    return (a["rgba"] is None) == (b["rgba"] is None) and M.store_equal(a, b)


EQUAL = dict(points=points_equal, mesh=mesh_equal, reentry=R.stores_equal)


def grids_equal(a, b):
    return (a["off"] == b["off"] and np.array_equal(a["q"], b["q"]) and np.array_equal(a["w"], b["w"]) and
            (a["col"] is None) == (b["col"] is None) and (a["col"] is None or np.array_equal(a["col"], b["col"])))


def states_equal(a, b):
    """Two walks: the same grids, windows and stores behind every shift."""
    return len(a) == len(b) and all(grids_equal(x, y) and all((x[s] is None) == (y[s] is None) and (x[s] is None or EQUAL[s](x[s], y[s]))
                                                               for s in STORES) for x, y in zip(a, b))


def logs_equal(a, b, store):
    """One store of two walks: the same contents and counters behind every shift."""
    return len(a) == len(b) and all(EQUAL[store](x[store], y[store]) for x, y in zip(a, b))


# ---- what a shift appended -----------------------------------------------------------------------------------------------------------
def appended_points(states, n):
    """xyz0, nrmw, rgba that shift n (1-based) appended to the point store."""
    first, count = states[n]["app"]["points"]
    s = states[n]["points"]
    return s["xyz0"][first:first + count], s["nrmw"][first:first + count], (None if s["rgba"] is None else s["rgba"][first:first + count])


def appended_mesh(states, n):
    """xyz0, nrmw, tri (the store's indices), rgba that shift n appended to the mesh store, and the store's vertex fill before it."""
    v0, nv, t0, nt, _ = states[n]["app"]["mesh"]
    s = states[n]["mesh"]
    return s["xyz0"][v0:v0 + nv], s["nrmw"][v0:v0 + nv], s["tri"][t0:t0 + nt], (None if s["rgba"] is None else s["rgba"][v0:v0 + nv]), v0


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def counts(states):
    """What the stores saw over the walk: points, vertices and triangles appended, voxels saved and restored."""
    end = states[-1]
    return dict(points=len(end["points"]["xyz0"]) if end["points"] else 0, vertices=len(end["mesh"]["xyz0"]) if end["mesh"] else 0,
                triangles=len(end["mesh"]["tri"]) if end["mesh"] else 0, saved=end["reentry"]["saved"] if end["reentry"] else 0,
                restored=end["reentry"]["restored"] if end["reentry"] else 0)


# ---- the walks -----------------------------------------------------------------------------------------------------------------------
GRID = "dyadic 9x8x7 20%"
D = (2, -1, 1)
WHOLE = (9, 0, 0)                                                    # |dx| = nx: the whole window leaves
TWICE = [D, R.neg(D), D]
TWO_PIECES = [D, (-1, 0, 1), (-1, 1, -2), D]      # (the second goes on along z while x comes back: its leaving plane is not empty)
# the overflow walk: a small first spill, a large second one (refused by a mesh store one item short of it, cut by the point store,
# partly dropped by the re-entry store), the way back, and the small one again, which the mesh store takes behind its first
OVERFLOW = [(0, 0, 1), D, R.neg(D), (0, 0, -1), (0, 0, 1)]


def grid(name=GRID):
    return M.all_grids()[name]


@functools.lru_cache(maxsize=None)
def short_capacities():
    """Per store, the capacity one item short of what OVERFLOW needs at the store's second non-empty append, from the ample walk
    (the mesh store a vertex short: either count refuses the whole spill)."""
    p, q, w, col = grid()
    st = stores_walk_model(p, q, w, col, OVERFLOW, AMPLE, ALL_COLOUR)
    pts = [s["app"]["points"] for s in st[1:] if s["app"]["points"][1] > 0]
    msh = [s["app"]["mesh"] for s in st[1:] if s["app"]["mesh"][1] > 0]
    # (what the re-entry store needs at a save is its live count behind it: the entries it kept and the ones it appended)
    need = [b["reentry"]["live"] for a, b in zip(st, st[1:]) if b["reentry"]["saved"] > a["reentry"]["saved"]]
    return dict(points=pts[1][0] + pts[1][1] - 1, mesh=(msh[1][0] + msh[1][1] - 1, AMPLE["mesh"][1]), reentry=need[1] - 1)


# ---- the predicates ------------------------------------------------------------------------------------------------------------------
def _walk(row, **change):
    r = dict(row, **change)
    p, q, w, col = grid(r["grid"])
    return stores_walk_model(p, q, w, col, r["shifts"], r["capacities"], r["colour_flags"], variant=r.get("variant"))


def _twice(row, st):
    """Appends 1 and 3 are the same bytes for points and vertices, the third append's triangles are the first's plus the store's
    fill, and voxels were restored."""
    a, b = appended_points(st, 1), appended_points(st, 3)
    m1, m3 = appended_mesh(st, 1), appended_mesh(st, 3)
    return (len(a[0]) > 0 and all(same_bits(x, y) for x, y in zip(a, b)) and len(m1[0]) > 0 and len(m1[2]) > 0 and
            all(same_bits(m1[i], m3[i]) for i in (0, 1, 3)) and m3[4] > m1[4] == 0 and np.array_equal(m3[2], m1[2] + m3[4]) and
            st[-1]["reentry"]["restored"] > 0)


def _two_pieces(row, st):
    """The second and third shifts restore one piece each; the second also keeps and saves, and its mesh spill is not empty: a partly
    restored slab is spilled."""
    a, b, c = st[1]["reentry"], st[2]["reentry"], st[3]["reentry"]
    kept = b["live"] - (b["saved"] - a["saved"])
    return (b["restored"] > a["restored"] and kept > 0 and b["saved"] > a["saved"] and st[2]["spill"]["mesh"][0] > 0 and
            c["restored"] > b["restored"] and st[4]["spill"]["points"] > 0 and st[4]["spill"]["mesh"][1] > 0)


def _closed(row, st):
    """The re-entry store ends empty, the grid ends as it started, and all three stores were used on the way."""
    c = counts(st)
    return (st[-1]["reentry"]["live"] == 0 and st[-1]["off"] == st[0]["off"] and grids_equal(st[-1], st[0]) and
            min(c.values()) > 0 and st[-1]["reentry"]["dropped"] == 0)


def first_grid_difference(a, b):
    """The first shift (1-based) behind which the grids of two walks differ; None: never."""
    return next((n for n in range(1, len(a)) if not grids_equal(a[n], b[n])), None)


def _overflow(row, st):
    """Every store equals that of the walk in which the other two are ample; the point and mesh logs depend on the re-entry store's
    capacity from the first shift on that reads a grid with a dropped voxel missing, and on nothing else."""
    short, caps = row["short"], row["capacities"]
    ok = True
    for s in STORES:
        alone = dict(AMPLE, **{s: caps[s]})
        if s != "reentry":
            alone["reentry"] = caps["reentry"]                    # (the grid that the spills read is the re-entry store's work)
        ok = ok and logs_equal(st, _walk(row, capacities=alone), s)
    ample = _walk(row, capacities=AMPLE)
    if "reentry" in short:
        k = first_grid_difference(st, ample)
        free = _walk(row, capacities=dict(AMPLE, reentry=caps["reentry"]))     # (the other two ample: every spill is appended)
        full = _walk(row, capacities=AMPLE)
        ok = ok and k is not None and st[-1]["reentry"]["dropped"] > 0 and st[-1]["reentry"]["restored"] > 0
        for n in range(1, len(st)):
            same = all(same_bits(x, y) for x, y in zip(appended_points(free, n), appended_points(full, n))) and \
                free[n]["spill"] == full[n]["spill"]
            ok = ok and (same or n > k)                            # up to shift k the spills read equal grids
        ok = ok and any(free[n]["spill"] != full[n]["spill"] for n in range(k + 1, len(st)))
    else:
        ok = ok and st[-1]["reentry"]["dropped"] == 0 and grids_equal(st[-1], ample[-1])
    if "points" in short:
        ok = ok and st[-1]["points"]["dropped"] > 0 and len(st[-1]["points"]["xyz0"]) == caps["points"]
    else:
        ok = ok and st[-1]["points"]["dropped"] == 0
    taken = [s["app"]["mesh"][4] for s in st[1:]]
    if "mesh" in short:          # the large spill is refused; a later, smaller one is appended behind the first
        ok = ok and not taken[1] and st[-1]["mesh"]["dropped"][0] > 0 and \
            any(t and s["app"]["mesh"][0] > 0 and s["app"]["mesh"][3] > 0 for t, s in zip(taken[2:], st[3:]))
    else:
        ok = ok and all(taken) and st[-1]["mesh"]["dropped"] == (0, 0)
    return ok


def _mixed_colour(row, st):
    """The third append's colours differ from the first's while its positions do not: the restored voxels came back with colour word
    0, and the coloured point and mesh stores log those."""
    a, b = appended_points(st, 1), appended_points(st, 3)
    m1, m3 = appended_mesh(st, 1), appended_mesh(st, 3)
    return (st[-1]["reentry"]["col"] is None and st[-1]["reentry"]["restored"] > 0 and len(a[0]) > 0 and len(m1[0]) > 0 and
            same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and not same_bits(a[2], b[2]) and
            same_bits(m1[0], m3[0]) and same_bits(m1[1], m3[1]) and not same_bits(m1[3], m3[3]) and np.array_equal(m3[2], m1[2] + m3[4]))


def _subset(row, st):
    """A store's log does not depend on whether the point or the mesh store is there; it depends on the re-entry store as the model
    says: without it the grid is shift_model's and the third shift finds the slab empty."""
    have = row["stores"]
    both = AMPLE if "reentry" in have else dict(AMPLE, reentry=None)
    full = _walk(row, capacities=both)
    ok = all(logs_equal(st, full, s) for s in have) and all(grids_equal(x, y) for x, y in zip(st, full))
    if "reentry" in have:
        ok = ok and st[-1]["reentry"]["restored"] > 0 and st[3]["spill"] == st[1]["spill"]
    else:
        p, q, w, col = grid(row["grid"])
        m = (q, w, col)
        for d, s in zip(row["shifts"], st[1:]):
            m = shift_model(*m, d)
            ok = ok and np.array_equal(s["q"], m[0]) and np.array_equal(s["w"], m[1]) and np.array_equal(s["col"], m[2])
        ok = ok and st[3]["spill"]["points"] == 0 and st[3]["spill"]["mesh"][1] == 0 and st[1]["spill"]["points"] > 0
    return ok


# ---- the rows ------------------------------------------------------------------------------------------------------------------------
def _row(name, shifts, holds, reason, grid=GRID, capacities=AMPLE, colour_flags=ALL_COLOUR, **more):
    return dict(name=name, grid=grid, shifts=list(shifts), capacities=dict(capacities), colour_flags=dict(colour_flags), holds=holds,
                reason=reason, stores=tuple(s for s in STORES if capacities.get(s)), **more)


def _subsets():
    return [c for n in (1, 2, 3) for c in itertools.combinations(STORES, n)]


@functools.lru_cache(maxsize=None)
def rows():
    out = [
        _row("twice", TWICE, _twice, "geometry that leaves, returns and leaves again is in both logs twice"),
        _row("twice, whole window", [WHOLE, R.neg(WHOLE), WHOLE], _twice, "the same with |d| = n: everything leaves and returns"),
        _row("two pieces", TWO_PIECES, _two_pieces, "back in two pieces: one shift restores, keeps, saves and spills a partly restored slab"),
        _row("closed walk", R.CLOSED_WALK, _closed, "seven shifts over all axes and signs that end where they began", grid="dyadic 9x8x7 0%"),
        _row("mixed colour", TWICE, _mixed_colour, "a re-entry store without colours beside coloured logs",
             colour_flags=dict(points=True, mesh=True, reentry=False)),
    ]
    short = short_capacities()
    for n in range(4):
        for which in itertools.combinations(STORES, n):
            caps = dict(AMPLE, **{s: short[s] for s in which})
            out.append(_row("overflow: " + (", ".join(which) or "none") + " short", OVERFLOW, _overflow,
                            "each store overflows by its own rule and the others do not notice", capacities=caps, short=which))
    for have in _subsets():
        caps = {s: AMPLE[s] if s in have else None for s in STORES}
        out.append(_row("stores: " + ", ".join(have), TWICE, _subset, "each store alone and in every company", capacities=caps))
    return out


def row(name):
    return next(r for r in rows() if r["name"] == name)


@functools.lru_cache(maxsize=None)
def row_states(name, variant=None, off=OFF0):
    r = row(name)
    p, q, w, col = grid(r["grid"])
    return stores_walk_model(p, q, w, col, r["shifts"], r["capacities"], r["colour_flags"], off=off, variant=variant)


# Which rows each switch must change; it changes no other.
#   stale        a spill store beside the re-entry store: some spill reads voxels that a restore brought back
#   no-offset    a mesh store that refuses a spill and takes a later one behind its first
#   colour       a re-entry store made before the colour grid
#   save-behind  every row with a re-entry store (the leaving slab is read after the shift has dropped it)
MUTANT_ROWS = {
    "stale": lambda r: "reentry" in r["stores"] and len(r["stores"]) > 1,
    "no-offset": lambda r: "mesh" in r.get("short", ()),
    "colour": lambda r: not r["colour_flags"]["reentry"],
    "save-behind": lambda r: "reentry" in r["stores"],
}
