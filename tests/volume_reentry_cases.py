"""The re-entry store of the moving TSDF volume (odo_volume_enable_reentry): the numpy model of the
specification over shift_model / leaves_model of tests/test_volume_shift_cpu.py, the same as plain loops, and the table of rows that
tests/test_volume_reentry_cpu.py holds on the model and tests/test_gpu_volume_reentry.py asks the GPU for, bit for bit.

A store is a dict: g (m, 3) int64 global voxel indices, vox (m,) uint32 voxel words, col (m,) uint32 colour words or None (a store
without colours), and the four counters live, saved, restored, dropped. A colour grid is (nz, ny, nx, 4) uint8; its word is the four
bytes read little-endian, as the device holds it."""
import functools

import numpy as np

from test_volume_cpu import params, tiny_cases, words
from test_volume_shift_cpu import leaves_model, offset_model, shift_model, shifts_for

OFF0 = (0, 0, 0)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def colour_words(col):
    """(nz, ny, nx, 4) uint8 -> (n,) uint32 in raster order."""
    return np.ascontiguousarray(col, np.uint8).reshape(-1, 4).view("<u4").reshape(-1).copy()


def unwords(W, shape):
    """(n,) uint32 -> q int16, w uint16 of `shape`."""
    return (W & 0xFFFF).astype(np.uint16).view(np.int16).reshape(shape), (W >> 16).astype(np.uint16).reshape(shape)


def empty_store(colour):
    return dict(g=np.zeros((0, 3), np.int64), vox=np.zeros(0, np.uint32), col=np.zeros(0, np.uint32) if colour else None,
                live=0, saved=0, restored=0, dropped=0)


def reentry_model(q, w, col, off, store, d, capacity):
    """One shift by d != 0 of the grid (q, w, col; col may be None) in the window `off` with the store `store` of `capacity` entries:
    (q2, w2, col2, off2, store2). Restore, keep, save, in that order."""
    nz, ny, nx = q.shape
    dims = np.array([nx, ny, nz], np.int64)
    off2 = offset_model(off, d)
    assert off2 is not None and tuple(d) != (0, 0, 0)
    q2, w2, c2 = shift_model(q, w, col, d)
    W2 = words(q2, w2).copy()
    C2 = colour_words(c2) if c2 is not None else None
    # restore
    t = store["g"] - np.array(off2, np.int64)
    inside = ((t >= 0) & (t < dims)).all(1)
    at = (t[inside, 2] * ny + t[inside, 1]) * nx + t[inside, 0]
    W2[at] = store["vox"][inside]
    if store["col"] is not None and C2 is not None:
        C2[at] = store["col"][inside]
    # keep
    kept = ~inside
    # save: the leaving voxels with a non-zero bit, in raster order
    W = words(q, w)
    some = W != 0
    if col is not None:
        some = some | (colour_words(col) != 0)
    sel = np.nonzero(leaves_model(q.shape, d).reshape(-1) & some)[0]
    take = min(len(sel), capacity - int(kept.sum()))
    sel_in = sel[:take]
    k, rem = np.divmod(sel_in, nx * ny)
    j, i = np.divmod(rem, nx)
    g_new = np.stack([i, j, k], 1).astype(np.int64) + np.array(off, np.int64)
    out = dict(g=np.concatenate([store["g"][kept], g_new]), vox=np.concatenate([store["vox"][kept], W[sel_in]]), col=None)
    if store["col"] is not None:
        out["col"] = np.concatenate([store["col"][kept], colour_words(col)[sel_in]])
    out.update(live=len(out["g"]), saved=store["saved"] + take, restored=store["restored"] + int(inside.sum()),
               dropped=store["dropped"] + len(sel) - take)
    q2, w2 = unwords(W2, q.shape)
    if C2 is not None:
        c2 = C2.view(np.uint8).reshape(q.shape + (4,))
    return q2, w2, c2, off2, out


def reentry_loop(q, w, col, off, store, d, capacity):
    """The same from the prose, voxel by voxel and entry by entry."""
    nz, ny, nx = q.shape
    dims = (nx, ny, nz)
    off2 = tuple(int(a) + int(b) for a, b in zip(off, d))
    q2, w2 = np.zeros_like(q), np.zeros_like(w)
    c2 = None if col is None else np.zeros_like(col)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                s = (i + d[0], j + d[1], k + d[2])
                if all(0 <= s[c] < dims[c] for c in range(3)):
                    q2[k, j, i], w2[k, j, i] = q[s[2], s[1], s[0]], w[s[2], s[1], s[0]]
                    if col is not None:
                        c2[k, j, i] = col[s[2], s[1], s[0]]
    g, vox, cw = [], [], []
    restored = 0
    for e in range(len(store["g"])):
        t = [int(store["g"][e][c]) - off2[c] for c in range(3)]
        if all(0 <= t[c] < dims[c] for c in range(3)):
            word = int(store["vox"][e])
            assert q2[t[2], t[1], t[0]] == 0 and w2[t[2], t[1], t[0]] == 0     # it overwrites zeros only
            q2[t[2], t[1], t[0]] = (word & 0xFFFF) - (65536 if word & 0x8000 else 0)
            w2[t[2], t[1], t[0]] = word >> 16
            if store["col"] is not None and c2 is not None:
                c2[t[2], t[1], t[0]] = np.array([int(store["col"][e])], "<u4").view(np.uint8)
            restored += 1
        else:
            g.append([int(x) for x in store["g"][e]])
            vox.append(int(store["vox"][e]))
            if store["col"] is not None:
                cw.append(int(store["col"][e]))
    saved = dropped = 0
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                v = (i, j, k)
                if all(0 <= v[c] - d[c] < dims[c] for c in range(3)):
                    continue
                word = (int(w[k, j, i]) << 16) | (int(q[k, j, i]) & 0xFFFF)
                cword = int(np.ascontiguousarray(col[k, j, i]).view("<u4")[0]) if col is not None else 0
                if word == 0 and cword == 0:
                    continue
                if len(g) >= capacity:
                    dropped += 1
                    continue
                g.append([off[c] + v[c] for c in range(3)])
                vox.append(word)
                if store["col"] is not None:
                    cw.append(cword)
                saved += 1
    out = dict(g=np.array(g, np.int64).reshape(-1, 3), vox=np.array(vox, np.uint32), col=np.array(cw, np.uint32) if store["col"] is not None else None,
               live=len(g), saved=store["saved"] + saved, restored=store["restored"] + restored, dropped=store["dropped"] + dropped)
    return q2, w2, c2, off2, out


def stores_equal(a, b):
    return all(a[k] == b[k] for k in ("live", "saved", "restored", "dropped")) and np.array_equal(a["g"], b["g"]) and \
        np.array_equal(a["vox"], b["vox"]) and (a["col"] is None) == (b["col"] is None) and \
        (a["col"] is None or np.array_equal(a["col"], b["col"]))


def invariant_holds(store, off, dims):
    """Between shifts every stored g lies outside the window and no g occurs twice."""
    t = store["g"] - np.array(off, np.int64)
    outside = ~((t >= 0) & (t < np.array(dims, np.int64))).all(1)
    return bool(outside.all()) and len(np.unique(store["g"], axis=0)) == len(store["g"])


def walk_model(q, w, col, shifts, capacity, store_colour=None, off=OFF0, step=reentry_model):
    """Every state of a walk: [(q, w, col, off, store)] in front of the first shift and behind each one."""
    store = empty_store(col is not None if store_colour is None else store_colour)
    states = [(q, w, col, tuple(off), store)]
    for d in shifts:
        q, w, col, off, store = step(q, w, col, off, store, d, capacity)
        states.append((q, w, col, off, store))
    return states


# ---- content -------------------------------------------------------------------------------------------------------------------
def random_content(dims, seed):
    """q, w, col with every bit pattern in play: w = 0 beside q != 0, colours without weights, and 20 % of the voxels all zero."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    shape = (nz, ny, nx)
    q = rng.integers(-32768, 32768, shape).astype(np.int16)
    w = rng.integers(0, 65536, shape).astype(np.uint16)
    w[rng.uniform(size=shape) < 0.15] = 0           # w = 0 with any q: saved for its bits, not for its weight
    col = rng.integers(0, 256, shape + (4,)).astype(np.uint8)
    col[rng.uniform(size=shape) < 0.3] = 0          # no colour bits beside voxel bits
    only_colour = rng.uniform(size=shape) < 0.1     # no voxel bits beside colour bits
    q[only_colour], w[only_colour] = 0, 0
    zero = rng.uniform(size=shape) < 0.2
    q[zero], w[zero], col[zero] = 0, 0, 0
    return q, w, col


@functools.lru_cache(maxsize=None)
def grids():
    """name -> (p, q, w, col): the dimensions of test_volume_shift_cpu.grids() (2 x 2 x 2, 64 x 4 x 4, 65 x 5 x 4 and the four tiny
    volumes of test_volume_cpu) with random_content."""
    out = {}
    cases = [((2, 2, 2), 0.5, (0.25, -0.5, 1.0)), ((64, 4, 4), 0.04, (-1.3, 0.1, 0.7)), ((65, 5, 4), 0.04, (-1.3, 0.1, 0.7))]
    for n, (dims, vs, origin) in enumerate(cases):
        p = params((40.0, 15.5, 11.5), 1000.0, (24, 32), dims=dims, vs=vs, origin=origin)
        out["random %dx%dx%d" % dims] = (p,) + random_content(dims, 41 + n)
    for n, (p, _) in enumerate(tiny_cases()):
        out["tiny %d" % n] = (p,) + random_content(p["dims"], 51 + n)
    return out


def neg(d):
    return tuple(-x for x in d)


def walk_for(dims, n):
    """Row n of a grid: its n-th shift d, the next of the list e, then -d and -e: a closed walk whose second shift finds a store."""
    s = shifts_for(dims)
    d, e = s[n], s[(n + 1) % len(s)]
    return [d, e, neg(d), neg(e)]


def rows():
    """(name, n, p, q, w, col, shifts): 7 grids x 14 shifts."""
    return [(name, n, p, q, w, col, walk_for(p["dims"], n)) for name, (p, q, w, col) in grids().items() for n in range(14)]


# a closed walk that mixes axes and signs, one |d_c| >= n_c included (dims 64 x 4 x 4: dy = -4 empties the window)
CLOSED_WALK = [(3, 0, 0), (0, 1, -1), (-5, 0, 2), (0, -4, 0), (1, 2, 0), (0, 0, -1), (1, 1, 0)]
assert tuple(np.sum(CLOSED_WALK, 0)) == (0, 0, 0) and len(CLOSED_WALK) >= 6

CHAIN = [(1, 0, 0)] * 24 + [(-1, 0, 0)] * 24

# restore, keep and save all non-empty in one shift (64 x 4 x 4): out along x, out along y, then back along x and on along z
MIXED = [(5, 0, 0), (0, 2, 0), (-5, 0, 1)]


def capacity_rows():
    """(capacity tag, shifts) on random 64x4x4: two shifts whose saves are n1 and n2 voxels; the capacities cut at more than the
    total, exactly the total, one less, one, and inside the second shift."""
    p, q, w, col = grids()["random 64x4x4"]
    shifts = [(2, 0, 0), (0, 1, 0)]
    st = walk_model(q, w, col, shifts, 1 << 20)
    n1, n2 = st[1][4]["live"], st[2][4]["live"] - st[1][4]["live"]
    assert n1 > 2 and n2 > 2 and st[2][4]["restored"] == 0
    return shifts, n1, n2, [n1 + n2 + 7, n1 + n2, n1 + n2 - 1, 1, n1 + n2 // 2]
