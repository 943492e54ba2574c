"""The semi-global mode of the dense stereo matcher as code (include/odometry_hip.h, odo_stereo_depth_enable_sgm; DESIGN.md section
9.18), shared by tests/test_stereo_sgm_cpu.py and tests/test_gpu_stereo_sgm.py: the launch constants read out of the kernels' header,
the numpy model (the cost volume is stereo_depth_cases' census and box sum; a direction is walked one step at a time, vectorised over
its lines and the candidates), a plain-loop second implementation written independently of it (per direction, per pixel, per
candidate, Python integers), and the rows — each with the situation it is in the table for as a predicate on the model's
intermediates. Nothing here loads the GPU library.

A row is (name, L, R, params, sgm, predicate): params as in stereo_depth_cases, sgm = dict(p1, p2, paths). The model can be told to get
one of four things wrong (SWITCHES); caught_by() works out, from the unswitched model's path costs, which rows must notice."""
import functools
import os
import re

import numpy as np

import stereo_depth_cases as sdc

ROOT = sdc.ROOT
CSRC = sdc.CSRC
BIG = sdc.BIG
NONE = 65535                  # an entry of S that is not admissible
INF = 1 << 40                 # a path cost that is not there (the model works in int64)
DIRS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))
TERMS = ("a0", "a1", "a2", "P2")
SWITCHES = ("no_d_plus_1", "inadmissible_is_zero", "m_not_subtracted", "diagonal_twice")
KEEP_L = 1_000_000            # volumes up to this many entries keep every direction's costs among the model's details
LOOP_WORK = 250_000          # rows whose active pixels x candidates x paths stay below this go through the loop


def constants():
    """{kName: value} of every `constexpr int kName = <integer>;` line of the matcher's and the mode's headers."""
    out = sdc.constants()
    for name in ("stereo_sgm_math.h", "stereo_sgm.hip.h"):
        for m in re.finditer(r"^constexpr\s+int\s+(k\w+)\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, name)).read(), re.M):
            out[m.group(1)] = int(m.group(2))
    return out


def sgm(p1=None, p2=None, paths=8, A=2):
    """The penalties' defaults are api.StereoDepth.enable_sgm's: 4 and 24 times the window's area."""
    n = (2 * A + 1) ** 2
    return dict(p1=4 * n if p1 is None else p1, p2=24 * n if p2 is None else p2, paths=paths)


def check_params(rows, cols, p, sg):
    """The number of the first bound of odo_stereo_depth_enable_sgm that fails, 0 if none."""
    n = (2 * p["A"] + 1) ** 2
    if sg["p1"] < 1 or sg["p1"] > sg["p2"]:
        return 1
    if sg["paths"] not in (4, 8):
        return 2
    if sg["paths"] * (62 * n + sg["p2"]) > 65534:
        return 3
    if rows * cols * (p["dmax"] - p["dmin"] + 1) > 1 << 30:
        return 4
    return 0


def rect(rows, cols, p):
    """(x0, x1, y0, y1) of the active rectangle; empty if x1 <= x0 or y1 <= y0."""
    A = p["A"]
    return A + 4 + p["dmin"], cols - A - 4, A + 3, rows - A - 3


# ---- the model ------------------------------------------------------------------------------------------------------------------
def cost_volume(L, R, p):
    """C as (rows, cols, D) int64, INF where the candidate is not admissible: stereo_depth_cases' census, Hamming planes and box sum."""
    L, R = np.asarray(L, np.float32), np.asarray(R, np.float32)
    rows, cols = L.shape
    dmin, dmax, A = p["dmin"], p["dmax"], p["A"]
    D = dmax - dmin + 1
    cl, cr = sdc.census(L), sdc.census(R)
    H = np.zeros((D, rows, cols), np.int32)
    for i in range(D):
        d = dmin + i
        if cols - 4 > d + 4:
            H[i, :, d + 4:cols - 4] = np.bitwise_count(cl[:, d + 4:cols - 4] ^ cr[:, 4:cols - 4 - d])
    C = sdc._box(H, A).astype(np.int64)
    y, x = np.mgrid[0:rows, 0:cols]
    inner = (x >= A + 4) & (x < cols - A - 4) & (y >= A + 3) & (y < rows - A - 3)
    adm = inner[None] & (x[None] - (dmin + np.arange(D))[:, None, None] >= A + 4)
    return np.ascontiguousarray(np.where(adm, C, INF).transpose(1, 2, 0))


def step(Cp, Lq, q_active, sg, switch=None):
    """One step of a path for n pixels at once. Cp, Lq: (n, D) int64, INF where not admissible (Lq: also where q is not active);
    q_active: (n,) bool. Returns (L_r(p, .), which term took the minimum: 0 .. 3 = TERMS, -1 where the path starts or d is not
    admissible)."""
    p1, p2 = sg["p1"], sg["p2"]
    if switch == "inadmissible_is_zero":
        Lq = np.where(q_active[:, None] & (Lq >= INF), 0, Lq)
    M = np.zeros(len(Lq), np.int64) if switch == "m_not_subtracted" else np.where(q_active, Lq.min(axis=1), 0)
    pad = np.full((len(Lq), 1), INF, np.int64)
    lm = np.concatenate([pad, Lq[:, :-1]], axis=1)
    lp = np.concatenate([Lq[:, 1:], pad], axis=1)
    if switch == "no_d_plus_1":
        lp = np.full_like(lp, INF)
    terms = np.stack([np.where(Lq >= INF, INF, Lq - M[:, None]), np.where(lm >= INF, INF, lm - M[:, None] + p1),
                      np.where(lp >= INF, INF, lp - M[:, None] + p1), np.full_like(Lq, p2)])
    which = terms.argmin(axis=0)                                   # ties to the first of TERMS
    go = q_active[:, None] & (Cp < INF)
    Lp = np.where(Cp >= INF, INF, np.where(go, Cp + terms.min(axis=0), Cp))
    return Lp, np.where(go, which, -1).astype(np.int8)


def predecessors(Lr, dx, dy, r):
    """(Lq, q_active) for every pixel at once: Lr shifted by the direction, INF / False where q = p - r is not active."""
    rows, cols, D = Lr.shape
    x0, x1, y0, y1 = r
    Lq = np.full_like(Lr, INF)
    ys, yd = (slice(max(dy, 0), rows + min(dy, 0)), slice(max(-dy, 0), rows + min(-dy, 0)))
    xs, xd = (slice(max(dx, 0), cols + min(dx, 0)), slice(max(-dx, 0), cols + min(-dx, 0)))
    Lq[ys, xs] = Lr[yd, xd]
    y, x = np.mgrid[0:rows, 0:cols]
    q_active = (x - dx >= x0) & (x - dx < x1) & (y - dy >= y0) & (y - dy < y1)
    Lq[~q_active] = INF
    return Lq, q_active


def path_costs(C, p, sg, dx, dy, switch=None):
    """L_r of one direction over the whole frame, (rows, cols, D) int64 with INF where not admissible, and the winning terms."""
    rows, cols, D = C.shape
    x0, x1, y0, y1 = rect(rows, cols, p)
    Lr = np.full_like(C, INF)
    which = np.full(C.shape, -1, np.int8)
    if x1 <= x0 or y1 <= y0:
        return Lr, which
    if dy == 0:                                                    # a column at a time, all rows at once
        for x in (range(x0, x1) if dx > 0 else range(x1 - 1, x0 - 1, -1)):
            act = np.zeros(rows, bool)
            act[y0:y1] = x0 <= x - dx < x1
            Lq = Lr[:, x - dx] if x0 <= x - dx < x1 else np.full((rows, D), INF, np.int64)
            Lr[:, x], which[:, x] = step(C[:, x], Lq, act, sg, switch)
    else:                                                          # a row at a time, all columns at once
        for y in (range(y0, y1) if dy > 0 else range(y1 - 1, y0 - 1, -1)):
            Lq = np.full((cols, D), INF, np.int64)
            act = np.zeros(cols, bool)
            if y0 <= y - dy < y1:
                lo, hi = max(x0, x0 + dx), min(x1, x1 + dx)         # the p whose q's column is active
                Lq[lo:hi] = Lr[y - dy, lo - dx:hi - dx]
                act[lo:hi] = True
            Lr[y], which[y] = step(C[y], Lq, act, sg, switch)
    return Lr, which


def select(S, p):
    """Section 9.16's selection over a cost volume S (rows, cols, D) int64 with INF where not admissible: (depth, q, stats,
    details)."""
    rows, cols, D = S.shape
    dmin = p["dmin"]
    k = sdc.k_of(p)
    cost = np.where(S >= INF, BIG, S).transpose(2, 0, 1)          # (D, rows, cols)
    y, x = np.mgrid[0:rows, 0:cols]
    il, c0 = np.argmin(cost, axis=0), cost.min(axis=0)
    interior = c0 < BIG
    dl = il + dmin
    idx = np.arange(D)[:, None, None]
    c2 = np.where(np.abs(idx - il[None]) <= 1, BIG, cost).min(axis=0)
    unique = (c2 < BIG) & (c2 * (100 - p["uniq"]) > c0 * 100)
    cright = np.full((D, rows, cols), BIG, np.int64)
    for i in range(D):
        d = dmin + i
        if d < cols:
            cright[i, :, :cols - d] = cost[i, :, d:]
    dr = np.where(cright.min(axis=0) < BIG, np.argmin(cright, axis=0) + dmin, sdc.NO_RIGHT)
    lr_ok = np.abs(dr[y, np.clip(x - dl, 0, cols - 1)] - dl) <= p["lr_max"] if p["lr_max"] >= 0 else np.ones((rows, cols), bool)
    take = lambda plane: np.take_along_axis(cost, np.clip(plane, 0, D - 1)[None], axis=0)[0]
    cm = np.where(il >= 1, take(il - 1), BIG)
    cp = np.where(il + 1 <= D - 1, take(il + 1), BIG)
    have = (cm < BIG) & (cp < BIG)
    den = np.where(have, cm - 2 * c0 + cp, 0)
    num = np.where(have, cm - cp, 0)
    dpos = np.maximum(den, 1)
    f = np.where(den > 0, np.sign(num) * ((16 * np.abs(num) + dpos) // (2 * dpos)), 0)
    qv = 16 * dl + f
    with np.errstate(over="ignore"):
        ratio = k / np.maximum(qv, 1).astype(np.float32)
    assert ratio.dtype == np.float32
    raw = np.rint(ratio).astype(np.float64)
    in_range = raw <= p["max_raw"]
    outcome = np.zeros((rows, cols), np.int8)
    outcome[interior] = 1
    outcome[interior & ~unique] = 2
    outcome[interior & unique & ~lr_ok] = 3
    outcome[interior & unique & lr_ok & ~in_range] = 4
    matched = outcome == 1
    depth = np.where(matched, raw, 0).astype(np.uint16)
    q = np.where(matched, qv, 0).astype(np.uint16)
    stats = dict(interior=int(interior.sum()), matched=int(matched.sum()), rej_unique=int((outcome == 2).sum()),
                 rej_lr=int((outcome == 3).sum()), rej_range=int((outcome == 4).sum()), sum_q=int(q.astype(np.int64).sum()))
    return depth, q, stats, dict(outcome=outcome, dl=dl, f=f, c0=c0, c2=c2, dr=dr, x=x, y=y)


def directions(sg, switch=None):
    d = list(DIRS[:sg["paths"]])
    if switch == "diagonal_twice" and sg["paths"] == 8:
        d[d.index((1, 1))] = (1, -1)
    return d


def sgm_model(L, R, p, sg, switch=None, details=False):
    """(depth uint16, q uint16, stats dict, S) of one pair; S is (rows, cols, D) uint16 with 65535 where not admissible (int64 with
    INF under a switch, which may leave uint16). With details=True a fifth value: the per-pixel intermediates."""
    C = cost_volume(L, R, p)
    S = np.where(C < INF, 0, INF)
    Ls, whichs = [], []
    for dx, dy in directions(sg, switch):
        Lr, which = path_costs(C, p, sg, dx, dy, switch)
        S = S + np.where(C < INF, Lr, 0)
        Ls.append(Lr)
        whichs.append(which)
    depth, q, stats, T = select(S, p)
    if switch is None:
        assert S[C < INF].max(initial=0) <= 65534
        S = np.where(C < INF, S, NONE).astype(np.uint16)
    if not details:
        return depth, q, stats, S
    T.update(C=C, L=Ls if C.size <= KEEP_L else None, which=np.stack(whichs), adm=C < INF, n_cand=(C < INF).sum(axis=2), rect=rect(C.shape[0], C.shape[1], p))
    return depth, q, stats, S, T


def sgm_loop(L, R, p, sg):
    """The rule read off the prose, one direction, one pixel and one candidate at a time in Python integers, over the same C:
    (depth, q, stats, S). A direction visits the pixels so that q = p - r always comes before p."""
    import math
    C = cost_volume(L, R, p)
    rows, cols, D = C.shape
    dmin, dmax, A, uniq, lr_max, max_raw = (p[n] for n in ("dmin", "dmax", "A", "uniq", "lr_max", "max_raw"))
    p1, p2 = sg["p1"], sg["p2"]
    k = sdc.k_of(p)
    cands = {}
    for y in range(A + 3, rows - A - 3):
        for x in range(A + 4, cols - A - 4):
            ds = [d for d in range(dmin, dmax + 1) if x - d >= A + 4]
            if ds:
                cands[(x, y)] = ds
    cost = {(x, y): {d: int(C[y, x, d - dmin]) for d in ds} for (x, y), ds in cands.items()}
    S = {pix: dict.fromkeys(ds, 0) for pix, ds in cands.items()}
    for dx, dy in DIRS[:sg["paths"]]:
        Lr = {}
        for y in (range(rows) if dy >= 0 else range(rows - 1, -1, -1)):
            for x in (range(cols) if dx >= 0 else range(cols - 1, -1, -1)):
                if (x, y) not in cands:
                    continue
                prev = Lr.get((x - dx, y - dy))
                mine = {}
                for d in cands[(x, y)]:
                    if prev is None:
                        mine[d] = cost[(x, y)][d]
                        continue
                    m = min(prev.values())
                    opts = [p2]
                    if d in prev:
                        opts.append(prev[d] - m)
                    if d - 1 in prev:
                        opts.append(prev[d - 1] - m + p1)
                    if d + 1 in prev:
                        opts.append(prev[d + 1] - m + p1)
                    mine[d] = cost[(x, y)][d] + min(opts)
                    assert 0 <= mine[d] - cost[(x, y)][d] <= p2
                Lr[(x, y)] = mine
                for d, v in mine.items():
                    S[(x, y)][d] += v
    vol = np.full((rows, cols, D), NONE, np.uint16)
    for (x, y), sv in S.items():
        for d, v in sv.items():
            vol[y, x, d - dmin] = v

    def right_winner(xr, y):
        best = None
        for d in range(dmin, dmax + 1):
            if (xr + d, y) in S and d in S[(xr + d, y)] and (best is None or S[(xr + d, y)][d] < best[0]):
                best = (S[(xr + d, y)][d], d)
        return best[1]

    depth, q = np.zeros((rows, cols), np.uint16), np.zeros((rows, cols), np.uint16)
    n = dict.fromkeys(sdc.STATS, 0)
    for (x, y), sv in sorted(S.items()):
        n["interior"] += 1
        c0 = min(sv.values())
        dl = min(d for d in sv if sv[d] == c0)
        others = [sv[d] for d in sv if abs(d - dl) > 1]
        if not others or not (min(others) * (100 - uniq) > c0 * 100):
            n["rej_unique"] += 1
            continue
        if lr_max >= 0 and abs(right_winner(x - dl, y) - dl) > lr_max:
            n["rej_lr"] += 1
            continue
        f = 0
        if dl != dmin and dl != dmax and dl - 1 in sv and dl + 1 in sv:
            cm, cp = sv[dl - 1], sv[dl + 1]
            den, num = cm - 2 * c0 + cp, cm - cp
            if den > 0:
                f = (16 * abs(num) + den) // (2 * den)
                f = -f if num < 0 else f
        qq = 16 * dl + f
        ratio = float(k / np.float32(qq))
        lo = math.floor(ratio)
        frac = ratio - lo
        raw = lo + 1 if frac > 0.5 or (frac == 0.5 and lo % 2 == 1) else lo
        if raw > max_raw:
            n["rej_range"] += 1
            continue
        n["matched"] += 1
        n["sum_q"] += qq
        depth[y, x], q[y, x] = raw, qq
    return depth, q, n, vol


# ---- the rows ---------------------------------------------------------------------------------------------------------------------
def _won(T):
    """The set of TERMS that took the minimum somewhere."""
    return {TERMS[i] for i in np.unique(T["which"]) if i >= 0}


def _paths_sum(T, sg, combine):
    """True iff S equals combine(C, L list) on every admissible entry."""
    a = T["adm"]
    return np.array_equal(sum(np.where(a, Lr, 0) for Lr in T["L"])[a], combine(T["C"], T["L"])[a])


@functools.lru_cache(maxsize=None)
def rows():
    kc = constants()
    TW, TH, LPB, CH = kc["kSdTileW"], kc["kSdTileH"], kc["kSgmLinesPerBlock"], kc["kSgmChunk"]
    assert (TW, TH, LPB, CH, kc["kSgmSlots"]) == (64, 4, 4, 64, 4)
    out = []
    P = sdc.params

    def add(name, pair, p, sg, pred):
        L, R = (np.ascontiguousarray(a, np.float32) for a in pair[:2])
        for a in (L, R):
            a.setflags(write=False)
        assert check_params(L.shape[0], L.shape[1], p, sg) == 0, name
        out.append((name, L, R, p, sg, pred))

    active = lambda T: int(T["adm"].any(axis=2).sum())
    # degenerate frames
    add("no census window: 6 x 8", sdc.shifted_pair(1, (6, 8), 2), P(A=0), sgm(A=0), lambda s, T, sg: active(T) == 0)
    add("census words but no active pixel: 9 x 11, dmin 3", sdc.shifted_pair(1, (9, 11), 2), P(A=0, dmin=3, dmax=6), sgm(A=0),
        lambda s, T, sg: active(T) == 0 and s["interior"] == 0)
    for paths in (4, 8):
        add(f"one active pixel, {paths} paths", sdc.shifted_pair(2, (7, 10), 1), P(A=0, dmin=1, dmax=3), sgm(A=0, paths=paths),
            lambda s, T, sg: active(T) == 1 and _paths_sum(T, sg, lambda C, L: sg["paths"] * C))
        add(f"one active row, {paths} paths", sdc.shifted_pair(2, (7, 40), 3), P(A=0, dmin=1, dmax=20), sgm(A=0, paths=paths),
            lambda s, T, sg: T["rect"][3] - T["rect"][2] == 1 and active(T) > 20
            and _paths_sum(T, sg, lambda C, L: L[0] + L[1] + (sg["paths"] - 2) * C) and not np.array_equal(T["L"][0], T["C"]))
        add(f"one active column, {paths} paths", sdc.shifted_pair(2, (30, 10), 1), P(A=0, dmin=1, dmax=3), sgm(A=0, paths=paths),
            lambda s, T, sg: T["rect"][1] - T["rect"][0] == 1 and active(T) == 24 and _paths_sum(T, sg, lambda C, L: sg["paths"] * C))

    def newest(s, T, sg):
        """In the left strip the candidate count grows with x: along (1, 0) the newest candidate has neither itself nor d + 1 at q."""
        n = T["n_cand"]
        grow = np.zeros(n.shape, bool)
        grow[:, 1:] = (n[:, 1:] > n[:, :-1]) & (n[:, :-1] > 0)
        ys, xs = np.nonzero(grow)
        w = T["which"][0][ys, xs, n[ys, xs] - 1]
        return len(w) > 20 and set(np.unique(w)) <= {1, 3} and 1 in w
    add("left strip, cols 50 below dmax 60", sdc.shifted_pair(3, (40, 50), 7), P(dmax=60), sgm(), lambda s, T, sg: newest(s, T, sg)
        and T["n_cand"].max() < 60)
    add("left strip, 4 paths, A = 0", sdc.shifted_pair(3, (20, 60), 5), P(A=0, dmax=30), sgm(A=0, paths=4), newest)
    # the lane and slot seams
    for D, size in ((3, (9, 20)), (64, (12, 90)), (65, (12, 90)), (128, (10, 150)), (129, (10, 150)), (192, (10, 220)), (193, (10, 220)),
                    (255, (10, 280))):
        add(f"D = {D}", sdc.shifted_pair(4, size, min(D - 1, 70)), P(A=0, dmin=1, dmax=D), sgm(A=0),
            lambda s, T, sg, D=D, size=size: T["n_cand"].max() == min(D, size[1] - 9) and s["interior"] > 0)
    # diagonal lines enter through both sides
    for size in ((40, 24), (24, 40)):
        add(f"frame {size[0]} x {size[1]}", sdc.shifted_pair(5, size, 3), P(A=1, dmax=10), sgm(A=1),
            lambda s, T, sg, size=size: (T["rect"][3] - T["rect"][2] > T["rect"][1] - T["rect"][0]) == (size[0] > size[1])
            and not np.array_equal(T["L"][4], T["L"][6]))
    # line lengths round the path kernel's load-ahead ring (kSgmAhead steps; a line's loop runs in rounds of that many): one short of
    # it, the ring itself, one more, and two rounds and one. The vertical and diagonal launches meet them as the active rectangle's
    # height, the horizontal ones (instantiations of their own) as its width. At A = 1 the rectangle is rows - 8 high and, with
    # dmin = 1, cols - 11 wide.
    AH = kc["kSgmAhead"]
    for n in (AH - 1, AH, AH + 1, 2 * AH + 1):
        add(f"active rectangle {n} high", sdc.shifted_pair(12, (8 + n, 60), 3), P(A=1, dmax=10), sgm(A=1),
            lambda s, T, sg, n=n: T["rect"][3] - T["rect"][2] == n and T["rect"][1] - T["rect"][0] >= 40 and s["matched"] > 0)
        add(f"active rectangle {n} wide", sdc.shifted_pair(13, (22, 11 + n), 1), P(A=1, dmax=10), sgm(A=1),
            lambda s, T, sg, n=n: T["rect"][1] - T["rect"][0] == n and T["rect"][3] - T["rect"][2] >= 12 and s["matched"] > 0)
    # either side of the tile (64 x 4), of the lines per workgroup (4) and every cols % 4
    for r_, c_ in ((3 * TH, TW - 1), (3 * TH, TW), (3 * TH, TW + 1), (3 * TH - 1, TW), (3 * TH + 1, TW), (3 * TH + 1, 2 * TW + 1),
                   (3 * TH + 1, TW + 2), (3 * TH + 2, TW + 3)):
        add(f"tile geometry {r_} x {c_}", sdc.shifted_pair(6, (r_, c_), 5), P(A=1, dmax=12), sgm(A=1),
            lambda s, T, sg: s["matched"] > 0)
    # ties. Constant images have C = 0 everywhere, and every path that starts with its pixel's full candidate set ties at 0. But along
    # a direction with dx > 0 the admissible set GROWS: a candidate that appears has neither itself nor d + 1 at q, so it enters P1
    # above its lower neighbour (P2 at the most) and keeps that. Every candidate but dmin therefore costs more than 0 in S, and dmin wins uniquely: a flat frame is matched at dmin,
    # not rejected as by the box matcher.
    def flat(s, T, sg):
        a, m = T["adm"], T["outcome"] == 1
        above = a & (np.arange(a.shape[2]) > 0)[None, None]
        return ((T["C"][a] == 0).all() and all((T["L"][k][a] == 0).all() for k, r in enumerate(DIRS[:sg["paths"]]) if r[0] <= 0)
                and (T["L"][0][above] > 0).all() and (T["c0"][T["outcome"] > 0] == 0).all() and s["matched"] > 0
                and (T["dl"][m] == 1).all() and s["interior"] == s["matched"] + s["rej_unique"])
    add("constant images, L == R", (np.full((20, 40), 7.0), np.full((20, 40), 7.0)), P(), sgm(), flat)
    add("constant images, L != R", (np.full((20, 40), 3.0), np.full((20, 40), 200.0)), P(uniq=0), sgm(paths=4), flat)
    for period in (5, 17):
        add(f"right image of period {period}", sdc.periodic_pair(5, (24, 90), period, 3), P(dmin=1, dmax=40), sgm(),
            lambda s, T, sg: (T["outcome"] == 2).any())
    add("occluding step", sdc.occluding_step(9, (40, 120)), P(dmin=1, dmax=24), sgm(), lambda s, T, sg: _won(T) == set(TERMS))
    add("occluding step, 4 paths, no left-right check", sdc.occluding_step(9, (40, 120)), P(dmin=1, dmax=24, lr_max=-1), sgm(paths=4),
        lambda s, T, sg: _won(T) == set(TERMS) and s["rej_lr"] == 0)
    # the penalties' edges
    add("P1 = P2", sdc.shifted_pair(7, (24, 70), 6), P(A=1), sgm(p1=40, p2=40), lambda s, T, sg: "a0" in _won(T) and "a1" in _won(T))
    add("P1 = 1", sdc.half_pixel_pair(7, (24, 70), 6), P(A=1), sgm(p1=1, p2=300), lambda s, T, sg: {"a1", "a2"} <= _won(T))
    for A, size in ((0, (20, 60)), (3, (24, 70))):
        p2 = 65534 // 8 - 62 * (2 * A + 1) ** 2
        add(f"P2 {p2} at the bound, 8 paths, A = {A}", sdc.occluding_step(8, size, 3, 9), P(A=A, dmax=16), sgm(p1=10, p2=p2),
            lambda s, T, sg, A=A: check_params(1, 1, P(A=A), dict(sg, p2=sg["p2"] + 1)) == 3 and s["interior"] > 0)
    add("NaN, +inf and -inf pixels", sdc.non_finite_pair(11, (36, 80), 5), P(dmin=1, dmax=20), sgm(), lambda s, T, sg: s["matched"] > 0)
    for A in (0, 1, 2, 3):
        for paths in (4, 8):
            add(f"integer disparity pair 96 x 320, A = {A}, {paths} paths", sdc.integer_pair(), P(dmin=1, dmax=63, A=A), sgm(A=A, paths=paths),
                lambda s, T, sg: s["matched"] > s["interior"] // 2)
    return out


def row_ids():
    return [r[0] for r in rows()]


@functools.lru_cache(maxsize=None)
def model_of(index, switch=None):
    """(depth, q, stats, S, details) of row `index` from the vectorised model (details only without a switch); read-only."""
    _, L, R, p, sg, _ = rows()[index]
    res = sgm_model(L, R, p, sg, switch=switch, details=switch is None)
    for a in (res[0], res[1], res[3]):
        a.setflags(write=False)
    return res


def loop_work(index):
    _, L, _, p, sg, _ = rows()[index]
    x0, x1, y0, y1 = rect(L.shape[0], L.shape[1], p)
    return max(x1 - x0, 0) * max(y1 - y0, 0) * (p["dmax"] - p["dmin"] + 1) * sg["paths"]


def caught_by(index, switch):
    """True iff row `index` must notice the switch, worked out of the UNSWITCHED model's path costs: a switch of the step changes a
    direction's costs iff it changes some single step taken from the unswitched predecessors (the first step at which a switched walk
    leaves the model is such a step); the swapped diagonal is noticed iff the two diagonals' costs differ."""
    _, L, _, p, sg, _ = rows()[index]
    T = model_of(index)[4]
    if switch == "diagonal_twice":
        if sg["paths"] != 8:
            return False
        a, b = (T["L"][DIRS.index(r)] if T["L"] is not None else path_costs(T["C"], p, sg, *r)[0] for r in ((1, 1), (1, -1)))
        return not np.array_equal(a, b)
    rows_, cols, D = T["C"].shape
    for k, (dx, dy) in enumerate(DIRS[:sg["paths"]]):
        Lr = T["L"][k] if T["L"] is not None else path_costs(T["C"], p, sg, dx, dy)[0]
        Lq, q_active = predecessors(Lr, dx, dy, T["rect"])
        got, _ = step(T["C"].reshape(-1, D), Lq.reshape(-1, D), q_active.reshape(-1), sg, switch)
        if not np.array_equal(got.reshape(Lr.shape), Lr):
            return True
    return False


# Rows that are in the table for a switch by name: caught_by() must hold for each of them (test_stereo_sgm_cpu.py).
PLACED = {
    "no_d_plus_1": ["occluding step", "P1 = 1", "integer disparity pair 96 x 320, A = 2, 8 paths"],
    "inadmissible_is_zero": ["left strip, cols 50 below dmax 60", "left strip, 4 paths, A = 0", "D = 255"],
    "m_not_subtracted": ["one active row, 4 paths", "occluding step", "P2 5153 at the bound, 8 paths, A = 3"],
    "diagonal_twice": ["frame 40 x 24", "frame 24 x 40", "occluding step"],
}
