"""Designed inputs that drive the map's voxel hash (map_kernels.hip: map_key, map_hash, map_claim_kernel's linear probe and payload
fold; map_api.hip.h: the slot rule) where natural frames never take it: long chains, the wrap at the table's end, the edges of the
key's 21-bit fields, the fullest table the sizing rule allows. Held by tests/test_map_hash_cases_cpu.py (the models against each other
and against RefMap) and tests/test_gpu_map_hash_cases.py (the device's table, read out slot by slot, against them).

  mirror     pack / mix / n_slots / home: the key packing, the splitmix64 finaliser, the slot rule and the home slot, with kMapBlock and
             kMapEmpty read out of map.hip.h and the slot rule's factor out of odo_map_create
  pipeline   frame_keys: candidates, world points and voxel indices exactly as RefMap (tests/test_gpu_map.py) computes them
  models     table_model: {key: (insertion, pixel)} of the first claimant, by np.unique; simulate: the claim and count kernels one
             pixel after the other on a host table, with the four switches; probe_replay: sequential linear probing of a key list
  design     inverse depths whose keys' homes satisfy a predicate
  rows       case(name) for name in NAMES, each with the switches that must show on it; the rows' predicates, on order-independent
             quantities, are tests/test_map_hash_cases_cpu.py's test_row_*

Linear probing without deletion has the property all of this rests on: the set of occupied slots, and the number of keys carried over
each boundary between two slots (so also over the table's end, from the last slot to slot 0), do not depend on the order of insertion.
Which key sits in which slot of a run does; the checks use only what does not. Nothing here imports the GPU library."""
import os
import re

import numpy as np

from test_gpu_map import RefMap, ref_candidates, ref_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "odometry_amd", "csrc")
f32 = np.float32
u64 = np.uint64
SWITCHES = ("no_wrap", "stop_at_foreign_key", "shift_20", "last_claimant_wins")


# ---- the mirror -------------------------------------------------------------------------------------------------------------------
_constants = {}


def constants():
    """kMapBlock, kMapEmpty (map.hip.h) and the slot rule's factor (odo_map_create: slots = a power of two >= factor * (capacity + n))."""
    if _constants:
        return _constants
    hdr = open(os.path.join(CSRC, "map.hip.h")).read()
    block = re.findall(r"^constexpr\s+int\s+kMapBlock\s*=\s*(\d+)\s*;", hdr, re.M)
    empty = re.findall(r"^constexpr\s+unsigned long long\s+kMapEmpty\s*=\s*~0ull\s*;", hdr, re.M)
    api = open(os.path.join(CSRC, "map_api.hip.h")).read()
    start = api.index('extern "C" int odo_map_create(')
    body = api[start:api.index("\n}\n", start)]
    rule = re.findall(r"while \(m->slots < (\d+)ull \* \(unsigned long long\)\(capacity \+ n\)\) m->slots <<= 1;", body)
    assert len(block) == 1 and len(empty) == 1, (block, empty)
    assert len(rule) == 1, f"the slot rule must be found exactly once in odo_map_create, found {len(rule)} times"
    _constants.update(kMapBlock=int(block[0]), kMapEmpty=(1 << 64) - 1, slot_factor=int(rule[0]))
    return _constants


EMPTY = (1 << 64) - 1
M64 = (1 << 64) - 1


def pack(kx, ky, kz, shift_20=False):
    """map_key: three fields k + 2^20, 21 bits each (shift_20: the second and third field one bit too low)."""
    b = 20 if shift_20 else 21
    f = [(np.asarray(k, np.int64) + (1 << 20)).astype(u64) for k in (kx, ky, kz)]
    return f[0] | (f[1] << u64(b)) | (f[2] << u64(2 * b))


def mix(k):
    """map_hash: the splitmix64 finaliser on uint64 (products modulo 2^64)."""
    k = np.array(k, u64)
    with np.errstate(over="ignore"):
        k ^= k >> u64(30)
        k *= u64(0xbf58476d1ce4e5b9)
        k ^= k >> u64(27)
        k *= u64(0x94d049bb133111eb)
        return k ^ (k >> u64(31))


def mix_int(k):
    """The same with Python integers."""
    k ^= k >> 30
    k = (k * 0xbf58476d1ce4e5b9) & M64
    k ^= k >> 27
    k = (k * 0x94d049bb133111eb) & M64
    return k ^ (k >> 31)


def n_slots(capacity, n):
    """odo_map_create: the smallest power of two >= factor * (capacity + rows * cols)."""
    s = 1
    while s < constants()["slot_factor"] * (capacity + n):
        s <<= 1
    return s


def home(key, slots):
    return mix(key) & u64(slots - 1)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------
def frame_keys(case, val, dep, A, shift_20=False):
    """One insertion's candidates as RefMap sees them: (pixels, in range, keys as uint64 (0 where out of range), voxel indices)."""
    pix = ref_candidates(val, dep)
    with np.errstate(all="ignore"):
        w = ref_world(pix, dep, A, case["size"][1], case["K"])
        q = [np.floor(c / f32(case["voxel"])) for c in w]
        inr = np.all([np.abs(c) < f32(2 ** 20) for c in q], axis=0)
        k = [np.where(inr, c, 0).astype(np.int64) for c in q]
    return pix, inr, np.where(inr, pack(*k, shift_20=shift_20), u64(0)), k, w


def case_slots(case):
    return n_slots(case["capacity"], case["size"][0] * case["size"][1])


# ---- the models -------------------------------------------------------------------------------------------------------------------
def table_model(case, upto=None):
    """{key: (insertion, pixel)} of the first claimant over the insertions made while the map was open (those whose survivors the
    capacity then dropped included), after `upto` insertions (None: all)."""
    tab, size = {}, 0
    for ins, (val, dep, img, A) in enumerate(case["inputs"][:upto]):
        if size >= case["capacity"]:
            continue
        pix, inr, key, _, _ = frame_keys(case, val, dep, A)
        uk, first = np.unique(key[inr], return_index=True)
        new = 0
        for k, p in zip(uk.tolist(), pix[inr][first].tolist()):
            if k not in tab:
                tab[k] = (ins, p)
                new += 1
        size += min(new, case["capacity"] - size)
    return tab


def simulate(case, switch=None):
    """map_claim_kernel and map_count_kernel one pixel after the other on a host table (one of the schedules the device may take; the
    occupied slots, the payloads and the survivors are the same for every schedule). Returns, after each insertion, a snapshot
    dict(keys, payload: uint64 [slots]; survivors: pixels whose slot's payload is their own, before the capacity cut; size; stuck: keys
    a probe without the wrap never placed). Switches: see SWITCHES."""
    assert switch is None or switch in SWITCHES
    slots = case_slots(case)
    mask = slots - 1
    tk, tp = [EMPTY] * slots, [EMPTY] * slots
    size, stuck, out = 0, 0, []
    for ins, (val, dep, img, A) in enumerate(case["inputs"]):
        surv = []
        if size < case["capacity"]:
            pix, inr, key, _, _ = frame_keys(case, val, dep, A, shift_20=switch == "shift_20")
            p, k = pix[inr], key[inr]
            uk, first = np.unique(k, return_index=True)
            _, rlast = np.unique(k[::-1], return_index=True)
            last = len(k) - 1 - rlast
            order = np.argsort(first)
            homes = (mix(uk) & u64(mask)).tolist()
            uk, fp, lp = uk.tolist(), p[first].tolist(), p[last].tolist()
            claims = []
            for j in order.tolist():
                key_j, s = uk[j], homes[j]
                while True:
                    cur = tk[s]
                    if cur == EMPTY:
                        tk[s] = key_j
                        break
                    if cur == key_j or switch == "stop_at_foreign_key":
                        break
                    if switch == "no_wrap" and s == mask:
                        s = None          # the device would stay here for ever
                        stuck += 1
                        break
                    s = (s + 1) & mask
                if s is None:
                    continue
                if switch == "last_claimant_wins":
                    mine = (ins << 32) | lp[j]
                    tp[s] = mine if tp[s] == EMPTY else max(tp[s], mine)      # the last in (insertion, pixel) order
                else:
                    mine = (ins << 32) | fp[j]
                    tp[s] = min(tp[s], mine)
                claims.append((s, mine))
            surv = sorted(m & 0xffffffff for s, m in claims if tp[s] == m)
            size += min(len(surv), case["capacity"] - size)
        out.append(dict(keys=np.array(tk, u64), payload=np.array(tp, u64), survivors=surv, size=size, stuck=stuck))
    return out


def probe_replay(keys, slots, no_wrap=False, stop_at_foreign_key=False):
    """Sequential linear probing of distinct keys in the order given. dict(slot: {key: slot}, occupied: bool [slots], over: int64
    [slots], over[b] = keys carried over the boundary behind slot b (over[slots - 1]: over the table's end), carried = over[-1],
    below_home = keys that sit below their home (each was carried over the end exactly once), stuck, merged)."""
    mask = slots - 1
    tab = [EMPTY] * slots
    homes = (mix(np.array(keys, u64)) & u64(mask)).tolist() if len(keys) else []
    place, diff, carried, stuck, merged = {}, np.zeros(slots + 1, np.int64), 0, 0, 0
    for key, h in zip([int(k) for k in keys], homes):
        s = h
        while tab[s] != EMPTY:
            assert tab[s] != key, "probe_replay takes distinct keys"
            if stop_at_foreign_key or (no_wrap and s == mask):
                break
            s = (s + 1) & mask
        if tab[s] != EMPTY:
            stuck += no_wrap
            merged += stop_at_foreign_key
            continue
        tab[s] = key
        place[key] = s
        if s >= h:
            diff[h] += 1
            diff[s] -= 1
        else:
            diff[h] += 1
            diff[slots] -= 1
            diff[0] += 1
            diff[s] -= 1
            carried += 1
    over = np.cumsum(diff)[:slots]
    assert over[-1] == carried
    return dict(slot=place, occupied=np.array([t != EMPTY for t in tab]), over=over, carried=carried,
                below_home=sum(1 for k, h in zip([int(k) for k in keys], homes) if k in place and place[k] < h), stuck=stuck,
                merged=merged, table=np.array(tab, u64))


def runs(occupied):
    """(load, longest cyclic run of occupied slots)."""
    occ = np.asarray(occupied, bool)
    if occ.all():
        return 1.0, len(occ)
    if not occ.any():
        return 0.0, 0
    z = int(np.nonzero(~occ)[0][0])
    r = np.roll(occ, -z).astype(np.int8)          # starts at an empty slot: no run crosses the array's end
    edges = np.diff(np.concatenate([[0], r, [0]]))
    return float(occ.mean()), int((np.nonzero(edges == -1)[0] - np.nonzero(edges == 1)[0]).max())


def home_stats(keys, slots):
    """(largest number of keys that share a home, keys carried over the table's end) of a set of distinct keys."""
    if len(keys) == 0:
        return 0, 0
    h = home(np.array(sorted(keys), u64), slots)
    return int(np.unique(h, return_counts=True)[1].max()), probe_replay(sorted(keys), slots)["carried"]


def check_table(keys, payload, want, slots):
    """What the device's table (keys, payload: uint64 [slots], from odo_debug_map_table) must satisfy given the model's snapshot `want`
    (simulate's), whatever order the claims took: checks 3 to 7 of tests/test_gpu_map_hash_cases.py."""
    keys, payload = np.asarray(keys, u64), np.asarray(payload, u64)
    assert keys.shape == payload.shape == (slots,) == want["keys"].shape
    occ, wocc = keys != u64(EMPTY), want["keys"] != u64(EMPTY)
    # 3: the set of keys
    o, wo = np.argsort(keys[occ]), np.argsort(want["keys"][wocc])
    assert np.array_equal(keys[occ][o], want["keys"][wocc][wo]), "the table's keys are not the model's"
    assert len(np.unique(keys[occ])) == int(occ.sum()), "a key sits in two slots"
    # 4: every key's payload, and all ones in every empty slot
    assert np.array_equal(payload[occ][o], want["payload"][wocc][wo]), "a key's payload is not the model's first claimant"
    assert np.all(payload[~occ] == u64(EMPTY)), "an empty slot has a payload"
    # 5: every slot from a key's home to its place, cyclically, is occupied
    at = np.nonzero(occ)[0]
    h = home(keys[occ], slots).astype(np.int64)
    dist = (at - h) & (slots - 1)
    c = np.concatenate([[0], np.cumsum(np.concatenate([occ, occ]).astype(np.int64))])
    assert np.array_equal(c[h + dist + 1] - c[h], dist + 1), "an empty slot between a key's home and its place"
    # 6: the occupied slots
    assert np.array_equal(occ, wocc), "the occupied slots are not the replay's"
    # 7: keys below their home = keys carried over the table's end
    wat = np.nonzero(wocc)[0]
    wh = home(want["keys"][wocc], slots).astype(np.int64)
    assert int((at < h).sum()) == int((wat < wh).sum()), "keys carried over the table's end"
    return dict(n_keys=int(occ.sum()), carried=int((at < h).sum()), longest_probe=int(dist.max()) if len(dist) else 0)


# ---- input design -----------------------------------------------------------------------------------------------------------------
def design(size, K, pose, voxel, slots, predicate, pixels=None, avoid=(), kz0=1000, n_cand=16384):
    """An inverse-depth frame: pixel i of `pixels` (None: all) gets d = fl32(1 / ((kz + 0.5) voxel)), kz the first of n_cand candidates
    from kz0 for which the key the pixel really produces (frame_keys' pipeline) is new, not in `avoid`, and has a home satisfying the
    predicate; every other pixel gets 0. Every d lies outside the 0.01 validity band (asserted). Returns (frame, keys in pixel order)."""
    rows, cols = size
    pixels = np.arange(rows * cols) if pixels is None else np.asarray(pixels, np.int64)
    kz = np.arange(kz0, kz0 + n_cand)
    d = (f32(1) / ((kz.astype(np.float64) + 0.5) * voxel).astype(f32)).astype(f32)
    assert np.all(d >= f32(0.0101)), "candidates inside the validity band"
    f0, cx, cy = (f32(v) for v in K)
    a = np.asarray(pose, f32).T.reshape(16)
    x = (pixels % cols).astype(f32)[:, None]
    y = (pixels // cols).astype(f32)[:, None]
    z = (f32(1) / d)[None, :]
    X = (z * (x - cx)) / f0
    Y = (z * (y - cy)) / f0
    q = [np.floor((((a[r] * X + a[4 + r] * Y) + a[8 + r] * z) + a[12 + r]) / f32(voxel)) for r in range(3)]
    assert all(np.all(np.abs(c) < f32(2 ** 20)) for c in q)
    key = pack(*[c.astype(np.int64) for c in q])
    ok = predicate(home(key, slots).astype(np.int64))
    used, dep, keys = set(int(k) for k in avoid), np.zeros(rows * cols, f32), []
    for i, p in enumerate(pixels.tolist()):
        for j in np.nonzero(ok[i])[0].tolist():
            if int(key[i, j]) not in used:
                used.add(int(key[i, j]))
                dep[p] = d[j]
                keys.append(int(key[i, j]))
                break
        else:
            raise AssertionError(f"no candidate for pixel {p}")
    return dep.reshape(rows, cols), keys


def _eye(t=(0, 0, 0)):
    A = np.eye(4, dtype=f32)
    A[:3, 3] = np.asarray(t, f32)
    return A


def _case(name, size, K, capacity, voxel, inputs, classes, why, **extra):
    return dict(name=name, size=size, K=K, capacity=capacity, voxel=voxel, inputs=inputs, classes=frozenset(classes), why=why, **extra)


SMALL, SMALL_K, FINE = (16, 16), (40.0, 7.5, 7.5), 1e-3
COLLIDING = ("no_wrap", "stop_at_foreign_key")


def _wrap():
    slots = n_slots(256, 256)
    dep, keys = design(SMALL, SMALL_K, _eye(), FINE, slots, lambda h: h >= slots - 4)
    return _case("wrap", SMALL, SMALL_K, 256, FINE, [(None, dep, None, _eye())], COLLIDING,
                 "256 distinct keys homed in the last four slots", designed=[keys], homed=lambda h, s: h >= s - 4)


def _one_home():
    slots = n_slots(256, 256)
    dep, keys = design(SMALL, SMALL_K, _eye(), FINE, slots, lambda h: h == slots // 2)
    return _case("one_home", SMALL, SMALL_K, 256, FINE, [(None, dep, None, _eye())], ("stop_at_foreign_key",),
                 "256 distinct keys homed in one slot in mid-table", designed=[keys], homed=lambda h, s: h == s // 2)


def _ends_at_the_end():
    slots = n_slots(256, 256)
    dep0, k0 = design(SMALL, SMALL_K, _eye(), FINE, slots, lambda h: h == slots - 128, pixels=np.arange(0, 256, 2))
    dep1, k1 = design(SMALL, SMALL_K, _eye(), FINE, slots, lambda h: h == slots - 128, pixels=[77], avoid=k0)
    return _case("ends_at_the_end", SMALL, SMALL_K, 256, FINE, [(None, dep0, None, _eye()), (None, dep1, None, _eye())], COLLIDING,
                 "a run of 128 keys that ends in the last slot, then one more key with its home", designed=[k0, k1],
                 homed=lambda h, s: h == s - 128)


def _repeat_and_extend():
    slots = n_slots(512, 256)
    dep0, k0 = design(SMALL, SMALL_K, _eye(), FINE, slots, lambda h: h >= slots - 4)
    odd = np.arange(1, 256, 2)
    new, k1 = design(SMALL, SMALL_K, _eye(), FINE, slots, lambda h: h >= slots - 4, pixels=odd, avoid=k0)
    dep1 = dep0.copy()
    dep1.reshape(-1)[odd] = new.reshape(-1)[odd]
    return _case("repeat_and_extend", SMALL, SMALL_K, 512, FINE, [(None, dep0, None, _eye()), (None, dep1, None, _eye())],
                 COLLIDING + ("last_claimant_wins",),
                 "the wrap's insertion again: the even pixels repeat their keys, the odd ones bring new keys with the same homes",
                 designed=[k0, k1], homed=lambda h, s: h >= s - 4)


ONE_VOXEL_FIRST = 310


def _one_voxel():
    size, K = (24, 32), (40.0, 15.5, 11.5)
    rng = np.random.default_rng(11)
    dep = rng.uniform(0.05, 1.0, size).astype(f32)
    flat = dep.reshape(-1)
    flat[300:ONE_VOXEL_FIRST:2] = rng.uniform(-0.5, 0.0, 5).astype(f32)          # d <= 0
    flat[301:ONE_VOXEL_FIRST:2] = f32([0.0099, -0.0099, 0.005, 0.0, 0.001])       # inside the validity band
    flat[600:640] = rng.uniform(-0.0099, 0.0099, 40).astype(f32)
    flat[700:720] = -flat[700:720]
    val = np.ones(size, np.uint8)
    val.reshape(-1)[:300] = 0
    A = _eye((500, 500, 500))
    return _case("one_voxel", size, K, 16, 1000.0, [(val, dep, None, A), (val, dep, None, A)], ("last_claimant_wins",),
                 "three blocks of candidates of one voxel")


EDGE_K = (1.0, 1.0, 0.0)        # 1 x 3 frames, d = 1: the camera points are (-1, 0, 1), (0, 0, 1), (1, 0, 1), exact
AXIS_ROT = [np.array(r, f32) for r in ([[1, 0, 0], [0, 1, 0], [0, 0, 1]],      # camera X on world x
                                       [[0, 0, 1], [1, 0, 0], [0, 1, 0]],      # ... on world y
                                       [[0, 1, 0], [0, 0, 1], [1, 0, 0]])]     # ... on world z
EDGE_T = [2.0 ** 20 - 0.5, 2.0 ** 20 - 1.5, -(2.0 ** 20 - 0.5), -(2.0 ** 20 - 1.5)]


def _field_edges():
    dep = np.ones((1, 3), f32)
    inputs = []
    for axis in range(3):
        for t in EDGE_T:
            A = np.eye(4, dtype=f32)
            A[:3, :3] = AXIS_ROT[axis]
            A[axis, 3] = f32(t)
            inputs.append((None, dep, None, A))
    return _case("field_edges", (1, 3), EDGE_K, 64, 1.0, inputs, ("shift_20", "last_claimant_wins"),
                 "per axis and sign, exact world coordinates one voxel inside and one outside the 21-bit field", axes=True)


NEIGHBOURS = [(0, 0, 0), (-1, 0, 0), (2 ** 20 - 1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (-2 ** 20 + 1, 2 ** 20 - 1, 0),
              (0, -2 ** 20 + 1, 2 ** 20 - 1), (2 ** 20 - 1, 2 ** 20 - 1, 2 ** 20 - 1), (-2 ** 20 + 1, -2 ** 20 + 1, -2 ** 20 + 1),
              (-2 ** 20 + 1, 0, 0), (0, 2 ** 20 - 1, 0), (0, 0, -2 ** 20 + 1), (1, 0, 0), (-1, -1, -1)]


def _field_neighbours():
    dep = np.array([[0.0, 1.0, 0.0]], f32)      # the middle pixel alone: camera point (0, 0, 1)
    inputs = [(None, dep, None, _eye((a + 0.5, b + 0.5, c - 0.5))) for a, b, c in NEIGHBOURS]
    return _case("field_neighbours", (1, 3), EDGE_K, 1024, 1.0, inputs, ("shift_20",),
                 "voxels that differ only across a field boundary, one insertion each", voxels=NEIGHBOURS)


def _fullest_table():
    slots = n_slots(256, 256)
    dep0, k0 = design(SMALL, SMALL_K, _eye(), FINE, slots, lambda h: h >= 0, pixels=np.arange(1, 256))
    dep1, k1 = design(SMALL, SMALL_K, _eye(), FINE, slots, lambda h: h >= 0, avoid=k0, kz0=3000)
    dep2, _ = design(SMALL, SMALL_K, _eye(), FINE, slots, lambda h: h >= 0, kz0=6000)
    ins = [(None, d, None, _eye()) for d in (dep0, dep1, dep2)]
    return _case("fullest_table", SMALL, SMALL_K, 256, FINE, ins, FULLEST_CLASSES, "255 + 256 keys in 1 024 slots, the most the sizing rule allows",
                 designed=[k0, k1])


def _not_a_number():
    rng = np.random.default_rng(13)
    dep = rng.uniform(-0.1, 0.6, SMALL).astype(f32)
    val = (rng.uniform(size=SMALL) < 0.8).astype(np.uint8)
    poses = []
    for r, c, v in ((0, 3, np.inf), (1, 3, -np.inf), (2, 3, np.nan), (0, 0, np.inf)):      # the last: inf * X, and inf * 0 = NaN
        A = _eye((0.1, 0.2, 0.3))
        A[r, c] = f32(v)
        poses.append(A)
    return _case("not_a_number", SMALL, SMALL_K, 256, 0.05, [(val, dep, None, A) for A in poses], (),
                 "world coordinates that are +-inf or NaN")


NATURAL_SIZE = (240, 424)


def _natural():
    import geometry_cases as G
    return _case("natural", NATURAL_SIZE, G.map_K(NATURAL_SIZE), 1 << 17, G.MAP_VOXEL, G.map_inputs(NATURAL_SIZE), NATURAL_CLASSES,
                 "the natural scene: the load and the runs real frames give")


# The switches that show on the two rows that were not designed for one: computed by tests/test_map_hash_cases_cpu.py and stated here.
FULLEST_CLASSES = ("stop_at_foreign_key",)
NATURAL_CLASSES = ("stop_at_foreign_key", "shift_20", "last_claimant_wins")

BUILDERS = dict(wrap=_wrap, one_home=_one_home, ends_at_the_end=_ends_at_the_end, repeat_and_extend=_repeat_and_extend,
                one_voxel=_one_voxel, field_edges=_field_edges, field_neighbours=_field_neighbours, fullest_table=_fullest_table,
                not_a_number=_not_a_number, natural=_natural)
NAMES = list(BUILDERS)
_cases, _sims, _refs = {}, {}, {}


def case(name):
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]


def sim(name, switch=None):
    """simulate(case(name), switch), once per process."""
    if (name, switch) not in _sims:
        _sims[(name, switch)] = simulate(case(name), switch)
    return _sims[(name, switch)]


def ref_trail(name):
    """RefMap (imported unchanged) after each insertion of a row: [(statistics, points, keyframe / pixel records)]."""
    if name not in _refs:
        c = case(name)
        ref, trail = RefMap(c["capacity"], c["voxel"], cols=c["size"][1], k=c["K"]), []
        with np.errstate(all="ignore"):
            for val, dep, img, A in c["inputs"]:
                ref.insert(val, dep, img, A)
                trail.append((dict(ref.st), ref.xyzi.copy(), ref.kp.copy()))
        _refs[name] = trail
    return _refs[name]


class Snapshot:
    """What assert_same (tests/test_gpu_map.py) reads of a RefMap, at one point of a row's trail."""
    def __init__(self, st, xyzi, kp):
        self.st, self.xyzi, self.kp = st, xyzi, kp


def table_keys(snap):
    k = snap["keys"]
    return k[k != u64(EMPTY)]


def geometry_case(size):
    """A small MAP row of tests/geometry_cases.py as a case: its existing inputs, capacity and voxel."""
    import geometry_cases as G
    return _case(f"{size[0]}x{size[1]}", tuple(size), G.map_K(size), G.map_capacity(size), G.MAP_VOXEL, G.map_inputs(size), (), "geometry row")
