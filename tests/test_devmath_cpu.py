"""The reference side of the device-math tests, without a GPU: every input class of tests/devmath_cases.py reaches the branch it is
there for (counted), the host build of odo_math.h equals the oracle bit for bit on every class the oracle exports, the LM scripts'
host replay (emu_lm_script) equals a Python restatement composed from the oracle's own solve and exponential, both builds of the
device harness cross-compile and export every entry, the ctypes mirrors match the C++ structures, and the oracle's sine / cosine /
exponential are anchored to mpmath. tests/test_gpu_devmath.py then holds the device to this host build by bit pattern."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
import devmath as D
import devmath_cases as Cs

f32 = np.float32


@pytest.fixture(scope="module")
def host():
    return D.load_host()


def rowmajor(M16):
    return np.asarray(M16, f32).reshape(4, 4).T


# ---- the harness itself -----------------------------------------------------------------------------------------------------------
def test_harness_cross_compiles_and_exports_every_entry():
    """Both builds (the main unit's scheduler, the chain unit's) compile for gfx950 with the product's flags and export every entry."""
    assert D.flags("main") == D.B._flags_for(D.B.SRC, D.B.FLAGS) and D.flags("chain") == D.B._flags_for(D.B.SRC_CHAIN, D.B.FLAGS)
    assert "--offload-arch=gfx950" in D.flags("main") and "-ffp-contract=off" in D.flags("main")
    paths = D.build_all()
    assert len(set(paths)) == (2 if D.scheduler("main") != D.scheduler("chain") else 1)
    for so in paths:
        lib = C.CDLL(so)
        for name in D.ENTRIES:
            assert hasattr(lib, name), "%s does not export %s" % (so, name)


def test_struct_mirrors_match_the_device_structures(host):
    for unit in D.UNITS:
        lib = C.CDLL(D.build(unit))
        lay = np.zeros(lib.dm_layout_count(), np.int32)
        lib.dm_layout(lay.ctypes.data_as(C.c_void_p))
        assert [int(v) for v in lay[:-2]] == D.mirror_layout()
        assert lay[0] == 256 and D.LM_STATE.itemsize == 256 and lay[-2] in (256, 512, 1024)
    assert host.lib.emu_sizeof_lm_state() == C.sizeof(D.LmState)
    assert host.lib.emu_sizeof_lm_script() == C.sizeof(D.LmScript) == D.LM_SCRIPT.itemsize
    assert host.lib.emu_sizeof_pix_level() == C.sizeof(D.PixLevel)


# ---- sincos -----------------------------------------------------------------------------------------------------------------------
def test_sincos_classes_reach_their_quadrants():
    cl = Cs.sincos_classes()
    x = cl["quadrants"]
    q = Cs.sincos_quadrant(x)
    for sign in (1, -1):
        for qq in range(4):
            assert int(((np.sign(x) == sign) & (q == qq)).sum()) == 500
    # 'straddle': both sides of every multiple of pi / 4 — at the odd multiples the quadrant changes inside the seven values
    st = cl["straddle"].reshape(7, -1)
    changes = (Cs.sincos_quadrant(st[0]) != Cs.sincos_quadrant(st[6])).sum()
    assert changes == 64                                   # the 64 odd multiples among -64 .. 64
    assert len(np.unique(Cs.sincos_quadrant(cl["grid"]))) == 4 and (cl["grid"] < 0).sum() == 32768
    la, lp = np.abs(cl["large_accurate"]), np.abs(cl["large_parity"])
    assert la.max() < 2.0 ** Cs.SINCOS_ACCURATE_LOG2 and la.min() >= 8 and len(la) > 19990
    assert lp.min() >= 2.0 ** Cs.SINCOS_ACCURATE_LOG2 and lp.max() <= 2.0 ** Cs.SINCOS_PARITY_LOG2 < 1.45e19   # below the (long long)kf limit
    assert (np.bincount(np.log2(lp).astype(int), minlength=63)[23:62] > 300).all()                # every binade of it
    sp = cl["special"]
    assert np.isnan(sp).sum() == 1 and np.isinf(sp).sum() == 2 and (sp == 0).sum() == 2
    assert ((np.abs(sp) > 0) & (np.abs(sp) < np.finfo(f32).tiny)).sum() == 8


def test_sincos_host_equals_oracle(host):
    lib = O.lib()
    for name, x in Cs.sincos_classes().items():
        s, c = host.sincos(x)
        so = np.array([lib.orc_sinf(float(v)) for v in x], f32)
        co = np.array([lib.orc_cosf(float(v)) for v in x], f32)
        assert D.same_bits(s, so).all() and D.same_bits(c, co).all(), name


def _ulp_error(got, true_mp, mp):
    """|got - true| in units of the float32 spacing at the true value."""
    if true_mp == 0:
        return 0.0 if got == 0 else np.inf
    e = int(mp.floor(mp.log(abs(true_mp), 2)))
    ulp = mp.mpf(2) ** max(e - 23, -149)
    return float(abs(mp.mpf(float(got)) - true_mp) / ulp)


def test_oracle_sincos_within_one_ulp_of_the_true_value():
    """orc_sinf / orc_cosf evaluate in fp64 (error far below half an fp32 ulp) and round once, so they are faithful: within 1 ulp of
    the true sine / cosine, on every class inside the domain |x| < 2^SINCOS_ACCURATE_LOG2. Measured: max 0.5000 ulp, no result that
    is not correctly rounded. And the bound is the largest power of two for which this holds: the sampled binade above it breaks it
    (the two-constant reduction loses k * pio2_1's exactness once k needs more than 20 bits; measured 32 ulp in [2^23, 2^24))."""
    import mpmath as mp
    mp.mp.prec = 200
    lib = O.lib()
    cl = Cs.sincos_classes()
    rng = np.random.default_rng(5)
    inside = np.concatenate([cl["quadrants"], cl["straddle"], rng.choice(cl["grid"], 3000, replace=False),
                             rng.choice(cl["large_accurate"], 6000, replace=False)])
    worst, not_cr, n = 0.0, 0, 0
    for x in inside:
        xm = mp.mpf(float(x))
        for got, true in ((lib.orc_sinf(float(x)), mp.sin(xm)), (lib.orc_cosf(float(x)), mp.cos(xm))):
            e = _ulp_error(got, true, mp)
            worst = max(worst, e)
            not_cr += e > 0.5
            n += 1
    print("sincos inside the domain: max %.4f ulp, %d of %d not correctly rounded" % (worst, not_cr, n))
    assert worst < 1.0
    above = cl["large_parity"]
    above = above[np.abs(above) < 2.0 ** (Cs.SINCOS_ACCURATE_LOG2 + 1)]
    assert len(above) > 300
    worst_above = 0.0
    for x in above:
        xm = mp.mpf(float(x))
        worst_above = max(worst_above, _ulp_error(lib.orc_sinf(float(x)), mp.sin(xm), mp), _ulp_error(lib.orc_cosf(float(x)), mp.cos(xm), mp))
    print("sincos in the binade above the domain: max %.4g ulp" % worst_above)
    assert worst_above > 1.0


# ---- SE(3) ------------------------------------------------------------------------------------------------------------------------
def test_se3_classes_reach_their_branches(host):
    ex = Cs.se3_exp_classes()
    small = {k: int(Cs.se3_is_small(v).sum()) for k, v in ex.items()}
    assert small["omega_1e-07"] == small["omega_1e-06"] == Cs.SE3_PER_SCALE
    assert all(small["omega_%g" % s] == 0 for s in Cs.OMEGA_SCALES[2:])
    th = Cs.se3_theta(ex["threshold"])
    assert small["threshold"] == 42 and len(th) == 90 and (th == f32(1e-5)).sum() >= 3       # both sides of the test and the value itself
    # every sincos quadrant behind the exponential: theta / 2 and theta of the large-angle classes
    big = np.concatenate([ex["omega_%g" % s] for s in Cs.OMEGA_SCALES[3:]])
    for arg in (Cs.se3_theta(big), f32(0.5) * Cs.se3_theta(big)):
        assert (np.bincount(Cs.sincos_quadrant(arg), minlength=4) >= 100).all()
    assert (np.abs(np.concatenate(list(ex.values()))[:, :3]).max(axis=1) > 1e3).sum() > 300          # translations up to 1e4
    mats = Cs.pose_matrices()
    br = {k: np.bincount(Cs.quat_branch(v), minlength=4).tolist() for k, v in mats.items()}
    n = Cs.MATS_PER_BRANCH
    assert br == {"trace_pos": [n, 0, 0, 0], "diag_x": [0, n, 0, 0], "diag_y": [0, 0, n, 0], "diag_z": [0, 0, 0, n], "ties": [0, 6, 2, 1]}
    # compositions: the branch of the PRODUCT, from the host build's own result (its quaternion's largest component names the branch)
    d6, cur = Cs.compose_cases()
    tr = Cs.compose_trace(d6, cur)
    assert (tr < -0.05).sum() == 395 and (tr > 0.05).sum() == 197
    q, M = host.se3_left_update(d6, cur)
    taken = Cs.quat_branch(_product_matrix(host, d6, cur))
    assert (taken[tr < -0.05] != 0).all() and (taken[tr > 0.05] == 0).all()
    assert (np.bincount(taken, minlength=4) >= 80).all()


def _product_matrix(host, d6, cur):
    """exp(d6).matrix() * cur.matrix() in float32 in se3_left_update_mat's order: the matrix rot_to_quat is then given."""
    _, Dm = host.se3_exp(d6)
    _, Cm = host.se3_roundtrip(cur)
    out = np.zeros_like(Cm)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                out[:, j * 4 + i] = ((Dm[:, 0 + i] * Cm[:, j * 4 + 0] + Dm[:, 4 + i] * Cm[:, j * 4 + 1]) + Dm[:, 8 + i] * Cm[:, j * 4 + 2]) + \
                    Dm[:, 12 + i] * Cm[:, j * 4 + 3]
    return out


def test_se3_host_equals_oracle(host):
    for name, a in Cs.se3_exp_classes().items():
        _, M = host.se3_exp(a)
        ref = np.array([O.se3_exp(v).T.reshape(16) for v in a])
        assert D.same_bits(M, ref).all(), name
    for name, Min in Cs.pose_matrices().items():
        _, M = host.se3_roundtrip(Min)
        ref = np.array([O.se3_roundtrip(rowmajor(v)).T.reshape(16) for v in Min])
        assert D.same_bits(M, ref).all(), name
    d6, cur = Cs.compose_cases()
    ref = np.array([O.se3_left_update(d, rowmajor(c)).T.reshape(16) for d, c in zip(d6, cur)])
    for variant in (0, 1):
        _, M = host.se3_left_update(d6, cur, variant)
        assert D.same_bits(M, ref).all(), variant


def test_oracle_se3_exp_against_the_matrix_exponential():
    """No derived bound here: the oracle's exponential against mpmath's expm of the 4x4 twist matrix over theta <= pi, error measured as
    max |M - expm| / max(1, |upsilon|_inf). Measured maximum 5.01e-6 (the fp32 (1 - cos theta) / theta^2 of the translation's V matrix cancels at small angles); twice that is asserted, which only guards the oracle
    against regressions — the device is held to the oracle bit for bit."""
    import mpmath as mp
    mp.mp.prec = 120
    worst, n_cases = 0.0, 0
    ex = Cs.se3_exp_classes()
    for name in ["omega_%g" % s for s in Cs.OMEGA_SCALES[:6]] + ["threshold"]:
        for a in ex[name][::2]:
            if not Cs.se3_theta(a)[0] <= np.pi:
                continue
            n_cases += 1
            v = [mp.mpf(float(t)) for t in a]
            X = mp.matrix([[0, -v[5], v[4], v[0]], [v[5], 0, -v[3], v[1]], [-v[4], v[3], 0, v[2]], [0, 0, 0, 0]])
            E = mp.expm(X)
            M = O.se3_exp(a)
            err = max(abs(mp.mpf(float(M[i, j])) - E[i, j]) for i in range(3) for j in range(4))
            worst = max(worst, float(err) / max(1.0, float(np.abs(a[:3]).max())))
    print("se3_exp against expm: max error %.3g over %d cases" % (worst, n_cases))
    assert n_cases >= 600
    assert worst <= 2 * SE3_EXP_MEASURED


SE3_EXP_MEASURED = 5.01e-6


# ---- solver, weights, intrinsics, the depth LM's driver ---------------------------------------------------------------------------
def test_solver_classes_and_host_equals_oracle(host):
    acc, lam, kind = Cs.solver_cases()
    assert len(acc) == 5 * 5 * 40 and sorted(set(lam.tolist())) == sorted(f32(v) for v in Cs.LAMBDAS)
    diag = acc[:, [0, 6, 11, 15, 18, 20]]
    assert ((diag == 0).sum(axis=1) == 1)[kind == 1].all() and not (diag == 0)[kind != 1].any()      # the zero pivot is in the input
    A = np.zeros((len(acc), 6, 6))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            A[:, a, b] = A[:, b, a] = acc[:, k]
            k += 1
    assert (np.linalg.matrix_rank(A[kind == 2]) == 5).all() and (np.linalg.matrix_rank(A[kind == 0]) == 6).all()
    assert np.isnan(acc[kind == 3]).any(axis=1).all() and np.isinf(acc[kind == 4]).any(axis=1).all()
    d = host.solve_damped(acc, lam)
    ref = np.array([O.solve_damped(a, float(l)) for a, l in zip(acc, lam)])
    assert D.same_bits(d, ref).all()
    zero_col = np.argmax(diag[kind == 1] == 0, axis=1)
    assert (d[kind == 1][np.arange(len(zero_col)), zero_col] == 0).all()             # "a zero pivot leaves that component at zero"
    assert np.isfinite(d[kind == 0]).all() and np.isnan(d[kind == 3]).any(axis=1).sum() >= 100 and \
        (~np.isfinite(d[kind == 4])).any(axis=1).sum() >= 100


def test_robust_weight_class(host):
    r, robust, huber, scale = Cs.robust_cases()
    w = host.robust_weight(r, robust, huber, scale)
    assert (w[:300] == 1).all()                                      # |r| == delta takes the `<=`
    inside = np.abs(r[300:900]) <= huber[300:900]                   # one float32 step either side of it
    assert np.array_equal(w[300:900] == 1, inside) and np.array_equal(w[300:900] < 1, ~inside) and inside.sum() >= 250 and (~inside).sum() >= 250
    assert sorted(np.bincount(robust)[:3] > 1500) == [True, True, True] and np.isnan(w[900:910]).sum() == 1
    with np.errstate(all="ignore"):
        ar = np.abs(r)
        ref = np.where(robust == 1, np.where(ar <= huber, f32(1), huber / ar),
                       np.where(robust == 2, f32(201.0) / (f32(200.0) + r * r / scale), f32(1))).astype(f32)
    assert D.same_bits(w, ref).all()


def test_level_intrinsics_host_equal_oracle(host):
    f0, cx, cy, lv = Cs.level_cases()
    fl, cxy = host.level_k(f0, cx, cy, lv)
    lib = O.lib()
    for i in range(len(f0)):
        assert fl[i] == float(f0[i]) / 2.0 ** int(lv[i])
        assert cxy[i, 0] == cxy[i, 2] == lib.orc_cx_level(float(cx[i]), int(lv[i])) and cxy[i, 1] == lib.orc_cx_level(float(cy[i]), int(lv[i]))


def test_depth_schedule_class_equals_the_pinned_replay(host):
    """The batched replay (devmath_ops.h, what the device runs) against emu_depth_lm_schedule, the replay tests/test_ref_pin.py pins to
    the reference's own lines; and every outcome is reached."""
    errs, n_errs, lam, prec, mi = Cs.depth_schedule_cases()
    rec, fin = host.depth_schedule(errs, n_errs, lam, prec, mi)
    emu = host.lib
    broke = 0
    for i in range(len(errs)):
        r1 = np.zeros(5 * errs.shape[1], np.int32)
        fc, it = C.c_int(0), C.c_int(0)
        e = np.ascontiguousarray(errs[i])
        k = emu.emu_depth_lm_schedule(e.ctypes.data_as(C.c_void_p), int(n_errs[i]), C.c_float(lam[i]), C.c_float(prec[i]), int(mi[i]),
                                      r1.ctypes.data_as(C.c_void_p), C.byref(fc), C.byref(it))
        assert (k, fc.value, it.value) == tuple(fin[i]) and np.array_equal(rec[i].reshape(-1)[:5 * k], r1[:5 * k])
        broke += int(k > 0 and rec[i, k - 1, 4] == 1)
    print('depth schedules that broke:', broke)
    assert broke >= 50 and (fin[:, 0] == 0).sum() >= 40 and (fin[:, 0] == n_errs).sum() >= 20


# ---- lm_apply_step ----------------------------------------------------------------------------------------------------------------
def test_apply_step_class(host):
    st = Cs.apply_step_states(D.LM_STATE)
    out = host.apply_step(st)
    assert len(st) == 2090 and (out["iter"] == st["iter"] + 1).all()
    stop = out["stop_reason"] == 3
    assert 1100 < stop.sum() < 1400 and (out["active"][stop] == 0).all() and (out["active"][~stop] == 1).all()
    taken = Cs.quat_branch(_apply_product(host, st))
    assert (np.bincount(taken, minlength=4) >= 150).all()             # the compose behind the step leaves the positive-trace branch
    for i in range(0, len(st), 7):                                    # T = matrix(inc) = what the oracle's left update returns
        assert D.same_bits(out["T"][i], O.se3_left_update(st["delta"][i], rowmajor(_matrix_of(host, st["cur"][i]))).T.reshape(16)).all() or \
            not _roundtrip_exact(host, st["cur"][i])


def _matrix_of(host, se3):
    return se3_matrix(tuple(f32(v) for v in se3))


def _roundtrip_exact(host, se3):
    """Whether SE3(matrix(q)) gives q back bit for bit (the oracle's left update takes cur as a matrix)."""
    q, _ = host.se3_roundtrip(_matrix_of(host, se3))
    return D.same_bits(q[0], np.array(tuple(se3), f32)).all()


def _apply_product(host, st):
    d6 = st["delta"]
    cur = np.array([_matrix_of(host, s) for s in st["cur"]])
    return _product_matrix(host, d6, cur)


# ---- the Python restatement of the LM state machine -------------------------------------------------------------------------------
def quat_to_rot(q):
    """odo::quat_to_rot on float32 scalars, operation for operation. q = (qx, qy, qz, qw, ...)."""
    qx, qy, qz, qw = q[0], q[1], q[2], q[3]
    two = f32(2)
    tx, ty, tz = two * qx, two * qy, two * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    one = f32(1)
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)]


def rot_to_quat(R):
    """odo::rot_to_quat: (qx, qy, qz, qw)."""
    half, one = f32(0.5), f32(1)
    t = (R[0] + R[4]) + R[8]
    if t > 0:
        t = np.sqrt(t + one)
        qw = half * t
        t = half / t
        return ((R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t, qw)
    i = 1 if R[4] > R[0] else 0
    if R[8] > (R[4] if i == 1 else R[0]):
        i = 2
    if i == 0:
        t = np.sqrt(((R[0] - R[4]) - R[8]) + one)
        qx = half * t
        t = half / t
        return (qx, (R[3] + R[1]) * t, (R[6] + R[2]) * t, (R[7] - R[5]) * t)
    if i == 1:
        t = np.sqrt(((R[4] - R[8]) - R[0]) + one)
        qy = half * t
        t = half / t
        return ((R[1] + R[3]) * t, qy, (R[7] + R[5]) * t, (R[2] - R[6]) * t)
    t = np.sqrt(((R[8] - R[0]) - R[4]) + one)
    qz = half * t
    t = half / t
    return ((R[2] + R[6]) * t, (R[5] + R[7]) * t, qz, (R[3] - R[1]) * t)


def se3_matrix(s):
    """odo::se3_to_colmajor: 16 float32, column-major. s = (qx, qy, qz, qw, tx, ty, tz)."""
    R = quat_to_rot(s)
    M = [f32(0)] * 16
    for i in range(3):
        for j in range(3):
            M[j * 4 + i] = R[i * 3 + j]
    M[12], M[13], M[14], M[15] = s[4], s[5], s[6], f32(1)
    return np.array(M, f32)


def se3_from_matrix(M):
    R = [M[j * 4 + i] for i in range(3) for j in range(3)]
    return tuple(rot_to_quat(R)) + (M[12], M[13], M[14])


def restate_script(sc, acc):
    """One script through lm_begin_solve / lm_begin_level / lm_decide + solve + apply with the walk of lm_state_machine, in Python: the
    schedule rule spelled out (ref: src/lm_optimizer.cpp:110-155), the step from O.solve_damped, its exponential from O.se3_exp, the
    compose as the float32 4x4 product followed by the quaternion conversion above. Returns (states, events per evaluation)."""
    st = np.zeros(1, D.LM_STATE)[0]
    init = np.array(sc["init"], f32)
    cur = inc = last = se3_from_matrix(init)
    s = dict(status=0, n_evals=0, active=0, stop_reason=0, max_iters=0, finished=0, err_now=f32(0), iters_level=[0] * 8, delta=np.zeros(6, f32),
             level=-1, iter=0, lam=f32(0), err_last=f32(1e10), T=init.copy())
    n_levels, stop_level, lambda0, precision = int(sc["n_levels"]), int(sc["stop_level"]), f32(sc["lambda0"]), f32(sc["precision"])
    events = []
    zero_levels = [0]

    def walk():
        nonlocal inc
        while not s["active"] and s["status"] == 0 and not s["finished"]:
            nxt = n_levels - 1 if s["level"] < 0 else s["level"] - 1
            if nxt < stop_level:
                s["finished"] = 1
                break
            s["stop_reason"] = 0
            mi = int(sc["max_iters"][nxt])
            s["level"], s["iter"], s["err_last"], s["lam"] = nxt, 0, f32(1e10), lambda0
            inc = cur
            s["active"] = 1 if (s["status"] == 0 and mi > 0) else 0
            s["max_iters"] = mi
            s["T"] = se3_matrix(inc)
            zero_levels[0] += mi == 0
        if s["status"] != 0:
            s["finished"] = 1

    def record():
        r = st.copy()
        r["cur"], r["inc"], r["last"] = tuple(cur), tuple(inc), tuple(last)
        r["T"], r["lambda_"], r["err_last"], r["err_now"] = s["T"], s["lam"], s["err_last"], s["err_now"]
        for k in ("level", "iter", "active", "status", "n_evals", "stop_reason", "max_iters", "finished"):
            r[k] = s[k]
        r["iters_level"], r["delta"] = s["iters_level"], s["delta"]
        return r

    walk()
    out = []
    first = int(sc["acc_first"])
    with np.errstate(all="ignore"):
        for e in range(int(sc["n_evals"])):
            if not (s["active"] and s["status"] == 0 and not s["finished"]):
                break
            a = acc[first + e]
            ev = dict(level=s["level"], first_of_level=s["iters_level"][s["level"] & 7] == 0)
            s["n_evals"] += 1
            s["iters_level"][s["level"] & 7] += 1
            step = False
            if not (a[28] > 0.0):
                s["status"], s["active"] = -1, 0
                ev["n0"] = True
            else:
                err_now = f32(a[27] / a[28])
                s["err_now"] = err_now
                ev["nan"] = bool(np.isnan(err_now))
                if err_now > s["err_last"]:
                    ev["reject"] = True
                    s["lam"] = s["lam"] * f32(5)
                    if s["lam"] > f32(1e5):
                        s["active"], s["stop_reason"] = 0, 2
                    else:
                        cur = last
                        step = True
                else:
                    ev["accept"] = True
                    cur = inc
                    last = cur
                    if err_now / s["err_last"] > precision:
                        s["active"], s["stop_reason"] = 0, 1
                    else:
                        s["err_last"] = err_now
                        s["lam"] = max(s["lam"] / f32(5), f32(1e-5))
                        step = True
            if step:
                d = O.solve_damped(a, float(s["lam"]))
                s["delta"] = d
                ev["zero_pivot"] = bool((a[[0, 6, 11, 15, 18, 20]] == 0).any())
                ev["theta"] = float(Cs.se3_theta(d)[0])
                Dm = O.se3_exp(d).T.reshape(16)          # se3_to_colmajor(exp(delta))
                Cm = se3_matrix(cur)
                M = np.zeros(16, f32)
                for i in range(4):
                    for j in range(4):
                        M[j * 4 + i] = ((Dm[0 + i] * Cm[j * 4 + 0] + Dm[4 + i] * Cm[j * 4 + 1]) + Dm[8 + i] * Cm[j * 4 + 2]) + Dm[12 + i] * Cm[j * 4 + 3]
                ev["branch"] = int(Cs.quat_branch(M)[0])
                inc = se3_from_matrix(M)
                s["T"] = se3_matrix(inc)
                s["iter"] += 1
                if not (s["max_iters"] > s["iter"]):
                    s["active"], s["stop_reason"] = 0, 3
            ev["stop"] = 0 if s["active"] else s["stop_reason"]
            walk()
            ev["finished"] = s["finished"]
            events.append(ev)
            out.append(record())
    return out, events, zero_levels[0]


def test_python_quaternion_restatement_equals_oracle():
    """The two conversions the restatement adds to the oracle's calls, against the oracle's own round trip on every pose class."""
    for name, Ms in Cs.pose_matrices().items():
        for M in Ms:
            assert D.same_bits(se3_matrix(se3_from_matrix(M)), O.se3_roundtrip(rowmajor(M)).T.reshape(16)).all(), name


@pytest.fixture(scope="module")
def scripts():
    return Cs.lm_scripts(D.LM_SCRIPT)


def test_lm_scripts_host_replay_equals_restatement_and_covers_every_outcome(host, scripts):
    sc, acc, kinds = scripts
    assert len(sc) >= 200 and sc["n_evals"].max() <= Cs.MAX_EVALS and set(sc["n_levels"]) == {3, 4, 5}
    assert set(np.unique(sc["max_iters"])) == set(Cs.ITER_CHOICES)
    states, count = host.lm_script(sc, acc)
    feats = {k: 0 for k in ("accept", "reject", "stop2", "stop1", "stop3", "n0_first", "n0_mid", "nan", "zero_pivot", "zero_level", "stop_level_1",
                            "left_positive_trace", "tiny_step", "huge_step")}
    for i in range(len(sc)):
        ref, ev, zero_levels = restate_script(sc[i], acc)
        assert len(ref) == count[i], "script %d (%s): %d evaluations, the restatement makes %d" % (i, kinds[i], count[i], len(ref))
        first = int(sc["acc_first"][i])
        if ref:
            eq = D.same_states(states[first:first + count[i]], np.array(ref, D.LM_STATE))
            assert eq.all(), "script %d (%s): evaluation %d, dword %d" % ((i, kinds[i]) + tuple(np.argwhere(~eq)[0]))
        f = dict(accept=any(e.get("accept") for e in ev), reject=any(e.get("reject") for e in ev), stop2=any(e["stop"] == 2 for e in ev),
                 stop1=any(e["stop"] == 1 for e in ev), stop3=any(e["stop"] == 3 for e in ev),
                 n0_first=any(e.get("n0") and e["first_of_level"] for e in ev), n0_mid=any(e.get("n0") and not e["first_of_level"] for e in ev),
                 nan=any(e.get("nan") for e in ev), zero_pivot=any(e.get("zero_pivot") for e in ev), zero_level=zero_levels > 0,
                 stop_level_1=bool(ev and ev[-1]["finished"] and sc["stop_level"][i] == 1 and states[first + count[i] - 1]["status"] == 0),
                 left_positive_trace=any(e.get("branch", 0) != 0 for e in ev), tiny_step=any(e.get("theta", 1) < 1e-5 for e in ev),
                 huge_step=any(e.get("theta", 0) > np.pi / 2 for e in ev))
        for k, v in f.items():
            feats[k] += bool(v)
    print("scripts reaching each outcome:", feats, "evaluations consumed:", int(count.sum()))
    assert all(v >= 10 for v in feats.values()), feats
    assert count.sum() >= 2000


# ---- the per-pixel chain ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def levels(kitti_seq, small_seq):
    return Cs.pixel_levels(kitti_seq, small_seq)


def level_k_of(host, lv):
    fl, cxy = host.level_k([lv["K"]["f0"]], [lv["K"]["cx0"]], [lv["K"]["cy0"]], [lv["level"]])
    return float(fl[0]), float(cxy[0, 0]), float(cxy[0, 1])


def test_pixel_classes_reach_their_branches(host, levels):
    tot = dict(behind=0, off_left=0, off_right=0, off_top=0, off_bottom=0, last_col=0, last_row=0, first_col=0, first_row=0, integer_u=0,
               below_001=0, at_001=0, negative=0, above_4096=0, at_4096=0)
    for lv in levels:
        k = level_k_of(host, lv)
        rows, cols = lv["I1"].shape
        D1 = lv["D1"]
        inner = D1[4:rows - 4, 4:cols - 4]
        tot["below_001"] += int(((np.abs(inner) < f32(0.01)) & (inner != 0)).sum())
        tot["at_001"] += int((np.abs(inner) == f32(0.01)).sum())
        tot["negative"] += int((inner <= f32(-0.01)).sum())
        tot["above_4096"] += int((np.abs(inner) > 4096).sum())
        tot["at_4096"] += int((np.abs(inner) == 4096).sum())
        for name, T in Cs.level_poses(lv["K"], lv["level"], rows, cols, lv["motion"]).items():
            valid, front, u, v = Cs.warp_np(D1, k + (0,), T)
            with np.errstate(all="ignore"):
                fu, fv = np.floor(u), np.floor(v)
            vis = valid & front
            tot["behind"] += int((valid & ~front).sum())
            tot["off_left"] += int((vis & (fu < 0)).sum()); tot["off_right"] += int((vis & (fu >= cols)).sum())
            tot["off_top"] += int((vis & (fv < 0)).sum()); tot["off_bottom"] += int((vis & (fv >= rows)).sum())
            inside = vis & (fu >= 0) & (fu < cols) & (fv >= 0) & (fv < rows)
            tot["last_col"] += int((inside & (fu == cols - 1)).sum()); tot["last_row"] += int((inside & (fv == rows - 1)).sum())
            tot["first_col"] += int((inside & (fu == 0)).sum()); tot["first_row"] += int((inside & (fv == 0)).sum())
            tot["integer_u"] += int((inside & (fu == u) & (fv == v)).sum())
            hit = host.pixels(lv["I1"], lv["I2"], D1, k + (0,), T, 0)[0]
            assert np.array_equal(hit.astype(bool), inside), (lv["name"], name)         # the numpy restatement of the warp IS the host build's
            if name == "inf_entry":
                assert hit.sum() == 0 and valid.sum() > 0                              # every point skipped
            if lv["name"] == "pow2" and name == "integer_and_last":
                assert (inside & (fu == u) & (fv == v)).sum() == inside.sum() > 2000   # whole-pixel shift: every landing point an integer
                assert (inside & (fu == cols - 1)).sum() == rows - 9 and (inside & (fv == rows - 1)).sum() == cols - 10
    print("pixels per branch:", tot)
    assert all(v >= 40 for v in tot.values()), tot


@pytest.mark.parametrize("bilinear", [0, 1])
def test_pixel_chain_host_equals_oracle_dump(host, levels, bilinear):
    """hit count = the oracle's N; r, w, J of every hit in scan order = the oracle's dump, by bit pattern; on every level, pose and
    robust mode 0 / 1. The lean form (point_residual<false>) and the residual-only form equal the full one in floor mode."""
    O.set_sampling(bool(bilinear))
    try:
        for lv in levels:
            k = level_k_of(host, lv) + (bilinear,)
            rows, cols = lv["I1"].shape
            for name, T in Cs.level_poses(lv["K"], lv["level"], rows, cols, lv["motion"]).items():
                for robust in (0, 1):
                    hit, r, w, J = host.pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 0, robust=robust)
                    n = int(hit.sum())
                    ref = O.lm_accumulate(lv["I1"], lv["I2"], lv["D1"], lv["level"], T, robust=robust, K=lv["K"], dump=max(n, 1))
                    assert int(ref["acc"][28]) == n and ref["status"] == (0 if n else -1), (lv["name"], name)
                    m = hit.astype(bool)
                    assert D.same_bits(r[m], ref["r"][:n]).all() and D.same_bits(w[m], ref["w"][:n]).all() and \
                        D.same_bits(J[m], ref["J"][:n]).all(), (lv["name"], name, robust)
                if not bilinear:
                    h1, r1, w1, J1 = host.pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 1)
                    h3, r3, _, _ = host.pixels(lv["I1"], lv["I2"], lv["D1"], k, T, 3)
                    assert np.array_equal(h1, hit) and np.array_equal(h3, hit) and D.same_bits(r1, r).all() and D.same_bits(r3, r).all() and \
                        D.same_bits(J1, J).all()
    finally:
        O.set_sampling(False)


# ---- division operands ------------------------------------------------------------------------------------------------------------
def test_division_operand_classes_cover_their_intervals():
    for name, (form, ne, de) in Cs.DIV32_FORMS.items():
        f, a, b = Cs.div32_operands(name, n=1 << 16)
        assert f == form and len(b) == 1 << 16 and np.isfinite(a).all() and np.isfinite(b).all() and (b != 0).all()
        eb = np.frexp(np.abs(b[8:]))[1] - 1
        lo, hi = (de[0], de[1] - 1)
        assert eb.min() >= (lo if name != "1/d" else -7) and eb.max() == hi and len(np.unique(eb)) >= hi - lo      # every exponent of the interval
        man = np.abs(b).view(np.uint32) & 0x7fffff
        assert (man == 0).sum() > 2000 and (man == 1).sum() > 2000 and (man == 0x7fffff).sum() > 2000
        if name == "1/d":
            assert np.abs(b).min() == f32(0.01) and (np.abs(b) == 4096).sum() >= 2 and np.abs(b).max() <= 4096
    a, b = Cs.div64_operands(1 << 16)
    assert (b > 0).all() and np.isfinite(a).all() and (a == 0).sum() > 500
    x, y, d, fl, cx, cy, T = Cs.callsite_cases(1 << 16)
    ok = np.array([Cs_dense_fast_ok(fl[i], cx[i], cy[i]) for i in range(0, len(x), 64)])
    assert ok.all() and (np.abs(d) >= f32(0.01)).all() and (np.abs(d) <= 4096).all() and (np.abs(T) <= 2.0 ** 20).all()
    assert (x.astype(f32) == cx).sum() > 500 and (x == 65530).sum() > 5000 and {1.0, 65536.0} <= set(fl.tolist()) and (np.abs(T) == 2.0 ** 20).any()
    x, y, d, fl, cx, cy, T = Cs.callsite_cases(1 << 12, outside=True)
    assert (np.abs(d) > 4096).all() and (np.abs(d) < 2.0 ** 14).all() and (fl == 131072.0).all()
    assert not Cs_dense_fast_ok(fl[0], cx[0], cy[0])


def Cs_dense_fast_ok(fl, cx, cy, rows=1080, cols=1920):
    """dense_fast_ok (dense.hip.h) restated; tests/test_gpu_devmath.py checks the restatement against the function itself."""
    def frac_ok(c):
        c = f32(c)
        r = c - np.floor(c)
        dist = r if r < f32(0.5) else f32(1) - r
        return dist == 0 or dist >= f32(1.0 / 256.0)
    return bool(1.0 <= fl <= 65536.0 and abs(f32(cx)) <= 65536 and abs(f32(cy)) <= 65536 and frac_ok(cx) and frac_ok(cy) and rows <= 65535
                and cols <= 65535)
