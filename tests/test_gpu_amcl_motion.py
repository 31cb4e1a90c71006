"""amcl's odometry motion model on the device (navgpu_amcl_odom_configure / navgpu_amcl_update_action) against the reference's goldens
(tests/golden/g11_amcl_motion.npz, written by tools/make_amcl_motion_goldens.py from the reference amcl core itself), a pure-Python
restatement of pf_ran_gaussian's drand48 consumption on large batches, the data the call must leave alone, the device generator's
statistics, and a resident motion -> sensor -> resample cycle against the same steps with a host round trip."""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "g11_amcl_motion.npz")
RTOL, ATOL = 1e-12, 1e-12
OK, ERR_INVALID, ERR_STATE = 0, -1, -5
DIFF, OMNI, DIFF_CORRECTED, OMNI_CORRECTED, GAUSSIAN = range(5)
A48, C48, M48 = 0x5DEECE66D, 0xB, 1 << 48


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if nav.lib().navgpu_device_count() <= 0:
        pytest.skip("no GPU")
    return nav


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return {k: g[k] for k in g.files}


def gauss_stream(state, n):
    """pf_ran_gaussian's drand48 consumption (pf_pdf.c:132-146): skip 0.0, pair the rest, accept 0 < w <= 1.
    -> (state after, x2 (n,), w (n,))"""
    x, pend, x2s, ws = state, None, [], []
    while len(ws) < n:
        x = (A48 * x + C48) % M48
        if x == 0:
            continue
        r = x / float(M48)
        if pend is None:
            pend = r
            continue
        x1, x2, pend = 2.0 * pend - 1.0, 2.0 * r - 1.0, None
        w = x1 * x1 + x2 * x2
        if w > 1.0 or w == 0.0:
            continue
        x2s.append(x2)
        ws.append(w)
    return x, np.array(x2s), np.array(ws)


def angle_diff(a, b):
    a = np.arctan2(np.sin(a), np.cos(a))
    b = np.arctan2(np.sin(b), np.cos(b))
    d1 = a - b
    d2 = 2 * np.pi - np.abs(d1)
    d2 = np.where(d1 > 0, -d2, d2)
    return np.where(np.abs(d1) < np.abs(d2), d1, d2)


def motion_numpy(params, odom, poses, x2, w):
    """numpy restatement of AMCLOdom::UpdateAction for one filter with the deviates' records (x2, w) in draw order"""
    model, a1, a2, a3, a4, a5 = params
    model = int(model)
    pose, delta, absm = odom[:3], odom[3:6], odom[6:]
    s = np.sqrt(-2.0 * np.log(w) / w)
    x2, s = x2.reshape(-1, 3), s.reshape(-1, 3)
    g = lambda j, sd: sd * x2[:, j] * s[:, j]  # noqa: E731
    p = poses.copy()
    old_th = pose[2] - delta[2]
    dt = math.sqrt(delta[0] * delta[0] + delta[1] * delta[1])
    if model in (OMNI, OMNI_CORRECTED):
        dr = delta[2]
        sd = [a3 * dt * dt + a1 * dr * dr, a4 * dr * dr + a2 * dt * dt, a1 * dr * dr + a5 * dt * dt]
        if model == OMNI_CORRECTED:
            sd = [math.sqrt(v) if v >= 0 else math.nan for v in sd]
        b = angle_diff(math.atan2(delta[1], delta[0]), old_th) + p[:, 2]
        th, rh, sh = dt + g(0, sd[0]), dr + g(1, sd[1]), g(2, sd[2])
        p[:, 0] += th * np.cos(b) + sh * np.sin(b)
        p[:, 1] += th * np.sin(b) - sh * np.cos(b)
        p[:, 2] += rh
    elif model in (DIFF, DIFF_CORRECTED):
        r1 = 0.0 if dt < 0.01 else float(angle_diff(math.atan2(delta[1], delta[0]), old_th))
        r2 = float(angle_diff(delta[2], r1))
        n1 = min(abs(float(angle_diff(r1, 0.0))), abs(float(angle_diff(r1, math.pi))))
        n2 = min(abs(float(angle_diff(r2, 0.0))), abs(float(angle_diff(r2, math.pi))))
        sd = [a1 * n1 * n1 + a2 * dt * dt, a3 * dt * dt + a4 * n1 * n1 + a4 * n2 * n2, a1 * n2 * n2 + a2 * dt * dt]
        if model == DIFF_CORRECTED:
            sd = [math.sqrt(v) if v >= 0 else math.nan for v in sd]
        r1h = angle_diff(r1, g(0, sd[0]))
        th = dt - g(1, sd[1])
        r2h = angle_diff(r2, g(2, sd[2]))
        p[:, 0] += th * np.cos(p[:, 2] + r1h)
        p[:, 1] += th * np.sin(p[:, 2] + r1h)
        p[:, 2] += r1h + r2h
    else:
        t2, s2, r2 = absm[0] ** 2, absm[1] ** 2, absm[2] ** 2
        sr, st, ss = math.sqrt(a1 * r2 + a2 * t2), math.sqrt(a3 * t2 + a4 * r2), math.sqrt(a4 * r2 + a5 * s2)
        h = p[:, 2] + delta[2] / 2
        b = angle_diff(math.atan2(delta[1], delta[0]), old_th) + p[:, 2]
        th, sh, rh = g(0, st), g(1, ss), g(2, sr)
        p[:, 0] += dt * np.cos(b) + (th * np.cos(h) + sh * np.sin(h))
        p[:, 1] += dt * np.sin(b) + (th * np.sin(h) - sh * np.cos(h))
        p[:, 2] += delta[2] + rh
    return p


def compare(got, ref, what, rtol=RTOL, atol=ATOL):
    """x, y within rtol relative + atol; theta the same modulo 2 pi.  NaN where the reference has NaN.  -> wraps by 2 pi (counted)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    g, r = np.where(nan, 0, got), np.where(nan, 0, ref)
    tol = rtol * np.abs(r) + atol
    assert np.all(np.abs(g[:, :2] - r[:, :2]) <= tol[:, :2]), (what, np.max(np.abs(g[:, :2] - r[:, :2])))
    d = g[:, 2] - r[:, 2]
    wraps = int(np.sum(np.abs(d) > np.pi))
    d = (d + np.pi) % (2 * np.pi) - np.pi
    assert np.all(np.abs(d) <= tol[:, 2] + 4 * np.pi * 2.0 ** -52 * (np.abs(d) > 0)), (what, np.max(np.abs(d)))
    return wraps


def golden_case(g, name):
    return (g[name + "_params"], g[name + "_odom"], int(g[name + "_state"][0]), int(g[name + "_state"][1]), int(g[name + "_count"][0]),
            g[name + "_poses_in"], g[name + "_poses_out"])


def handle(nav, n_filters, max_samples, params=None):
    a = nav.AmclLaser(n_filters, max(max_samples, 1))
    if params is not None:
        a.configure_odom(int(params[0]), *[float(v) for v in params[1:]])
    return a


def upload(a, poses_list, counts, rng=None, first=0):
    rng = rng or np.random.default_rng(0)
    nf = len(poses_list)
    P = np.zeros((nf, a.max_samples, 3))
    for k, p in enumerate(poses_list):
        P[k, :len(p)] = p
    W = rng.uniform(0.1, 1.0, (nf, a.max_samples))
    a.set_samples(P, W, sample_counts=np.asarray(counts, np.int32), converged=np.arange(nf) % 2, first=first)
    return P, W


def test_golden_cases_alone(nav, golden):
    wraps = {}
    for name in golden["cases"]:
        name = str(name)
        params, odom, s_in, s_out, n, P_in, P_out = golden_case(golden, name)
        a = handle(nav, 1, len(P_in), params)
        upload(a, [P_in], [n])
        rc, st, states = a.update_action(odom[None], drand48_state=[s_in])
        assert rc == OK and st[0] == OK
        assert int(states[0]) == s_out, name
        _, P, _, _ = a.get_samples()
        wraps[name] = compare(P[0, :n], P_out, name)
        assert np.array_equal(P[0, n:len(P_in)], P_in[n:]), name  # the tail past sample_count
        a.close()
    print("theta wraps by 2 pi (1-ulp atan2 at +-pi):", {k: v for k, v in wraps.items() if v} or "none")
    assert sum(wraps.values()) <= 3


@pytest.mark.parametrize("model", [DIFF, OMNI, DIFF_CORRECTED, OMNI_CORRECTED, GAUSSIAN])
def test_golden_cases_batched(nav, golden, model):
    """every golden case of one model in one call: different sample counts, states and odometry per filter"""
    names = [str(n) for n in golden["cases"] if int(golden[str(n) + "_params"][0]) == model]
    groups = {}
    for nm in names:  # one configure per handle: the alphas must agree within a call
        groups.setdefault(tuple(golden[nm + "_params"]), []).append(nm)
    for params, group in groups.items():
        cases = [golden_case(golden, nm) for nm in group]
        ms = max(len(c[5]) for c in cases)
        a = handle(nav, len(cases) + 1, ms, params)
        upload(a, [c[5] for c in cases], [c[4] for c in cases], first=1)
        odom = np.stack([c[1] for c in cases])
        rc, st, states = a.update_action(odom, drand48_state=[c[2] for c in cases], first=1)
        assert rc == OK and np.all(st == OK)
        _, P, _, _ = a.get_samples()
        for k, (nm, c) in enumerate(zip(group, cases)):
            assert int(states[k]) == c[3], nm
            compare(P[k + 1, :c[4]], c[6], nm)
            assert np.array_equal(P[k + 1, c[4]:len(c[5])], c[5][c[4]:]), nm
        a.close()


@pytest.mark.parametrize("model", [DIFF, GAUSSIAN])
def test_large_batch_matches_the_python_stream(nav, model):
    """256 filters x 5000 particles in one call; 16 of them replayed in Python: exact states, poses against a numpy restatement"""
    nf, n = 256, 5000
    rng = np.random.default_rng(11 + model)
    params = [model, 0.2, 0.1, 0.3, 0.05, 0.15]
    a = handle(nav, nf, n, params)
    counts = np.full(nf, n)
    counts[::7] = rng.integers(1, n, len(counts[::7]))
    poses = [np.column_stack([rng.normal(0, 2, n), rng.normal(0, 2, n), rng.uniform(-math.pi, math.pi, n)]) for _ in range(nf)]
    P_in, _ = upload(a, poses, counts, rng)
    odom = np.column_stack([rng.normal(0, 3, (nf, 2)), rng.uniform(-3, 3, nf), rng.normal(0, 0.1, (nf, 2)), rng.normal(0, 0.1, nf),
                            rng.normal(0, 0.1, (nf, 3))])
    states = np.array([rng.integers(0, M48) for _ in range(nf)], np.uint64)
    rc, st, out = a.update_action(odom, drand48_state=states)
    assert rc == OK and np.all(st == OK)
    _, P, _, _ = a.get_samples()
    check = rng.choice(nf, 16, replace=False)
    wraps = 0
    for f in check:
        c = int(counts[f])
        s_after, x2, w = gauss_stream(int(states[f]), 3 * c)
        assert int(out[f]) == s_after, f
        ref = motion_numpy(params, odom[f], P_in[f, :c], x2, w)
        wraps += compare(P[f, :c], ref, f"filter {f}", rtol=1e-9, atol=1e-9)  # numpy's libm is not the reference's
        assert np.array_equal(P[f, c:], P_in[f, c:])
    print(f"model {model}: {wraps} theta wraps by 2 pi in {int(counts[check].sum())} samples")
    a.close()


def test_untouched_state_stays_bit_identical(nav):
    rng = np.random.default_rng(5)
    nf, n = 4, 600
    a = handle(nav, nf, n, [OMNI_CORRECTED, 0.2, 0.2, 0.2, 0.2, 0.2])
    poses = [np.column_stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-3, 3, n)]) for _ in range(nf)]
    upload(a, poses, [n] * nf, rng)
    a.set_filter_state(np.tile([[0.4, 0.4]], (nf, 1)))
    a.configure_resample(resample_model=1, min_samples=50)
    rc, _ = a.update_resample(draws={"systematic_start": rng.uniform(0, 1e-3, nf), "random_poses": [np.zeros((0, 3))] * nf})
    assert rc == OK
    a.set_filter_state(np.tile([[0.3, 0.7]], (nf, 1)))
    before = (a.get_samples(), a.get_filter_state(), a.kd_leaf_counts(), [a.clusters(f) for f in range(nf)], a.rng_counters())
    odom = np.tile([0.3, 0.2, 0.1, 0.2, 0.1, 0.05, 0, 0, 0], (nf, 1))
    rc, st, _ = a.update_action(odom, drand48_state=[0x330E + k for k in range(nf)])
    assert rc == OK
    (sc0, P0, W0, cv0), ws0, leaf0, cl0, ctr0 = before
    sc, P, W, cv = a.get_samples()
    assert np.array_equal(sc, sc0) and np.array_equal(W, W0) and np.array_equal(cv, cv0)
    assert np.array_equal(a.get_filter_state(), ws0) and np.array_equal(a.kd_leaf_counts(), leaf0)
    assert np.array_equal(a.rng_counters(), ctr0)  # drand48 mode does not use the device generator
    for f in range(nf):
        c = int(sc[f])
        assert not np.array_equal(P[f, :c], P0[f, :c])
        assert np.array_equal(P[f, c:], P0[f, c:])
        for x, y in zip(a.clusters(f), cl0[f]):
            assert np.array_equal(x, y)
    a.close()


def test_state_out_of_range_is_invalid_and_leaves_the_filter(nav, golden):
    params, odom, s_in, s_out, n, P_in, P_out = golden_case(golden, "diff_forward")
    a = handle(nav, 2, len(P_in), params)
    upload(a, [P_in, P_in], [n, n])
    rc, st, states = a.update_action(np.stack([odom, odom]), drand48_state=np.array([M48, s_in], np.uint64), raise_on_error=False)
    assert rc == ERR_INVALID and list(st) == [ERR_INVALID, OK]
    assert int(states[0]) == M48 and int(states[1]) == s_out
    _, P, _, _ = a.get_samples()
    assert np.array_equal(P[0, :len(P_in)], P_in)
    compare(P[1, :n], P_out, "the valid filter")
    a.close()


def test_validation(nav):
    from navigation_amd import _lib
    a = nav.AmclLaser(2, 10)
    L, h = a.L, a.h
    odom = np.zeros((2, 9))
    x = np.full(2, 0x330E, np.uint64)
    st = np.zeros(2, np.int32)
    p = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.navgpu_amcl_update_action(h, 0, 2, p(odom), _lib.AMCL_DRAW_DRAND48, p(x), 0, p(st)) == ERR_STATE
    assert L.navgpu_amcl_update_action(h, 0, 2, p(odom), _lib.AMCL_DRAW_DEVICE, None, 0, p(st)) == ERR_STATE
    a.configure_odom(DIFF)
    assert L.navgpu_amcl_update_action(h, 0, 2, p(odom), _lib.AMCL_DRAW_SUPPLIED, p(x), 0, p(st)) == ERR_INVALID
    assert L.navgpu_amcl_update_action(h, 0, 2, p(odom), 3, p(x), 0, p(st)) == ERR_INVALID
    assert L.navgpu_amcl_update_action(h, 0, 2, None, _lib.AMCL_DRAW_DRAND48, p(x), 0, p(st)) == ERR_INVALID
    assert L.navgpu_amcl_update_action(h, 0, 2, p(odom), _lib.AMCL_DRAW_DRAND48, None, 0, p(st)) == ERR_INVALID
    assert L.navgpu_amcl_update_action(h, 1, 2, p(odom), _lib.AMCL_DRAW_DRAND48, p(x), 0, p(st)) == ERR_INVALID
    for bad in (dict(model_type=5), dict(model_type=-1), dict(alpha3=math.nan)):
        q = _lib.AmclOdomParams(**bad)
        assert L.navgpu_amcl_odom_configure(h, C.byref(q)) == ERR_INVALID
    # the resampler still rejects the drand48 source
    assert L.navgpu_amcl_update_resample(h, 0, 2, _lib.AMCL_DRAW_DRAND48, None, None, None, None, 0, p(st)) == ERR_INVALID
    a.close()


def test_invalid_configure_keeps_the_previous_one(nav, golden):
    params, odom, s_in, s_out, n, P_in, P_out = golden_case(golden, "omni_forward")
    a = handle(nav, 1, len(P_in), params)
    with pytest.raises(nav.NavgpuError):
        a.configure_odom(7, 0.1, 0.1, 0.1, 0.1, 0.1)
    with pytest.raises(nav.NavgpuError):
        a.configure_odom(DIFF, math.nan)
    upload(a, [P_in], [n])
    _, _, states = a.update_action(odom[None], drand48_state=[s_in])
    assert int(states[0]) == s_out
    compare(a.get_samples()[1][0, :n], P_out, "omni after rejected configures")
    a.close()


def device_run(nav, model, seed, counters=None, nf=3, n=700):
    rng = np.random.default_rng(9)
    a = handle(nav, nf, n, [model, 0.2, 0.2, 0.2, 0.2, 0.2])
    upload(a, [rng.normal(0, 1, (n, 3)) for _ in range(nf)], [n] * nf, rng)
    if counters is not None:
        a.set_rng_counters(counters)
    rc, st, _ = a.update_action(np.tile([0.5, 0.2, 0.3, 0.1, 0.05, 0.1, 0.1, 0.05, 0.1], (nf, 1)), seed=seed)
    assert rc == OK and np.all(st == OK)
    out = a.get_samples()[1], a.rng_counters()
    a.close()
    return out


def test_device_draws_repeat_with_seed_and_counter(nav):
    for model in (DIFF, OMNI, GAUSSIAN):
        p0, c0 = device_run(nav, model, 42)
        p1, c1 = device_run(nav, model, 42)
        p2, _ = device_run(nav, model, 43)
        p3, c3 = device_run(nav, model, 42, counters=np.full(3, 5, np.uint64))
        assert p0.tobytes() == p1.tobytes()
        assert np.array_equal(c0, np.ones(3, np.uint64)) and np.array_equal(c3, np.full(3, 6, np.uint64))
        assert not np.any(np.all(p0 == p2, axis=2)[:, :700]) and not np.any(np.all(p0 == p3, axis=2)[:, :700])
        assert not np.array_equal(p0[0, :700], p0[1, :700])  # filters draw from their own streams


def free_map():
    occ = -np.ones((80, 100), np.int8)
    occ[0, :] = occ[-1, :] = occ[:, 0] = occ[:, -1] = 1
    occ[30:50, 40:45] = 1
    return occ, 0.05, (0.3, -0.2)


def test_device_counter_is_shared_with_resample(nav):
    """motion (counter 0) -> device resample (counter 1) -> motion draws with counter 2: the same bytes as that last motion call
    on a handle holding the resampled set with its counter set to 2"""
    rng = np.random.default_rng(4)
    nf, n = 2, 400
    odom = np.tile([0.5, 0.2, 0.3, 0.1, 0.05, 0.1, 0, 0, 0], (nf, 1))
    a = handle(nav, nf, n, [DIFF, 0.2, 0.2, 0.2, 0.2, 0.2])
    occ, scale, org = free_map()
    a.set_map_cells(occ, scale, org, max_occ_dist=0.5)
    upload(a, list(rng.normal(0, 0.5, (nf, n, 3))), [n] * nf)
    a.set_filter_state(np.tile([[1.0, 1.0]], (nf, 1)))
    a.update_action(odom, seed=77)
    assert np.array_equal(a.rng_counters(), np.ones(nf, np.uint64))
    a.configure_resample(resample_model=0, min_samples=n)
    rc, _ = a.update_resample(seed=77)
    assert rc == OK and np.array_equal(a.rng_counters(), np.full(nf, 2, np.uint64))
    sc, P, W, cv = a.get_samples()
    a.update_action(odom, seed=77)
    assert np.array_equal(a.rng_counters(), np.full(nf, 3, np.uint64))
    moved = a.get_samples()[1]
    a.close()
    b = handle(nav, nf, n, [DIFF, 0.2, 0.2, 0.2, 0.2, 0.2])
    b.set_samples(P, W, sample_counts=sc, converged=cv)
    b.set_rng_counters(np.full(nf, 2, np.uint64))
    b.update_action(odom, seed=77)
    assert b.get_samples()[1].tobytes() == moved.tobytes()
    b.set_samples(P, W, sample_counts=sc, converged=cv)
    b.set_rng_counters(np.full(nf, 1, np.uint64))  # the resample's counter: different draws
    b.update_action(odom, seed=77)
    assert not np.any(np.all(b.get_samples()[1] == moved, axis=2)[:, :int(sc.min())])
    b.close()


@pytest.mark.parametrize("model", [DIFF, OMNI, DIFF_CORRECTED, OMNI_CORRECTED, GAUSSIAN])
def test_device_draws_have_the_model_sigmas(nav, model):
    """identical particles: the recovered deviates have mean 0, the model's sigma and no correlation, within 5 standard errors"""
    nf, n = 4, 5000
    al = [0.05, 0.05, 0.01, 0.05, 0.05]
    if model == GAUSSIAN:
        odom, th0 = [1.0, 2.0, 0.05, 0.1, 0.0, 0.05, 0.1, 0.02, 0.05], -0.025  # heading p + dth / 2 = 0
    else:
        odom, th0 = [1.0, 2.0, 0.05, 0.1, 0.0, 0.05, 0.0, 0.0, 0.0], 0.0        # bearing angle_diff(0, 0) + 0 = 0
    P0 = np.tile([0.0, 0.0, th0], (n, 1))

    def run(alphas, seed=3):
        a = handle(nav, nf, n, [model] + alphas)
        upload(a, [P0] * nf, [n] * nf)
        a.update_action(np.tile(odom, (nf, 1)), seed=seed)
        P = a.get_samples()[1].reshape(-1, 3)
        a.close()
        return P

    P, Z = run(al), run([0.0] * 5)
    dt, dr = 0.1, 0.05
    if model in (OMNI, OMNI_CORRECTED, GAUSSIAN):  # cos = 1, sin = 0 where the noise enters: (e_trans, -e_strafe, e_rot)
        e = np.column_stack([P[:, 0] - Z[:, 0], -(P[:, 1] - Z[:, 1]), P[:, 2] - Z[:, 2]])
    else:  # diff: rot1_hat = atan2(dy, dx) = -e1, trans_hat = |d| = dt - e2, rot2_hat = dth - rot1_hat = dr - e3
        r1h = np.arctan2(P[:, 1], P[:, 0])
        e = np.column_stack([-r1h, dt - np.hypot(P[:, 0], P[:, 1]), dr - (P[:, 2] - r1h)])
    a1, a2, a3, a4, a5 = al
    if model in (OMNI, OMNI_CORRECTED):
        sd = np.array([a3 * dt * dt + a1 * dr * dr, a1 * dr * dr + a5 * dt * dt, a4 * dr * dr + a2 * dt * dt])
    elif model in (DIFF, DIFF_CORRECTED):
        sd = np.array([a2 * dt * dt, a3 * dt * dt + a4 * dr * dr, a1 * dr * dr + a2 * dt * dt])  # rot1 = 0, rot2 = dr
    else:
        t2, s2, r2 = 0.1 ** 2, 0.02 ** 2, 0.05 ** 2
        sd = np.sqrt([a3 * t2 + a4 * r2, a4 * r2 + a5 * s2, a1 * r2 + a2 * t2])
    if model in (DIFF_CORRECTED, OMNI_CORRECTED):
        sd = np.sqrt(sd)
    N = len(e)
    z = e / sd
    assert np.all(np.abs(z.mean(0)) <= 5 / math.sqrt(N)), z.mean(0)
    assert np.all(np.abs(z.var(0) - 1) <= 5 * math.sqrt(2 / N)), z.var(0)
    c = np.corrcoef(z.T)
    assert np.all(np.abs(c[np.triu_indices(3, 1)]) <= 5 / math.sqrt(N)), c


@pytest.mark.parametrize("resample_model", [0, 1])
def test_resident_cycle_equals_a_host_round_trip(nav, resample_model):
    """update_action -> update_sensor -> update_resample twice on a resident set, against the same steps with get_samples /
    set_samples after each motion update (set_samples recounts the kd leaves from the moved poses; the saved counts go back)"""
    rng = np.random.default_rng(21)
    nf, n = 6, 1500
    occ, scale, org = free_map()
    P0 = np.stack([rng.uniform(-1.5, 1.5, (nf, n)), rng.uniform(-1.2, 1.2, (nf, n)), rng.uniform(-3, 3, (nf, n))], 2) + 0.0123
    W0 = np.full((nf, n), 1.0 / n)
    bearings = np.linspace(-1.5, 1.5, 90)
    scans = [[np.stack([rng.uniform(0.5, 3.0, 90), bearings], 1) for _ in range(nf)] for _ in range(2)]
    odoms = [np.column_stack([rng.normal(0, 1, (nf, 3)), rng.normal(0, 0.1, (nf, 3)), np.zeros((nf, 3))]) for _ in range(2)]
    states = np.array([rng.integers(0, M48) for _ in range(nf)], np.uint64)
    outs = []
    for round_trip in (False, True):
        a = nav.AmclLaser(nf, n)
        a.set_map_cells(occ, scale, org, max_occ_dist=0.5)
        a.configure(model_type=1, max_beams=30)
        a.set_laser_pose(np.tile([0.1, 0.0, 0.0], (nf, 1)))
        a.configure_resample(resample_model=resample_model, min_samples=100)
        a.configure_odom(DIFF_CORRECTED, 0.2, 0.2, 0.2, 0.2)
        a.set_samples(P0, W0)
        a.set_filter_state(np.tile([[0.0, 0.0]], (nf, 1)))
        x = states.copy()
        for r in range(2):
            _, _, x = a.update_action(odoms[r], drand48_state=x)
            if round_trip:
                leaf = a.kd_leaf_counts()
                sc, P, W, cv = a.get_samples()
                a.set_samples(P, W, sample_counts=sc, converged=cv)
                a.set_kd_leaf_counts(leaf)
            a.update_sensor(scans[r], 4.0)
            rc, st = a.update_resample(seed=1000 + r)
            assert rc == OK and np.all(st == OK)
        outs.append((a.get_samples(), a.get_filter_state(), a.kd_leaf_counts(), x))
        a.close()
    (s0, w0, l0, x0), (s1, w1, l1, x1) = outs
    for u, v in zip(s0, s1):
        assert u.tobytes() == v.tobytes()
    assert w0.tobytes() == w1.tobytes() and np.array_equal(l0, l1) and np.array_equal(x0, x1)
