"""amcl's laser sensor update on the device (navgpu_amcl_*) against the reference's goldens (tests/golden/g9_amcl.npz, written
by tools/make_amcl_goldens.py from the reference amcl core itself) and the exact distance-transform specification."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import amcl_spec as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "g9_amcl.npz")
LASER = (0.12, -0.03, 0.05)
RTOL = 1e-12



@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if nav.lib().navgpu_device_count() <= 0:
        pytest.skip("no GPU")
    return nav


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def params_of(golden, name, nav):
    v = golden[f"{name}_params"]
    d = {str(k): (int(x) if k in ("model_type", "max_beams", "do_beamskip") else float(x)) for k, x in zip(golden["param_order"], v)}
    return nav._lib.AmclLaserParams(**d)


def load_map(a, golden, m, first=0, ref_dist=True):
    g = golden[f"map{m}_geom"]
    a.set_map(golden[f"map{m}_data"], g[2], (g[4], g[5]), max_occ_dist=g[6], scale_up_factor=int(g[3]), first=first, count=1)
    if ref_dist:
        a.set_distance_map(golden[f"map{m}_dist"], first=first, count=1)


def case(golden, name, m):
    k = f"{name}_m{m}"
    st = golden[k + "_state_in"]
    return dict(poses=golden[k + "_poses"], w=golden[k + "_weights_in"], scan=golden[k + "_scan"], w0=st[:2], conv=int(st[2]),
                range_max=st[3], out=golden[k + "_out"])


def assert_close(got, want, what):
    want = np.asarray(want, np.float64)
    err = np.abs(np.asarray(got) - want)
    assert np.all(err <= RTOL * np.abs(want) + 1e-300), f"{what}: max rel {np.max(err / np.maximum(np.abs(want), 1e-300)):.3g}"


# ---------------------------------------------------------------------------------------------------- distance map


def test_distance_map_golden_maps(nav, golden):
    a = nav.AmclLaser(3, 16, 30)
    for m in range(3):
        load_map(a, golden, m, first=m, ref_dist=False)
    for m in range(3):
        g = golden[f"map{m}_geom"]
        occ = S.convert_map(golden[f"map{m}_data"], int(g[3]))
        d = a.distance_map(m)
        spec = S.exact_cspace(occ, g[9], g[6])
        assert d.tobytes() == spec.tobytes(), m
        assert (d <= golden[f"map{m}_dist"]).all(), m
    a.close()


@pytest.mark.parametrize("shape,res,f,radius_cells,density", [
    ((2000, 2000), 0.05, 1, 40, 0.003), ((300, 517), 0.05, 1, 1, 0.02), ((421, 233), 0.05, 2, 120, 0.0005),
    ((1000, 700), 0.02, 1, 100, 0.001), ((64, 90), 0.1, 1, 7, 0.0)])
def test_distance_map_exact(nav, shape, res, f, radius_cells, density):
    rng = np.random.default_rng(sum(shape) + radius_cells)
    data = np.zeros(shape, np.int8)
    r = rng.random(shape)
    data[r < density] = 100
    data[(r > 0.5) & (r < 0.51)] = -1
    data[(r > 0.7) & (r < 0.702)] = 30
    if density:
        data[shape[0] // 2, 10:shape[1] // 2] = 100
    max_occ = (radius_cells + 0.5) * res / f
    a = nav.AmclLaser(2, 8, 30)
    a.set_map(data, res, (-1.0, 2.0), max_occ_dist=max_occ, scale_up_factor=f)
    spec = S.exact_cspace(S.convert_map(data, f), res / f, max_occ)
    for k in range(2):
        assert a.distance_map(k).tobytes() == spec.tobytes()
    a.close()


def test_distance_map_shared_vs_per_filter(nav):
    rng = np.random.default_rng(3)
    maps = np.where(rng.random((3, 80, 120)) < 0.01, 100, 0).astype(np.int8)
    a = nav.AmclLaser(4, 8, 30)
    a.set_map(maps[0], 0.05, (0, 0), max_occ_dist=0.6)              # shared by all 4
    a.set_map(maps, 0.05, (0, 0), max_occ_dist=0.6, first=1, count=3)  # then per filter on 1..3
    assert a.distance_map(0).tobytes() == S.exact_cspace(S.convert_map(maps[0]), 0.05, 0.6).tobytes()
    for k in range(3):
        assert a.distance_map(k + 1).tobytes() == S.exact_cspace(S.convert_map(maps[k]), 0.05, 0.6).tobytes()
    a.close()


# ---------------------------------------------------------------------------------------------------- weights vs goldens


def run_case(nav, golden, name, m):
    c = case(golden, name, m)
    p = params_of(golden, name, nav)
    n = len(c["poses"])
    a = nav.AmclLaser(1, n, 64)
    load_map(a, golden, m)
    a.configure(p)
    a.set_laser_pose(LASER)
    a.set_samples(c["poses"][None], c["w"][None], converged=[c["conv"]])
    a.set_filter_state(c["w0"])
    st, upd = a.update_sensor([c["scan"]], c["range_max"])
    _, _, W, _ = a.get_samples()
    ws = a.get_filter_state()[0]
    skip = a.beam_skip_state(0)
    a.close()
    return c, upd, W[0, :n], ws, skip


def golden_cases():
    g = np.load(GOLDEN)
    return [(str(n), m) for n in g["configs"] for m in range(3)]


@pytest.mark.parametrize("name,m", golden_cases())
def test_weights_match_reference(nav, golden, name, m):
    c, upd, W, ws, skip = run_case(nav, golden, name, m)
    out = c["out"]
    assert upd[0] == int(out[0])
    assert_close(W, out[4:], f"{name} map{m} weights")
    assert_close(ws, out[1:3], f"{name} map{m} w_slow/w_fast")
    oc, mask, err, active = skip
    if name.startswith("prob_skip") and c["conv"]:
        assert active == 1 and err == int(out[3])
        n = len(c["poses"])
        p = params_of(golden, name, nav)
        ref_count = golden[f"{name}_m{m}_obs_count"]  # the reference's per-beam counts (tools/amcl_golden_harness.cpp)
        assert np.array_equal(oc[:p.max_beams], ref_count)
        assert np.array_equal(mask[:p.max_beams], ref_count / n > p.beam_skip_threshold)  # amcl_laser.cpp:545-553
        assert not mask[p.max_beams:].any()
        if not err:
            assert mask.any() and not mask[:p.max_beams].all()  # the skip path skipped some beams and kept others
    else:
        assert active == 0 and err == 0 and not mask.any()


@pytest.mark.parametrize("name", ["beam", "field_factors", "prob_skip", "gompertz"])
def test_batched_filters_match_reference(nav, golden, name):
    """The three maps' cases of one configuration as three filters of one handle (different maps, sample and range counts)."""
    cs = [case(golden, name, m) for m in range(3)]
    ms = max(len(c["poses"]) for c in cs)
    a = nav.AmclLaser(3, ms, 64)
    for m in range(3):
        load_map(a, golden, m, first=m)
    a.configure(params_of(golden, name, nav))
    a.set_laser_pose(np.tile(LASER, (3, 1)))
    for m, c in enumerate(cs):
        a.set_samples(c["poses"][None], c["w"][None], converged=[c["conv"]], first=m)
        a.set_filter_state(c["w0"], first=m)
    st, upd = a.update_sensor([c["scan"] for c in cs], [c["range_max"] for c in cs])
    sc, _, W, _ = a.get_samples()
    ws = a.get_filter_state()
    for m, c in enumerate(cs):
        assert upd[m] == 1
        assert_close(W[m, :sc[m]], c["out"][4:], f"{name} filter {m}")
        assert_close(ws[m], c["out"][1:3], f"{name} filter {m} w")
    a.close()


# ---------------------------------------------------------------------------------------------------- edge cases


def simple_handle(nav, n_filters=1, max_samples=64, capacity=30, **params):
    a = nav.AmclLaser(n_filters, max_samples, capacity)
    data = np.zeros((60, 80), np.int8)
    data[0, :] = data[-1, :] = data[:, 0] = data[:, -1] = 100
    data[20:25, 30:33] = 100
    data[40:44, 50:60] = -1
    a.set_map(data, 0.05, (-2.0, -1.5), max_occ_dist=0.5)
    a.configure(**params)
    return a


def scan_of(rc, rng, rmax=3.0):
    s = np.zeros((rc, 2))
    s[:, 0] = rng.uniform(0.2, rmax, rc)
    s[:, 1] = np.linspace(-1.5, 1.5, rc)
    return s


def poses_of(n, rng):
    p = np.zeros((n, 3))
    p[:, 0] = rng.uniform(-2.2, 2.2, n)
    p[:, 1] = rng.uniform(-1.7, 1.7, n)
    p[:, 2] = rng.uniform(-3, 3, n)
    return p


def test_zero_total_gives_uniform_weights(nav):
    rng = np.random.default_rng(1)
    a = simple_handle(nav, model_type=1)
    a.set_samples(poses_of(50, rng)[None], np.zeros((1, 50)))
    a.set_filter_state([0.3, 0.4])
    st, upd = a.update_sensor([scan_of(100, rng)], 3.0)
    assert st == 0 and upd[0] == 1
    _, _, W, _ = a.get_samples()
    assert np.all(W[0, :50] == 1.0 / 50)
    assert np.array_equal(a.get_filter_state()[0], [0.3, 0.4])  # running averages untouched (pf.c:305-313)


def test_max_beams_below_two_leaves_filter_untouched(nav):
    rng = np.random.default_rng(2)
    a = simple_handle(nav, model_type=1, max_beams=1)
    w = rng.random((1, 40))
    a.set_samples(poses_of(40, rng)[None], w)
    a.set_filter_state([0.1, 0.2])
    st, upd = a.update_sensor([scan_of(100, rng)], 3.0)
    assert st == 0 and upd[0] == 0
    assert np.array_equal(a.get_samples()[2][0, :40], w[0]) and np.array_equal(a.get_filter_state()[0], [0.1, 0.2])


def test_beam_model_with_fewer_ranges_than_beams_is_invalid_not_a_hang(nav):
    rng = np.random.default_rng(3)
    a = simple_handle(nav, n_filters=2, model_type=0, max_beams=30)
    w = rng.random((2, 40))
    a.set_samples(poses_of(40, rng)[None].repeat(2, 0), w)
    st, upd = a.update_sensor([scan_of(29, rng), scan_of(60, rng)], 3.0, raise_on_error=False)
    assert st == -1
    assert upd[0] == -1 and upd[1] == 1
    W = a.get_samples()[2]
    assert np.array_equal(W[0, :40], w[0]) and not np.array_equal(W[1, :40], w[1])


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_range_count_zero(nav, model):
    rng = np.random.default_rng(4)
    a = simple_handle(nav, model_type=model)
    poses = poses_of(30, rng)
    w = rng.uniform(0.5, 1, (1, 30))
    a.set_samples(poses[None], w)
    st, upd = a.update_sensor([np.zeros((0, 2))], 3.0)
    assert st == 0 and upd[0] == 1
    W = a.get_samples()[2][0, :30]
    assert abs(W.sum() - 1.0) < 1e-12  # p = 1 for every particle: weights only renormalised (map factors are 1)
    assert np.allclose(W, w[0] / w[0].sum(), rtol=1e-12, atol=0)


def test_map_factors_without_a_map_is_a_state_error(nav):
    a = nav.AmclLaser(1, 8, 30)
    a.configure(model_type=0, non_free_space_radius=0.3)
    a.set_samples(np.zeros((1, 4, 3)), np.ones((1, 4)))
    st, _ = a.update_sensor([scan_of(40, np.random.default_rng(0))], 3.0, raise_on_error=False)
    assert st == -5


def test_update_before_configure_is_a_state_error(nav):
    a = nav.AmclLaser(1, 8, 30)
    a.set_samples(np.zeros((1, 4, 3)), np.ones((1, 4)))
    st, _ = a.update_sensor([np.zeros((0, 2))], 3.0, raise_on_error=False)
    assert st == -5


# ---------------------------------------------------------------------------------------------------- batch independence


def batch_setup(nav, rng, model, counts, rcs):
    nF = len(counts)
    a = nav.AmclLaser(nF, max(counts), 60)
    maps = np.zeros((nF, 70, 90), np.int8)
    for k in range(nF):
        maps[k][rng.random((70, 90)) < 0.02] = 100
        maps[k][rng.random((70, 90)) < 0.01] = -1
    a.set_map(maps, 0.05, (-2.25, -1.75), max_occ_dist=0.8)
    a.configure(model_type=model, max_beams=60, do_beamskip=1 if model == 2 else 0, off_map_factor=0.5, non_free_space_factor=0.3,
                non_free_space_radius=0.2)
    P = np.zeros((nF, max(counts), 3))
    W = np.zeros((nF, max(counts)))
    for k, n in enumerate(counts):
        P[k, :n] = poses_of(n, rng)
        W[k, :n] = rng.uniform(0.1, 1, n)
    scans = [scan_of(rc, rng, 3.9) for rc in rcs]
    for s in scans:
        s[rng.random(len(s)) < 0.05, 0] = np.nan
    a.set_laser_pose(rng.normal(0, 0.1, (nF, 3)))
    return a, P, W, scans


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_sub_slice_equals_whole_batch_and_is_deterministic(nav, model):
    counts, rcs = [1, 5000, 333, 2048, 64], [1081, 720, 181, 60, 541]
    results = []
    for mode in ("whole", "whole", "slice"):
        rng = np.random.default_rng(11)
        a, P, W, scans = batch_setup(nav, rng, model, counts, rcs)
        a.set_samples(P, W, sample_counts=counts, converged=[1, 1, 0, 1, 1])
        a.set_filter_state(np.tile([0.01, 0.02], (5, 1)))
        if mode == "whole":
            st, upd = a.update_sensor(scans, 4.0)
        else:
            st, upd = a.update_sensor(scans[1:4], 4.0, first=1)
            _, _, Wk, _ = a.get_samples()
            assert np.array_equal(Wk[0], W[0]) and np.array_equal(Wk[4], W[4])  # outside the slice: untouched
            assert np.array_equal(a.get_filter_state()[[0, 4]], [[0.01, 0.02]] * 2)
        assert st == 0 and (upd == 1).all()
        _, _, Wk, _ = a.get_samples()
        results.append((Wk, a.get_filter_state()))
        a.close()
    assert results[0][0].tobytes() == results[1][0].tobytes() and results[0][1].tobytes() == results[1][1].tobytes()
    assert results[0][0][1:4].tobytes() == results[2][0][1:4].tobytes()
    assert results[0][1][1:4].tobytes() == results[2][1][1:4].tobytes()


# ---------------------------------------------------------------------------------------------------- status codes


def test_configure_is_all_or_nothing(nav):
    from navigation_amd._lib import AmclLaserParams
    rng = np.random.default_rng(5)
    P, W, scan = poses_of(100, rng), rng.random((1, 100)), scan_of(181, rng)

    def run(a):
        a.set_samples(P[None], W)
        a.set_filter_state([0.0, 0.0])
        a.update_sensor([scan], 3.0)
        return a.get_samples()[2].copy()

    a = simple_handle(nav, max_samples=100, model_type=3, gompertz_b=2.0)
    before = run(a)
    L = a.L
    import ctypes as C
    for bad in (dict(model_type=4), dict(model_type=-1), dict(do_beamskip=2), dict(max_beams=-3), dict(z_hit=float("nan"))):
        assert L.navgpu_amcl_laser_configure(a.h, C.byref(AmclLaserParams(**bad))) == -1, bad
    assert L.navgpu_amcl_laser_configure(a.h, C.byref(AmclLaserParams(max_beams=31))) == -4  # above the handle's capacity
    assert run(a).tobytes() == before.tobytes()  # the gompertz configuration is still in force


def test_capacities(nav):
    import ctypes as C
    a = nav.AmclLaser(2, 16, 30)
    L = a.L
    sc = np.array([17, 1], np.int32)
    P = np.zeros((2, 16, 3))
    W = np.zeros((2, 16))
    cv = np.zeros(2, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.navgpu_amcl_set_samples(a.h, 0, 2, p(sc), p(P), p(W), p(cv)) == -4
    assert L.navgpu_amcl_set_samples(a.h, 1, 2, p(sc), p(P), p(W), p(cv)) == -1  # slice past the handle
    h = C.c_void_p()
    assert L.navgpu_amcl_create(1, 10, 2000, 0, C.byref(h)) == -4
    big = np.zeros((1, 1), np.int8)
    org = np.zeros(2)
    assert L.navgpu_amcl_set_map(a.h, 0, 1, p(big), 20000, 1, 0.05, p(org), 1, 1, 1.0) == -4
    assert L.navgpu_amcl_set_map(a.h, 0, 1, p(big), 1, 1, 0.05, p(org), 17, 1, 1.0) == -1
    assert L.navgpu_amcl_distance_map(a.h, 0, p(np.zeros(1, np.float32))) == -5  # no map yet
    a.close()


def test_map_cells_equals_converted_map(nav, golden):
    """navgpu_amcl_set_map_cells (a map_t as it stands, as the adapter uploads it) gives the same map, distances and weights as
    navgpu_amcl_set_map on the OccupancyGrid it came from."""
    name, m = "field_factors", 1
    g = golden[f"map{m}_geom"]
    occ = S.convert_map(golden[f"map{m}_data"], int(g[3]))
    c = case(golden, name, m)
    n = len(c["poses"])
    a = nav.AmclLaser(1, n, 64)
    a.set_map_cells(occ, g[9], (g[7], g[8]), max_occ_dist=g[6])
    assert a.distance_map(0).tobytes() == S.exact_cspace(occ, g[9], g[6]).tobytes()
    a.set_distance_map(golden[f"map{m}_dist"])
    a.configure(params_of(golden, name, nav))
    a.set_laser_pose(LASER)
    a.set_samples(c["poses"][None], c["w"][None], converged=[c["conv"]])
    a.set_filter_state(c["w0"])
    a.update_sensor([c["scan"]], c["range_max"])
    assert_close(a.get_samples()[2][0, :n], c["out"][4:], "set_map_cells weights")
    a.close()


def test_filter_and_range_count_bounds(nav):
    import ctypes as C
    h = C.c_void_p()
    L = nav.lib()
    assert L.navgpu_amcl_create(65536, 1, 30, 0, C.byref(h)) == -4  # filters are a launch grid dimension
    a = simple_handle(nav, model_type=1)
    a.set_samples(np.zeros((1, 4, 3)), np.ones((1, 4)))
    rc = np.array([2 ** 31], np.uint32)
    xy = np.zeros(2)
    rmax = np.array([3.0])
    upd = np.zeros(1, np.int32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.navgpu_amcl_update_sensor(a.h, 0, 1, p(xy), p(rc), p(rmax), p(upd)) == -1  # validated before any range is read
    assert np.array_equal(a.get_samples()[2][0, :4], np.ones(4))
    a.close()
