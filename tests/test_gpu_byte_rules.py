"""The byte-translation kernels over their whole domains (need a real MI355X): k_static_interpret under every static-layer
setting, k_merge's rules over all 65 536 byte pairs, a grey (scaled) static map through whole update cycles with inflation,
and k_navfn_costmap in every cost mode, read back through navgpu_navfn_costarr.  The expected bytes come from
tests/byte_rules_ref.py, plain restatements of the reference text that tests/test_byte_rules_host.py pins against the oracle
on the CPU; part C compares with the oracle itself.  Everything is bytes: every comparison is np.array_equal."""
import numpy as np
import pytest

import byte_rules_ref as R
from test_gpu_parity import L, nav  # noqa: F401

pytestmark = pytest.mark.gpu

NOINFO = R.NO_INFORMATION
SUB_BOXES = [(37, 21, 201, 98), (0, 100, 18, 263)]                                 # min_i, min_j, max_i, max_j per robot
SUB_BOXES_WORLD = [(37.5, 21.5, 200.5, 97.5), (0.5, 100.5, 17.5, 262.5)]           # the same at 1 m / cell (max is inclusive)


# ----------------------------------------------------------------------------------------------
# A. k_static_interpret: StaticLayer::interpretValue (static_layer.cpp:149-163) under onInitialize's clamp and wrap (:80-81)
# ----------------------------------------------------------------------------------------------
def _report(bad):
    return f"{len(bad)} settings differ; ((track_unknown_space, trinary, lethal, unknown), occupancy byte, got, expected): {bad[:5]}"


@pytest.mark.parametrize("ny,nx", [(16, 16), (17, 16)])  # 256 cells: one full block; 272: the tail of a second block
def test_static_interpret_whole_domain(nav, ny, nx):
    """All 4708 settings (107 thresholds x 11 unknown values x trinary x track_unknown_space) on the 256 int8 bit patterns,
    broadcast to robots 1 and 2 of 3; robot 0's static grid keeps what it held."""
    N = L(nav)
    occ = R.all_int8(ny, nx)
    fl = nav.Fleet(3, nx, ny, 0.05, layers=N.LAYER_STATIC | N.LAYER_OBSTACLE, max_points=16, max_observations=1)
    sentinel = np.full((3, ny, nx), 0xA5, np.uint8)
    fl.upload(N.GRID_STATIC, sentinel)
    bad = []
    for tu, tri, thr, unk in R.static_parameter_table():
        fl.add_static_map(occ, first=1, count=2, track_unknown_space=tu, trinary_costmap=tri, lethal_cost_threshold=thr, unknown_cost_value=unk)
        got = fl.download(N.GRID_STATIC)
        exp = R.interpret(occ, tu, tri, thr, unk)
        assert np.array_equal(got[0], sentinel[0]), "the broadcast left its range"
        for k in (1, 2):
            if not np.array_equal(got[k], exp):
                c = int(np.flatnonzero(got[k].reshape(-1) != exp.reshape(-1))[0])
                bad.append(((tu, tri, thr, unk), c & 0xFF, int(got[k].reshape(-1)[c]), int(exp.reshape(-1)[c])))
    fl.close()
    assert not bad, _report(bad)


def test_static_interpret_whole_domain_rolling(nav):
    """The same 4708 settings through navgpu_static_set_rolling_map, read through one update each: static map and master
    share one geometry, identity transform, plain copy (use_maximum off), obstacle layer disabled."""
    N = L(nav)
    n, res = 16, 0.5
    occ = R.all_int8(n, n)
    fl = nav.Fleet(1, n, n, res, layers=N.LAYER_STATIC | N.LAYER_OBSTACLE, max_points=16, max_observations=1, rolling_window=True)
    fl.configure_obstacle(enabled=False, footprint_clearing_enabled=False)
    centre = (n - 1 + 0.5) * res / 2  # Costmap2D::getSizeInMetersX / 2: the window's origin stays at (0, 0)
    bad = []
    for tu, tri, thr, unk in R.static_parameter_table():
        fl.set_rolling_static_map(occ, res, 0.0, 0.0, track_unknown_space=tu, use_maximum=False, trinary_costmap=tri,
                                  lethal_cost_threshold=thr, unknown_cost_value=unk)
        fl.stage_observations([[centre, centre, 0.0]], [])
        fl.update_map()
        got = fl.master()[0]
        exp = R.interpret(occ, tu, tri, thr, unk)
        if not np.array_equal(got, exp):
            c = int(np.flatnonzero(got.reshape(-1) != exp.reshape(-1))[0])
            bad.append(((tu, tri, thr, unk), c & 0xFF, int(got.reshape(-1)[c]), int(exp.reshape(-1)[c])))
    assert list(fl.origins()[0]) == [0.0, 0.0] and list(fl.bounds()[0]) == [0, n, 0, n]
    fl.close()
    assert not bad, _report(bad)


# ----------------------------------------------------------------------------------------------
# B. k_merge: Costmap2D::resetMap, StaticLayer::updateCosts, ObstacleLayer::updateCosts over every pair of bytes
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny,nx", R.GEOMETRIES)
@pytest.mark.parametrize("track_unknown", [False, True])
def test_merge_pair_tables(nav, ny, nx, track_unknown):
    """reset -> static rule -> obstacle rule with robot 0 pairing static byte a with obstacle byte b and robot 1 the other
    way round, for use_maximum x combination_method; then one update whose bounds are a strict sub-box (the box of
    CostmapLayer::resetBoundingBox alone): inside it the rule on new layers, outside it the bytes of the first update."""
    N = L(nav)
    a, b = R.pair_tables(ny, nx)
    statics, layers = np.stack([a, b]), np.stack([b, a])
    sentinel = np.full((2, ny, nx), 0x5A, np.uint8)
    fl = nav.Fleet(2, nx, ny, 1.0, layers=N.LAYER_STATIC | N.LAYER_OBSTACLE, track_unknown=track_unknown, max_points=16, max_observations=1)
    poses = [[0.0, 0.0, 0.0]] * 2
    boxes = [tuple(min(v, lim) for v, lim in zip(bx, (nx, ny, nx, ny))) for bx in SUB_BOXES]
    for use_maximum in (False, True):
        for comb in (0, 1):
            fl.configure_obstacle(footprint_clearing_enabled=False, combination_method=comb)
            fl.add_static_map(np.zeros((ny, nx), np.int8), use_maximum=use_maximum)  # the layer counts as received, with new data
            fl.upload(N.GRID_STATIC, statics)
            fl.upload(N.GRID_OBSTACLE, layers)
            fl.upload(N.GRID_MASTER, sentinel)
            fl.stage_observations(poses, [])
            fl.update_map()
            got, bounds = fl.master(), fl.bounds()
            first = [R.update_map(sentinel[k], track_unknown, statics[k], use_maximum, layers[k], comb) for k in range(2)]
            for k in range(2):
                assert list(bounds[k]) == [0, nx, 0, ny]
                assert np.array_equal(got[k], first[k]), (use_maximum, comb, k, int((got[k] != first[k]).sum()))
            assert np.array_equal(fl.download(N.GRID_STATIC), statics) and np.array_equal(fl.download(N.GRID_OBSTACLE), layers)
            # second cycle: other layers (static and obstacle swapped, the obstacle bytes inverted); no new static data
            fl.upload(N.GRID_STATIC, layers)
            fl.reset_bounding_box(np.array(SUB_BOXES_WORLD))
            fl.upload(N.GRID_OBSTACLE, ~statics)  # (resetBoundingBox has reset the layer inside the box)
            fl.stage_observations(poses, [])
            fl.update_map()
            got, bounds = fl.master(), fl.bounds()
            for k in range(2):
                x0, y0, xn, yn = boxes[k]
                assert list(bounds[k]) == [x0, xn, y0, yn] and (xn - x0) * (yn - y0) < nx * ny
                want = R.update_map(first[k], track_unknown, layers[k], use_maximum, ~statics[k], comb, box=boxes[k])
                outside = np.ones((ny, nx), bool)
                outside[y0:yn, x0:xn] = False
                assert np.array_equal(got[k][outside], first[k][outside]), ("outside the box", use_maximum, comb, k)
                assert np.array_equal(got[k], want), ("sub-box", use_maximum, comb, k, int((got[k] != want).sum()))
                assert (want[~outside] != first[k][~outside]).any()
    fl.close()


def test_static_use_maximum_is_one_setting_of_the_fleet(nav):
    """navgpu_static_set_map stores use_maximum for the fleet, the map bytes per robot (include/navgpu.h): after two
    sub-range calls that differ in it, the later call's value holds for both robots.  (Master default 0 and an obstacle
    layer without information: the two static rules part on the static NO_INFORMATION cells.)"""
    N = L(nav)
    ny, nx = 256, 256
    a, _ = R.pair_tables(ny, nx)
    occ = np.zeros((ny, nx), np.int8)
    nothing = np.full((ny, nx), NOINFO, np.uint8)
    for later in (False, True):
        fl = nav.Fleet(2, nx, ny, 1.0, layers=N.LAYER_STATIC | N.LAYER_OBSTACLE, track_unknown=False, max_points=16, max_observations=1)
        fl.configure_obstacle(footprint_clearing_enabled=False, combination_method=1)
        fl.add_static_map(occ, first=0, count=1, use_maximum=not later)
        fl.add_static_map(occ, first=1, count=1, use_maximum=later)
        fl.upload(N.GRID_STATIC, np.stack([a, a]))
        fl.upload(N.GRID_OBSTACLE, np.stack([nothing, nothing]))
        fl.stage_observations([[0.0, 0.0, 0.0]] * 2, [])
        fl.update_map()
        want = R.update_map(np.zeros((ny, nx), np.uint8), False, a, later, nothing, 1)
        other = R.update_map(np.zeros((ny, nx), np.uint8), False, a, not later, nothing, 1)
        got = fl.master()
        assert (want != other).sum() == ny
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want), later
        fl.close()


@pytest.mark.parametrize("ny,nx", R.GEOMETRIES)
@pytest.mark.parametrize("combination_method", [0, 1])
def test_merge_layer_only_pair_tables(nav, ny, nx, combination_method):
    """navgpu_obstacle_update_costs (ObstacleLayer::updateCosts alone, no reset, no static merge): preset master byte a,
    layer byte b over the whole map (robot 0) and the other way round over a sub-box (robot 1)."""
    N = L(nav)
    a, b = R.pair_tables(ny, nx)
    masters, layers = np.stack([a, b]), np.stack([b, a])
    boxes = [(0, 0, nx, ny), tuple(min(v, lim) for v, lim in zip(SUB_BOXES[0], (nx, ny, nx, ny)))]
    fl = nav.Fleet(2, nx, ny, 1.0, layers=N.LAYER_OBSTACLE, track_unknown=True, max_points=16, max_observations=1)
    fl.configure_obstacle(footprint_clearing_enabled=False, combination_method=combination_method)
    fl.upload(N.GRID_MASTER, masters)
    fl.upload(N.GRID_OBSTACLE, layers)
    fl.obstacle_update_costs(boxes)
    got = fl.master()
    for k in range(2):
        want = R.obstacle_update_costs(masters[k], layers[k], combination_method, boxes[k])
        assert np.array_equal(got[k], want), (k, int((got[k] != want).sum()))
    fl.close()


@pytest.mark.parametrize("track_unknown", [False, True])
def test_merge_rolling_static_pair_tables(nav, track_unknown):
    """The rolling branch (static_layer.cpp:329-332): a plain copy or a plain std::max of the static byte (column x: the
    scaled reading of int8 pattern x - 100 greys, 254, 255) and the master's default, then the obstacle rule with layer byte y."""
    N = L(nav)
    n, res = 256, 0.5
    occ = R.rolling_occupancy(n)
    static = R.interpret(occ, True, False, 100, -1)
    layer = np.broadcast_to(np.arange(n, dtype=np.uint8)[:, None], (n, n)).copy()
    centre = (n - 1 + 0.5) * res / 2
    fl = nav.Fleet(2, n, n, res, layers=N.LAYER_STATIC | N.LAYER_OBSTACLE, track_unknown=track_unknown, max_points=16, max_observations=1,
                   rolling_window=True)
    for use_maximum in (False, True):
        for comb in (0, 1):
            fl.configure_obstacle(footprint_clearing_enabled=False, combination_method=comb)
            fl.set_rolling_static_map(occ, res, 0.0, 0.0, track_unknown_space=True, use_maximum=use_maximum, trinary_costmap=False,
                                      lethal_cost_threshold=100, unknown_cost_value=-1)
            fl.upload(N.GRID_OBSTACLE, np.stack([layer, layer]))
            fl.upload(N.GRID_MASTER, np.full((2, n, n), 0x5A, np.uint8))
            fl.stage_observations([[centre, centre, 0.0]] * 2, [])
            fl.update_map()
            got, bounds, origins, ol = fl.master(), fl.bounds(), fl.origins(), fl.download(N.GRID_OBSTACLE)
            want = R.update_map(np.zeros((n, n), np.uint8), track_unknown, static, use_maximum, layer, comb, rolling_static=True)
            for k in range(2):
                assert list(origins[k]) == [0.0, 0.0] and list(bounds[k]) == [0, n, 0, n]
                assert np.array_equal(ol[k], layer)
                assert np.array_equal(got[k], want), (use_maximum, comb, k, int((got[k] != want).sum()))
    fl.close()


# ----------------------------------------------------------------------------------------------
# C. a grey static map through whole cycles: the inflation kernels merge into a master holding 1..252
# ----------------------------------------------------------------------------------------------
GREY = dict(trinary=False, lethal_threshold=65, unknown_cost_value=40)


def _grey_occupancy(n, seed):
    rs = np.random.RandomState(seed)
    occ = rs.randint(0, 65, (n, n)).astype(np.int8)   # below the threshold: scaled greys (40 is the unknown value)
    occ[20, 8:60] = 100                               # a few walls
    occ[30:80, 70] = 100
    occ[66:69, 10:40] = 100
    wild = rs.choice(n * n, 256, replace=False)       # the whole int8 range, every bit pattern once (3 in 4 of them lethal)
    occ.reshape(-1)[wild] = np.arange(256, dtype=np.uint8).view(np.int8)
    return occ


@pytest.mark.parametrize("track_unknown,use_maximum,pq", [(False, False, False), (False, True, False), (True, False, False), (True, True, False),
                                                          (True, False, True)])
def test_grey_static_map_cycles(nav, orc, track_unknown, use_maximum, pq):
    """Bounds, obstacle layer and master against the oracle over three LaserScan cycles: byte for byte against the exact
    Euclidean transform in the default inflation mode, against the reference's own priority-queue walk with
    priority_queue_order - the contracts of test_costmap_cycles_overwrite and test_layered_cycles_reference_priority_queue_order."""
    from navigation_amd import synth
    N = L(nav)
    n, nI = 97, 2
    insc = synth.inscribed_radius(synth.FOOTPRINT)
    fl = nav.Fleet(nI, n, n, synth.RES, layers=N.LAYER_STATIC | N.LAYER_OBSTACLE | N.LAYER_INFLATION, max_points=720, max_observations=1,
                   track_unknown=track_unknown)
    fl.configure_obstacle()
    fl.set_footprint(synth.FOOTPRINT)
    fl.configure_inflation(synth.INFLATION_RADIUS, synth.COST_SCALING, insc, priority_queue_order=pq)
    insts, oracles, statics = [], [], []
    for i in range(nI):
        occ = _grey_occupancy(n, 300 + i)
        assert len(np.unique(occ)) == 256
        stat = R.interpret(occ, track_unknown, False, 65, 40)
        ins = synth.make_instance(n, 300 + i)
        ins["cells"] = np.where(stat == 254, 254, 0).astype(np.uint8)  # what the scan hits
        fl.add_static_map(occ, first=i, count=1, track_unknown_space=track_unknown, use_maximum=use_maximum, trinary_costmap=False,
                          lethal_cost_threshold=65, unknown_cost_value=40)
        o = orc.LayeredCostmap(track_unknown)
        o.set_footprint(synth.FOOTPRINT)
        o.add_static(occ, res=synth.RES, track_unknown_space=track_unknown, use_maximum=use_maximum, **GREY)
        o.add_obstacle()
        o.add_inflation(synth.INFLATION_RADIUS, synth.COST_SCALING, exact=not pq)
        o.set_footprint(synth.FOOTPRINT)
        insts.append(ins)
        oracles.append(o)
        statics.append(stat)
    assert np.array_equal(fl.download(N.GRID_STATIC), np.stack(statics))
    n_raised = n_kept = 0
    for cyc in range(3):
        obs, poses = [], []
        for i, ins in enumerate(insts):
            pts = synth.laser_scan(ins, cyc)
            org = (float(ins["pos"][0]), float(ins["pos"][1]), 0.3)
            obs.append(dict(instance=i, points=pts, origin=org, obstacle_range=2.5, raytrace_range=3.0))
            poses.append([float(v) for v in ins["pos"]])
            oracles[i].clear_observations()
            oracles[i].add_observation(pts, origin=org, obstacle_range=2.5, raytrace_range=3.0)
            oracles[i].update_map(*poses[-1])
        fl.stage_observations(poses, obs)
        fl.update_map()
        m, ol, b = fl.master(), fl.download(N.GRID_OBSTACLE), fl.bounds()
        for i in range(nI):
            assert np.array_equal(b[i], oracles[i].bounds()), (cyc, i)
            assert np.array_equal(ol[i], oracles[i].layer(2)), (cyc, i)
            assert np.array_equal(m[i], oracles[i].master()), (cyc, i, int((m[i] != oracles[i].master()).sum()))
            if cyc == 0:  # the first update covers the whole map: what the master held before inflation is the two merges
                pre = R.update_map(m[i], track_unknown, statics[i], use_maximum, ol[i], 1)
                grey = ~np.isin(pre, (0, 253, 254, 255))
                assert grey.sum() > n * n // 2, "the map has degenerated to a trinary one"
                n_raised += int((grey & (m[i] > pre)).sum())
                n_kept += int((grey & (m[i] == pre)).sum())
    assert n_raised > 100 and n_kept > 100  # max(old, cost) went both ways over grey cells
    fl.close()


# ----------------------------------------------------------------------------------------------
# D. k_navfn_costmap: NavFn::setCostmap (navfn.cpp:227-287), read back with navgpu_navfn_costarr
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,maps,step", R.NAVFN_SIZES)
def test_navfn_costarr_whole_domain(nav, nx, ny, maps, step):
    """Every cost mode x allow_unknown: per-plan maps into plans 1.. (plan 0 keeps what it held), then one map shared by
    all plans.  The maps bring every byte into the cells cost_mode 2's frame leaves (one cell at 15 x 15, none at 14 x 30)."""
    cmaps = R.navfn_byte_maps(ny, nx, maps, step)
    nf = nav.NavFn(nx, ny, n_plans=maps + 1)
    poison = np.full((ny, nx), 0x77, np.uint8)
    for mode in (0, 1, 2):
        for au in (0, 1):
            nf.set_costmap(poison, cost_mode=0)
            nf.set_costmap(cmaps, first=1, count=maps, cost_mode=mode, allow_unknown=au)
            assert np.array_equal(nf.costarr(0), poison)
            for p in range(maps):
                got, want = nf.costarr(1 + p), R.navfn_costarr(cmaps[p], mode, au)
                assert np.array_equal(got, want), (mode, au, p, int((got != want).sum()))
            nf.set_costmap(cmaps[maps - 1], cost_mode=mode, allow_unknown=au)
            want = R.navfn_costarr(cmaps[maps - 1], mode, au)
            for p in (0, maps // 2, maps):
                assert np.array_equal(nf.costarr(p), want), ("shared", mode, au, p)
    nf.close()


@pytest.mark.parametrize("allow_unknown", [0, 1])
def test_navfn_costarr_from_fleet(nav, allow_unknown):
    """navgpu_navfn_set_costmap_from_fleet: the strided read of the fleet's master grids (robots 1, 2 -> plans 1, 2)"""
    N = L(nav)
    nx, ny = 40, 33
    cmaps = R.navfn_byte_maps(ny, nx, 3)
    assert all(len(np.unique(c)) == 256 for c in cmaps)
    fl = nav.Fleet(3, nx, ny, 0.05, layers=N.LAYER_OBSTACLE, max_points=16, max_observations=1)
    fl.upload(N.GRID_MASTER, cmaps)
    nf = nav.NavFn(nx, ny, n_plans=3)
    poison = np.full((ny, nx), 0x77, np.uint8)
    nf.set_costmap(poison, cost_mode=0)
    nf.set_costmap_from_fleet(fl, first=1, count=2, fleet_first=1, allow_unknown=allow_unknown)
    assert np.array_equal(nf.costarr(0), poison)
    for p in (1, 2):
        assert np.array_equal(nf.costarr(p), R.navfn_costarr(cmaps[p], 1, allow_unknown)), p
    nf.close()
    fl.close()
