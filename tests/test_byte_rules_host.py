"""CPU half of the byte-table tests: the restatements in tests/byte_rules_ref.py against the oracle (oracle/costmap_oracle.hpp,
oracle/navfn_oracle.hpp), each over its whole domain - every occupancy byte under every static-layer setting, every pair of
bytes under every merge rule, every cost byte in every cell class of NavFn::setCostmap.  Two independent readings of the same
reference text have to agree before either is used to judge the device (tests/test_gpu_byte_rules.py).  No GPU here."""
import numpy as np
import pytest

import byte_rules_ref as R

NOINFO = R.NO_INFORMATION


# ----------------------------------------------------------------------------------------------
# A. StaticLayer::interpretValue (static_layer.cpp:149-163) with onInitialize's clamp and wrap (:80-81)
# ----------------------------------------------------------------------------------------------
def test_interpret_value_anchors():
    """a few values worked out by hand from the reference text, so that the restatement is not only checked against a
    second restatement"""
    assert R.static_params(-7, -1) == (0, 255) and R.static_params(1000, 256) == (100, 0) and R.static_params(65, 511) == (65, 255)
    iv = R.interpret_value
    assert iv(50, True, False, 100, 255) == 127           # 0.5 * 254
    assert iv(64, True, False, 65, 40) == 250             # 64 / 65 * 254 = 250.09...
    assert iv(99, True, False, 100, 255) == 251           # 251.46
    assert iv(1, True, False, 100, 255) == 2              # 2.54
    assert iv(40, True, False, 65, 40) == NOINFO and iv(40, False, False, 65, 40) == 0
    assert iv(0x80, True, True, 100, 255) == 254          # occupancy -128 reads as 128 >= 100
    assert iv(0xFF, True, True, 100, 255) == NOINFO and iv(0xFF, True, True, 100, 0) == 254
    assert iv(0, True, False, 0, 255) == 254              # threshold 0: every known cell is lethal
    assert iv(100, True, True, 100, 100) == NOINFO        # unknown is tested before lethal


@pytest.mark.parametrize("rolling", [False, True])
def test_interpret_value_whole_domain_equals_oracle(orc, rolling):
    occ = R.all_int8(16, 16)
    assert len(np.unique(occ)) == 256
    o = orc.LayeredCostmap(False)
    if rolling:
        o.resize(16, 16, 1.0, 0.0, 0.0)
        o.set_rolling(True)
    table = R.static_parameter_table()
    assert len(table) == 2 * 2 * 107 * 11
    bad = []
    n_grey = 0
    for tu, tri, thr, unk in table:
        kw = dict(track_unknown_space=tu, use_maximum=False, trinary=tri, lethal_threshold=thr, unknown_cost_value=unk)
        if rolling:
            o.add_static_rolling(occ, 1.0, 0.0, 0.0, **kw)
        else:
            o.add_static(occ, res=1.0, **kw)
        got = o.layer(1)
        exp = R.interpret(occ, tu, tri, thr, unk)
        n_grey += int(((exp > 0) & (exp < 253)).sum())
        if not np.array_equal(got, exp):
            k = int(np.flatnonzero(got.reshape(-1) != exp.reshape(-1))[0])
            bad.append(((tu, tri, thr, unk), k, int(got.reshape(-1)[k]), int(exp.reshape(-1)[k])))
    assert not bad, f"{len(bad)} settings differ; (params, occupancy byte, oracle, restatement): {bad[:5]}"
    assert n_grey > 50000  # the scaled branch is in the table


# ----------------------------------------------------------------------------------------------
# B. the merge rules over all 65 536 (master | static, layer) pairs
# ----------------------------------------------------------------------------------------------
GEOMETRIES = R.GEOMETRIES


@pytest.mark.parametrize("ny,nx", GEOMETRIES)
def test_costmap_layer_rules_equal_oracle(orc, ny, nx):
    """updateWithOverwrite / updateWithMax / updateWithTrueOverwrite (costmap_layer.cpp:62-124): master byte a, layer byte b"""
    a, b = R.pair_tables(ny, nx)
    assert len(np.unique(a.astype(np.uint32) * 256 + b)) == 65536
    rules = [R.update_with_overwrite, R.update_with_max, R.update_with_true_overwrite]
    for mode, rule in enumerate(rules):
        for box in (None, (37, 21, 201, 98), (0, 100, 18, ny)):
            assert np.array_equal(orc.merge(b, a, mode, box), rule(a, b, box)), (mode, box)
    # the three rules are three rules: each pair of them differs somewhere
    outs = [rule(a, b) for rule in rules]
    assert all((outs[i] != outs[j]).any() for i in range(3) for j in range(i))


def _oracle_costmap(orc, ny, nx, track_unknown, use_maximum, combination_method, static, obstacle, master, res=1.0):
    o = orc.LayeredCostmap(track_unknown)
    o.add_static(np.zeros((ny, nx), np.int8), res=res, use_maximum=use_maximum)  # the layer counts as received, new data
    o.set_layer(static, 1)
    o.add_obstacle(combination_method=combination_method, footprint_clearing=False)
    o.set_layer(obstacle, 2)
    o.set_master(master)
    return o


@pytest.mark.parametrize("ny,nx", GEOMETRIES)
@pytest.mark.parametrize("track_unknown", [False, True])
def test_update_map_pair_tables_equal_oracle(orc, ny, nx, track_unknown):
    """reset -> static rule -> obstacle rule over the whole map, static byte a, obstacle byte b; then one update of a
    strict sub-box with other layers, outside of which the master keeps its bytes"""
    a, b = R.pair_tables(ny, nx)
    sentinel = np.full((ny, nx), 0x5A, np.uint8)
    for use_maximum in (False, True):
        for comb in (0, 1):
            o = _oracle_costmap(orc, ny, nx, track_unknown, use_maximum, comb, a, b, sentinel)
            o.update_map(0.0, 0.0, 0.0)
            assert list(o.bounds()) == [0, nx, 0, ny]
            first = R.update_map(sentinel, track_unknown, a, use_maximum, b, comb)
            assert np.array_equal(o.master(), first), (use_maximum, comb)
            # second cycle: other layers (static b, obstacle ~a), only CostmapLayer::resetBoundingBox's box is in the bounds
            o.set_layer(b, 1)
            o.reset_bounding_box(37.5, 21.5, 200.5, 97.5)
            o.set_layer(~a, 2)  # (resetBoundingBox has reset the layer inside the box)
            o.update_map(0.0, 0.0, 0.0)
            assert list(o.bounds()) == [37, 201, 21, 98]
            want = R.update_map(first, track_unknown, b, use_maximum, ~a, comb, box=(37, 21, 201, 98))
            assert np.array_equal(o.master(), want), ("sub-box", use_maximum, comb)
            outside = np.ones((ny, nx), bool)
            outside[21:98, 37:201] = False
            assert np.array_equal(want[outside], first[outside]) and (want[~outside] != first[~outside]).any()


ROLLING_STATIC = dict(track_unknown_space=True, trinary=False, lethal_threshold=100, unknown_cost_value=-1)


@pytest.mark.parametrize("track_unknown", [False, True])
def test_rolling_static_branch_equals_oracle(orc, track_unknown):
    """static_layer.cpp:329-332 for a static map in the master's own geometry under the identity transform: a plain copy or
    a plain std::max of the static byte and the master's default, then the obstacle rule"""
    n, res = 256, 0.5
    occ = R.rolling_occupancy(n)
    static = R.interpret(occ, True, False, 100, -1)
    assert len(np.unique(static)) >= 100 and NOINFO in static and 254 in static
    layer = np.broadcast_to(np.arange(n, dtype=np.uint8)[:, None], (n, n)).copy()  # row y holds obstacle byte y
    centre = (n - 1 + 0.5) * res / 2  # getSizeInMetersX / 2: updateOrigin leaves the origin at (0, 0)
    for use_maximum in (False, True):
        for comb in (0, 1):
            o = orc.LayeredCostmap(track_unknown)
            o.resize(n, n, res, 0.0, 0.0)
            o.set_rolling(True)
            o.add_static_rolling(occ, res, 0.0, 0.0, use_maximum=use_maximum, **ROLLING_STATIC)
            o.add_obstacle(combination_method=comb, footprint_clearing=False)
            o.set_layer(layer, 2)
            o.update_map(centre, centre, 0.0)
            assert list(o.origin()) == [0.0, 0.0] and list(o.bounds()) == [0, n, 0, n]
            assert np.array_equal(o.layer(2), layer)
            want = R.update_map(np.zeros((n, n), np.uint8), track_unknown, static, use_maximum, layer, comb, rolling_static=True)
            assert np.array_equal(o.master(), want), (use_maximum, comb)
    # the plain max is another rule than updateWithMax: they part exactly where either side is NO_INFORMATION
    m = R.reset_map(np.zeros((n, n), np.uint8), track_unknown)
    plain, with_max = R.static_update_costs(m, static, True, rolling=True), R.update_with_max(m, static)
    differ = plain != with_max
    assert np.array_equal(differ, (m == NOINFO) ^ (static == NOINFO)) and differ.any()


# ----------------------------------------------------------------------------------------------
# D. NavFn::setCostmap (navfn.cpp:227-287)
# ----------------------------------------------------------------------------------------------
NAVFN_SIZES = R.NAVFN_SIZES


def test_navfn_costarr_anchors():
    one = lambda v, mode, au: int(R.navfn_costarr(np.full((15, 15), v, np.uint8), mode, au)[7, 7])  # noqa: E731
    assert one(0, 1, 1) == 50 and one(1, 1, 1) == 50 and one(2, 1, 1) == 51      # 50.8 truncates
    assert one(252, 1, 1) == 251 and one(253, 1, 1) == 254 and one(254, 1, 1) == 254
    assert one(255, 1, 1) == 253 and one(255, 1, 0) == 254 and one(255, 2, 0) == 253
    frame = R.navfn_costarr(np.zeros((15, 15), np.uint8), 2, 1)
    assert (frame == 254).sum() == 15 * 15 - 1 and frame[7, 7] == 50
    assert (R.navfn_costarr(np.zeros((30, 14), np.uint8), 2, 1) == 254).all()
    # COST_NEUTRAL + COST_FACTOR * v stays below COST_OBS for every v < COST_OBS_ROS: the clamp at :247-248 never acts
    assert max(int(50 + 0.8 * v) for v in range(253)) == 251


@pytest.mark.parametrize("nx,ny,maps,step", NAVFN_SIZES)
def test_navfn_costarr_equals_oracle(orc, nx, ny, maps, step):
    cmaps = R.navfn_byte_maps(ny, nx, maps, step)
    if min(nx, ny) >= 15:
        assert len(np.unique(cmaps[:, 7:ny - 7, 7:nx - 7])) == 256  # every byte inside cost_mode 2's frame
    for mode in (0, 1, 2):
        for au in (0, 1):
            for p in range(maps):
                assert np.array_equal(orc.navfn_costarr(cmaps[p], mode, au), R.navfn_costarr(cmaps[p], mode, au)), (mode, au, p)


@pytest.mark.parametrize("mode,au", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_navfn_potentials_over_restated_costarr(orc, mode, au):
    """the oracle's whole expansion (no early stop) on a translated map == the same on the restated costarr taken as it is:
    a wrong byte anywhere the wavefront reaches shows in the potentials"""
    nx, ny = 40, 33
    rs = np.random.RandomState(40 + mode)
    cmap = R.navfn_byte_maps(ny, nx, 1)[0]
    cmap[rs.random_sample(cmap.shape) < 0.5] = 0  # half the cells free, so the wavefront gets everywhere
    cmap[16, 20] = cmap[10, 9] = 0
    goal, start = (20, 16), (9, 10)
    _, pot_a, _ = orc.navfn_plan(cmap, goal, start, cost_mode=mode, allow_unknown=bool(au), at_start=False)
    _, pot_b, _ = orc.navfn_plan(R.navfn_costarr(cmap, mode, au), goal, start, cost_mode=0, at_start=False)
    assert np.array_equal(pot_a, pot_b)
    assert (pot_a < 1e9).sum() > (200 if mode == 2 else 600)
