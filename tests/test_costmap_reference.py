"""CPU checks of the costmap yardstick: tests/golden/g17_costmap_reference.npz is what the reference's own LayeredCostmap, StaticLayer,
ObstacleLayer, VoxelLayer / VoxelGrid and InflationLayer compute (compiled in place by tools/make_costmap_goldens.py), the fixture covers
the rules the costmap kernels implement, and oracle/costmap_oracle.hpp - what every other GPU costmap test compares with - reproduces it
bit for bit.  No tolerance anywhere: bytes, integers, 32-bit words, and doubles out of the same -ffp-contract=off operations."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import costmap_reference_cases as K  # noqa: E402
import make_costmap_goldens as M  # noqa: E402

needs_reference = pytest.mark.skipif(not M.available(), reason="the reference costmap_2d / voxel_grid trees are not on this machine")


@pytest.fixture(scope="module")
def golden():
    g, meta = K.load()
    return g, meta, {n: K.case(g, meta, n) for n in meta["cases"]}


@needs_reference
def test_goldens_reproduce_from_the_reference(tmp_path):
    out = tmp_path / "g17.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_costmap_goldens.py"), "--out", str(out)], check=True, capture_output=True)
    new, old = np.load(out), np.load(K.GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        a, b = old[k], new[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype.kind == "f":
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), k
        else:
            assert np.array_equal(a, b), k


def test_golden_size():
    golden_dir = os.path.join(ROOT, "tests", "golden")
    assert os.path.getsize(K.GOLDEN) <= max(os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir) if not f.startswith("g17_"))


def test_cases_are_what_the_generator_builds(golden):
    g, meta, cases = golden
    built = K.build_cases()
    assert [c["name"] for c in built] == meta["cases"]
    for c in built:
        assert np.array_equal(K.encode_input(c).view(np.uint64), g[c["name"] + "_in"].view(np.uint64)), c["name"]
        again = K.encode_input(dict(K.decode_input(g[c["name"] + "_in"]), name=c["name"]))
        assert np.array_equal(again.view(np.uint64), g[c["name"] + "_in"].view(np.uint64)), c["name"]


# ------------------------------------------------------------------------------------------------ coverage, from the inputs
def _origin_before(c, recs, k):
    """the layer's origin while cycle k's observations are applied (a rolling window has moved by then)"""
    return recs[k]["origin"]


def _rays(c, recs):
    """every clearing ray of a case: (cycle, observation, sensor xyz, endpoint xyz, window origin, raytrace_range)"""
    for k, cyc in enumerate(c["cycles"]):
        for ob in cyc["obs"]:
            if ob["clearing"]:
                yield k, ob, np.asarray(ob["origin"]), ob["points"].astype(np.float64), _origin_before(c, recs, k)


def _in_map(c, org, xy):
    ex, ey = org[0] + c["size_x"] * c["res"], org[1] + c["size_y"] * c["res"]
    return (xy[..., 0] >= org[0]) & (xy[..., 1] >= org[1]) & (xy[..., 0] < ex) & (xy[..., 1] < ey)


def test_obstacle_marking_coverage(golden):
    _, _, cases = golden
    at_range = beyond = too_high = 0
    sides = set()
    kinds, two_in_a_cycle = set(), False
    for name, (c, recs) in cases.items():
        if c["obstacle"] is None:
            continue
        for k, cyc in enumerate(c["cycles"]):
            two_in_a_cycle |= len(cyc["obs"]) >= 2
            for ob in cyc["obs"]:
                kinds.add((ob["marking"], ob["clearing"]))
                if not ob["marking"]:
                    continue
                p = ob["points"].astype(np.float64)
                d2 = ((p - np.asarray(ob["origin"])) ** 2).sum(1)
                at_range += int((d2 == ob["obstacle_range"] ** 2).sum())
                beyond += int((d2 > ob["obstacle_range"] ** 2).sum())
                too_high += int((p[:, 2] > c["obstacle"]["max_obstacle_height"]).sum())
                org = _origin_before(c, recs, k)
                close = d2 < ob["obstacle_range"] ** 2
                ex, ey = org[0] + c["size_x"] * c["res"], org[1] + c["size_y"] * c["res"]
                for side, off in (("left", p[:, 0] < org[0]), ("right", p[:, 0] >= ex), ("bottom", p[:, 1] < org[1]), ("top", p[:, 1] >= ey)):
                    if (off & close).any():
                        sides.add(side)
    assert at_range >= 2 and beyond and too_high
    assert sides == {"left", "right", "bottom", "top"}
    assert kinds == {(True, True), (True, False), (False, True)} and two_in_a_cycle
    obstacle = [c for c, _ in cases.values() if c["obstacle"] is not None]
    assert {c["track_unknown"] for c in obstacle} == {False, True}
    assert {c["obstacle"]["footprint_clearing"] for c in obstacle} == {False, True}
    # both combination methods over a static layer that is neither empty nor uniform
    for method in (0, 1):
        assert any(c["obstacle"]["combination_method"] == method and c["static"] is not None and len(np.unique(recs[0]["master_static"])) > 3
                   for c, recs in cases.values() if c["obstacle"] is not None), method
    # a footprint with a vertex off the map: setConvexPolygonCost refuses, the cells under the robot keep their marks
    c, recs = cases["obstacle_small_map"]
    x, y, yaw = c["cycles"][1]["pose"]
    fp = np.asarray(c["fp"])
    world = np.stack([x + fp[:, 0] * np.cos(yaw) - fp[:, 1] * np.sin(yaw), y + fp[:, 0] * np.sin(yaw) + fp[:, 1] * np.cos(yaw)], 1)
    inside = _in_map(c, recs[1]["origin"], world)
    assert inside.any() and not inside.all() and c["obstacle"]["footprint_clearing"]


def test_raytracing_coverage(golden):
    _, _, cases = golden
    sensor_off_map = zero_length = beyond_range = at_range = 0
    exits = set()
    for name, (c, recs) in cases.items():
        if c["obstacle"] is None or c["obstacle"]["voxel"]:
            continue
        for k, ob, s, p, org in _rays(c, recs):
            if not _in_map(c, org, s[:2]):
                sensor_off_map += 1
                continue
            d = np.hypot(p[:, 0] - s[0], p[:, 1] - s[1])
            zero_length += int((d == 0).sum())
            beyond_range += int((d > ob["raytrace_range"]).sum())
            at_range += int((d == ob["raytrace_range"]).sum())
            ex, ey = org[0] + c["size_x"] * c["res"], org[1] + c["size_y"] * c["res"]
            left, right, bottom, top = p[:, 0] < org[0], p[:, 0] > ex, p[:, 1] < org[1], p[:, 1] > ey
            for side, m in (("left", left & ~bottom & ~top), ("right", right & ~bottom & ~top), ("bottom", bottom & ~left & ~right),
                            ("top", top & ~left & ~right), ("corner", (left | right) & (bottom | top))):
                if m.any():
                    exits.add(side)
    assert sensor_off_map and zero_length and beyond_range and at_range
    assert exits == {"left", "right", "bottom", "top", "corner"}
    # updateRaytraceBounds grows the box: a cycle whose box reaches further than its marked points and its footprint
    c, recs = cases["static_trinary_overwrite_no_unknown"]
    assert c["inflation"] is None and tuple(recs[1]["box"]) != (0, c["size_x"], 0, c["size_y"])
    ob = c["cycles"][1]["obs"][0]
    p = ob["points"].astype(np.float64)
    marked = p[((p - np.asarray(ob["origin"])) ** 2).sum(1) < ob["obstacle_range"] ** 2]
    assert recs[1]["box"][0] < int((marked[:, 0].min() - c["ox"]) / c["res"]) or recs[1]["box"][1] > int((marked[:, 0].max() - c["ox"]) / c["res"]) + 1


def test_rolling_window_coverage(golden):
    _, _, cases = golden
    for kind in ("2d", "voxel"):
        shifts = []
        for tag in ("a", "b"):
            c, recs = cases[f"rolling_{kind}_{tag}"]
            assert c["rolling"] and bool(c["obstacle"]["voxel"]) == (kind == "voxel")
            for k in range(1, len(recs)):
                cells = np.rint((recs[k]["origin"] - recs[k - 1]["origin"]) / c["res"]).astype(int)
                moved = np.asarray(c["cycles"][k]["pose"][:2]) - np.asarray(c["cycles"][k - 1]["pose"][:2])
                shifts.append((tuple(cells), tuple(moved), (c["size_x"], c["size_y"])))
        assert any(s[0] > 0 and s[1] > 0 for s, _, _ in shifts) and any(s[0] < 0 and s[1] < 0 for s, _, _ in shifts), kind
        assert any(s[0] > 0 and s[1] < 0 for s, _, _ in shifts), kind
        assert any(s == (0, 0) and m == (0.0, 0.0) for s, m, _ in shifts), (kind, "no move")
        assert any(s == (0, 0) and m != (0.0, 0.0) for s, m, _ in shifts), (kind, "a move within a cell")
        assert any(abs(s[0]) > n[0] and abs(s[1]) > n[1] for s, _, n in shifts), (kind, "a shift larger than the window")
    # what survives a shift: the layer grid holds marks from the cycle before
    for name in ("rolling_2d_a", "rolling_voxel_a"):
        c, recs = cases[name]
        assert (recs[1]["layer"] == K.LETHAL).sum() > (recs[0]["layer"] == K.LETHAL).sum()
    for name in ("rolling_2d_b", "rolling_voxel_b"):
        c, recs = cases[name]
        assert (recs[3]["layer"] == K.LETHAL).sum() < (recs[2]["layer"] == K.LETHAL).sum()
    assert len(cases["rolling_voxel_a"][1]) == len([r for r in cases["rolling_voxel_a"][1] if "voxels" in r])


def test_voxel_coverage(golden):
    _, meta, cases = golden
    vox = {n: cr for n, cr in cases.items() if cr[0]["obstacle"] is not None and cr[0]["obstacle"]["voxel"]}
    fixed = [c["obstacle"] for c, _ in vox.values()]
    assert {o["z_voxels"] for o in fixed} == {1, 5, 10, 16}
    assert {o["origin_z"] for o in fixed} >= {0.0} and any(o["origin_z"] < 0 for o in fixed)
    assert {o["z_resolution"] for o in fixed} == {0.1, 0.2, 0.25}
    assert {o["unknown_threshold"] for o in fixed} == {0, 4, 15}
    assert {o["mark_threshold"] for o in fixed} == {0, 1}
    for name, (c, recs) in vox.items():
        assert "voxels" in recs[-1], name
        if c["rolling"]:
            continue
        o = c["obstacle"]
        top = o["origin_z"] + o["z_voxels"] * o["z_resolution"]
        above_height = below_origin = above_grid = mark_above = mark_below = 0
        for k, cyc in enumerate(c["cycles"]):
            for ob in cyc["obs"]:
                z = ob["points"][:, 2].astype(np.float64)
                assert o["origin_z"] <= ob["origin"][2] < top, name  # the sensor is inside the grid: its rays are traced
                if ob["clearing"]:
                    above_height += int((z > o["max_obstacle_height"]).sum())  # clipped to max_obstacle_height - 0.01
                    below_origin += int((z < o["origin_z"]).sum())             # clipped to origin_z
                    above_grid += int(((z >= top) & (z <= o["max_obstacle_height"])).sum())
                if ob["marking"]:
                    mark_above += int(((z >= top) & (z <= o["max_obstacle_height"])).sum())
                    mark_below += int((z < o["origin_z"]).sum())
        assert above_height and below_origin and mark_below, name
        assert (above_grid and mark_above) or top >= o["max_obstacle_height"], name
        # the thresholds decide something: the layer grid holds free, lethal and (where unknown is tracked) unknown cells
        values = set(np.unique(recs[-1]["layer"]).tolist())
        assert {K.FREE, K.LETHAL} <= values and (not c["track_unknown"] or K.NOINFO in values), name
    assert sum(len(v) > 1 for v in meta["voxel_cycles"].values()) >= 2  # the words after every cycle, for at least two cases
    # mark_threshold 1: columns with one marked voxel stay unmarked in the grid, columns with two are lethal
    c, recs = cases["voxel_z16_neg_origin"]
    marked = np.array([[bin(int(w) >> 16).count("1") for w in row] for row in recs[0]["voxels"]])
    assert (marked == 1).any() and (marked >= 2).any()
    assert not (recs[0]["layer"][marked == 1] == K.LETHAL).any() and (recs[0]["layer"][marked >= 2] == K.LETHAL).all()


def test_static_coverage(golden):
    _, _, cases = golden
    st = [(c, recs) for c, recs in cases.values() if c["static"] is not None]
    for key in ("trinary", "track_unknown_space", "use_maximum"):
        assert {c["static"][key] for c, _ in st} == {False, True}, key
    assert any(c["static"]["lethal_threshold"] != 100 and c["static"]["unknown_cost_value"] != -1 for c, _ in st)
    for trinary in (False, True):
        assert any(c["static"]["trinary"] == trinary and set(np.unique(c["static"]["occ"]).tolist()) == set(range(-128, 128)) for c, _ in st), trinary
    assert any(K.stages(c) == ["static"] for c, _ in st) and any(K.stages(c)[:2] == ["static", "obstacle"] for c, _ in st)
    rolling = [(c, recs) for c, recs in st if c["rolling"]]
    assert rolling
    for c, recs in rolling:
        s = c["static"]
        sy, sx = s["occ"].shape
        assert sx > c["size_x"] and sy > c["size_y"] and (s["ox"], s["oy"]) != (c["ox"], c["oy"])
        inside = [s["ox"] <= r["origin"][0] and s["oy"] <= r["origin"][1] and r["origin"][0] + c["size_x"] * c["res"] <= s["ox"] + sx * s["res"] and
                  r["origin"][1] + c["size_y"] * c["res"] <= s["oy"] + sy * s["res"] for r in recs]
        assert any(inside) and not all(inside)  # windows inside the static map, and one that hangs over its edge


def test_inflation_coverage(golden):
    _, meta, cases = golden
    inf = {n: cr for n, cr in cases.items() if cr[0]["inflation"] is not None}
    assert {K.cell_radius(c, 0) for c, _ in inf.values()} >= {1, 5, 11, 14}
    assert len({c["inflation"]["scaling"] for c, _ in inf.values()}) >= 2
    assert any(c["inflation"]["radius"] < 0.15 for c, _ in inf.values())  # below both footprints' inscribed radius
    c, recs = cases["inflation_r14_grey"]
    seeds = recs[0]["master_obstacle"] == K.LETHAL
    sy, sx = seeds.shape
    assert seeds[0, 0] and seeds[0, sx - 1] and seeds[sy - 1, 0] and seeds[sy - 1, sx - 1]
    assert seeds[0, 1:-1].any() and seeds[sy - 1, 1:-1].any() and seeds[1:-1, 0].any() and seeds[1:-1, sx - 1].any()
    # unknown beside lethal (the NO_INFORMATION write rule, both ways), and costs in the master above and below the inflated value
    unknown_kept = unknown_taken = above = below = 0
    for name, (c, recs) in inf.items():
        for r in recs:
            before = r["master_" + K.stages(c)[-2]]
            changed = before != r["master"]
            unknown_taken += int((changed & (before == K.NOINFO)).sum())
            near = np.zeros_like(changed)
            near[1:, :] |= before[:-1, :] == K.LETHAL
            near[:-1, :] |= before[1:, :] == K.LETHAL
            unknown_kept += int(((before == K.NOINFO) & ~changed & ~near).sum())
            below += int((changed & (before > 0) & (before < 253)).sum())
            grown = r["master_exact"] > 0
            above += int((~changed & grown & (before > 0) & (before < 253)).sum())
    assert unknown_kept and unknown_taken and above and below
    # boxes that cover part of the map and are clipped by each border once grown by the radius; a box remembered from the cycle before
    clipped = set()
    for name, (c, recs) in inf.items():
        R = K.cell_radius(c, 0)
        for r in recs:
            x0, xn, y0, yn = r["box"]
            if (x0, xn, y0, yn) == (0, c["size_x"], 0, c["size_y"]):
                continue
            clipped |= {s for s, hit in (("left", x0 - R < 0 <= x0), ("bottom", y0 - R < 0 <= y0), ("right", xn + R > c["size_x"]), ("top", yn + R > c["size_y"])) if hit}
    assert clipped == {"left", "bottom", "right", "top"}
    c, recs = cases["obstacle_fixed"]
    assert c["cycles"][2]["obs"][0]["raytrace_range"] == c["cycles"][3]["obs"][0]["raytrace_range"] == 1.0
    full = (0, c["size_x"], 0, c["size_y"])
    assert tuple(recs[2]["box"]) == full and tuple(recs[3]["box"]) != full  # cycle 2's data is as small as cycle 3's: its box is cycle 1's
    # a footprint change between cycles: the whole map again, and another cost table
    c, recs = cases["inflation_r5"]
    assert c["cycles"][3]["fp"] is not None and tuple(recs[2]["box"]) != (0, 64, 0, 64) and tuple(recs[3]["box"]) == (0, 64, 0, 64)
    assert not np.array_equal(recs[2]["cost_table"], recs[3]["cost_table"])
    # maps on which the priority-queue walk and the exact distance differ, and maps on which they do not
    assert set(meta["walk_equals_exact"]) == set(inf)
    assert sum(meta["walk_equals_exact"].values()) >= 1 and sum(not v for v in meta["walk_equals_exact"].values()) >= 1
    assert "not a reference output" in meta["master_exact"]


# ------------------------------------------------------------------------------------------------ the specification against the walk
def test_exact_specification_bounds_the_walk(golden):
    """The exact distance is never larger than the walk's, and the cost does not increase with distance: specification >= reference in
    every cell, and the same grid on the cases meta calls tie-free."""
    _, meta, cases = golden
    for name, same in meta["walk_equals_exact"].items():
        c, recs = cases[name]
        again = K.exact_masters(c, recs)  # (asserts on the way that the reference's grids keep what lies outside a cycle's box)
        for k, r in enumerate(recs):
            assert (r["master_exact"] >= r["master"]).all(), (name, k)
            assert np.array_equal(r["master_exact"], again[k]), (name, k)
            t = r["cost_table"].astype(int)
            R = t.shape[0] - 2
            order = np.argsort(np.hypot(*np.mgrid[0:R + 2, 0:R + 2]).reshape(-1), kind="stable")
            assert (np.diff(t.reshape(-1)[order]) <= 0).all(), (name, k, "the cost table decreases with distance")
        assert same == all(np.array_equal(r["master_exact"], r["master"]) for r in recs), name


# ------------------------------------------------------------------------------------------------ the oracle against the fixture
def oracle_costmap(orc, c, exact):
    o = orc.LayeredCostmap(c["track_unknown"])
    o.resize(c["size_x"], c["size_y"], c["res"], c["ox"], c["oy"])
    o.set_rolling(c["rolling"])
    s = c["static"]
    if s is not None:
        kw = dict(track_unknown_space=s["track_unknown_space"], use_maximum=s["use_maximum"], trinary=s["trinary"],
                  lethal_threshold=s["lethal_threshold"], unknown_cost_value=s["unknown_cost_value"])
        (o.add_static_rolling if c["rolling"] else o.add_static)(s["occ"], s["res"], s["ox"], s["oy"], **kw)
    ob = c["obstacle"]
    if ob is not None:
        kw = dict(combination_method=ob["combination_method"], footprint_clearing=ob["footprint_clearing"], max_obstacle_height=ob["max_obstacle_height"])
        if ob["voxel"]:
            o.add_voxel(z_voxels=ob["z_voxels"], origin_z=ob["origin_z"], z_resolution=ob["z_resolution"], unknown_threshold=ob["unknown_threshold"],
                        mark_threshold=ob["mark_threshold"], **kw)
        else:
            o.add_obstacle(**kw)
    if c["inflation"] is not None:
        o.add_inflation(c["inflation"]["radius"], c["inflation"]["scaling"], exact=exact)
    o.set_footprint(c["fp"])
    o.keep_layer_masters()
    return o


def oracle_cycle(o, cyc):
    if cyc["fp"] is not None:
        o.set_footprint(cyc["fp"])
    o.clear_observations()
    for ob in cyc["obs"]:
        o.add_observation(ob["points"], origin=ob["origin"], obstacle_range=ob["obstacle_range"], raytrace_range=ob["raytrace_range"],
                          marking=ob["marking"], clearing=ob["clearing"])
    o.update_map(*cyc["pose"])


@pytest.mark.parametrize("exact", [False, True], ids=["priority_queue_walk", "exact_distance"])
def test_oracle_equals_the_reference(golden, orc, exact):
    _, meta, cases = golden
    for name, (c, recs) in cases.items():
        if exact and c["inflation"] is None:
            continue
        o = oracle_costmap(orc, c, exact)
        for k, (cyc, r) in enumerate(zip(c["cycles"], recs)):
            where = f"{name} cycle {k}"
            oracle_cycle(o, cyc)
            assert np.array_equal(o.origin().view(np.uint64), r["origin"].view(np.uint64)), f"{where}: origin"
            assert np.array_equal(o.bounds(), r["box"]), f"{where}: box {o.bounds()} {r['box']}"
            if c["obstacle"] is not None:
                assert np.array_equal(o.layer(2), r["layer"]), f"{where}: layer grid"
            if "voxels" in r:
                assert np.array_equal(o.voxels(), r["voxels"]), f"{where}: voxel words"
            for which, key in ((1, "master_static"), (2, "master_obstacle")):
                if key in r and not exact:  # (outside a cycle's box these grids hold earlier cycles' inflation: the walk's in the fixture)
                    assert np.array_equal(o.master_after(which), r[key]), f"{where}: {key}"
            assert np.array_equal(o.master(), r["master_exact"] if exact else r["master"]), f"{where}: master"
            if c["inflation"] is not None:
                t = r["cost_table"]
                inscribed = o.inscribed_radius
                assert np.float64(inscribed).view(np.uint64) == np.float64(r["inscribed"]).view(np.uint64), f"{where}: inscribed radius"
                for i in range(t.shape[0]):
                    for j in range(t.shape[1]):
                        assert orc.lib().orc_compute_cost(c["res"], c["inflation"]["scaling"], inscribed, float(np.hypot(i, j))) == t[i, j], (where, i, j)
                R, costs, _ = orc.cost_lut(c["res"], c["inflation"]["radius"], c["inflation"]["scaling"], inscribed)
                assert R == t.shape[0] - 2 and np.array_equal(costs, t), f"{where}: cost table"
