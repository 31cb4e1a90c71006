"""The costmap kernels (k_obstacle, k_merge, k_inflate / k_inflate_bits / k_inflate_pq, the static layer's interpretation and its rolling
read, the rolling-window shift) against the reference's own numbers: tests/golden/g17_costmap_reference.npz, written by
tools/make_costmap_goldens.py from costmap_2d's LayeredCostmap and layers and voxel_grid's VoxelGrid compiled in place.  Reads the
fixture only: no reference tree, no CPU oracle.  Need a real MI355X.

Bar: bit equality.  origins() as float64 bits, bounds(), download(GRID_OBSTACLE), download(GRID_VOXEL) and master() after every cycle;
priority_queue_order=True against the reference's master grids, the default inflation against the exact-distance specification grids
(NAME_master_exact, built from the reference's cost table).

Every case runs twice.  Through stage_observations / update_map in a fleet of three, the case in the middle slot.  And through
stage_observations_list / update_map_list in a fleet of four, the case in slot 1 again and the list (1, 3): with three robots no list
that holds the middle one skips a robot; robots 0 and 2 stay out of the list and must keep their grids.  The neighbours get the
case's inputs mirrored in y (slot 0) and transposed - on a map that is not square: mirrored in x - (the last slot): other occupancy
grids, other poses, other points, so a batch-indexing error shows in the middle robot.  A rolling fleet shares one static map
(navgpu_static_set_rolling_map takes one per fleet): there the neighbours differ in poses and points only.

Every case of the fixture runs here: the library's API expresses them all.  One parameter goes another way than in the reference:
LayeredCostmap::setFootprint tells the inflation layer the inscribed radius itself, a Fleet takes it through configure_inflation; the
test passes the radius the reference computed (NAME_inscribed) together with every footprint."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costmap_reference_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

G, META = K.load()


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def _variant(c, how):
    """the case's inputs seen in a mirror: how = 'y' (y -> -y about the map's middle), 'x', or 't' (x <-> y, square maps at the origin's
    diagonal); returns (occupancy or None, per-cycle (pose, observations))"""
    cx, cy = c["ox"] + c["size_x"] * c["res"] / 2, c["oy"] + c["size_y"] * c["res"] / 2

    def xy(x, y):
        if how == "y":
            return x, 2 * cy - y
        if how == "x":
            return 2 * cx - x, y
        return c["ox"] + (y - c["oy"]), c["oy"] + (x - c["ox"])

    def yaw(a):
        return {"y": -a, "x": np.pi - a, "t": np.pi / 2 - a}[how]

    occ = None
    if c["static"] is not None and not c["rolling"]:
        o = c["static"]["occ"]
        occ = np.ascontiguousarray({"y": o[::-1], "x": o[:, ::-1], "t": o.T}[how])
    cycles = []
    for cyc in c["cycles"]:
        x, y, a = cyc["pose"]
        obs = []
        for ob in cyc["obs"]:
            p = ob["points"].astype(np.float64)
            px, py = xy(p[:, 0], p[:, 1])
            sx, sy = xy(ob["origin"][0], ob["origin"][1])
            obs.append(dict(ob, points=np.stack([px, py, p[:, 2]], 1).astype(np.float32), origin=(sx, sy, ob["origin"][2])))
        cycles.append((xy(x, y) + (yaw(a),), obs))
    return occ, cycles


def _fleet(nav, c, n):
    from navigation_amd import _lib as N
    layers = 0
    if c["static"] is not None:
        layers |= N.LAYER_STATIC
    if c["obstacle"] is not None:
        layers |= N.LAYER_VOXEL if c["obstacle"]["voxel"] else N.LAYER_OBSTACLE
    if c["inflation"] is not None:
        layers |= N.LAYER_INFLATION
    fl = nav.Fleet(n, c["size_x"], c["size_y"], c["res"], layers=layers, track_unknown=c["track_unknown"], max_points=1024, max_observations=2,
                   rolling_window=c["rolling"], max_sim_steps=32, max_plan=64)
    fl.set_origin(np.tile([c["ox"], c["oy"]], (n, 1)))
    o = c["obstacle"]
    if o is not None:
        fl.configure_obstacle(footprint_clearing_enabled=o["footprint_clearing"], combination_method=o["combination_method"],
                              max_obstacle_height=o["max_obstacle_height"], z_voxels=o["z_voxels"], origin_z=o["origin_z"],
                              z_resolution=o["z_resolution"], unknown_threshold=o["unknown_threshold"], mark_threshold=o["mark_threshold"])
    fl.set_footprint(c["fp"])
    return fl


def _static(fl, c, slot_occ):
    s = c["static"]
    if s is None:
        return
    kw = dict(track_unknown_space=s["track_unknown_space"], use_maximum=s["use_maximum"], trinary_costmap=s["trinary"],
              lethal_cost_threshold=s["lethal_threshold"], unknown_cost_value=s["unknown_cost_value"])
    if c["rolling"]:
        fl.set_rolling_static_map(s["occ"], s["res"], s["ox"], s["oy"], **kw)
    else:
        for slot, occ in slot_occ.items():
            fl.add_static_map(occ, first=slot, count=1, **kw)


def _run(nav, name, pq, listed):
    from navigation_amd import _lib as N
    c, recs = K.case(G, META, name)
    n = 4 if listed else 3
    me, last = 1, n - 1
    robots = [1, 3] if listed else list(range(n))
    second = "t" if c["size_x"] == c["size_y"] and c["ox"] == c["oy"] else "x"
    variants = {0: _variant(c, "y"), last: _variant(c, second), me: (None if c["static"] is None or c["rolling"] else c["static"]["occ"],
                                                                   [(cyc["pose"], cyc["obs"]) for cyc in c["cycles"]])}
    if n == 4:
        variants[2] = variants[0]
    voxel = c["obstacle"] is not None and c["obstacle"]["voxel"]
    fl = _fleet(nav, c, n)
    try:
        _static(fl, c, {slot: v[0] for slot, v in variants.items()})
        if c["static"] is not None and not c["rolling"]:
            assert not np.array_equal(variants[0][0], variants[me][0]) and not np.array_equal(variants[last][0], variants[me][0])
        if c["inflation"] is not None:
            fl.configure_inflation(c["inflation"]["radius"], c["inflation"]["scaling"], float(recs[0]["inscribed"]), priority_queue_order=pq)
        untouched = {i: (fl.master(i, 1)[0], fl.origins()[i]) for i in range(n) if i not in robots}
        for k, (cyc, r) in enumerate(zip(c["cycles"], recs)):
            where = f"{name} cycle {k} ({'walk' if pq else 'exact'}, {'list ' + str(robots) if listed else 'range'})"
            if cyc["fp"] is not None:
                fl.set_footprint(cyc["fp"])
                if c["inflation"] is not None:
                    fl.configure_inflation(c["inflation"]["radius"], c["inflation"]["scaling"], float(r["inscribed"]), priority_queue_order=pq)
            poses = [variants[i][1][k][0] for i in robots]
            obs = [dict(ob, instance=i) for i in robots for ob in variants[i][1][k][1]]
            assert not np.array_equal(poses[0], poses[-1])
            if listed:
                fl.stage_observations_list(robots, poses, obs)
                fl.update_map_list(robots)
                box = fl.bounds_list(robots)[robots.index(me)]
            else:
                fl.stage_observations(poses, obs)
                fl.update_map()
                box = fl.bounds()[me]
            assert np.array_equal(fl.origins()[me].view(np.uint64), r["origin"].view(np.uint64)), f"{where}: origin {fl.origins()[me]} {r['origin']}"
            assert np.array_equal(box, r["box"]), f"{where}: box {box} {r['box']}"
            if c["obstacle"] is not None:
                assert np.array_equal(fl.download(N.GRID_OBSTACLE, me, 1)[0], r["layer"]), f"{where}: layer grid"
            if voxel and "voxels" in r:
                assert np.array_equal(fl.download(N.GRID_VOXEL, me, 1)[0], r["voxels"]), f"{where}: voxel words"
            want = r["master"] if (pq or c["inflation"] is None) else r["master_exact"]
            got = fl.master(me, 1)[0]
            assert np.array_equal(got, want), f"{where}: master, {int((got != want).sum())} cells differ"
            for i, (m, org) in untouched.items():
                assert np.array_equal(fl.master(i, 1)[0], m) and np.array_equal(fl.origins()[i], org), f"{where}: unlisted robot {i} changed"
    finally:
        fl.close()


INFLATED = [n for n in META["cases"] if n in META["walk_equals_exact"]]


@pytest.mark.parametrize("name", META["cases"])
def test_range_update_exact_inflation(nav, name):
    _run(nav, name, pq=False, listed=False)


@pytest.mark.parametrize("name", META["cases"])
def test_listed_update_exact_inflation(nav, name):
    _run(nav, name, pq=False, listed=True)


@pytest.mark.parametrize("name", INFLATED)
def test_range_update_priority_queue_walk(nav, name):
    _run(nav, name, pq=True, listed=False)


@pytest.mark.parametrize("name", INFLATED)
def test_listed_update_priority_queue_walk(nav, name):
    _run(nav, name, pq=True, listed=True)
