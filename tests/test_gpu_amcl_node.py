"""AmclNode's laser cycle for a fleet (navgpu_amcl_node_laser_received, navgpu_amcl_hypotheses).  What the node decides comes from the
Python restatement in tests/amcl_node_ref.py; everything the device answers comes from a TWIN HANDLE driven by hand through the
existing entry points (update_action / update_sensor / update_resample on count = 1 slices of the filters the restatement says are
due, with host-built AMCLLaserData), and the two handles' sets must agree byte for byte.

Shapes: 6 filters, max_samples 96, min_samples 16, one shared 48 x 48 map at 0.1 m, scans of 24 rays with max_beams 8 (step 3)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amcl_node_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
OK, ERR_INVALID, ERR_STATE = 0, -1, -5
BEAM, LF = 0, 1
ODOM_DIFF, ODOM_GAUSSIAN = 0, 4
NF, MS, MINS, MB, RAYS = 6, 96, 16, 8, 24
FLAGS = ("moved", "updated", "resampled", "cloud_due", "published", "republish", "global_localization_converged")


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    if nav.lib().navgpu_device_count() <= 0:
        pytest.skip("no GPU")
    return nav


def the_map():
    occ = np.zeros((48, 48), np.int8)       # OccupancyGrid data: 0 free, 100 occupied
    occ[30, 4:40] = 100                     # a wall
    occ[10:16, 28:36] = 100                 # a box
    return occ


def cloud(seed, centre=(1.5, 2.0, 0.3)):
    """(NF, MS, 3) poses around `centre`, a different cloud per filter"""
    rng = np.random.default_rng(seed)
    P = rng.normal(0.0, 1.0, (NF, MS, 3)) * np.array([0.15, 0.15, 0.1]) + np.array(centre)
    return P + np.arange(NF)[:, None, None] * np.array([0.05, -0.03, 0.02])


def make(nav, nf=NF, model=LF, odom=ODOM_DIFF, node=None, maps=None, samples=True, seed=5):
    a = nav.AmclLaser(nf, MS, max_beams=MB)
    a.set_map(the_map(), 0.1, (0.0, 0.0), max_occ_dist=1.0, first=0, count=nf if maps is None else maps)
    a.configure(model_type=model, max_beams=MB)
    a.set_laser_pose(np.tile([0.1, 0.0, 0.0], (nf, 1)))
    a.configure_odom(odom, 0.2, 0.2, 0.2, 0.2, 0.2)
    a.configure_resample(min_samples=MINS)
    if node is not None:
        a.configure_node(**node)
    if samples:
        a.set_samples(cloud(seed)[:nf], np.full((nf, MS), 1.0 / MS))
    return a


def rays(call, f, n=RAYS):
    """the message's float32 ranges of filter f at call `call`"""
    i = np.arange(n)
    return (1.2 + 0.8 * np.sin(0.37 * i + 0.9 * f + 0.23 * call) + 0.05 * f).astype(np.float32)


def scan_of(r, pose, range_min=0.1, range_max=4.0, yaw_min=-1.0, yaw_inc=None):
    yaw_inc = yaw_min + 2.0 / 23 if yaw_inc is None else yaw_inc
    return dict(ranges=np.asarray(r, np.float32), range_min=range_min, range_max=range_max, yaw_min=yaw_min, yaw_inc=yaw_inc,
                odom_pose=tuple(pose))


def host_laser_data(s, node):
    """the AMCLLaserData the reference would build from scan dict s -> ((n, 2) array, range_max)"""
    b, rmax = ref.convert_scan([float(v) for v in s["ranges"]], s["range_min"], s["range_max"], s["yaw_min"], s["yaw_inc"],
                               node.get("laser_min_range", -1.0), node.get("laser_max_range", -1.0))
    return np.array(b, np.float64).reshape(-1, 2), rmax


def clusters_or_none(nav, a, f):
    try:
        return a.clusters(f)
    except nav.NavgpuError:
        return None


def dump(nav, a, nf=None):
    """everything a set consists of, per filter, as bytes-comparable arrays (poses and weights up to sample_count)"""
    nf = a.n if nf is None else nf
    sc, P, W, cv = a.get_samples()
    w = a.get_filter_state()
    leaf, ctr = a.kd_leaf_counts(), a.rng_counters()
    out = []
    for f in range(nf):
        c = clusters_or_none(nav, a, f)
        out.append(dict(count=int(sc[f]), converged=int(cv[f]), poses=P[f, :sc[f]].copy(), weights=W[f, :sc[f]].copy(), w=w[f].copy(),
                        leaf=int(leaf[f]), ctr=int(ctr[f]), clusters=None if c is None else [np.asarray(x).copy() for x in c]))
    return out


def same_bytes(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def assert_same_set(d1, d2, what):
    for k in ("count", "converged", "leaf", "ctr"):
        assert d1[k] == d2[k], (what, k, d1[k], d2[k])
    for k in ("poses", "weights", "w"):
        assert same_bytes(d1[k], d2[k]), (what, k)
    assert (d1["clusters"] is None) == (d2["clusters"] is None), what
    if d1["clusters"] is not None:
        for x, y in zip(d1["clusters"], d2["clusters"]):
            assert same_bytes(x, y), (what, "clusters")


# ---------------------------------------------------------------- 1. scan conversion
def conversion_cases():
    nan, inf = float("nan"), float("inf")
    c = {}
    r = [rays(0, f) for f in range(NF)]
    short = [x.copy() for x in r]
    for f in range(NF):
        short[f][[0, 3, 6, 21]] = [0.05, np.float32(0.1), 0.0, -1.0]   # subsampled rays (step 3): below, at, zero, negative
        short[f][1] = 0.01                                              # a ray the step skips
    c["short_rays"] = dict(ranges=short)
    odd = [x.copy() for x in r]
    for f in range(NF):
        odd[f][3 * (f % 8)] = nan
        odd[f][(3 * (f + 2)) % 24] = inf
        odd[f][(3 * (f + 4)) % 24] = -inf
    c["nan_and_inf"] = dict(ranges=odd)
    c["overrides_set"] = dict(ranges=short, node=dict(laser_min_range=0.9, laser_max_range=1.7))
    c["overrides_looser_than_msg"] = dict(ranges=short, node=dict(laser_min_range=0.01, laser_max_range=30.0))
    c["overrides_unset_zero"] = dict(ranges=short, node=dict(laser_min_range=0.0, laser_max_range=0.0))
    c["upside_down"] = dict(ranges=r, yaw_min=1.0, yaw_inc=1.0 - 2.0 / 23)
    c["wrap_positive"] = dict(ranges=r, yaw_min=3.1, yaw_inc=-3.1)          # inc - min = -6.2 -> +0.0832 after the fmod
    c["wrap_negative"] = dict(ranges=r, yaw_min=-3.1, yaw_inc=3.1)          # inc - min = +6.2 -> -0.0832
    c["beam_model_count_eq_max_beams"] = dict(ranges=[x[:MB] for x in r], model=BEAM)
    c["beam_model"] = dict(ranges=r, model=BEAM)
    return c


CASES = conversion_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_scan_conversion_bytes_match_a_host_built_scan(nav, name):
    case = CASES[name]
    node = dict(d_thresh=0.2, a_thresh=0.5, resample_interval=2)
    node.update(case.get("node", {}))
    a = make(nav, model=case.get("model", LF), node=node)
    twin = make(nav, model=case.get("model", LF))
    scans = [scan_of(case["ranges"][f], (1.0, 1.0, 0.1 * f), yaw_min=case.get("yaw_min", -1.0), yaw_inc=case.get("yaw_inc"))
             for f in range(NF)]
    rc, res = a.laser_received(scans, seed=11)
    assert rc == OK
    # freshly set samples: the first-scan branch, so the sensor step alone ran
    assert res.updated.tolist() == [1] * NF and res.moved.tolist() == [0] * NF and res.resampled.tolist() == [0] * NF
    data = [host_laser_data(s, node) for s in scans]
    twin.update_sensor([d[0] for d in data], [d[1] for d in data])
    _, _, W, _ = a.get_samples()
    _, _, Wt, _ = twin.get_samples()
    assert same_bytes(W, Wt)
    assert same_bytes(a.get_filter_state(), twin.get_filter_state())
    assert not same_bytes(W[:, :MS], np.full((NF, MS), 1.0 / MS))   # the model did weigh the particles
    a.close()
    twin.close()


# ---------------------------------------------------------------- 2. closed loop
def odom_pose(call, f, frozen4=None):
    if f == 0:
        return (1.0, 1.0, 0.0)
    if f == 1:
        return (1.0 + 0.25 * call, 1.0, 0.2)
    if f == 2:
        return (1.0, 1.0, 0.6 * call)        # only the heading; passes +pi at call 6
    if f == 3:
        return (2.0, 0.5, -1.0)
    if f == 4:
        c = call if frozen4 is None else min(call, frozen4)
        return (0.5, 1.0 + 0.25 * c, 1.0)
    return (1.0 + 0.15 * call, 2.0, 0.0)     # f == 5: 0.3 m between the scans it gets


@pytest.mark.parametrize("integrator, odom_model", [(False, ODOM_DIFF), (True, ODOM_GAUSSIAN)])
def test_closed_loop_matches_the_restatement_and_a_twin_driven_by_hand(nav, integrator, odom_model):
    node = dict(d_thresh=0.2, a_thresh=0.5, resample_interval=2, use_odom_integrator=int(integrator))
    a = make(nav, odom=odom_model, node=node)
    twin = make(nav, odom=odom_model)
    R = [ref.NodeRef(0.2, 0.5, 2, integrator) for _ in range(NF)]
    a.node_reset(global_localization=True, first=1, count=1)
    R[1].reset(True)
    seen = {k: 0 for k in FLAGS}
    for call in range(12):
        seed = 1000 + call
        if call in (4, 5):
            a.request_nomotion_update(first=3, count=1)
            R[3].request_nomotion_update()
        if call == 7:   # a nomotion request, then a new initial pose: the request must survive the reset and the first scan
            a.request_nomotion_update(first=4, count=1)
            R[4].request_nomotion_update()
            for h in (a, twin):
                h.init_gaussian([1.4, 2.1, 0.2], np.diag([0.04, 0.04, 0.01]), seed=77, first=4, count=1)
            a.node_reset(first=4, count=1)
            R[4].reset()
        if integrator:  # two odometry messages per filter between scans, the second at the scan's pose
            for f in range(NF):
                p0, p1 = odom_pose(max(call - 1, 0), f, 7), odom_pose(call, f, 7)
                mid = [(u + v) / 2 for u, v in zip(p0, p1)]
                for m in (mid, p1):
                    a.integrate_odom([m], first=f)
                    R[f].integrate_odom(m)
        scans = [None if (f == 5 and call % 2) else scan_of(rays(call, f), odom_pose(call, f, 7)) for f in range(NF)]
        rc, res = a.laser_received(scans, seed=seed)
        assert rc == OK, call
        st = a.node_state()
        for f in range(NF):
            what = (call, f)
            if scans[f] is None:
                assert all(res[k][f] == 0 for k in FLAGS) and res.status[f] == 0, what
                continue
            pose = scans[f]["odom_pose"]
            step = R[f].laser_received(pose)
            # the twin, by hand, in the order motion, sensor, resample
            if step["moved"]:
                twin.update_action([step["odom"]], seed=seed, first=f)
            if step["updated"]:
                b, rmax = host_laser_data(scans[f], node)
                twin.update_sensor([b], rmax, first=f)
            if step["resampled"]:
                twin.update_resample(seed=seed, first=f, count=1)
            hyp = None
            if step["resampled"] or step["force_publication"]:
                c = clusters_or_none(nav, twin, f)
                if c is not None:
                    mw, mh, mean = ref.argmax_hypothesis(c.weight, c.mean)
                    hyp = (mw, mean)
                    assert res.max_weight[f] == mw and res.max_weight_hyp[f] == mh and res.cluster_count[f] == len(c.weight), what
                    if mean is not None:
                        assert res.pose[f].tolist() == mean, what
                    assert [res.cov_xx[f], res.cov_xy[f], res.cov_yx[f], res.cov_yy[f], res.cov_aa[f]] == [
                        c.set_cov[0, 0], c.set_cov[0, 1], c.set_cov[1, 0], c.set_cov[1, 1], c.set_cov[2, 2]], what
            conv = int(twin.get_samples(first=f, count=1)[3][0])
            fin = R[f].finish(step, pose, conv, hyp)
            want = dict(moved=step["moved"], updated=step["updated"], resampled=step["resampled"], cloud_due=step["cloud_due"],
                        published=fin["published"], republish=fin["republish"],
                        global_localization_converged=fin["global_localization_converged"])
            for k in FLAGS:
                assert res[k][f] == int(want[k]), (what, k)
                seen[k] += int(want[k])
            assert res.status[f] == OK, what
            if fin["map_to_odom"] is not None:
                assert np.max(np.abs(res.map_to_odom[f] - np.array(fin["map_to_odom"]))) <= 1e-12, what
        for f in range(NF):
            what, r, s = (call, f), R[f], st[f]
            assert (s.pf_init, s.lasers_update, s.force_update, s.resample_count) == (
                int(r.pf_init), int(r.lasers_update), int(r.m_force_update), r.resample_count), what
            assert s.pf_odom_pose.tolist() == r.pf_odom_pose, what                    # copies and differences of the inputs
            assert s.odom_integrator_ready == int(r.integrator_ready), what
            assert s.odom_integrator_last_pose.tolist() == r.integrator_last_pose, what
            assert np.max(np.abs(s.odom_integrator_absolute_motion - np.array(r.absolute_motion))) <= 1e-12, what
            assert s.global_localization_active == int(r.global_localization_active), what
            assert s.latest_tf_valid == int(r.latest_tf_valid), what
            assert np.max(np.abs(s.latest_tf - np.array(r.latest_tf))) <= 1e-12, what
        d1, d2 = dump(nav, a), dump(nav, twin)
        for f in range(NF):
            assert_same_set(d1[f], d2[f], (call, f))
        if call == 7:
            assert res.cloud_due[4] == 0 and res.updated[4] == 1 and st.force_update[4] == 1   # the request survived the first scan
        if call == 8:
            assert res.moved[4] == 1 and st.force_update[4] == 0                               # and forced this update: f4 stands still
    # the scenario did exercise every branch but (perhaps) the convergence of a global localisation
    for k in ("moved", "updated", "resampled", "cloud_due", "published", "republish"):
        assert seen[k] > 0, k
    assert R[0].resample_count == 1 and R[3].resample_count == 3
    if not integrator:   # (the integrator restarts after the first scan, so filter 1's first 0.25 m is only half seen)
        assert R[1].resample_count == 12 and R[5].resample_count == 6
    a.close()
    twin.close()


# ---------------------------------------------------------------- 3. independence
def test_a_filter_in_the_fleet_equals_the_same_filter_alone(nav):
    """The device generator is keyed by the filter's index in its handle, so `alone` keeps the index: filter 0 against a one-filter
    handle, filter 1 against a two-filter handle whose filter 0 never gets a scan (first = 1, count = 1 calls)."""
    node = dict(d_thresh=0.2, a_thresh=0.5, resample_interval=2)
    fleet = make(nav, node=node)
    one = make(nav, nf=1, node=node)
    two = make(nav, nf=2, node=node)
    fleet.set_rng_counters([3, 9, 0, 0, 0, 0])
    one.set_rng_counters([3])
    two.set_rng_counters([0, 9])
    before = dump(nav, two)[0]
    for call in range(4):
        scans = [scan_of(rays(call, f), (1.0 + 0.3 * call * (1 + f), 1.0, 0.1 * call)) for f in range(NF)]
        _, rf = fleet.laser_received(scans, seed=500 + call)
        _, r1 = one.laser_received(scans[:1], seed=500 + call)
        _, r2 = two.laser_received(scans[1:2], seed=500 + call, first=1)
        assert rf[0].tobytes() == r1[0].tobytes() and rf[1].tobytes() == r2[0].tobytes(), call
    assert rf.moved.tolist() == [1] * NF and rf.resampled.tolist() == [1] * NF and rf.published.tolist() == [1] * NF
    df = dump(nav, fleet)
    assert_same_set(df[0], dump(nav, one)[0], "filter 0")
    d2 = dump(nav, two)
    assert_same_set(df[1], d2[1], "filter 1")
    assert_same_set(before, d2[0], "the filter beside it")
    assert df[1]["ctr"] == 9 + 3 + 2    # three motions (calls 1-3) and two resamples (calls 1 and 3)
    assert fleet.node_state()[1].tobytes() == two.node_state()[1].tobytes()
    for h in (fleet, one, two):
        h.close()


# ---------------------------------------------------------------- 4. hypotheses
def check_hypotheses(nav, a, H):
    for f in range(a.n):
        c = a.clusters(f)
        mw, mh, mean = ref.argmax_hypothesis(c.weight, c.mean)
        assert (H.cluster_count[f], H.max_weight_hyp[f], H.max_weight[f]) == (len(c.weight), mh, mw), f
        assert H.published[f] == 1 and H.pose[f].tolist() == mean, f
        assert [H.cov_xx[f], H.cov_xy[f], H.cov_yx[f], H.cov_yy[f], H.cov_aa[f]] == [
            c.set_cov[0, 0], c.set_cov[0, 1], c.set_cov[1, 0], c.set_cov[1, 1], c.set_cov[2, 2]], f
    sc, _, _, cv = a.get_samples()
    assert H.sample_count.tolist() == sc.tolist() and H.converged.tolist() == cv.tolist()


def test_hypotheses_equal_the_argmax_over_get_clusters(nav):
    node = dict(d_thresh=0.2, a_thresh=0.5, resample_interval=2)
    a = make(nav, node=node, samples=False)
    H = a.hypotheses()
    assert H.published.tolist() == [0] * NF and H.cluster_count.tolist() == [0] * NF and H.max_weight_hyp.tolist() == [-1] * NF
    # wide enough for several clusters per filter (bins of 0.5 m): the argmax has something to choose from
    means = np.array([[1.0 + 0.2 * f, 2.0, 0.1 * f] for f in range(NF)])
    a.init_gaussian(means, np.diag([0.5, 0.4, 0.3]), seed=21)
    H = a.hypotheses()
    check_hypotheses(nav, a, H)
    assert max(H.cluster_count) > 1
    # the first scan after the init publishes from these clusters (force_publication), with map -> odom from the scan's pose
    a.node_reset()
    poses = [(3.0 - f, 7.5 * f - 20.0, 2.9 - 1.3 * f) for f in range(NF)]
    _, res = a.laser_received([scan_of(rays(0, f), poses[f]) for f in range(NF)], seed=3)
    assert res.published.tolist() == [1] * NF and res.resampled.tolist() == [0] * NF
    st = a.node_state()
    for f in range(NF):
        assert res.pose[f].tolist() == H.pose[f].tolist() and res.max_weight[f] == H.max_weight[f]
        m2o = ref.map_to_odom(H.pose[f].tolist(), poses[f])
        assert np.max(np.abs(res.map_to_odom[f] - np.array(m2o))) <= 1e-12, f
        assert np.max(np.abs(st.latest_tf[f] - np.array(ref.invert_planar(m2o)))) <= 1e-12 and st.latest_tf_valid[f] == 1, f
    # after a resample (interval 2: the next scan that moves resamples), and through the stand-alone call again
    _, res = a.laser_received([scan_of(rays(1, f), (poses[f][0] + 0.5, poses[f][1], poses[f][2])) for f in range(NF)], seed=4)
    assert res.resampled.tolist() == [1] * NF
    H2 = a.hypotheses()
    check_hypotheses(nav, a, H2)
    for k in ("cluster_count", "max_weight_hyp", "max_weight", "pose", "cov_xx", "cov_xy", "cov_yx", "cov_yy", "cov_aa", "published"):
        assert same_bytes(res[k], H2[k]), k
    # a slice of the fleet
    H3 = a.hypotheses(first=2, count=3)
    assert same_bytes(H3.pose, H2.pose[2:5]) and same_bytes(H3.max_weight, H2.max_weight[2:5])
    a.close()


# ---------------------------------------------------------------- 5. failures
def everything(nav, a):
    return dump(nav, a), a.node_state().tobytes()


def assert_untouched(nav, a, before, filters=None):
    d, s = everything(nav, a)
    for f in (range(a.n) if filters is None else filters):
        assert_same_set(before[0][f], d[f], f)
    if filters is None:
        assert s == before[1]
    else:
        n = len(s) // a.n
        for f in filters:
            assert s[f * n:(f + 1) * n] == before[1][f * n:(f + 1) * n], f


def test_state_errors_run_nothing(nav):
    scans = [scan_of(rays(0, f), (1.0, 1.0, 0.0)) for f in range(NF)]
    a = make(nav)                       # no configure_node
    a.request_nomotion_update()
    before = everything(nav, a)
    rc, _ = a.laser_received(scans, raise_on_error=False)
    assert rc == ERR_STATE
    assert_untouched(nav, a, before)
    a.close()
    node = dict(d_thresh=0.2, a_thresh=0.5, resample_interval=2)
    b = make(nav, node=node, maps=NF - 1)   # filter 5 has no map
    before = everything(nav, b)
    rc, _ = b.laser_received(scans, raise_on_error=False)
    assert rc == ERR_STATE
    assert_untouched(nav, b, before)
    rc, res = b.laser_received(scans[:5] + [None])     # without a scan the mapless filter is no obstacle
    assert rc == OK and res.updated.tolist() == [1, 1, 1, 1, 1, 0]
    b.close()
    for missing in ("laser", "odom", "resample"):
        c = nav.AmclLaser(NF, MS, max_beams=MB)
        c.set_map(the_map(), 0.1)
        if missing != "laser":
            c.configure(max_beams=MB)
        if missing != "odom":
            c.configure_odom(ODOM_DIFF)
        if missing != "resample":
            c.configure_resample(min_samples=MINS)
        c.configure_node(**node)
        c.set_samples(cloud(5), np.full((NF, MS), 1.0 / MS))
        before = everything(nav, c)
        rc, _ = c.laser_received(scans, raise_on_error=False)
        assert rc == ERR_STATE, missing
        assert_untouched(nav, c, before)
        c.close()


def test_a_looping_beam_model_fails_only_its_own_filter(nav):
    node = dict(d_thresh=0.2, a_thresh=0.5, resample_interval=2)
    a = make(nav, model=BEAM, node=node)
    twin = make(nav, model=BEAM)
    scans = [scan_of(rays(0, f, 5 if f == 2 else RAYS), (1.0, 1.0, 0.0)) for f in range(NF)]   # 1 <= 5 < max_beams 8
    a.request_nomotion_update(first=2, count=1)
    before = everything(nav, a)
    rc, res = a.laser_received(scans, raise_on_error=False)
    assert rc == ERR_INVALID
    assert res.status.tolist() == [0, 0, ERR_INVALID, 0, 0, 0] and res.updated.tolist() == [1, 1, 0, 1, 1, 1]
    assert_untouched(nav, a, before, filters=[2])
    for f in (0, 1, 3, 4, 5):
        b, rmax = host_laser_data(scans[f], node)
        twin.update_sensor([b], rmax, first=f)
    d1, d2 = dump(nav, a), dump(nav, twin)
    for f in range(NF):
        assert_same_set(d1[f], d2[f], f)
    # an empty scan is no loop (range_count 0): the beam model's `for` does not start
    scans[2]["ranges"] = np.zeros(0, np.float32)
    rc, res = a.laser_received(scans, raise_on_error=False)
    assert rc == OK and res.status[2] == 0 and res.updated[2] == 1
    a.close()
    twin.close()
