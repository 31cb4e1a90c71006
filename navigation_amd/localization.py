"""AmclLaser: thin Python handle over navgpu_amcl_* — amcl's laser sensor update for a batch of particle filters on one GPU.

  set_map            AmclNode::convertMap + map_update_cspace      (amcl_node.cpp:1062-1093, map_cspace.cpp)
  set_map_cells      the same from a map_t's occ_state / scale / origin as they stand
  set_distance_map   map_t::distances as computed elsewhere (e.g. the reference's own map_update_cspace)
  configure          AMCLLaser::SetModel* / SetMapFactors, pf_alloc's alpha_slow / alpha_fast
  update_sensor      AMCLLaser::UpdateSensor -> pf_update_sensor    (amcl_laser.cpp:160-236, pf.c:270-316)
  configure_resample pf_set_resample_model and pf_alloc's KLD / convergence parameters
  update_resample    pf_update_resample: resampling, kd-tree histogram, pf_cluster_stats, pf_update_converged (pf.c:222-720)
  clusters           pf_get_cluster_stats / the set's cluster_count and mean / cov
  configure_odom     AMCLOdom::SetModel*                              (amcl_odom.cpp:68-125)
  update_action      AMCLOdom::UpdateAction -> pf_update_action: the odometry motion model (amcl_odom.cpp:128-379)
  init_gaussian      pf_init: a Gaussian set                             (pf.c:138-176)
  init_uniform       pf_init_model with AmclNode::uniformPoseGenerator (global localisation, amcl_node.cpp:1200-1263)
  configure_node     AmclNode's update_min_d / update_min_a / resample_interval / laser range overrides / odom integrator
  laser_received     AmclNode::laserReceived for the fleet, one call per scan                (amcl_node.cpp:1381-1756)
  hypotheses         the hypothesis read-out alone                                           (amcl_node.cpp:1584-1651)
  node_reset, request_nomotion_update, integrate_odom, node_state, set_node_state: the node's state between scans
All compute happens in libnavgpu.so on the GPU; this file only marshals numpy buffers.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from ._lib import (AMCL_DRAW_DEVICE, AMCL_DRAW_DRAND48, AMCL_DRAW_SUPPLIED, AMCL_RESAMPLE_SYSTEMATIC, AMCL_SCAN_PRESENT, AmclLaserParams,
                   AmclNodeParams, AmclNodeResult, AmclNodeState, AmclOdomParams, AmclResampleParams, AmclScan, AmclUniformParams, check,
                   lib)

# pf_sample_set_t's clusters and overall statistics: count (C,), weight (C,), mean (C, 3), cov (C, 3, 3), set_mean (3,), set_cov (3, 3)
AmclClusters = namedtuple("AmclClusters", "count weight mean cov set_mean set_cov")
# numpy layouts of navgpu_amcl_node_result / navgpu_amcl_node_state, taken from their ctypes mirrors
NODE_RESULT_DTYPE = np.dtype(AmclNodeResult)
NODE_STATE_DTYPE = np.dtype(AmclNodeState)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def drand48_state(seed):
    """drand48's 48-bit state after srand48(seed): the low 32 bits of seed, then 0x330E."""
    return ((int(seed) & 0xFFFFFFFF) << 16) | 0x330E


class AmclLaser:
    def __init__(self, n_filters, max_samples, max_beams=30, device=0):
        self.L = lib()
        self.n, self.max_samples, self.max_beams = n_filters, max_samples, max_beams
        h = C.c_void_p()
        check(self.L.navgpu_amcl_create(n_filters, max_samples, max_beams, device, C.byref(h)), "navgpu_amcl_create")
        self.h = h
        self.map_shape = [None] * n_filters

    def close(self):
        if getattr(self, "h", None):
            self.L.navgpu_amcl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _count(self, first, count):
        return (self.n - first) if count is None else count

    def set_map(self, occupancy, resolution, origin_xy=(0.0, 0.0), max_occ_dist=2.0, scale_up_factor=1, first=0, count=None):
        """occupancy: OccupancyGrid data (height, width) int8 shared by `count` filters, or (count, height, width)."""
        a = np.ascontiguousarray(occupancy, np.int8)
        shared = a.ndim == 2
        count = self._count(first, count)
        if not shared:
            assert a.shape[0] == count
        h, w = a.shape[-2:]
        org = np.ascontiguousarray(origin_xy, np.float64)
        check(self.L.navgpu_amcl_set_map(self.h, first, count, _p(a), w, h, float(resolution), _p(org), int(scale_up_factor), int(shared),
                                         float(max_occ_dist)), "amcl_set_map")
        for k in range(first, first + count):
            self.map_shape[k] = (h * scale_up_factor, w * scale_up_factor)

    def set_map_cells(self, occ_state, scale, origin_xy, max_occ_dist=2.0, first=0, count=None):
        """occ_state: map_t occ_state values (size_y, size_x) shared by `count` filters, or (count, size_y, size_x); origin_xy: map_t's
        origin_x / origin_y (the map centre)."""
        a = np.ascontiguousarray(occ_state, np.int8)
        shared = a.ndim == 2
        count = self._count(first, count)
        if not shared:
            assert a.shape[0] == count
        sy, sx = a.shape[-2:]
        check(self.L.navgpu_amcl_set_map_cells(self.h, first, count, _p(a), sx, sy, float(scale), float(origin_xy[0]), float(origin_xy[1]),
                                               int(shared), float(max_occ_dist)), "amcl_set_map_cells")
        for k in range(first, first + count):
            self.map_shape[k] = (sy, sx)

    def set_distance_map(self, distances, first=0, count=None):
        """distances: (size_y, size_x) float32 for every filter of the slice, or (count, size_y, size_x)."""
        a = np.ascontiguousarray(distances, np.float32)
        count = self._count(first, count)
        shared = a.ndim == 2
        check(self.L.navgpu_amcl_set_distance_map(self.h, first, count, _p(a), int(shared)), "amcl_set_distance_map")

    def distance_map(self, filter=0):
        out = np.zeros(self.map_shape[filter], np.float32)
        check(self.L.navgpu_amcl_distance_map(self.h, filter, _p(out)), "amcl_distance_map")
        return out

    def configure(self, params=None, **kw):
        p = params if params is not None else AmclLaserParams(**kw)
        check(self.L.navgpu_amcl_laser_configure(self.h, C.byref(p)), "amcl_laser_configure")
        return p

    def set_laser_pose(self, xyth, first=0):
        a = np.ascontiguousarray(xyth, np.float64).reshape(-1, 3)
        check(self.L.navgpu_amcl_set_laser_pose(self.h, first, len(a), _p(a)), "amcl_set_laser_pose")

    def set_samples(self, poses, weights, sample_counts=None, converged=None, first=0):
        """poses: (count, max_samples, 3) or (count, n, 3) with n <= max_samples; weights likewise (count, n)."""
        poses = np.asarray(poses, np.float64)
        count, n = poses.shape[0], poses.shape[1]
        if n > self.max_samples:
            raise ValueError(f"{n} samples per filter > max_samples {self.max_samples}")
        P = np.zeros((count, self.max_samples, 3))
        W = np.zeros((count, self.max_samples))
        P[:, :n] = poses
        W[:, :n] = np.asarray(weights, np.float64).reshape(count, n)
        sc = np.ascontiguousarray(np.full(count, n) if sample_counts is None else sample_counts, np.int32)
        cv = np.ascontiguousarray(np.zeros(count) if converged is None else converged, np.int32)
        check(self.L.navgpu_amcl_set_samples(self.h, first, count, _p(sc), _p(P), _p(W), _p(cv)), "amcl_set_samples")

    def get_samples(self, first=0, count=None):
        """-> (sample_counts, poses (count, max_samples, 3), weights (count, max_samples), converged)"""
        count = self._count(first, count)
        sc = np.zeros(count, np.int32)
        cv = np.zeros(count, np.int32)
        P = np.zeros((count, self.max_samples, 3))
        W = np.zeros((count, self.max_samples))
        check(self.L.navgpu_amcl_get_samples(self.h, first, count, _p(sc), _p(P), _p(W), _p(cv)), "amcl_get_samples")
        return sc, P, W, cv

    def set_filter_state(self, w_slow_fast, first=0):
        a = np.ascontiguousarray(w_slow_fast, np.float64).reshape(-1, 2)
        check(self.L.navgpu_amcl_set_filter_state(self.h, first, len(a), _p(a)), "amcl_set_filter_state")

    def get_filter_state(self, first=0, count=None):
        count = self._count(first, count)
        a = np.zeros((count, 2))
        check(self.L.navgpu_amcl_get_filter_state(self.h, first, count, _p(a)), "amcl_get_filter_state")
        return a

    def update_sensor(self, scans, range_max, first=0, raise_on_error=True):
        """scans: a list of (range_count, 2) arrays {range, bearing}, one per filter of the slice; range_max: scalar or per filter.
        -> (status, updated[count])"""
        count = len(scans)
        rc_ = np.ascontiguousarray([len(s) for s in scans], np.uint32)
        flat = [np.asarray(s, np.float64).reshape(-1, 2) for s in scans]
        xy = np.ascontiguousarray(np.concatenate(flat) if rc_.sum() else np.zeros((1, 2)), np.float64)
        rm = np.ascontiguousarray(np.broadcast_to(np.asarray(range_max, np.float64), (count,)))
        upd = np.zeros(count, np.int32)
        st = self.L.navgpu_amcl_update_sensor(self.h, first, count, _p(xy), _p(rc_), _p(rm), _p(upd))
        if raise_on_error:
            check(st, "amcl_update_sensor")
        return st, upd

    def beam_skip_state(self, filter=0):
        """-> (obs_count[max_beams], obs_mask[max_beams], error, active) of the last update"""
        oc = np.zeros(self.max_beams, np.int32)
        om = np.zeros(self.max_beams, np.uint8)
        err, act = C.c_int32(), C.c_int32()
        check(self.L.navgpu_amcl_beam_skip_state(self.h, filter, _p(oc), _p(om), C.byref(err), C.byref(act)), "amcl_beam_skip_state")
        return oc, om.astype(bool), err.value, act.value

    def configure_resample(self, params=None, **kw):
        """navgpu_amcl_resample_params fields: resample_model, min_samples, pop_err, pop_z, dist_threshold."""
        p = params if params is not None else AmclResampleParams(**kw)
        check(self.L.navgpu_amcl_resample_configure(self.h, C.byref(p)), "amcl_resample_configure")
        self.resample_params = p
        return p

    def update_resample(self, draws=None, seed=None, first=0, count=None, raise_on_error=True):
        """draws=None: the device generator with `seed`.  Supplied draws, a dict for the `count` filters of the slice:
          u:                (count, n_u, 2) {u_flag, u_pick} per candidate (multinomial; padded to max_samples with 1.0, i.e.
                            never random and never a valid pick - pad generously, the KLD limit stops early);
          systematic_start: (count,) (systematic);
          random_poses:     a list of (k_i, 3) pools, one per filter, consumed in order.
        -> (status, status[count])"""
        count = self._count(first, count) if draws is None else len(draws["random_poses"])
        st = np.zeros(count, np.int32)
        if draws is None:
            rc = self.L.navgpu_amcl_update_resample(self.h, first, count, AMCL_DRAW_DEVICE, None, None, None, None,
                                                    int(0 if seed is None else seed) & (2 ** 64 - 1), _p(st))
        else:
            pools = [np.asarray(q, np.float64).reshape(-1, 3) for q in draws["random_poses"]]
            pc = np.ascontiguousarray([len(q) for q in pools], np.uint32)
            pool = np.ascontiguousarray(np.concatenate(pools) if pc.sum() else np.zeros((1, 3)))
            u = np.ones((count, self.max_samples, 2))
            if draws.get("u") is not None:
                uu = np.asarray(draws["u"], np.float64).reshape(count, -1, 2)
                u[:, :uu.shape[1]] = uu[:, :self.max_samples]
            ss = np.ascontiguousarray(np.broadcast_to(np.asarray(draws.get("systematic_start", 0.0), np.float64), (count,)))
            rc = self.L.navgpu_amcl_update_resample(self.h, first, count, AMCL_DRAW_SUPPLIED, _p(u), _p(ss), _p(pool), _p(pc), 0, _p(st))
        if raise_on_error:
            check(rc, "amcl_update_resample")
        return rc, st

    def clusters(self, filter=0):
        """-> AmclClusters of the filter's current set after a resample (clusters numbered by their lowest sample index)."""
        n = C.c_int32()
        rc = self.L.navgpu_amcl_get_clusters(self.h, filter, C.byref(n), 0, None, None, None, None, None, None)
        if rc < 0 and n.value <= 0:
            check(rc, "amcl_get_clusters")
        k = n.value
        cnt, w = np.zeros(k, np.int32), np.zeros(k)
        mean, cov = np.zeros((k, 3)), np.zeros((k, 3, 3))
        sm, sc = np.zeros(3), np.zeros((3, 3))
        check(self.L.navgpu_amcl_get_clusters(self.h, filter, C.byref(n), k, _p(cnt), _p(w), _p(mean), _p(cov), _p(sm), _p(sc)),
              "amcl_get_clusters")
        return AmclClusters(cnt, w, mean, cov, sm, sc)

    def kd_leaf_counts(self, first=0, count=None):
        count = self._count(first, count)
        a = np.zeros(count, np.int32)
        check(self.L.navgpu_amcl_get_kd_leaf_counts(self.h, first, count, _p(a)), "amcl_get_kd_leaf_counts")
        return a

    def set_kd_leaf_counts(self, leaf_counts, first=0):
        a = np.ascontiguousarray(leaf_counts, np.int32).ravel()
        check(self.L.navgpu_amcl_set_kd_leaf_counts(self.h, first, len(a), _p(a)), "amcl_set_kd_leaf_counts")

    def rng_counters(self, first=0, count=None):
        count = self._count(first, count)
        a = np.zeros(count, np.uint64)
        check(self.L.navgpu_amcl_get_rng_counters(self.h, first, count, _p(a)), "amcl_get_rng_counters")
        return a

    def set_rng_counters(self, counters, first=0):
        a = np.ascontiguousarray(counters, np.uint64).ravel()
        check(self.L.navgpu_amcl_set_rng_counters(self.h, first, len(a), _p(a)), "amcl_set_rng_counters")

    def configure_odom(self, model, alpha1=0.2, alpha2=0.2, alpha3=0.2, alpha4=0.2, alpha5=0.2):
        """AMCLOdom::SetModel(model, alpha1..alpha5); model: AMCL_ODOM_* (odom_model_t)."""
        p = AmclOdomParams(model_type=int(model), alpha1=alpha1, alpha2=alpha2, alpha3=alpha3, alpha4=alpha4, alpha5=alpha5)
        check(self.L.navgpu_amcl_odom_configure(self.h, C.byref(p)), "amcl_odom_configure")
        self.odom_params = p
        return p

    def update_action(self, odom, drand48_state=None, seed=None, first=0, raise_on_error=True):
        """odom: (count, 9) {pose[3], delta[3], absolute_motion[3]} per filter of the slice (AMCLOdomData).
        drand48_state: (count,) 48-bit states, the reference's drand48() stream (parity); otherwise the device generator with `seed`.
        -> (status, status[count], the advanced drand48 states or None)"""
        o = np.ascontiguousarray(odom, np.float64).reshape(-1, 9)
        count = len(o)
        st = np.zeros(count, np.int32)
        if drand48_state is not None:
            x = np.array(np.broadcast_to(np.asarray(drand48_state, np.uint64), (count,)))  # a copy: the caller's states stay as given
            rc = self.L.navgpu_amcl_update_action(self.h, first, count, _p(o), AMCL_DRAW_DRAND48, _p(x), 0, _p(st))
        else:
            x = None
            rc = self.L.navgpu_amcl_update_action(self.h, first, count, _p(o), AMCL_DRAW_DEVICE, None,
                                                  int(0 if seed is None else seed) & (2 ** 64 - 1), _p(st))
        if raise_on_error:
            check(rc, "amcl_update_action")
        return rc, st, x

    def init_gaussian(self, mean, cov, drand48_state=None, seed=None, first=0, count=None, raise_on_error=True):
        """pf_init(pf, mean, cov) for every filter of the slice.  mean: (3,) or (count, 3); cov: (3, 3) or (count, 3, 3).
        drand48_state: (count,) 48-bit states (parity: (pf_pdf_seed << 16) | 0x330E); otherwise the device generator with `seed`.
        -> (status, status[count], the advanced drand48 states or None)"""
        count = self._count(first, count)
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(mean, np.float64).reshape(-1, 3), (count, 3)))
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(cov, np.float64).reshape(-1, 9), (count, 9)))
        st = np.zeros(count, np.int32)
        x, src, sd = self._draws(drand48_state, seed, count)
        rc = self.L.navgpu_amcl_init_gaussian(self.h, first, count, _p(m), _p(c), src, None if x is None else _p(x), sd, _p(st))
        if raise_on_error:
            check(rc, "amcl_init_gaussian")
        return rc, st, x

    def init_uniform(self, scans=None, range_max=None, threshold=0.0, deweight_multiplier=0.0, max_candidates=0, drand48_state=None,
                     seed=None, first=0, count=None, raise_on_error=True):
        """pf_init_model(pf, uniformPoseGenerator) for every filter of the slice.  scans: None (no scan yet) or a list of
        (range_count, 2) arrays {range, bearing} per filter, with range_max (scalar or per filter), as update_sensor takes them.
        threshold / deweight_multiplier: uniform_pose_starting_weight_threshold / uniform_pose_deweight_multiplier (amcl_node's
        defaults 0 and 0: no scoring).  -> (status, status[count], the advanced drand48 states or None, candidates_used[count])"""
        count = self._count(first, count) if scans is None else len(scans)
        p = AmclUniformParams(starting_weight_threshold=threshold, deweight_multiplier=deweight_multiplier,
                              max_candidates=int(max_candidates))
        st = np.zeros(count, np.int32)
        used = np.zeros(count, np.uint64)
        x, src, sd = self._draws(drand48_state, seed, count)
        flat = rc_ = rm = None
        if scans is not None:
            rc_ = np.ascontiguousarray([len(s) for s in scans], np.uint32)
            parts = [np.asarray(s, np.float64).reshape(-1, 2) for s in scans]
            flat = np.ascontiguousarray(np.concatenate(parts) if rc_.sum() else np.zeros((1, 2)))
            rm = np.ascontiguousarray(np.broadcast_to(np.asarray(range_max, np.float64), (count,)))
        rc = self.L.navgpu_amcl_init_uniform(self.h, first, count, C.byref(p), None if flat is None else _p(flat),
                                             None if rc_ is None else _p(rc_), None if rm is None else _p(rm), src,
                                             None if x is None else _p(x), sd, _p(used), _p(st))
        if raise_on_error:
            check(rc, "amcl_init_uniform")
        return rc, st, x, used

    # ---- AmclNode::laserReceived for the fleet (navgpu_amcl_node_*) ----
    def configure_node(self, params=None, **kw):
        """navgpu_amcl_node_params fields: d_thresh, a_thresh, laser_min_range, laser_max_range, resample_interval,
        use_odom_integrator."""
        p = params if params is not None else AmclNodeParams(**kw)
        check(self.L.navgpu_amcl_node_configure(self.h, C.byref(p)), "amcl_node_configure")
        self.node_params = p
        return p

    def laser_received(self, scans, seed=0, first=0, raise_on_error=True):
        """AmclNode::laserReceived for the filters first .. first + len(scans) - 1.  scans: one entry per filter, None (no scan for
        this filter in this call) or a dict with ranges (the raw LaserScan::ranges), range_min, range_max, yaw_min, yaw_inc (the two
        tf::getYaw results of amcl_node.cpp:1505-1506) and odom_pose (x, y, yaw).
        -> (status, a numpy record array with navgpu_amcl_node_result's fields, one record per filter)"""
        count = len(scans)
        recs = (AmclScan * count)()
        parts, off = [], 0
        for k, s in enumerate(scans):
            if s is None:
                continue
            r = np.ascontiguousarray(s["ranges"], np.float32).ravel()
            recs[k].flags = AMCL_SCAN_PRESENT
            recs[k].range_count = len(r)
            recs[k].range_offset = off
            recs[k].range_min = s["range_min"]
            recs[k].range_max = s["range_max"]
            recs[k].yaw_min = s["yaw_min"]
            recs[k].yaw_inc = s["yaw_inc"]
            recs[k].odom_pose = tuple(float(v) for v in s["odom_pose"])
            parts.append(r)
            off += len(r)
        raw = np.ascontiguousarray(np.concatenate(parts) if off else np.zeros(1), np.float32)
        out = np.zeros(count, NODE_RESULT_DTYPE)
        rc = self.L.navgpu_amcl_node_laser_received(self.h, first, count, C.byref(recs), _p(raw), int(seed) & (2 ** 64 - 1), _p(out))
        if raise_on_error:
            check(rc, "amcl_node_laser_received")
        return rc, out.view(np.recarray)

    def hypotheses(self, first=0, count=None):
        """The hypothesis read-out (amcl_node.cpp:1584-1651) of every filter of the slice, from the clusters the last resample or
        init left -> a numpy record array (cluster_count, max_weight_hyp, max_weight, published, pose, cov_*, sample_count,
        converged; the other fields 0)."""
        count = self._count(first, count)
        out = np.zeros(count, NODE_RESULT_DTYPE)
        check(self.L.navgpu_amcl_hypotheses(self.h, first, count, _p(out)), "amcl_hypotheses")
        return out.view(np.recarray)

    def node_reset(self, global_localization=False, first=0, count=None):
        """After an init the caller made itself: pf_init_ = false, global_localization_active_ = global_localization."""
        check(self.L.navgpu_amcl_node_reset(self.h, first, self._count(first, count), int(bool(global_localization))), "amcl_node_reset")

    def request_nomotion_update(self, first=0, count=None):
        check(self.L.navgpu_amcl_node_request_nomotion_update(self.h, first, self._count(first, count)),
              "amcl_node_request_nomotion_update")

    def integrate_odom(self, poses, first=0):
        """AmclNode::integrateOdom for one odometry message per filter of the slice; poses: (count, 3) {x, y, yaw}."""
        a = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        check(self.L.navgpu_amcl_node_integrate_odom(self.h, first, len(a), _p(a)), "amcl_node_integrate_odom")

    def node_state(self, first=0, count=None):
        """-> a numpy record array with navgpu_amcl_node_state's fields, one record per filter (a copy)"""
        count = self._count(first, count)
        out = np.zeros(count, NODE_STATE_DTYPE)
        check(self.L.navgpu_amcl_node_get_state(self.h, first, count, _p(out)), "amcl_node_get_state")
        return out.view(np.recarray)

    def set_node_state(self, states, first=0):
        a = np.ascontiguousarray(states, NODE_STATE_DTYPE).ravel()
        check(self.L.navgpu_amcl_node_set_state(self.h, first, len(a), _p(a)), "amcl_node_set_state")

    @staticmethod
    def _draws(drand48_state, seed, count):
        """update_action's draw-source handling -> (a copy of the states or None, draw_source, seed)"""
        if drand48_state is not None:
            return np.array(np.broadcast_to(np.asarray(drand48_state, np.uint64), (count,))), AMCL_DRAW_DRAND48, 0
        return None, AMCL_DRAW_DEVICE, int(0 if seed is None else seed) & (2 ** 64 - 1)
