"""numpy restatement of costmap_2d::ObservationBuffer as include/navgpu.h states it for navgpu_obsbuf_*: the list, the purge,
isCurrent, the scan projection, the cloud transform, the height filter and setGlobalFrame - float32 arithmetic in the stated
order (every numpy operation below is one rounding: nothing is fused), int64 times.

The trig of a scan's beams is an argument (`trig(angles) -> (sin, cos)`, float64 arrays): tests/test_gpu_obs_buffer.py passes
what navgpu_device_sincos returns, tests/test_obs_buffer_host.py the host's libm.

costmap_2d/src/observation_buffer.cpp: bufferCloud :129-195, getObservations :198-209, purgeStaleObservations :211-236,
isCurrent :238-251, setGlobalFrame :66-109; plugins/obstacle_layer.cpp:281-289 for the inf rule."""
import math

import numpy as np

F32 = np.float32
IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
DEFAULTS = dict(observation_keep_time_ns=0, expected_update_rate_ns=0, min_obstacle_height=0.0, max_obstacle_height=2.0,
                obstacle_range=2.5, raytrace_range=3.0, flags=3, inf_is_valid=0)


def host_trig(angles):
    """sin / cos of float64 angles with the host's libm, one call per angle (math.sin / math.cos)."""
    a = np.asarray(angles, np.float64)
    return np.array([math.sin(v) for v in a], np.float64), np.array([math.cos(v) for v in a], np.float64)


def transform_cloud(m12, pts):
    """x' = ((m00*x + m01*y) + m02*z) + m03 in fp32, the 12 doubles narrowed first; likewise y', z'."""
    m = np.asarray(m12, np.float64).ravel().astype(F32)
    p = np.asarray(pts, F32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + m[9 + r]
    return out


def height_filter(pts, min_h, max_h):
    """keep iff (double)z <= max && (double)z >= min, order preserved; NaN drops"""
    z = pts[:, 2].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return pts[(z <= max_h) & (z >= min_h)]


def project_scan(ranges, angle_min, angle_increment, range_min, range_max, inf_is_valid, trig):
    """laser_geometry's projectLaser as restated: (points (k, 3) float32 of the kept beams in beam order, their beam indices)."""
    r = np.asarray(ranges, F32).copy()
    range_min, range_max = F32(range_min), F32(range_max)
    if inf_is_valid:
        with np.errstate(invalid="ignore"):
            fix = ~np.isfinite(r) & (r > 0)
        r[fix] = range_max - F32(0.0001)
    with np.errstate(invalid="ignore"):
        keep = (r >= range_min) & (r < range_max)
    idx = np.nonzero(keep)[0]
    a = np.float64(F32(angle_min)) + idx.astype(np.float64) * np.float64(F32(angle_increment))
    sn, cs = trig(a)
    rk = r[idx].astype(np.float64)
    pts = np.zeros((len(idx), 3), F32)
    pts[:, 0] = (rk * cs).astype(F32)
    pts[:, 1] = (rk * sn).astype(F32)
    return pts, idx


class RefList:
    """one ObservationBuffer: observation_list_ (newest first) and last_updated_"""

    def __init__(self, params):
        self.p = dict(DEFAULTS)
        self.p.update(params)
        self.entries = []
        self.last_updated = 0

    def purge(self):
        if not self.entries:
            return
        keep = self.p["observation_keep_time_ns"]
        if keep == 0:
            del self.entries[1:]
            return
        for k, e in enumerate(self.entries):
            if self.last_updated - e["stamp"] > keep:
                del self.entries[k:]
                return

    def buffer(self, cloud, now, trig):
        if "ranges" in cloud:
            pts, _ = project_scan(cloud["ranges"], cloud["angle_min"], cloud["angle_increment"], cloud["range_min"], cloud["range_max"],
                                  self.p["inf_is_valid"], trig)
            n = len(np.asarray(cloud["ranges"]).ravel())
        else:
            pts = np.asarray(cloud["points"], F32).reshape(-1, 3)
            n = len(pts)
        pts = height_filter(transform_cloud(cloud.get("transform", IDENTITY), pts), self.p["min_obstacle_height"], self.p["max_obstacle_height"])
        self.entries.insert(0, dict(stamp=int(cloud["stamp_ns"]), origin=np.array(cloud.get("origin", (0.0, 0.0, 0.0)), np.float64),
                                    points=pts, n_unfiltered=n))
        self.last_updated = int(now)
        self.purge()

    def is_current(self, now):
        rate = self.p["expected_update_rate_ns"]
        return rate == 0 or int(now) - self.last_updated <= rate

    def set_global_frame(self, m12):
        m = np.asarray(m12, np.float64).ravel()
        for e in self.entries:
            x, y, z = e["origin"]
            e["origin"] = np.array([((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + m[9 + r] for r in range(3)], np.float64)
            e["points"] = transform_cloud(m, e["points"])


class RefObsBuf:
    """the buffers of a fleet: [robot][source], each bounded by `slots` (the stated departure: the oldest entry is evicted)"""

    def __init__(self, n_robots, sources, slots, trig=host_trig):
        self.lists = [[RefList(s) for s in sources] for _ in range(n_robots)]
        self.slots = slots
        self.trig = trig
        self.evicted = [0] * n_robots

    def buffer(self, clouds, now):
        for c in clouds:
            l = self.lists[c["instance"]][c.get("source", 0)]
            l.buffer(c, now, self.trig)
            if len(l.entries) > self.slots:
                l.entries.pop()
                self.evicted[c["instance"]] += 1

    def observations(self, robot):
        """getObservations of every source, sources in order, each newest first: what a cycle is staged with"""
        out = []
        for l in self.lists[robot]:
            l.purge()
            for e in l.entries:
                out.append(dict(instance=robot, points=e["points"], origin=tuple(e["origin"]), obstacle_range=l.p["obstacle_range"],
                                raytrace_range=l.p["raytrace_range"], flags=l.p["flags"], marking=bool(l.p["flags"] & 1),
                                clearing=bool(l.p["flags"] & 2), n_unfiltered=e["n_unfiltered"]))
        return out

    def current(self, robot, now):
        return all(l.is_current(now) for l in self.lists[robot])

    def set_global_frame(self, m12, robots=None):
        for r in (range(len(self.lists)) if robots is None else robots):
            for l in self.lists[r]:
                l.set_global_frame(m12)

    def reset_last_updated(self, now, robots=None):
        for r in (range(len(self.lists)) if robots is None else robots):
            for l in self.lists[r]:
                l.last_updated = int(now)
