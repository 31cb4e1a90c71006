"""An independent restatement of AmclNode's laser cycle, written from amcl/src/amcl_node.cpp with the math module, for the tests
of navgpu_amcl_node_*:

  angle_diff                        :87-106
  integrate_odom                    :1120-1172   AmclNode::integrateOdom
  NodeRef.laser_received            :1381-1440, :1442-1470, :1474-1562 (the decisions; the pf steps are the caller's)
  convert_scan                      :1505-1537   the LaserScan -> AMCLLaserData conversion
  argmax_hypothesis                 :1584-1651   the hypothesis read-out
  map_to_odom / invert_planar       :1678-1708   the planar form of the tf arithmetic

Nothing here calls the library; a float32 value is rounded with struct, as a C float is."""
import math
import struct


def f32(x):
    """x rounded to a C float and widened again"""
    return struct.unpack("f", struct.pack("f", x))[0]


def normalize(z):
    return math.atan2(math.sin(z), math.cos(z))


def angle_diff(a, b):
    a = normalize(a)
    b = normalize(b)
    d1 = a - b
    d2 = 2 * math.pi - math.fabs(d1)
    if d1 > 0:
        d2 *= -1.0
    if math.fabs(d1) < math.fabs(d2):
        return d1
    return d2


class NodeRef:
    """The members AmclNode keeps between scans, for one filter with one laser."""

    def __init__(self, d_thresh, a_thresh, resample_interval, use_odom_integrator=False):
        self.d_thresh, self.a_thresh = d_thresh, a_thresh
        self.resample_interval = resample_interval
        self.use_odom_integrator = use_odom_integrator
        self.pf_init = False
        self.lasers_update = True          # lasers_update_.push_back(true) when the laser is first seen (:1344)
        self.m_force_update = False        # :532
        self.resample_count = 0
        self.pf_odom_pose = [0.0, 0.0, 0.0]
        self.absolute_motion = [0.0, 0.0, 0.0]
        self.integrator_ready = False
        self.integrator_last_pose = [0.0, 0.0, 0.0]
        self.global_localization_active = False
        self.latest_tf_valid = False
        self.latest_tf = [0.0, 0.0, 0.0]

    # applyInitialPose / globalLocalizationCallback, after the init itself
    def reset(self, global_localization=False):
        self.pf_init = False
        self.global_localization_active = bool(global_localization)

    def request_nomotion_update(self):     # :1296-1303
        self.m_force_update = True

    def integrate_odom(self, pose):        # :1120-1172
        pose = [float(v) for v in pose]
        if not self.integrator_ready:
            self.absolute_motion = [0.0, 0.0, 0.0]
            self.integrator_ready = True
        else:
            last = self.integrator_last_pose
            dx = pose[0] - last[0]
            dy = pose[1] - last[1]
            dth = angle_diff(pose[2], last[2])
            delta_trans = math.sqrt(dx * dx + dy * dy)
            delta_rot = dth
            if delta_trans < 1e-6:
                delta_bearing = 0.0
            else:
                delta_bearing = angle_diff(math.atan2(dy, dx), last[2] + delta_rot / 2)
            cs_bearing = math.cos(delta_bearing)
            sn_bearing = math.sin(delta_bearing)
            self.absolute_motion[0] += math.fabs(delta_trans * cs_bearing)
            self.absolute_motion[1] += math.fabs(delta_trans * sn_bearing)
            self.absolute_motion[2] += math.fabs(delta_rot)
        self.integrator_last_pose = pose

    def laser_received(self, pose):
        """One scan with getOdomPose's result `pose`.  -> dict(moved, updated, resampled, force_publication, cloud_due, odom) where
        odom is AMCLOdomData's pose + delta + absolute_motion (9 values) when moved.  What depends on the filter (the
        global-localisation clear, the read-out) is finish()'s."""
        pose = [float(v) for v in pose]
        delta = [0.0, 0.0, 0.0]
        if self.pf_init:                                                    # :1393
            delta[0] = pose[0] - self.pf_odom_pose[0]
            delta[1] = pose[1] - self.pf_odom_pose[1]
            delta[2] = angle_diff(pose[2], self.pf_odom_pose[2])
            if self.use_odom_integrator:
                am = self.absolute_motion
                abs_trans = math.sqrt(am[0] * am[0] + am[1] * am[1])
                abs_rot = am[2]
                update = abs_trans >= self.d_thresh or abs_rot >= self.a_thresh
            else:
                update = (math.fabs(delta[0]) > self.d_thresh or math.fabs(delta[1]) > self.d_thresh or
                          math.fabs(delta[2]) > self.a_thresh)
            update = update or self.m_force_update
            self.m_force_update = False
            if update:
                self.lasers_update = True
        out = dict(moved=False, updated=False, resampled=False, force_publication=False, cloud_due=False, odom=None)
        if not self.pf_init:                                                # :1423
            self.pf_odom_pose = list(pose)
            self.pf_init = True
            self.lasers_update = True
            out["force_publication"] = True
            self.resample_count = 0
            self.integrator_ready = False
        elif self.pf_init and self.lasers_update:                           # :1442
            out["moved"] = True
            out["odom"] = list(pose) + list(delta) + list(self.absolute_motion)
            self.absolute_motion = [0.0, 0.0, 0.0]
        if self.lasers_update:                                              # :1474
            out["updated"] = True
            self.lasers_update = False
            self.pf_odom_pose = list(pose)
            self.resample_count += 1
            if not (self.resample_count % self.resample_interval):          # :1546
                out["resampled"] = True
            out["cloud_due"] = not self.m_force_update                      # :1562
        return out

    def finish(self, step, pose, converged, hyp):
        """The rest of the scan once the filter's steps ran: converged = pf_->converged after the resample, hyp = the read-out
        (max_weight, pose) or None when nothing was read.  -> dict(global_localization_converged, published, republish,
        map_to_odom)"""
        out = dict(global_localization_converged=False, published=False, republish=False, map_to_odom=None)
        if step["resampled"] and converged and self.global_localization_active:   # :1550
            self.global_localization_active = False
            out["global_localization_converged"] = True
        if step["resampled"] or step["force_publication"]:                  # :1584
            if hyp is not None and hyp[0] > 0.0:                            # :1614
                out["published"] = True
                m2o = map_to_odom(hyp[1], pose)
                out["map_to_odom"] = m2o
                self.latest_tf = invert_planar(m2o)
                self.latest_tf_valid = True
        elif self.latest_tf_valid:                                          # :1726
            out["republish"] = True
            out["map_to_odom"] = invert_planar(self.latest_tf)
        return out


def convert_scan(ranges_f32, msg_range_min, msg_range_max, yaw_min, yaw_inc, laser_min_range=-1.0, laser_max_range=-1.0):
    """:1505-1537.  ranges_f32: the message's floats (already float32 values).  -> (AMCLLaserData ranges as a list of
    [range, bearing], AMCLLaserData::range_max)"""
    angle_min = yaw_min
    angle_increment = yaw_inc - angle_min
    angle_increment = math.fmod(angle_increment + 5 * math.pi, 2 * math.pi) - math.pi
    if laser_max_range > 0.0:
        range_max = min(f32(msg_range_max), f32(laser_max_range))
    else:
        range_max = f32(msg_range_max)
    if laser_min_range > 0.0:
        range_min = max(f32(msg_range_min), f32(laser_min_range))
    else:
        range_min = f32(msg_range_min)
    out = []
    for i, r in enumerate(ranges_f32):
        r = float(r)
        if r <= range_min:
            rng = range_max
        else:
            rng = r
        out.append([rng, angle_min + (i * angle_increment)])
    return out, range_max


def argmax_hypothesis(weights, means):
    """:1587-1612: the first cluster whose weight is strictly above every earlier one's and above 0 -> (max_weight,
    max_weight_hyp, mean or None)"""
    max_weight, max_weight_hyp = 0.0, -1
    for k, w in enumerate(weights):
        if w > max_weight:
            max_weight, max_weight_hyp = float(w), k
    return max_weight, max_weight_hyp, (None if max_weight_hyp < 0 else [float(v) for v in means[max_weight_hyp]])


def map_to_odom(h, o):
    """latest_tf_.inverse() of :1678-1708 in the plane: (map -> base) composed with the inverse of (odom -> base)"""
    th = h[2] - o[2]
    c, s = math.cos(th), math.sin(th)
    return [h[0] - (c * o[0] - s * o[1]), h[1] - (s * o[0] + c * o[1]), th]


def invert_planar(t):
    """the inverse of the planar transform {x, y, theta}"""
    c, s = math.cos(t[2]), math.sin(t[2])
    return [-(c * t[0] + s * t[1]), -(-s * t[0] + c * t[1]), -t[2]]
