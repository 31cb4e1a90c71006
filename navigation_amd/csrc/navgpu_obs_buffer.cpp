// C-ABI host side of costmap_2d::ObservationBuffer on the device (include/navgpu.h, navgpu_obsbuf_*).
// The host keeps what the reference keeps per buffer besides the points - the time-ordered list (stamp, origin, which ring
// slot), last_updated_, the purge and isCurrent rules, all exact int64 comparisons - and queues the kernels of
// obs_buffer_kernels.hip on the fleet's stream for everything that touches a point.  Ring slots are reused only behind
// launches already queued on that stream, so no call here waits for the device except the read-backs.
#include "navgpu_fleet.h"

namespace {

using ObsBuf = navgpu_fleet::ObsBuf;
constexpr uint32_t kUnplaced = 0xFFFFFFFFu;  // slot of an entry whose cloud is part of the running navgpu_obsbuf_buffer call

bool finiteAll(const double* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// ObservationBuffer::purgeStaleObservations (observation_buffer.cpp:211-236): how many entries, from the front, it leaves
size_t keptAfterPurge(const std::deque<ObsBuf::Entry>& l, int64_t last_updated, int64_t keep_time) {
  if (l.empty()) return 0;
  if (keep_time == 0) return 1;
  for (size_t k = 0; k < l.size(); ++k)
    if (last_updated - l[k].stamp > keep_time) return k;
  return l.size();
}

// ObservationBuffer::isCurrent (:238-251) of every source of a robot.  The reference compares the two durations as seconds
// in double; for nanosecond counts below 2^53 that is the integer comparison.
int32_t robotCurrent(const ObsBuf& ob, uint32_t inst, int64_t now) {
  for (uint32_t s = 0; s < ob.n_sources; ++s) {
    const int64_t rate = ob.src[s].expected_update_rate_ns;
    if (rate != 0 && now - ob.lists[(size_t)inst * ob.n_sources + s].last_updated > rate) return 0;
  }
  return 1;
}

// room for a call's hand-over in the pinned block and its device twin; the old pair is let go once nothing queued reads it
int reserveInput(navgpu_fleet* f, size_t bytes) {
  ObsBuf& ob = f->ob;
  if (bytes <= ob.in_bytes) return NAVGPU_OK;
  size_t cap = std::max<size_t>(ob.in_bytes, (size_t)1 << 16);
  while (cap < bytes) cap *= 2;
  uint8_t *d = nullptr, *h = nullptr;
  int rc = f->alloc(&d, cap);
  if (rc) return rc;
  if ((rc = f->allocPinned(&h, cap))) {
    f->release(d);
    return rc;
  }
  HIP_TRY(waitStream(f->stream));
  f->release(ob.d_in);
  f->releasePinned(ob.h_in);
  ob.d_in = d;
  ob.h_in = h;
  ob.in_bytes = cap;
  return NAVGPU_OK;
}

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// the pinned block is free again, then `bytes` of it go to the device twin
int waitInput(navgpu_fleet* f) {
  HIP_TRY(f->waitMirrors(f->ob.ev_h2d, f->ob.ev_set));
  return NAVGPU_OK;
}
int sendInput(navgpu_fleet* f, size_t bytes) {
  ObsBuf& ob = f->ob;
  HIP_TRY(hipMemcpyAsync(ob.d_in, ob.h_in, bytes, hipMemcpyHostToDevice, f->stream));
  if (f->cycles_in_flight > 1) {
    HIP_TRY(hipEventRecord(ob.ev_h2d, f->stream));
    ob.ev_set = true;
  }
  return NAVGPU_OK;
}

// what getObservations would return for a robot: (source, entry) of every list after its purge, sources in configuration order,
// each newest first.  Works on copies: the lists change only when the caller commits.
struct Kept {
  uint32_t source;
  ObsBuf::Entry e;
};
void keptOf(const ObsBuf& ob, uint32_t inst, std::vector<Kept>& out, std::vector<std::deque<ObsBuf::Entry>>* purged) {
  for (uint32_t s = 0; s < ob.n_sources; ++s) {
    const ObsBuf::List& l = ob.lists[(size_t)inst * ob.n_sources + s];
    std::deque<ObsBuf::Entry> c = l.entries;
    c.resize(keptAfterPurge(c, l.last_updated, ob.src[s].observation_keep_time_ns));
    for (const auto& e : c) out.push_back({s, e});
    if (purged) purged->push_back(std::move(c));
  }
}


// The kept entries of a set's robots, on copies, and what their lists look like after the purge; the host knows the clouds' unfiltered
// sizes only, so those bound the capacity.  Changes nothing.
struct KeptSet {
  std::vector<std::vector<Kept>> kept;             // [robot of the set]
  std::vector<std::deque<ObsBuf::Entry>> purged;   // [robot of the set][source]
};
int keptOfSet(const navgpu_fleet* f, const RobotSet& set, KeptSet& ks) {
  const ObsBuf& ob = f->ob;
  ks.kept.assign(set.count, {});
  ks.purged.clear();
  ks.purged.reserve((size_t)set.count * ob.n_sources);
  for (uint32_t li = 0; li < set.count; ++li) {
    keptOf(ob, set[li], ks.kept[li], &ks.purged);
    uint64_t upper = 0;
    for (const Kept& k : ks.kept[li]) upper += k.e.n;
    if (ks.kept[li].size() > f->cm.max_obs || upper > f->cm.max_points) return NAVGPU_ERR_CAPACITY;
  }
  return NAVGPU_OK;
}
// The commit of a stage call: the purged lists, last_now, isCurrent per robot of the set, and - once the pinned mirrors are free - the
// set's descriptors with the ring slot of each in `pad`; its obs_consumed flags fall.
int stageKept(navgpu_fleet* f, const RobotSet& set, KeptSet& ks, int64_t now, int32_t* current_out) {
  ObsBuf& ob = f->ob;
  const CostmapDev& cm = f->cm;
  ob.last_now = now;
  for (uint32_t li = 0; li < set.count; ++li)
    for (uint32_t s = 0; s < ob.n_sources; ++s) ob.lists[(size_t)set[li] * ob.n_sources + s].entries.swap(ks.purged[(size_t)li * ob.n_sources + s]);
  if (current_out)
    for (uint32_t li = 0; li < set.count; ++li) current_out[li] = robotCurrent(ob, set[li], now);
  HIP_TRY(f->waitMirrors(f->ev_cm_h2d, f->ev_cm_set));  // the pinned mirrors may still feed an earlier copy
  for (uint32_t li = 0; li < set.count; ++li) {
    const uint32_t i = set[li];
    f->obs_consumed[i] = 0;
    f->hp_cnt[i] = (uint32_t)ks.kept[li].size();
    f->hp_used[i] = 0;
    for (size_t k = 0; k < ks.kept[li].size(); ++k) {
      const Kept& kp = ks.kept[li][k];
      const navgpu_obs_source_params& sp = ob.src[kp.source];
      ObsCsr& d = f->hp_obs[(size_t)i * cm.max_obs + k];
      d.first_point = 0;  // k_obs_gather fills these two from the slots' counts
      d.n_points = 0;
      d.flags = sp.flags;
      d.pad = kp.source * ob.slots + kp.e.slot;  // the robot's ring slot, for k_obs_gather (which zeroes it)
      d.ox = kp.e.origin[0];
      d.oy = kp.e.origin[1];
      d.oz = kp.e.origin[2];
      d.obstacle_range = sp.obstacle_range;
      d.raytrace_range = sp.raytrace_range;
    }
  }
  return NAVGPU_OK;
}

}  // namespace

extern "C" {

int navgpu_obsbuf_configure(navgpu_fleet* f, const navgpu_obs_source_params* sources, uint32_t n_sources, uint32_t slots, uint32_t max_cloud_points) {
  if (!f || !sources || n_sources == 0 || n_sources > NAVGPU_OBSBUF_MAX_SOURCES || slots == 0 || max_cloud_points == 0 ||
      max_cloud_points > NAVGPU_OBSBUF_MAX_CLOUD_POINTS || (uint64_t)slots * n_sources > f->desc.max_observations)
    return NAVGPU_ERR_INVALID;
  for (uint32_t s = 0; s < n_sources; ++s)
    if (sources[s].observation_keep_time_ns < 0 || sources[s].expected_update_rate_ns < 0) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  ObsBuf& ob = f->ob;
  const uint32_t n = f->desc.n_instances;
  const size_t n_slots = (size_t)n * n_sources * slots;
  float* ring = nullptr;
  uint32_t* counts = nullptr;
  int rc = f->alloc(&ring, n_slots * max_cloud_points * 3);
  if (rc) return rc;
  if ((rc = f->alloc(&counts, n_slots))) {
    f->release(ring);
    return rc;
  }
  hipError_t e = hipSuccess;
  if (!ob.ev_h2d) e = hipEventCreateWithFlags(&ob.ev_h2d, hipEventDisableTiming);
  if (e == hipSuccess) e = waitStream(f->stream);  // the fresh buffers' memsets; whatever read the old rings
  if (e != hipSuccess) {
    f->release(ring);
    f->release(counts);
    g_last_error = std::string("navgpu_obsbuf_configure: ") + hipGetErrorString(e);
    return NAVGPU_ERR_HIP;
  }
  // ---- commit
  f->release(ob.dev.ring);
  f->release(ob.dev.counts);
  ob.dev.ring = ring;
  ob.dev.counts = counts;
  ob.dev.max_cloud_points = max_cloud_points;
  ob.dev.slots_per_robot = n_sources * slots;
  ob.n_sources = n_sources;
  ob.slots = slots;
  for (uint32_t s = 0; s < n_sources; ++s) ob.src[s] = sources[s];
  ob.lists.assign((size_t)n * n_sources, ObsBuf::List());
  ob.evicted.assign(n, 0);
  ob.last_now = 0;
  ob.configured = true;
  return NAVGPU_OK;
}

int navgpu_obsbuf_buffer(navgpu_fleet* f, const navgpu_cloud* clouds, uint32_t n_clouds, const float* points, uint32_t n_points, const float* ranges,
                         uint32_t n_ranges, int64_t now) {
  if (!f) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  ObsBuf& ob = f->ob;
  if (!ob.configured) return NAVGPU_ERR_STATE;
  if ((n_clouds && !clouds) || (n_points && !points) || (n_ranges && !ranges)) return NAVGPU_ERR_INVALID;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    const navgpu_cloud& c = clouds[k];
    if (c.instance >= f->desc.n_instances || c.source >= ob.n_sources || (c.kind != NAVGPU_CLOUD_XYZ && c.kind != NAVGPU_CLOUD_SCAN))
      return NAVGPU_ERR_INVALID;
    if ((uint64_t)c.first + c.n > (c.kind == NAVGPU_CLOUD_SCAN ? n_ranges : n_points)) return NAVGPU_ERR_INVALID;
    if (!finiteAll(c.origin, 3) || !finiteAll(c.transform, 12)) return NAVGPU_ERR_INVALID;
    if (c.n > ob.dev.max_cloud_points) return NAVGPU_ERR_CAPACITY;
  }
  if (n_clouds == 0) {
    ob.last_now = now;
    return NAVGPU_OK;
  }
  const size_t o_pts = align256(sizeof(ObsIngestCloud) * n_clouds), o_rng = o_pts + align256(sizeof(float) * 3 * (size_t)n_points),
               bytes = o_rng + align256(sizeof(float) * (size_t)n_ranges);
  int rc = reserveInput(f, bytes);
  if (rc) return rc;
  if ((rc = waitInput(f))) return rc;
  // ---- the lists (nothing below fails short of a HIP error): bufferCloud per cloud, in call order
  ob.last_now = now;
  std::vector<uint8_t> alive(n_clouds, 1);
  // an entry of this call carries slot = 0xFFFFFFFF and n = index of its cloud until the slots are handed out
  for (uint32_t k = 0; k < n_clouds; ++k) {
    const navgpu_cloud& c = clouds[k];
    const uint32_t li = c.instance * ob.n_sources + c.source;
    ObsBuf::List& l = ob.lists[li];
    ObsBuf::Entry e{};
    e.stamp = c.stamp_ns;
    memcpy(e.origin, c.origin, sizeof(e.origin));
    e.slot = kUnplaced;
    e.n = k;
    l.entries.push_front(e);
    l.last_updated = now;
    size_t n_keep = keptAfterPurge(l.entries, l.last_updated, ob.src[c.source].observation_keep_time_ns);
    if (n_keep > ob.slots) {  // the ring is full: the oldest entry goes (a departure from the unbounded reference list)
      n_keep = ob.slots;
      ++ob.evicted[c.instance];
    }
    for (size_t j = n_keep; j < l.entries.size(); ++j)
      if (l.entries[j].slot == kUnplaced) alive[l.entries[j].n] = 0;  // a cloud of this call that does not outlive it: never ingested
    l.entries.resize(n_keep);
  }
  // ---- slots: an entry of this call takes one that no entry of its list holds
  ObsIngestCloud* desc = reinterpret_cast<ObsIngestCloud*>(ob.h_in);
  uint32_t n_live = 0;
  for (uint32_t k = 0; k < n_clouds; ++k) {
    if (!alive[k]) continue;
    const navgpu_cloud& c = clouds[k];
    const uint32_t li = c.instance * ob.n_sources + c.source;
    ObsBuf::List& l = ob.lists[li];
    ObsBuf::Entry* mine = nullptr;
    for (auto& e : l.entries)
      if (e.slot == kUnplaced && e.n == k) mine = &e;
    uint32_t slot = 0;
    for (;; ++slot) {
      bool taken = false;
      for (const auto& e : l.entries) taken = taken || e.slot == slot;
      if (!taken) break;
    }
    mine->slot = slot;  // slot < ob.slots: the list holds at most ob.slots entries, this one still unplaced
    mine->n = c.n;
    ObsIngestCloud& d = desc[n_live++];
    memset(&d, 0, sizeof(d));
    d.kind = c.kind;
    d.first = c.first;
    d.n = c.n;
    d.slot = li * ob.slots + slot;
    for (int j = 0; j < 12; ++j) d.m[j] = (float)c.transform[j];
    d.min_h = ob.src[c.source].min_obstacle_height;
    d.max_h = ob.src[c.source].max_obstacle_height;
    d.angle_min = c.angle_min;
    d.angle_increment = c.angle_increment;
    d.range_min = c.range_min;
    d.range_max = c.range_max;
    d.inf_is_valid = ob.src[c.source].inf_is_valid;
  }
  if (n_live == 0) return NAVGPU_OK;
  if (n_points) memcpy(ob.h_in + o_pts, points, sizeof(float) * 3 * (size_t)n_points);
  if (n_ranges) memcpy(ob.h_in + o_rng, ranges, sizeof(float) * (size_t)n_ranges);
  if ((rc = sendInput(f, bytes))) return rc;
  PROFILED(f, NAVGPU_K_OBS_INGEST,
           launch_obs_ingest(ob.dev, reinterpret_cast<const ObsIngestCloud*>(ob.d_in), n_live, reinterpret_cast<const float*>(ob.d_in + o_pts),
                             reinterpret_cast<const float*>(ob.d_in + o_rng), f->stream));
  return checkLaunch();
}

int navgpu_obsbuf_stage(navgpu_fleet* f, uint32_t first, uint32_t count, const double* poses, int64_t now, int32_t* current_out) {
  if (!f) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  ObsBuf& ob = f->ob;
  if (!ob.configured) return NAVGPU_ERR_STATE;
  if (!poses || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  CostmapDev& cm = f->cm;
  if (f->desc.rolling_window && f->shift_pending) return NAVGPU_ERR_STATE;  // previous stage not consumed by an update yet
  const RobotSet set{first, count, nullptr};
  KeptSet ks;
  int rc = keptOfSet(f, set, ks);
  if (rc) return rc;
  if (f->desc.rolling_window) f->touchInputs(first, count);  // the origins move now
  if ((rc = stageKept(f, set, ks, now, current_out))) return rc;
  if ((rc = stageRobotPoses(f, first, count, poses))) return rc;
  // array by array also for the whole fleet: the block copy of navgpu_costmap_stage would carry the mirror of cm.points
  HIP_TRY(hipMemcpyAsync(cm.pose + (size_t)first * 3, f->hp_pose + (size_t)first * 3, sizeof(double) * 3 * count, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipMemcpyAsync(cm.fp_world + (size_t)first * kMaxFootprint * 2, f->hp_fpw + (size_t)first * kMaxFootprint * 2, sizeof(double) * 2 * kMaxFootprint * (size_t)count, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipMemcpyAsync(cm.fp_n + first, f->hp_fpn + first, sizeof(uint32_t) * count, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipMemcpyAsync(cm.obs + (size_t)first * cm.max_obs, f->hp_obs + (size_t)first * cm.max_obs, sizeof(ObsCsr) * (size_t)count * cm.max_obs, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipMemcpyAsync(cm.obs_count + first, f->hp_cnt + first, sizeof(uint32_t) * count, hipMemcpyHostToDevice, f->stream));
  if (f->cycles_in_flight > 1) {
    HIP_TRY(hipEventRecord(f->ev_cm_h2d, f->stream));
    f->ev_cm_set = true;
  }
  launch_obs_gather(ob.dev, cm, first, count, f->stream);
  return checkLaunch();
}

// navgpu_obsbuf_stage for a robot list: getMarkingObservations + getClearingObservations (obstacle_layer.cpp:449-478 over
// observation_buffer.cpp:199-236, :238-251) of the listed robots; the hand-over is the packed block of navgpu_costmap_stage_list
// without points, and k_obs_gather runs once, on the list
int navgpu_obsbuf_stage_list(navgpu_fleet* f, uint32_t n_robots, const uint32_t* instances, const double* poses, int64_t now, int32_t* current_out) {
  if (!f) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  ObsBuf& ob = f->ob;
  if (!instances) return NAVGPU_ERR_INVALID;
  if (!ob.configured) return NAVGPU_ERR_STATE;
  if (!poses || !listOk(f, n_robots, instances)) return NAVGPU_ERR_INVALID;
  CostmapDev& cm = f->cm;
  if (f->desc.rolling_window && f->shift_pending) return NAVGPU_ERR_STATE;  // previous stage not consumed by an update yet
  const RobotSet set{0, n_robots, instances};
  KeptSet ks;
  int rc = keptOfSet(f, set, ks);
  if (rc == NAVGPU_OK) rc = reserveCostmapList(f);
  if (rc) return rc;
  if ((rc = stageKept(f, set, ks, now, current_out))) return rc;
  stagePoseMirrors(f, set, poses);
  if ((rc = sendCostmapStageList(f, n_robots, instances, false))) return rc;
  // the list the gather reads: the block's records name the robots, the kernel wants them as a plain array
  if ((rc = f->cml.list.send(f, instances, n_robots))) return rc;
  launch_obs_gather(ob.dev, cm, RobotList{f->cml.list.d}, n_robots, f->stream);
  return checkLaunch();
}

int navgpu_obsbuf_observations(navgpu_fleet* f, uint32_t inst, int64_t now, navgpu_observation* obs, uint32_t obs_capacity, float* points,
                               uint32_t point_capacity, uint32_t* n_points_out) {
  (void)now;  // the purge compares with last_updated_, as getObservations' does
  if (!f) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  ObsBuf& ob = f->ob;
  if (!ob.configured) return NAVGPU_ERR_STATE;
  if (inst >= f->desc.n_instances || (obs_capacity && !obs) || (point_capacity && !points)) return NAVGPU_ERR_INVALID;
  std::vector<Kept> kept;
  keptOf(ob, inst, kept, nullptr);
  if (kept.size() > obs_capacity) return NAVGPU_ERR_CAPACITY;
  std::vector<uint32_t> counts(ob.dev.slots_per_robot);
  HIP_TRY(hipMemcpyAsync(counts.data(), ob.dev.counts + (size_t)inst * ob.dev.slots_per_robot, sizeof(uint32_t) * counts.size(), hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));
  uint64_t total = 0;
  for (const Kept& k : kept) total += counts[k.source * ob.slots + k.e.slot];
  if (total > point_capacity) return NAVGPU_ERR_CAPACITY;
  uint32_t off = 0;
  for (size_t k = 0; k < kept.size(); ++k) {
    const Kept& kp = kept[k];
    const uint32_t slot = kp.source * ob.slots + kp.e.slot, n = counts[slot];
    const navgpu_obs_source_params& sp = ob.src[kp.source];
    obs[k] = navgpu_observation{inst, off, n, sp.flags, kp.e.origin[0], kp.e.origin[1], kp.e.origin[2], sp.obstacle_range, sp.raytrace_range};
    if (n)
      HIP_TRY(hipMemcpyAsync(points + (size_t)off * 3, ob.dev.ring + ((size_t)inst * ob.dev.slots_per_robot + slot) * ob.dev.max_cloud_points * 3,
                             sizeof(float) * 3 * n, hipMemcpyDeviceToHost, f->stream));
    off += n;
  }
  HIP_TRY(waitStream(f->stream));
  if (n_points_out) *n_points_out = off;
  return (int)kept.size();
}

int navgpu_obsbuf_set_global_frame(navgpu_fleet* f, uint32_t first, uint32_t count, const double* M) {
  if (!f) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  ObsBuf& ob = f->ob;
  if (!ob.configured) return NAVGPU_ERR_STATE;
  if (!M || !f->rangeOk(first, count) || !finiteAll(M, 12 * (int)count)) return NAVGPU_ERR_INVALID;
  size_t n_items = 0;
  for (uint32_t li = 0; li < count; ++li)
    for (uint32_t s = 0; s < ob.n_sources; ++s) n_items += ob.lists[(size_t)(first + li) * ob.n_sources + s].entries.size();
  if (n_items == 0) return NAVGPU_OK;
  int rc = reserveInput(f, sizeof(ObsRetransform) * n_items);
  if (rc) return rc;
  if ((rc = waitInput(f))) return rc;
  ObsRetransform* items = reinterpret_cast<ObsRetransform*>(ob.h_in);
  size_t at = 0;
  for (uint32_t li = 0; li < count; ++li) {
    const double* m = M + (size_t)li * 12;
    for (uint32_t s = 0; s < ob.n_sources; ++s) {
      const size_t list = (size_t)(first + li) * ob.n_sources + s;
      for (auto& e : ob.lists[list].entries) {
        const double x = e.origin[0], y = e.origin[1], z = e.origin[2];  // tf::Transform::operator*(Vector3): row . v + origin
        for (int r = 0; r < 3; ++r) e.origin[r] = ((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + m[9 + r];
        ObsRetransform& it = items[at++];
        it.slot = (uint32_t)(list * ob.slots + e.slot);
        it.pad = 0;
        for (int j = 0; j < 12; ++j) it.m[j] = (float)m[j];
      }
    }
  }
  if ((rc = sendInput(f, sizeof(ObsRetransform) * n_items))) return rc;
  for (size_t done = 0; done < n_items; done += 32768)  // (a grid's y extent is limited to 65535)
    launch_obs_retransform(ob.dev, reinterpret_cast<const ObsRetransform*>(ob.d_in) + done, (uint32_t)std::min<size_t>(32768, n_items - done), f->stream);
  return checkLaunch();
}

int navgpu_obsbuf_reset_last_updated(navgpu_fleet* f, uint32_t first, uint32_t count, int64_t now) {
  if (!f) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  ObsBuf& ob = f->ob;
  if (!ob.configured) return NAVGPU_ERR_STATE;
  if (!f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  ob.last_now = now;
  for (size_t l = (size_t)first * ob.n_sources; l < (size_t)(first + count) * ob.n_sources; ++l) ob.lists[l].last_updated = now;
  return NAVGPU_OK;
}

int navgpu_obsbuf_status(navgpu_fleet* f, uint32_t first, uint32_t count, navgpu_obsbuf_robot_status* out) {
  if (!f) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  ObsBuf& ob = f->ob;
  if (!ob.configured) return NAVGPU_ERR_STATE;
  if (!out || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  const uint32_t spr = ob.dev.slots_per_robot;
  std::vector<uint32_t> counts((size_t)count * spr);
  HIP_TRY(hipMemcpyAsync(counts.data(), ob.dev.counts + (size_t)first * spr, sizeof(uint32_t) * counts.size(), hipMemcpyDeviceToHost, f->stream));
  HIP_TRY(waitStream(f->stream));
  for (uint32_t li = 0; li < count; ++li) {
    navgpu_obsbuf_robot_status st{};
    for (uint32_t s = 0; s < ob.n_sources; ++s)
      for (const auto& e : ob.lists[(size_t)(first + li) * ob.n_sources + s].entries) {
        ++st.kept;
        st.points += counts[(size_t)li * spr + s * ob.slots + e.slot];
      }
    st.evicted = ob.evicted[first + li];
    st.current = robotCurrent(ob, first + li, ob.last_now);
    out[li] = st;
  }
  return NAVGPU_OK;
}

}  // extern "C"
