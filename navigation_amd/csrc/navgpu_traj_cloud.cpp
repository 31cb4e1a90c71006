// C-ABI host side of DWAPlanner's trajectory cloud (include/navgpu.h):
//   navgpu_planner_set_trajectory_cloud  publish_traj_pc per robot (dwa_planner.cpp:160-163)
//   navgpu_planner_trajectory_cloud      the cloud findBestPath builds from all_explored (dwa_planner.cpp:318-348)
//   navgpu_planner_sample_terms          the per-critic breakdown of every sample slot behind it
// The cycle of an enabled robot pays for the terms pass only (termsPass: k_score_prep_gen + k_score_terms on that
// robot, between the scoring launch and k_select); the scan and the emit (traj_cloud_kernels.hip) run at the read call.
#include "navgpu_fleet.h"

namespace {

using Robot = navgpu_fleet::TrajCloud::Robot;

Robot* findRobot(navgpu_fleet* f, uint32_t inst) {
  for (Robot& r : f->tc.robots)
    if (r.inst == inst) return &r;
  return nullptr;
}

// the robot's records hold pl.max_samples slots (a reconfigure may have changed that).  All-or-nothing.
int reserveRecords(navgpu_fleet* f, Robot& r) {
  const uint32_t need = f->pl.max_samples;
  if (r.cap_samples >= need && r.d_terms) return NAVGPU_OK;
  SampleTerms* nt = nullptr;
  navgpu_sample_terms* no = nullptr;
  int rc = f->alloc(&nt, need);
  if (!rc) rc = f->alloc(&no, need);
  if (rc) {
    f->release(nt);
    return rc;
  }
  HIP_TRY(waitStream(f->stream));  // (nothing queued uses the old records)
  f->release(r.d_terms);
  f->release(r.d_out);
  r.d_terms = nt;
  r.d_out = no;
  r.cap_samples = need;
  r.have_cycle = false;
  return NAVGPU_OK;
}

int reservePoints(navgpu_fleet* f, size_t points) {
  navgpu_fleet::TrajCloud& tc = f->tc;
  if (points <= tc.points_cap) return NAVGPU_OK;
  size_t cap = std::max<size_t>(tc.points_cap, (size_t)1 << 12);
  while (cap < points) cap *= 2;
  float* q = nullptr;
  int rc = f->alloc(&q, cap * 7);
  if (rc) return rc;
  HIP_TRY(waitStream(f->stream));
  f->release(tc.d_points);
  tc.d_points = q;
  tc.points_cap = cap;
  return NAVGPU_OK;
}

// the checks the two read calls share, then k_traj_scan: f->tc.h_totals holds the cloud's points and the slots afterwards
int scanRobot(navgpu_fleet* f, uint32_t instance, int32_t reference_costs, TrajCloudDev* t) {
  if (!f->planner_configured) return NAVGPU_ERR_STATE;
  Robot* r = findRobot(f, instance);
  if (!r || !r->have_cycle || r->gen != f->inputs_gen[instance] || r->cap_samples < f->pl.max_samples) {
    navgpu::g_last_error = !r ? "trajectory cloud: the robot is not enabled"
                              : (!r->have_cycle ? "trajectory cloud: no cycle since the robot was enabled" : "trajectory cloud: staged or reconfigured after the cycle");
    return NAVGPU_ERR_STATE;
  }
  t->terms = r->d_terms;
  t->out = r->d_out;
  t->totals = f->tc.h_totals;
  t->points = nullptr;
  t->capacity = 0;
  t->slots_per_group = traj_emit_slots_per_group(f->pl.max_sim_steps);
  memcpy(t->scale, r->scale, sizeof(t->scale));
  t->reference_costs = reference_costs ? 1 : 0;
  launch_traj_scan(f->pl, *t, instance, f->stream);
  HIP_TRY(waitStream(f->stream));
  return checkLaunch();
}

// navgpu_planner_cycle, between the scoring launch and k_select, while robots are enabled (navgpu_fleet::TrajCloud::terms_pass)
int termsPass(navgpu_fleet* f, uint32_t first, uint32_t count) {
  const PlannerDev& pl = f->pl;
  for (Robot& r : f->tc.robots) {
    if (r.inst < first || r.inst - first >= count) continue;
    int rc = reserveRecords(f, r);
    if (rc) return rc;
    // the scales scoreSamples sums with: DWAPlanner::reconfigure's (dwa_planner.cpp:64-75), alignment off near the goal (:279-285)
    r.scale[0] = pl.scale_obstacle;
    r.scale[1] = pl.scale_goal;
    r.scale[2] = f->hp_align[r.inst] ? pl.scale_path : 0.0;
    r.scale[3] = pl.scale_path;
    r.scale[4] = pl.scale_goal;
    launch_score_terms(pl, r.inst, r.d_terms, f->stream);
    r.have_cycle = true;
    r.gen = f->cycle_gen[r.inst];
  }
  return NAVGPU_OK;
}

}  // namespace

extern "C" {

int navgpu_planner_set_trajectory_cloud(navgpu_fleet* f, uint32_t first, uint32_t count, int32_t enable) {
  if (!f || !f->rangeOk(first, count)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  navgpu_fleet::TrajCloud& tc = f->tc;
  if (!enable) {
    HIP_TRY(waitStream(f->stream));
    for (size_t k = tc.robots.size(); k-- > 0;) {
      Robot& r = tc.robots[k];
      if (r.inst < first || r.inst - first >= count) continue;
      f->release(r.d_terms);
      f->release(r.d_out);
      tc.robots.erase(tc.robots.begin() + (long)k);
    }
    return NAVGPU_OK;
  }
  if (f->cycles_in_flight > 1) return NAVGPU_ERR_STATE;
  if (traj_emit_slots_per_group(f->pl.max_sim_steps) == 0) return NAVGPU_ERR_CAPACITY;
  uint32_t fresh = 0;
  for (uint32_t i = first; i < first + count; ++i)
    if (!findRobot(f, i)) ++fresh;
  if (tc.robots.size() + fresh > NAVGPU_TRAJ_CLOUD_MAX_ROBOTS) {
    navgpu::g_last_error = "trajectory cloud: more than NAVGPU_TRAJ_CLOUD_MAX_ROBOTS robots enabled";
    return NAVGPU_ERR_INVALID;
  }
  if (!tc.h_totals) {
    int rc = f->allocPinned(&tc.h_totals, 2);
    if (rc) return rc;
  }
  tc.terms_pass = termsPass;
  for (uint32_t i = first; i < first + count; ++i)
    if (!findRobot(f, i)) {
      Robot r;
      r.inst = i;
      tc.robots.push_back(r);  // (its records are sized by the configuration of its first cycle)
    }
  return NAVGPU_OK;
}

int navgpu_planner_trajectory_cloud(navgpu_fleet* f, uint32_t instance, int32_t reference_costs, float* points, uint32_t capacity) {
  if (!f || instance >= f->desc.n_instances || (capacity && !points)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  TrajCloudDev t{};
  int rc = scanRobot(f, instance, reference_costs, &t);
  if (rc) return rc;
  const uint32_t total = f->tc.h_totals[0], n_slots = f->tc.h_totals[1];
  const uint32_t n_write = std::min(total, capacity);
  if (n_write) {
    if ((rc = reservePoints(f, n_write))) return rc;
    t.points = f->tc.d_points;
    t.capacity = n_write;
    launch_traj_emit(f->pl, t, instance, n_slots, f->stream);
    if ((rc = checkLaunch())) return rc;
    HIP_TRY(hipMemcpyAsync(points, t.points, sizeof(float) * 7 * (size_t)n_write, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(waitStream(f->stream));
  }
  return (int)std::min<uint32_t>(total, 0x7FFFFFFFu);  // points of the cloud (may exceed capacity: call again with a larger buffer)
}

int navgpu_planner_sample_terms(navgpu_fleet* f, uint32_t instance, navgpu_sample_terms* out, uint32_t capacity) {
  if (!f || instance >= f->desc.n_instances || (capacity && !out)) return NAVGPU_ERR_INVALID;
  FleetGuard guard_(f);
  TrajCloudDev t{};
  int rc = scanRobot(f, instance, 1, &t);
  if (rc) return rc;
  const uint32_t n_slots = f->tc.h_totals[1], n = std::min(n_slots, capacity);
  if (n) {
    HIP_TRY(hipMemcpyAsync(out, t.out, sizeof(navgpu_sample_terms) * (size_t)n, hipMemcpyDeviceToHost, f->stream));
    HIP_TRY(waitStream(f->stream));
  }
  return (int)n_slots;
}

}  // extern "C"
