// The navgpu_navfn handle, shared by the host files that work on it (navgpu_navfn.cpp, navgpu_global_plan.cpp, navgpu_navfn_ros.cpp).
#pragma once
#include "global_plan_kernels.h"
#include "navfn_ros_kernels.h"
#include "navfn_rules.h"
#include "navgpu_fleet.h"

// What navgpu_global_planner_make_plan leaves for navgpu_global_planner_plans, and navgpu_navfn_ros_make_plan / _plan_from_potential
// for navgpu_navfn_ros_plans: per plan, which of them is the last thing that wrote its path (any other plan call, or new costs,
// takes that away) and the record k_gp_plan_emit assembles it from.
constexpr uint8_t kMadeByGlobalPlanner = 1, kMadeByNavfnRos = 2;
struct MadePlans {
  std::vector<uint8_t> valid;           // [n] 0, or the maker
  std::vector<navgpu::GpPlanRec> rec;   // [n] host copy of d_rec
  navgpu::GpPlanRec* d_rec = nullptr;   // [n]
  int32_t* d_clear = nullptr;           // [n] clearRobotCell's cell of a call's plans (-1: plan not attempted)
  uint8_t* d_out = nullptr;             // offsets + poses of a navgpu_global_planner_plans call, grown on demand
  size_t out_bytes = 0;
  std::vector<uint8_t> h_out;           // where that call's one copy lands
  uint8_t* d_alt = nullptr;             // [n] final_array of a navgpu_global_planner_potential_grid call's plans
  int8_t* d_grids = nullptr;            // navgpu_global_planner_potential_grid's bytes, grown on demand
  size_t grid_bytes = 0;
  float* d_maxima = nullptr;            // [n]
  void forget(uint32_t first, uint32_t count) {
    if (!valid.empty()) std::fill(valid.begin() + first, valid.begin() + first + count, (uint8_t)0);
  }
};

// navgpu_navfn_ros_*'s state (navgpu_navfn_ros.cpp): NavFn's start and goal cell of each plan as the last of these calls left them
// (the potential cloud divides by the start's potential, getPlanFromPotential walks to the goal), and the device buffers of the
// calls, grown on demand
struct NavfnRosState {
  std::vector<int32_t> nav_start;       // [n] cell index; NavFn's constructor leaves (0, 0)
  std::vector<int32_t> nav_goal;        // [n][2]
  navgpu::NrWindow* d_win = nullptr;    // window jobs of a call
  size_t win_cap = 0;
  double* d_seq = nullptr;              // their coordinate sequences
  size_t seq_cap = 0;
  navgpu::NrBest* d_best = nullptr;     // their results
  size_t best_cap = 0;
  navgpu::NrPathJob* d_path = nullptr;  // [n] second-path jobs and what they found
  double* d_q = nullptr;                // point queries: {x, y} in, potential out
  size_t q_cap = 0;
  int32_t* d_qplan = nullptr;           // the plan of each query (relative to the call's first)
  size_t qplan_cap = 0;
  navgpu::NrCloudPlan* d_cloud_plans = nullptr;  // [n]
  uint32_t* d_totals = nullptr;         // the cloud's chunk totals / prefixes, then the plans' offsets
  size_t totals_cap = 0;
  uint8_t* d_cloud = nullptr;           // offsets + points of a navgpu_navfn_ros_potential_cloud call
  size_t cloud_bytes = 0;
};

struct navgpu_navfn {
  NavfnDev nv{};
  uint32_t n = 0;
  int device = 0;
  std::recursive_mutex mu;  // calls on one handle are serialised inside the library (as on a fleet)
  hipStream_t stream = nullptr;
  std::vector<void*> allocs;
  uint8_t* d_cmap = nullptr;   // staging for host cost maps: [n][ns_padded]
  int32_t* d_goal = nullptr;   // [n][2]
  int32_t* d_start = nullptr;  // [n][2]
  navgpu_navfn_result* h_results = nullptr;  // pinned
  double* d_xy = nullptr;      // [n][2][2] start / goal map coordinates (global_planner)
  void* d_heap = nullptr;      // [n][ns_padded] AStarExpansion's queue_, allocated when A* is first asked for
  NavfnWfStatus* h_wf_status = nullptr;  // pinned; the tiled wavefront's per-plan state as the host last read it
  int32_t *d_seed_cells = nullptr, *d_stop = nullptr;  // [n][4] / [n] the tiled wavefront's seeds and stop cells
  float* d_seed_vals = nullptr;                        // [n][4]
  std::vector<uint8_t> final_array;      // [n] which potential array holds a plan's result (1: potalt, wavefront mode only)
  MadePlans made;                        // navgpu_global_planner_make_plan's state (navgpu_global_plan.cpp)
  NavfnRosState ros;                     // navgpu_navfn_ros_*'s (navgpu_navfn_ros.cpp)
  template <class T>
  int alloc(T** p, size_t count) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    if (hipMalloc(&q, bytes) != hipSuccess) {
      g_last_error = "hipMalloc failed (navfn)";
      return NAVGPU_ERR_HIP;
    }
    hipMemsetAsync(q, 0, bytes, stream);
    allocs.push_back(q);
    *p = static_cast<T*>(q);
    return NAVGPU_OK;
  }
};

struct NavfnGuard {  // lock + make the handle's GPU current on the calling thread
  std::lock_guard<std::recursive_mutex> lk;
  explicit NavfnGuard(navgpu_navfn* h) : lk(h->mu) { (void)hipSetDevice(h->device); }
};

// the buffers of the made-plan calls, allocated when the first of them runs
inline int reserveMadePlans(navgpu_navfn* h) {
  MadePlans& m = h->made;
  if (m.d_maxima) return NAVGPU_OK;
  m.valid.assign(h->n, 0);
  m.rec.assign(h->n, navgpu::GpPlanRec{});
  int rc = 0;
  if (!rc && !m.d_rec) rc = h->alloc(&m.d_rec, h->n);
  if (!rc && !m.d_clear) rc = h->alloc(&m.d_clear, h->n);
  if (!rc && !m.d_alt) rc = h->alloc(&m.d_alt, h->n);
  if (!rc) rc = h->alloc(&m.d_maxima, h->n);  // last: its presence says the others exist
  return rc;
}

// a device buffer that only grows; what it replaces is freed with the handle
template <class T>
int growBuffer(navgpu_navfn* h, T** buf, size_t* have, size_t want) {
  if (want <= *have) return NAVGPU_OK;
  T* q = nullptr;
  const int rc = h->alloc(&q, want);
  if (rc) return rc;
  *buf = q;
  *have = want;
  return NAVGPU_OK;
}

// the plans of [first, first+count) as `maker` left them: offsets, then the poses that fit, in one device pass and one copy
// (navgpu_global_plan.cpp)
int assembleMadePlans(navgpu_navfn* h, uint32_t first, uint32_t count, uint8_t maker, uint32_t capacity, navgpu_global_pose* poses, uint32_t* offsets);

// the tiled wavefront expansion of a range of plans (navgpu_navfn.cpp)
int runWavefront(navgpu_navfn* h, uint32_t first, uint32_t count, const navgpu::NavfnWfRule& rule_in, const int32_t* seed_cells, const float* seed_vals,
                 const int32_t* stop_cells, int at_start);
inline bool navfnRange(const navgpu_navfn* h, uint32_t first, uint32_t count) { return count > 0 && first < h->n && count <= h->n - first; }

// DijkstraExpansion as the tiled wavefront: the rule, and the seeds and stop cells of count plans from their map coordinates
// (setPreciseStart(true)'s four cells unless old_navfn_behavior; the goal cell ends the search)
inline navgpu::NavfnWfRule gpWavefrontRule(const navgpu_global_planner_params& gp) {
  navgpu::NavfnWfRule rule{};
  rule.global_planner = 1;
  rule.quadratic = gp.use_quadratic ? 1 : 0;
  rule.outline = gp.outline_map ? 1 : 0;
  rule.allow_unknown = gp.allow_unknown ? 1 : 0;
  rule.lethal_cost = gp.lethal_cost;
  rule.neutral_cost = gp.neutral_cost;
  rule.cost_factor = gp.cost_factor;
  return rule;
}
inline void gpWavefrontSeeds(int nx, const navgpu_global_planner_params& gp, uint32_t count, const double* starts, const double* goals,
                             std::vector<int32_t>& seed_cells, std::vector<float>& seed_vals, std::vector<int32_t>& stop) {
  seed_cells.assign((size_t)count * 4, -1);
  seed_vals.assign((size_t)count * 4, 0.0f);
  stop.assign(count, 0);
  for (uint32_t q = 0; q < count; ++q) {
    if (!gp.old_navfn_behavior) {  // setPreciseStart(true)
      int cells[4];
      float vals[4];
      navgpu::preciseStartSeeds(starts[2 * q], starts[2 * q + 1], nx, gp.neutral_cost, cells, vals);
      std::copy(cells, cells + 4, seed_cells.begin() + 4 * q);
      std::copy(vals, vals + 4, seed_vals.begin() + 4 * q);
    } else {
      seed_cells[4 * q] = (int)starts[2 * q] + nx * (int)starts[2 * q + 1];  // toIndex(double, double)
    }
    stop[q] = (int)goals[2 * q] + nx * (int)goals[2 * q + 1];
  }
}
