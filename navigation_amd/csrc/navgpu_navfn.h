// The navgpu_navfn handle, shared by the host files that work on it (navgpu_navfn.cpp, navgpu_global_plan.cpp).
#pragma once
#include "global_plan_kernels.h"
#include "navfn_rules.h"
#include "navgpu_fleet.h"

// What navgpu_global_planner_make_plan leaves for navgpu_global_planner_plans: per plan, whether a make_plan call is the last
// thing that wrote its path (any other plan call, or new costs, takes that away) and the record k_gp_plan_emit assembles it from.
struct MadePlans {
  std::vector<uint8_t> valid;           // [n]
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
