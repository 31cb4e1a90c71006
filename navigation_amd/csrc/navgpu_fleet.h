// Internal to libnavgpu.so: the fleet object behind the opaque navgpu_fleet handle and the helpers the host
// translation units share (navgpu_host.cpp: lifetime / costmap layers / DWA planner / measurement,
// navgpu_local_planner.cpp: DWAPlannerROS control cycle, navgpu_tp.cpp: legacy TrajectoryPlanner, navgpu_tp_ros.cpp: its ROS class,
// navgpu_recovery.cpp: footprint-cost queries, RotateRecovery, CarrotPlanner, navgpu_voxel_export.cpp: voxel-layer debug
// outputs, navgpu_traj_cloud.cpp: DWAPlanner's trajectory cloud, navgpu_obs_buffer.cpp: ObservationBuffer on the device).
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "navgpu_device.h"

using namespace navgpu;

namespace navgpu {
extern thread_local std::string g_last_error;  // defined in navgpu_host.cpp

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      g_last_error = std::string(#expr) + ": " + hipGetErrorString(e_);                            \
      return NAVGPU_ERR_HIP;                                                                       \
    }                                                                                              \
  } while (0)

// hipStreamSynchronize also flushes the runtime's batched launches; a hipStreamQuery polling loop does
// not (measured: the queue then only drains when the poll gives up), so no polling here.
inline hipError_t waitStream(hipStream_t s) { return hipStreamSynchronize(s); }

struct EventPair {
  int kernel;
  hipEvent_t a, b;
};
int ensureCompleteGrids(navgpu_fleet* f, uint32_t first, uint32_t count);
// What a costmap cycle stages besides its observations, for [first, first + count): pose, transformed footprint and vertex
// count into the pinned mirrors, and for a rolling window the new origins and pending shift (host and device).  Shared by
// navgpu_costmap_stage and navgpu_obsbuf_stage; the caller has waited for the mirrors and copies them afterwards.
int stageRobotPoses(navgpu_fleet* f, uint32_t first, uint32_t count, const double* poses);
// The robots of a costmap stage call: the contiguous range of navgpu_costmap_stage / navgpu_obsbuf_stage, or the strictly increasing
// list of their listed forms.  What the two forms share - the checks of the observations, the pinned mirrors' arithmetic - takes one.
struct RobotSet {
  uint32_t first, count;
  const uint32_t* list;  // null: the range [first, first + count)
  uint32_t operator[](uint32_t k) const { return list ? list[k] : first + k; }
  bool has(uint32_t i) const { return list ? std::binary_search(list, list + count, i) : (i >= first && i - first < count); }
};
// instances[0 .. n_robots) strictly increasing, each < n_instances (navgpu_planner_check_trajectories' conventions)
bool listOk(const navgpu_fleet* f, uint32_t n_robots, const uint32_t* instances);
// finish the MapGrids of the set's robots whose last wavefronts stopped at their box - one listed launch for all of them, however
// they lie; fails, before any launch, when their inputs have changed since (ensureCompleteGrids(f, first, count) is the range's set)
int ensureCompleteGrids(navgpu_fleet* f, const RobotSet& r);
// what a costmap stage call checks of its observations before it changes anything: every one for a robot of the set, within the
// fleet's capacities and the caller's points
int checkStageObservations(navgpu_fleet* f, const RobotSet& r, const navgpu_observation* obs, uint32_t n_obs, uint32_t n_points_total);
// the set's pinned mirrors of descriptors and points from checked observations; its obs_consumed flags fall
void stageObservationMirrors(navgpu_fleet* f, const RobotSet& r, const navgpu_observation* obs, uint32_t n_obs, const float* points);
// the set's pinned mirrors of pose, transformed footprint and vertex count, and for a rolling window its host origins and shift
// mirrors (stageRobotPoses' arithmetic: poses[k] belongs to robot r[k])
void stagePoseMirrors(navgpu_fleet* f, const RobotSet& r, const double* poses);
// The listed costmap stage (navgpu_costmap_stage_list, navgpu_obsbuf_stage_list), behind the mirrors: the packed block of the listed
// robots - records, footprint vertices, descriptors in use and, with_points, the points in use - in one upload, k_cm_stage_scatter
// behind it, the marker of two cycles in flight, and for a rolling window the pending shift of this list (navgpu_costmap_list.cpp)
int reserveCostmapList(navgpu_fleet* f);
int sendCostmapStageList(navgpu_fleet* f, uint32_t n_robots, const uint32_t* instances, bool with_points);
// navgpu_planner_stage_poses(_list) without its "a plan was staged" check: for the robots of a range or a valid list whose plan is on
// the device and whose length and last point the pinned mirrors hold; pos_xyth / vel_xyth [k] belong to robot r[k] (navgpu_host.cpp)
int stagePoses(navgpu_fleet* f, const RobotSet& r, const float* pos_xyth, const float* vel_xyth);
// The robot list a listed launch reads: the device array, its pinned source and the marker behind the last copy out of it.
struct DeviceList {
  uint32_t *d = nullptr, *h = nullptr;  // [n]
  hipEvent_t ev = nullptr;              // behind the copy out of h
  bool set = false;
  hipError_t wait() { return set ? hipEventSynchronize(ev) : hipSuccess; }  // h may still feed the copy of the listed call before
  // src[0 .. n) into d on the fleet's stream, through h.  src == h: the caller has waited and written the list in place.
  int send(navgpu_fleet* f, const uint32_t* src, uint32_t n);
};
// device-resident global plans (navgpu_resident_plan.cpp), for the handover of navgpu_move_base.cpp: wait until the last adoption's
// copies out of ResidentPlans::h_off have run; a robot's slot has just taken a new plan of len poses (DWAPlannerROS::setPlan's host side)
int waitAdoption(navgpu_fleet* f);
void becomeResident(navgpu_fleet* f, uint32_t i, uint32_t len, const double* T);
}  // namespace navgpu

struct navgpu_fleet {
  navgpu_fleet_desc desc{};
  // Every entry point that takes the fleet holds this for its whole body (FleetGuard): the calls on one fleet are
  // serialised INSIDE the library, so a reconfigure from another host thread (dynamic_reconfigure's spinner thread:
  // DWAPlanner::configuration_mutex_, dwa_planner.cpp:55,301; InflationLayer::inflation_access_,
  // inflation_layer.cpp:68,112,175) can never run beside a stage / update / cycle of the same fleet.  Recursive because
  // the control-cycle mirror (navgpu_local_planner_*) calls other entry points.
  std::recursive_mutex mu;
  hipStream_t stream = nullptr;
  CostmapDev cm{};
  PlannerDev pl{};
  bool planner_configured = false, inflation_configured = false, planner_staged = false;
  bool shift_pending = false;                   // rolling window: staged origins not yet applied to the grids
  uint32_t shift_first = 0, shift_count = 0;
  bool shift_listed = false;                    // ... staged by a listed call, for the robots of shift_list: the update that names them applies it
  std::vector<uint32_t> shift_list;
  std::vector<void*> allocs;
  // host mirrors
  std::vector<double> h_origin;                 // [n][2]
  std::vector<double> h_fp_spec;                // [n][kMaxFootprint][2]
  std::vector<uint32_t> h_fp_n;                 // [n]
  navgpu_inflation_params infl{};
  navgpu_obstacle_params obsp{};
  double fp_radius = 0.0;                       // largest vertex distance over all instances
  // pinned host mirrors of the per-cycle staging arrays (full fleet size): H2D copies are truly
  // asynchronous and no per-call allocation happens on the staging path
  std::vector<void*> pinned;
  ObsCsr* hp_obs = nullptr;
  uint32_t *hp_cnt = nullptr, *hp_used = nullptr, *hp_plan_cnt = nullptr;
  float* hp_pts = nullptr;
  double *hp_fpw = nullptr, *hp_pose = nullptr, *hp_plan = nullptr, *hp_front = nullptr;
  int32_t *hp_shift = nullptr, *hp_align = nullptr;
  uint32_t *hp_reach = nullptr, *hp_fpn = nullptr;
  // the two staging blocks (device / pinned host, same layout): the pointers above and cm.pose ... / pl.state ... point into them
  uint8_t *cm_stage_dev = nullptr, *cm_stage_host = nullptr, *pl_stage_dev = nullptr, *pl_stage_host = nullptr;
  size_t cm_stage_bytes = 0, pl_stage_bytes = 0;
  // bounded MapGrid wavefronts (navgpu_planner_set_bounded_map_grids): which robots hold grids that are exact inside
  // their box only, that box, and whether the inputs of the cycle that made them are still the staged ones
  bool bounded_grids = true;
  // wavefront seed lists (navgpu_planner_set_seed_lists, navgpu_planner_set_seed_list_capacity): a cycle's k_samples turns every
  // robot's plan into the seed cells of its three grids, once, and the wavefronts behind it scatter them
  bool seed_lists = true;
  // split image build (navgpu_planner_set_split_prep): a cycle's wavefront launch carries the grid-free part of the scoring image
  bool split_prep = true;
  uint32_t seed_list_cap = kSeedListMax;
  std::vector<uint8_t> grid_partial;            // [n]
  std::vector<int32_t> h_box;                   // [n][4] x0, x1, y0, y1 of the last bounded cycle
  std::vector<uint64_t> inputs_gen, cycle_gen;  // [n] bumped by whatever a wavefront reads / value at the last cycle
  void touchInputs(uint32_t first, uint32_t count) {
    for (uint32_t i = first; i < first + count && i < inputs_gen.size(); ++i) ++inputs_gen[i];
  }
  void touchInputs(const RobotSet& r) {
    for (uint32_t k = 0; k < r.count; ++k) ++inputs_gen[r[k]];
  }
  navgpu_robot_state* hp_state = nullptr;
  navgpu_plan_result* hp_result = nullptr;      // [2][n]: the slot a cycle writes alternates while two cycles are in flight
  bool hp_dma_pending = false;  // a full stage's copies out of hp_state / hp_front / hp_align / hp_reach may still be queued
  // Two control cycles in flight on the stream (navgpu_planner_set_cycles_in_flight(f, 2)): cycle k + 1 is handed over and
  // queued while cycle k still runs, so the stream never idles between the end of a cycle and the host's next hand-over.
  // What has to be known for that is finer than "the stream has drained": that the copies out of the pinned mirrors have
  // run (ev_cm_h2d / ev_pl_h2d, recorded behind them) and that ONE cycle's results are in place (ev_cycle[slot], recorded
  // behind its k_select).
  int cycles_in_flight = 1;
  int res_slot = 0;                             // slot of hp_result the latest queued cycle writes
  hipEvent_t ev_cycle[2] = {nullptr, nullptr}, ev_cm_h2d = nullptr, ev_pl_h2d = nullptr;
  bool ev_cycle_set[2] = {false, false}, ev_cm_set = false, ev_pl_set = false;
  // the pinned mirrors are free again: the whole stream with one cycle in flight, the marker behind their copies with two
  hipError_t waitMirrors(hipEvent_t ev, bool set) {
    if (cycles_in_flight < 2) return navgpu::waitStream(stream);
    return set ? hipEventSynchronize(ev) : hipSuccess;
  }
  // DWAPlannerROS mirror (navgpu_local_planner_*): per-instance controller state, host only
  struct LocalPlannerState {
    std::vector<double> plan;      // stored global plan, (x, y, yaw) triples in the plan's frame (prunePlan shrinks it)
    double T[3] = {0, 0, 0};       // planar plan -> global transform
    bool has_T = false, have_plan = false;
    bool xy_tolerance_latch = false, rotating_to_goal = false;  // LatchedStopRotateController members
    std::vector<double> local;     // host path: the transformed, pruned plan of the last cycle (navgpu_local_planner_local_plan)
    navgpu_local_window window{-1, 0, 0, 0, 0, NAVGPU_LOCAL_WINDOW_NONE};  // what getLocalPlan did in the last cycle
  };
  std::vector<LocalPlannerState> lp;
  // device-resident global plans (navgpu_local_planner_reserve_plans ...): absent (cap 0) unless asked for
  struct ResidentPlans {
    uint32_t cap = 0;                         // max_global_plan
    navgpu_global_pose* d_poses = nullptr;    // [n][cap]
    PlanWindowIn *d_in = nullptr, *h_in = nullptr;     // [n] a cycle's inputs; h_: pinned
    PlanWindowRec *d_rec = nullptr, *h_rec = nullptr;  // [n] and what k_plan_window left
    uint32_t *d_off = nullptr, *h_off = nullptr;       // [n + 1] an adoption's slot offsets / an upload's plan offsets
    uint8_t* d_up = nullptr;                  // navgpu_local_planner_set_plans' concatenated poses, grown on demand
    size_t up_bytes = 0;
    hipEvent_t ev_fleet = nullptr, ev_nav = nullptr;   // adoption: the store is free / the plans are in place
    bool ev_nav_set = false;
    struct Robot {
      bool resident = false;       // the robot's plan is the one in its slot (not LocalPlannerState::plan)
      uint32_t start = 0, len = 0; // live part of the slot: prunePlan's erase is start += n, len -= n
      uint32_t dropped = 0;        // poses erased before a store resize: no longer in the slot (the resize moves the live part to its front)
      bool has_T = false;
      double T[3] = {0, 0, 0};     // planar plan -> global transform
      bool goal_known = false;
      double goal[3] = {0, 0, 0};  // getGoalPose of the stored plan (cached: the last pose stays until the plan is replaced)
      uint32_t loc_first = 0, loc_n = 0;  // slot positions of the last cycle's local plan
    };
    std::vector<Robot> robots;     // [n]
    bool residentAt(uint32_t i) const { return cap && robots[i].resident; }
    // What the control cycle's translation unit needs of the store, set by navgpu_local_planner_reserve_plans, so that it carries
    // no reference to the feature's launchers (as TrajCloud::terms_pass: it also links without them, tests/tsan).
    // window_pass: k_plan_window for the resident robots of the range with a pose and a plan, their records read into h_rec.
    // (prunePlan per robot: navgpu_fleet::lp_lim[i].prune_plan)
    int (*window_pass)(navgpu_fleet* f, uint32_t first, uint32_t count, const navgpu_robot_input* in, double dist_threshold) = nullptr;
    bool (*goal_pose)(navgpu_fleet* f, uint32_t i, double goal[3]) = nullptr;                    // getGoalPose of a resident robot
    int (*stored_plan)(navgpu_fleet* f, uint32_t i, double* xyyaw, uint32_t capacity) = nullptr;  // navgpu_local_planner_get_plan
  } rp;
  // move_base's executive (navgpu_move_base.cpp): per-robot persistence_end_ and the handover's and the polygon writes' staging,
  // allocated when the first of those calls runs
  struct MoveBaseState {
    int64_t* d_persist = nullptr;                           // [n] MoveBase::persistence_end_ in ns
    PlanPreferIn *d_in = nullptr, *h_in = nullptr;          // [n] a handover's inputs; h_: pinned
    navgpu_handover_record *d_rec = nullptr, *h_rec = nullptr;  // [n] and its records
    uint32_t *d_poly_off = nullptr, *h_poly_off = nullptr;  // [n + 1] a polygon write's vertex offsets
    int32_t *d_poly_ok = nullptr, *h_poly_ok = nullptr;     // [n] and what setConvexPolygonCost returned
    double* d_poly_xy = nullptr;                            // its vertices, grown on demand
    size_t poly_cap = 0;                                    // vertices d_poly_xy holds
  } mb;
  navgpu_local_limits lp_limits{};               // what navgpu_local_planner_configure handed over: sim_period and the latch switch stay fleet-wide
  std::vector<navgpu_local_limits> lp_lim;       // [n] the control cycle's half of every robot's limits (navgpu_planner_set_limits)
  bool lp_configured = false;
  // Per-robot limits (navgpu_planner_set_limits): the planner's half of every robot's record as the host knows it.  A robot whose
  // record has changed is dirty until the next call that stages it or probes it carries the record up to pl.limits (flushLimits):
  // the reach that call works out on the host and the k_samples behind it then see the same limits, in stream order behind
  // whatever cycle is still queued.
  std::vector<RobotLimits> h_limits;             // [n]
  std::vector<uint8_t> limits_dirty;             // [n]
  uint32_t n_limits_dirty = 0;
  double env_vmax = 0.0;                         // the speed the scoring window was planned for: the largest over the records since the last navgpu_planner_configure
  // legacy TrajectoryPlanner (navgpu_tp_*)
  struct TpHost {
    std::vector<double> plan;  // global_plan_ as x, y pairs
    double final_goal_x = 0, final_goal_y = 0;
    bool final_goal_position_valid = false;
    navgpu_tp_state st{};
    std::vector<navgpu_tp_sample> made;  // the generateTrajectory calls of the last cycle, in call order
    int n_points = 0;                    // of the winner
  };
  TpDev tp{};
  bool tp_configured = false;
  std::vector<TpHost> tph;
  std::vector<double> tp_h_samples, tp_h_start;
  std::vector<TpOut> tp_h_out;
  std::vector<uint32_t> tp_h_nsamples, tp_h_within, tp_h_within_count;
  std::vector<int32_t> tp_h_winner;
  // batched scoreTrajectory (navgpu_tp_score_trajectories): what a call hands over - the probes, then the robot of each - as one pinned
  // block and its device twin, and the costs coming back; grown on demand (all four or none) and kept.  Its own buffers: the sample
  // slots, start states and results of the last navgpu_tp_find_best_path stay as that cycle left them.
  struct TpProbes {
    static constexpr size_t kBytesPerProbe = 9 * sizeof(double) + sizeof(uint32_t);
    uint32_t cap = 0;             // probes the buffers hold
    uint8_t *d_in = nullptr, *h_in = nullptr;     // [cap][9] doubles, [cap] robot indices
    double *d_cost = nullptr, *h_cost = nullptr;  // [cap]
  } tpb;
  // the legacy planner for a robot list (navgpu_tp_update_plans_list, navgpu_tp_find_best_path_list), allocated by the first listed
  // call: the list its kernels read, the packed upload (TpStageRec ...) as a pinned block and its device twin, grown on demand, the
  // packed results coming back and the second pass's winners
  struct TpList {
    DeviceList list;
    uint8_t *d_stage = nullptr, *h_stage = nullptr;  // [stage_bytes]
    size_t stage_bytes = 0;
    TpOut *d_out = nullptr, *h_out = nullptr;        // [out_cap] results of the listed robots' samples, packed
    size_t out_cap = 0;
    int32_t *d_win = nullptr, *h_win = nullptr;      // [n] winners by list position
  } tpl;
  // TrajectoryPlannerROS mirror (navgpu_tp_ros.cpp): per-instance controller state, host only
  struct TpRosState {
    std::vector<double> plan;      // global_plan_: (x, y, yaw) triples in the plan's frame (prunePlan shrinks it)
    double T[3] = {0, 0, 0};       // planar plan -> global transform
    bool has_T = false, have_plan = false;
    bool xy_tolerance_latch = false, rotating_to_goal = false, reached_goal = false;  // TrajectoryPlannerROS members
    std::vector<double> transformed;  // transformed_plan of the last cycle (what g_plan_pub_ publishes)
  };
  std::vector<TpRosState> tpr;
  navgpu_tp_ros_params tpr_params{};
  bool tpr_configured = false;
  // footprint-cost queries, rotate recovery, carrot planner (navgpu_recovery.cpp): query staging, grown on demand
  struct FootprintQueries {
    uint32_t cap = 0;             // queries the buffers hold
    double *d_poses = nullptr, *d_costs = nullptr, *h_poses = nullptr, *h_costs = nullptr;  // [cap][3], [cap]; h_: pinned
    uint32_t *d_off = nullptr, *d_first = nullptr, *h_off = nullptr, *h_first = nullptr;    // [n + 1], [n]
  } fq;
  // voxel-layer debug outputs (navgpu_voxel_export.cpp): chunk totals and counts, sized at creation for a voxel fleet; the
  // point buffer grows on demand
  struct VoxelExport {
    uint32_t stride = 0;          // chunk totals per robot: the larger of the two exports' needs
    uint32_t *d_totals = nullptr, *d_counts = nullptr, *d_obs_counts = nullptr;  // [n][stride], [n], [n][max_obs]
    uint32_t *h_counts = nullptr, *h_obs_counts = nullptr;                       // pinned
    void* d_xyz = nullptr;
    size_t xyz_bytes = 0;
  } vx;
  // trajectory cloud (navgpu_traj_cloud.cpp): the robots navgpu_planner_set_trajectory_cloud enabled, each with the records
  // its cycles' terms pass writes - memory that exists only for them - and what the read calls share
  struct TrajCloud {
    struct Robot {
      uint32_t inst = 0;
      SampleTerms* d_terms = nullptr;         // [cap_samples] written by the terms pass
      navgpu_sample_terms* d_out = nullptr;   // [cap_samples] written by k_traj_scan at a read call
      uint32_t cap_samples = 0;
      bool have_cycle = false;                // a cycle has run since the robot was enabled
      uint64_t gen = 0;                       // cycle_gen of that cycle
      double scale[5] = {0, 0, 0, 0, 0};      // the critics' scales at that cycle
    };
    std::vector<Robot> robots;                // at most NAVGPU_TRAJ_CLOUD_MAX_ROBOTS
    // the terms pass navgpu_planner_cycle runs while robots are enabled; set by the enabling call, so that the cycle's
    // translation unit carries no reference to the feature's launchers (it also links without them: tests/tsan)
    int (*terms_pass)(navgpu_fleet* f, uint32_t first, uint32_t count) = nullptr;
    uint32_t* h_totals = nullptr;             // pinned [2]: points, slots (k_traj_scan)
    float* d_points = nullptr;
    size_t points_cap = 0;                    // points d_points holds
  } tc;
  // ObservationBuffer on the device (navgpu_obs_buffer.cpp): per (robot, source) a time-ordered list on the host, newest
  // first, whose entries name ring slots on the device
  struct ObsBuf {
    struct Entry {
      int64_t stamp;
      double origin[3];
      uint32_t slot, n;  // ring slot of the (robot, source); UNFILTERED points (the host never learns the filtered count)
    };
    struct List {
      std::deque<Entry> entries;  // observation_list_
      int64_t last_updated = 0;   // last_updated_
    };
    bool configured = false;
    uint32_t n_sources = 0, slots = 0;
    navgpu_obs_source_params src[NAVGPU_OBSBUF_MAX_SOURCES] = {};
    ObsBufDev dev{};
    std::vector<List> lists;        // [n][n_sources]
    std::vector<uint64_t> evicted;  // [n]
    int64_t last_now = 0;           // `now_ns` of the last call that took one (navgpu_obsbuf_status' `current`)
    // what a call hands over - descriptors, then points, then ranges - as one pinned block and its device twin, grown on demand
    uint8_t *h_in = nullptr, *d_in = nullptr;
    size_t in_bytes = 0;
    hipEvent_t ev_h2d = nullptr;    // behind the copy out of h_in
    bool ev_set = false;
  } ob;
  // batched checkTrajectory (navgpu_planner_check_trajectories): what a call hands over - robot list, offsets, samples - as one
  // pinned block and its device twin, and the costs coming back; grown on demand (all four or none) and kept
  struct Probes {
    uint32_t cap = 0;             // probes the buffers hold
    uint32_t *d_in = nullptr, *h_in = nullptr;    // [n] instances, [n + 1] offsets, [cap][3] samples (floats)
    double *d_cost = nullptr, *h_cost = nullptr;  // [cap]
  } pb;
  // the planner cycle for a robot list (navgpu_planner_*_list), allocated by the first listed call, sized for the whole fleet:
  // the list the cycle's kernels read, and navgpu_planner_stage_list's packed upload - a pinned block and its device twin
  struct CycleList {
    DeviceList list;
    uint8_t *d_stage = nullptr, *h_stage = nullptr; // [n] StageRec, then [n][max_plan][2] doubles (only the poses in use travel)
  } cl;
  // the costmap update for a robot list (navgpu_costmap_*_list), allocated by the first listed call, sized for the whole fleet: the
  // list the update's kernels read, and the listed stages' packed upload - a pinned block and its device twin
  struct CostmapList {
    DeviceList list;
    uint8_t *d_stage = nullptr, *h_stage = nullptr; // [n] CmStageRec, [n][kMaxFootprint][2] doubles, [n][max_obs] ObsCsr, [n][max_points][3] floats (only what is in use travels)
    hipEvent_t ev_stage = nullptr;                  // behind the copy out of h_stage
    bool ev_stage_set = false;
  } cml;
  std::vector<uint32_t> chk_cnt, chk_used;      // [n] checkStageObservations' running counts
  std::vector<uint8_t> obs_consumed;            // [n] an update has run on what navgpu_costmap_stage staged last
  navgpu_rotate_recovery_params rot{0.017, 3.2, 1.0, 0.4, 0.10, 0, 0};  // rotate_recovery.cpp:60-66
  // scratch device buffers
  double* d_bounds_tmp = nullptr;               // [n][4]
  int32_t* d_boxes_tmp = nullptr;               // [n][4]
  float* d_explicit = nullptr;                  // [3]
  int8_t* d_occ = nullptr;
  float4* d_cell_costs = nullptr;                // [cells] navgpu_planner_cost_cloud
  size_t alloc_limit = 0;                       // fault injection (navgpu_fleet_set_alloc_limit); 0 = none
  // profiling
  bool profiling = false;
  uint32_t prof_mask = ~0u;                     // kernels bracketed by events while profiling (navgpu_profile_select)
  std::vector<EventPair> events;
  std::vector<EventPair> free_events;
  double prof_ms[NAVGPU_K_COUNT] = {0};
  uint64_t prof_n[NAVGPU_K_COUNT] = {0};

  template <class T>
  int alloc(T** p, size_t count) {
    void* q = nullptr;
    size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    if (alloc_limit && bytes > alloc_limit) {  // navgpu_fleet_set_alloc_limit: tests make a large allocation fail on purpose
      g_last_error = "hipMalloc: refused by navgpu_fleet_set_alloc_limit";
      return NAVGPU_ERR_HIP;
    }
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
      g_last_error = std::string("hipMalloc: ") + hipGetErrorString(e);
      return NAVGPU_ERR_HIP;
    }
    e = hipMemsetAsync(q, 0, bytes, stream);
    if (e != hipSuccess) {
      g_last_error = std::string("hipMemsetAsync: ") + hipGetErrorString(e);
      return NAVGPU_ERR_HIP;
    }
    allocs.push_back(q);
    *p = static_cast<T*>(q);
    return NAVGPU_OK;
  }
  template <class T>
  int allocPinned(T** p, size_t count) {
    void* q = nullptr;
    hipError_t e = hipHostMalloc(&q, std::max<size_t>(count * sizeof(T), 16), hipHostMallocDefault);
    if (e != hipSuccess) {
      g_last_error = std::string("hipHostMalloc: ") + hipGetErrorString(e);
      return NAVGPU_ERR_HIP;
    }
    memset(q, 0, std::max<size_t>(count * sizeof(T), 16));
    pinned.push_back(q);
    *p = static_cast<T*>(q);
    return NAVGPU_OK;
  }
  void release(void* q) {
    if (!q) return;
    auto it = std::find(allocs.begin(), allocs.end(), q);
    if (it != allocs.end()) allocs.erase(it);
    hipFree(q);
  }
  void releasePinned(void* q) {
    if (!q) return;
    auto it = std::find(pinned.begin(), pinned.end(), q);
    if (it != pinned.end()) pinned.erase(it);
    hipHostFree(q);
  }
  bool rangeOk(uint32_t first, uint32_t count) const { return count > 0 && first < desc.n_instances && count <= desc.n_instances - first; }

  int beginKernel(int k, EventPair* ep) {
    if (!profiling || !((prof_mask >> k) & 1u)) return NAVGPU_OK;
    if (free_events.empty()) {
      EventPair n{};
      HIP_TRY(hipEventCreate(&n.a));
      HIP_TRY(hipEventCreate(&n.b));
      free_events.push_back(n);
    }
    *ep = free_events.back();
    free_events.pop_back();
    ep->kernel = k;
    HIP_TRY(hipEventRecord(ep->a, stream));
    return NAVGPU_OK;
  }
  int endKernel(EventPair* ep) {
    if (!profiling || !ep->a) return NAVGPU_OK;  // (not one of the selected kernels)
    HIP_TRY(hipEventRecord(ep->b, stream));
    events.push_back(*ep);
    if (events.size() > 8192) return foldEvents();
    return NAVGPU_OK;
  }
  int foldEvents() {
    if (events.empty()) return NAVGPU_OK;
    HIP_TRY(waitStream(stream));
    for (auto& e : events) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, e.a, e.b));
      prof_ms[e.kernel] += ms;
      prof_n[e.kernel] += 1;
      free_events.push_back(e);
    }
    events.clear();
    return NAVGPU_OK;
  }
};

inline int navgpu::DeviceList::send(navgpu_fleet* f, const uint32_t* src, uint32_t n) {
  if (src != h) {
    HIP_TRY(wait());
    memcpy(h, src, sizeof(uint32_t) * n);
  }
  HIP_TRY(hipMemcpyAsync(d, h, sizeof(uint32_t) * n, hipMemcpyHostToDevice, f->stream));
  HIP_TRY(hipEventRecord(ev, f->stream));
  set = true;
  return NAVGPU_OK;
}

// lock + "this thread talks to the fleet's GPU" (hipSetDevice is per host thread: a caller's second thread starts on
// device 0 whatever device the fleet lives on)
#ifndef NAVGPU_TEST_NO_FLEET_LOCK
struct FleetGuard {
  std::lock_guard<std::recursive_mutex> lk;
  explicit FleetGuard(navgpu_fleet* f) : lk(f->mu) { (void)hipSetDevice(f->desc.device); }
};
#else  // negative control of tests/test_fleet_threads_tsan.py only: ThreadSanitizer must object to this build
struct FleetGuard {
  explicit FleetGuard(navgpu_fleet* f) { (void)hipSetDevice(f->desc.device); }
};
#endif

#define PROFILED(fleet, kid, launch_expr)            \
  do {                                               \
    EventPair ep_{};                                 \
    int rc_ = (fleet)->beginKernel((kid), &ep_);     \
    if (rc_) return rc_;                             \
    launch_expr;                                     \
    rc_ = (fleet)->endKernel(&ep_);                  \
    if (rc_) return rc_;                             \
  } while (0)

inline int checkLaunch() {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_last_error = std::string("kernel launch: ") + hipGetErrorString(e);
    return NAVGPU_ERR_HIP;
  }
  return NAVGPU_OK;
}

