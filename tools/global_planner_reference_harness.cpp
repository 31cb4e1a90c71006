// Drives the reference's own global_planner classes (dijkstra.cpp, astar.cpp, gradient_path.cpp, grid_path.cpp and
// quadratic_calculator.cpp, compiled in place by tools/make_global_planner_goldens.py against the stand-in
// tools/global_planner_ref_stubs/global_planner/planner_core.h) exactly as GlobalPlanner does (global_planner/src/planner_core.cpp):
//   initialize (:109-141)    QuadraticCalculator or PotentialCalculator; DijkstraExpansion, with setPreciseStart(true) unless
//                            old_navfn_behavior, or AStarExpansion; GridPath or GradientPath; setHasUnknown
//   reconfigureCB (:168-171) setLethalCost on the expander and the traceback, setNeutralCost and setFactor - all through the
//                            Expander* / Traceback* members.  Expander::setNeutralCost is not virtual (expander.h:67), so
//                            DijkstraExpansion's own, which would recompute priorityIncrement_, is never the one called
//   makePlan (:291-308)      the three setSize calls, calculatePotentials with nx * ny * 2 cycles, clearEndpoint(..., 2) unless
//                            old_navfn_behavior, getPath when a legal potential was found
// The costmap arrives as makePlan's calculatePotentials sees it: robot cell cleared and border outlined by the caller.
//   in : int64 n_plans; per plan: int32 nx, ny, use_dijkstra, use_quadratic, use_grid_path, old_navfn_behavior, allow_unknown,
//        lethal_cost, neutral_cost, goal_x_i, goal_y_i; double cost_factor, start_x, start_y, goal_x, goal_y; ny x nx cost bytes
//   out: per plan: int32 found_legal; ny x nx float potential before clearEndpoint; ny x nx float potential after it;
//        int32 getPath's return value (-1: not called); int32 n; n x {x, y} float, the points getPath left (also when it returned false)
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include <global_planner/astar.h>
#include <global_planner/dijkstra.h>
#include <global_planner/gradient_path.h>
#include <global_planner/grid_path.h>
#include <global_planner/quadratic_calculator.h>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int64_t n_plans = 0;
  if (fread(&n_plans, sizeof n_plans, 1, in) != 1) return 3;
  for (int64_t c = 0; c < n_plans; ++c) {
    int32_t h[11];
    double d[5];
    if (fread(h, sizeof(int32_t), 11, in) != 11 || fread(d, sizeof(double), 5, in) != 5) return 3;
    const int nx = h[0], ny = h[1];
    const bool use_dijkstra = h[2] != 0, use_quadratic = h[3] != 0, use_grid_path = h[4] != 0, old_navfn_behavior = h[5] != 0;
    std::vector<unsigned char> costs((size_t)nx * ny);
    if (fread(costs.data(), 1, costs.size(), in) != costs.size()) return 3;

    global_planner::PotentialCalculator* p_calc;
    if (use_quadratic)
      p_calc = new global_planner::QuadraticCalculator(nx, ny);
    else
      p_calc = new global_planner::PotentialCalculator(nx, ny);
    global_planner::Expander* planner;
    if (use_dijkstra) {
      global_planner::DijkstraExpansion* de = new global_planner::DijkstraExpansion(p_calc, nx, ny);
      if (!old_navfn_behavior) de->setPreciseStart(true);
      planner = de;
    } else {
      planner = new global_planner::AStarExpansion(p_calc, nx, ny);
    }
    global_planner::Traceback* path_maker;
    if (use_grid_path)
      path_maker = new global_planner::GridPath(p_calc);
    else
      path_maker = new global_planner::GradientPath(p_calc);
    planner->setHasUnknown(h[6] != 0);
    planner->setLethalCost(h[7]);
    path_maker->setLethalCost(h[7]);
    planner->setNeutralCost(h[8]);
    planner->setFactor(d[0]);

    p_calc->setSize(nx, ny);
    planner->setSize(nx, ny);
    path_maker->setSize(nx, ny);
    std::vector<float> potential((size_t)nx * ny);
    const int32_t found_legal = planner->calculatePotentials(costs.data(), d[1], d[2], d[3], d[4], nx * ny * 2, potential.data()) ? 1 : 0;
    fwrite(&found_legal, sizeof found_legal, 1, out);
    fwrite(potential.data(), sizeof(float), potential.size(), out);
    if (!old_navfn_behavior) planner->clearEndpoint(costs.data(), potential.data(), h[9], h[10], 2);
    fwrite(potential.data(), sizeof(float), potential.size(), out);
    std::vector<std::pair<float, float> > path;
    int32_t ret = -1;
    if (found_legal) ret = path_maker->getPath(potential.data(), d[1], d[2], d[3], d[4], path) ? 1 : 0;
    const int32_t n = (int32_t)path.size();
    fwrite(&ret, sizeof ret, 1, out);
    fwrite(&n, sizeof n, 1, out);
    for (int32_t i = 0; i < n; ++i) {
      const float xy[2] = {path[i].first, path[i].second};
      fwrite(xy, sizeof(float), 2, out);
    }
    // (nothing is deleted: Expander and Traceback have no virtual destructor, and the process ends after a few dozen small plans)
  }
  fclose(out);
  fclose(in);
  return 0;
}
