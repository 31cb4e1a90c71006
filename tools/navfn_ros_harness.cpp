// Drives the reference's own navfn::NavFn (navfn/src/navfn.cpp, compiled in place by tools/make_navfn_ros_goldens.py) exactly as
// NavfnROS::makePlan and getPlanFromPotential drive it (navfn_ros.cpp:263-299, 426-437), one NavFn object per case, and writes the
// potential array and the second path it leaves.  The message and console headers come from tests/ros_stubs/.
//   in : int64 n_cases; per case: int32 nx, ny, allow_unknown, robot[2], goal[2], best[2] (best[0] < 0: no second path), ny x nx cost bytes
//   out: per case: int32 calcNavFnDijkstra's return value, ny x nx float potarr, int32 calcPath's return value (0: the walk failed),
//        int32 n = getPathLen() (after a failed walk: the points walked so far, which getPlanFromPotential takes for a plan), n x {x, y} float
#include <cstdint>
#include <cstdio>
#include <vector>

#include <navfn/navfn.h>

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  int64_t n_cases = 0;
  if (fread(&n_cases, sizeof n_cases, 1, in) != 1) return 3;
  for (int64_t c = 0; c < n_cases; ++c) {
    int32_t hdr[9];
    if (fread(hdr, sizeof(int32_t), 9, in) != 9) return 3;
    const int nx = hdr[0], ny = hdr[1];
    std::vector<unsigned char> cmap((size_t)nx * ny);
    if (fread(cmap.data(), 1, cmap.size(), in) != cmap.size()) return 3;
    navfn::NavFn planner(nx, ny);
    planner.setNavArr(nx, ny);
    planner.setCostmap(cmap.data(), true, hdr[2] != 0);
    int map_start[2] = {hdr[3], hdr[4]}, map_goal[2] = {hdr[5], hdr[6]}, best[2] = {hdr[7], hdr[8]};
    planner.setStart(map_goal);
    planner.setGoal(map_start);
    const int32_t found = planner.calcNavFnDijkstra(true) ? 1 : 0;
    fwrite(&found, sizeof found, 1, out);
    fwrite(planner.potarr, sizeof(float), (size_t)nx * ny, out);
    int32_t len = 0, ret = 0;
    if (best[0] >= 0) {
      planner.setStart(best);
      ret = planner.calcPath(nx * 4);
      len = planner.getPathLen();
    }
    fwrite(&ret, sizeof ret, 1, out);
    fwrite(&len, sizeof len, 1, out);
    for (int32_t i = 0; i < len; ++i) {
      const float xy[2] = {planner.getPathX()[i], planner.getPathY()[i]};
      fwrite(xy, sizeof(float), 2, out);
    }
  }
  fclose(out);
  fclose(in);
  return 0;
}
