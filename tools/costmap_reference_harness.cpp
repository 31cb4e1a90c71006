// Runs costmap update cycles through the reference's own classes, compiled in place by tools/make_costmap_goldens.py, and writes what
// they compute.  Nothing of the project (oracle or kernels) is linked.
//
// Wiring, per case: a costmap_2d::LayeredCostmap with, in plugin order, a StaticLayer, an ObstacleLayer or VoxelLayer and an
// InflationLayer (any subset), each followed by a Recorder: a Layer of this file that touches no bounds and copies the master grid and
// the box LayeredCostmap::updateMap hands to updateCosts.  The layers are initialised the way costmap_2d/testing_helper.h does it
// (initialize + addPlugin, no observation source), sized through LayeredCostmap::resizeMap, and driven through
// LayeredCostmap::setFootprint, ObstacleLayer::addStaticObservation / clearStaticObservations, InflationLayer::setInflationParameters
// and LayeredCostmap::updateMap.
//   StaticLayer    its parameters go through the parameter table of the ros::NodeHandle stand-in, so StaticLayer::onInitialize itself
//                  clamps and converts them; first_map_only keeps it from waiting for a map server (tools/costmap_ref_stubs/ros/ros.h),
//                  and the map arrives through StaticLayer::incomingMap.  nav_msgs/MapMetaData carries the resolution as a float32.
//   Obstacle/Voxel combination_method, footprint_clearing_enabled, max_obstacle_height and the voxel parameters go through the layers'
//                  own reconfigureCB.
// incomingMap, the reconfigureCB members and VoxelLayer's voxel grid are private.  The reference headers are therefore included with
// private and protected opened; the reference's sources are compiled unchanged (the Itanium C++ ABI lays classes out the same way
// whatever the access of their members).
//
// in : int64 n_cases; per case int64 n, n doubles:
//      size_x, size_y, resolution, origin_x, origin_y, rolling_window, track_unknown,
//      has_static, map size_x, size_y, resolution, origin_x, origin_y, track_unknown_space, use_maximum, trinary_costmap,
//        lethal_cost_threshold, unknown_cost_value,
//      obstacle kind (0 none, 1 ObstacleLayer, 2 VoxelLayer), combination_method, footprint_clearing_enabled, max_obstacle_height,
//        z_voxels, origin_z, z_resolution, unknown_threshold, mark_threshold,
//      has_inflation, inflation_radius, cost_scaling_factor,
//      n_fp, n_fp x {x, y}, the occupancy values (map size_x * size_y, when has_static), n_cycles, per cycle:
//      pose[3], n_new_fp (0: the footprint stays), n_new_fp x {x, y}, new_inflation (0 / 1), inflation_radius, cost_scaling_factor,
//      n_obs, per observation origin[3], obstacle_range, raytrace_range, marking, clearing, n_points, n_points x {x, y, z} (float32 values).
// out: per case int64 n_bytes, then per cycle: origin x, y (double); the box x0, xn, y0, yn (int32); the obstacle / voxel layer's grid
//      (when there is one); the voxel words (uint32, VoxelLayer); the master grid behind each layer present, in plugin order; and with an
//      InflationLayer: the cell inflation radius R (int32), LayeredCostmap::getInscribedRadius() (double) and
//      InflationLayer::computeCost(hypot(i, j)) for i, j <= R + 1 (i major).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

// the standard library and the stand-ins first, so that only the reference's own headers see the opened access
#include <algorithm>
#include <list>
#include <map>
#include <queue>
#include <set>
#include <sstream>
#include <string>
#include <boost/thread.hpp>
#include <ros/ros.h>
#include <tf/transform_listener.h>
#include <tf/message_filter.h>
#include <message_filters/subscriber.h>
#include <dynamic_reconfigure/server.h>
#include <laser_geometry/laser_geometry.h>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <nav_msgs/OccupancyGrid.h>
#include <map_msgs/OccupancyGridUpdate.h>
#include <sensor_msgs/LaserScan.h>
#include <sensor_msgs/PointCloud.h>
#include <sensor_msgs/PointCloud2.h>

#define private public
#define protected public
#include <costmap_2d/layered_costmap.h>
#include <costmap_2d/static_layer.h>
#include <costmap_2d/obstacle_layer.h>
#include <costmap_2d/voxel_layer.h>
#include <costmap_2d/inflation_layer.h>
#undef private
#undef protected

namespace {

struct Reader {
  const double* p;
  const double* end;
  double next() {
    if (p >= end) {
      fprintf(stderr, "costmap_reference_harness: case input too short\n");
      exit(3);
    }
    return *p++;
  }
  int i() { return (int)next(); }
};

struct Writer {
  std::vector<uint8_t> bytes;
  void put(const void* p, size_t n) { bytes.insert(bytes.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
  void f64(double v) { put(&v, 8); }
  void i32(int32_t v) { put(&v, 4); }
};

// copies what LayeredCostmap::updateMap hands the layer in front of it
class Recorder : public costmap_2d::Layer {
 public:
  bool called = false;
  int box[4] = {0, 0, 0, 0};
  std::vector<uint8_t> cells;
  virtual void updateCosts(costmap_2d::Costmap2D& master, int min_i, int min_j, int max_i, int max_j) {
    called = true;
    box[0] = min_i, box[1] = max_i, box[2] = min_j, box[3] = max_j;
    const size_t n = (size_t)master.getSizeInCellsX() * master.getSizeInCellsY();
    cells.assign(master.getCharMap(), master.getCharMap() + n);
  }
};

std::vector<geometry_msgs::Point> readFootprint(Reader& in, int n) {
  std::vector<geometry_msgs::Point> fp(n);
  for (int k = 0; k < n; ++k) {
    fp[k].x = in.next();
    fp[k].y = in.next();
    fp[k].z = 0.0;
  }
  return fp;
}

void runCase(Reader& in, Writer& out) {
  std::map<std::string, double>& params = dwa_ref::params();
  params.clear();
  const int size_x = in.i(), size_y = in.i();
  const double res = in.next(), ox = in.next(), oy = in.next();
  const bool rolling = in.i() != 0, track_unknown = in.i() != 0;
  const bool has_static = in.i() != 0;
  const int st_sx = in.i(), st_sy = in.i();
  const double st_res = in.next(), st_ox = in.next(), st_oy = in.next();
  const int st_track = in.i(), st_max = in.i(), st_trinary = in.i(), st_lethal = in.i(), st_unknown = in.i();
  const int obstacle_kind = in.i();
  const int comb = in.i(), fpclear = in.i();
  const double max_h = in.next();
  const int z_voxels = in.i();
  const double origin_z = in.next(), z_res = in.next();
  const int unknown_thr = in.i(), mark_thr = in.i();
  const bool has_inflation = in.i() != 0;
  const double radius = in.next(), scaling = in.next();
  const int n_fp = in.i();
  std::vector<geometry_msgs::Point> footprint = readFootprint(in, n_fp);

  tf::TransformListener tf;
  costmap_2d::LayeredCostmap layers("frame", rolling, track_unknown);
  costmap_2d::StaticLayer* slayer = NULL;
  costmap_2d::ObstacleLayer* olayer = NULL;
  costmap_2d::VoxelLayer* vlayer = NULL;
  costmap_2d::InflationLayer* ilayer = NULL;
  std::vector<Recorder*> recorders;
  auto addRecorder = [&]() {
    Recorder* r = new Recorder();
    r->initialize(&layers, "recorder", &tf);
    layers.addPlugin(boost::shared_ptr<costmap_2d::Layer>(r));
    recorders.push_back(r);
  };
  // the master has its size before the layers come, as in Costmap2DROS with a fixed-size or rolling costmap
  layers.resizeMap(size_x, size_y, res, ox, oy);
  if (has_static) {
    params["first_map_only"] = 1;
    params["track_unknown_space"] = st_track;
    params["use_maximum"] = st_max;
    params["trinary_costmap"] = st_trinary;
    params["lethal_cost_threshold"] = st_lethal;
    params["unknown_cost_value"] = st_unknown;
    slayer = new costmap_2d::StaticLayer();
    layers.addPlugin(boost::shared_ptr<costmap_2d::Layer>(slayer));
    slayer->initialize(&layers, "static", &tf);
    params.clear();
    addRecorder();
  }
  if (obstacle_kind) {
    if (obstacle_kind == 2)
      olayer = vlayer = new costmap_2d::VoxelLayer();
    else
      olayer = new costmap_2d::ObstacleLayer();
    olayer->initialize(&layers, "obstacles", &tf);
    layers.addPlugin(boost::shared_ptr<costmap_2d::Layer>(olayer));
    if (vlayer) {
      costmap_2d::VoxelPluginConfig c;
      c.enabled = true;
      c.footprint_clearing_enabled = fpclear != 0;
      c.max_obstacle_height = max_h;
      c.z_voxels = z_voxels;
      c.origin_z = origin_z;
      c.z_resolution = z_res;
      c.unknown_threshold = unknown_thr;
      c.mark_threshold = mark_thr;
      c.combination_method = comb;
      vlayer->reconfigureCB(c, 0);
    } else {
      costmap_2d::ObstaclePluginConfig c;
      c.enabled = true;
      c.footprint_clearing_enabled = fpclear != 0;
      c.max_obstacle_height = max_h;
      c.combination_method = comb;
      olayer->reconfigureCB(c, 0);
    }
    addRecorder();
  }
  if (has_inflation) {
    ilayer = new costmap_2d::InflationLayer();
    ilayer->initialize(&layers, "inflation", &tf);
    layers.addPlugin(boost::shared_ptr<costmap_2d::Layer>(ilayer));
    ilayer->setInflationParameters(radius, scaling);
    addRecorder();
  }
  if (has_static) {
    nav_msgs::OccupancyGrid* grid = new nav_msgs::OccupancyGrid();
    nav_msgs::OccupancyGridConstPtr msg(grid);
    grid->header.frame_id = "frame";
    grid->info.width = st_sx;
    grid->info.height = st_sy;
    grid->info.resolution = (float)st_res;
    grid->info.origin.position.x = st_ox;
    grid->info.origin.position.y = st_oy;
    grid->data.resize((size_t)st_sx * st_sy);
    for (size_t k = 0; k < grid->data.size(); ++k) grid->data[k] = (int8_t)in.i();
    slayer->incomingMap(msg);
  }
  layers.setFootprint(footprint);
  costmap_2d::Costmap2D* master = layers.getCostmap();
  if ((int)master->getSizeInCellsX() != size_x || (int)master->getSizeInCellsY() != size_y || master->getResolution() != res) {
    fprintf(stderr, "costmap_reference_harness: the static map resized the master: give the case the map's float32 resolution\n");
    exit(4);
  }
  const size_t n_cells = (size_t)size_x * size_y;

  const int n_cycles = in.i();
  for (int cyc = 0; cyc < n_cycles; ++cyc) {
    const double rx = in.next(), ry = in.next(), ryaw = in.next();
    const int n_new_fp = in.i();
    if (n_new_fp) layers.setFootprint(readFootprint(in, n_new_fp));
    const int new_inflation = in.i();
    const double new_radius = in.next(), new_scaling = in.next();
    if (new_inflation && ilayer) ilayer->setInflationParameters(new_radius, new_scaling);
    const int n_obs = in.i();
    if (olayer) olayer->clearStaticObservations(true, true);
    for (int k = 0; k < n_obs; ++k) {
      geometry_msgs::Point origin;
      origin.x = in.next(), origin.y = in.next(), origin.z = in.next();
      const double obstacle_range = in.next(), raytrace_range = in.next();
      const bool marking = in.i() != 0, clearing = in.i() != 0;
      const int n_points = in.i();
      pcl::PointCloud<pcl::PointXYZ> cloud;
      cloud.points.resize(n_points);
      for (int q = 0; q < n_points; ++q) {
        cloud.points[q].x = (float)in.next();
        cloud.points[q].y = (float)in.next();
        cloud.points[q].z = (float)in.next();
      }
      costmap_2d::Observation obs(origin, cloud, obstacle_range, raytrace_range);
      if (olayer) olayer->addStaticObservation(obs, marking, clearing);
    }
    for (Recorder* r : recorders) r->called = false;
    layers.updateMap(rx, ry, ryaw);

    out.f64(master->getOriginX());
    out.f64(master->getOriginY());
    unsigned int x0, xn, y0, yn;
    layers.getBounds(&x0, &xn, &y0, &yn);
    const int box[4] = {(int)x0, (int)xn, (int)y0, (int)yn};
    for (int k = 0; k < 4; ++k) out.i32(box[k]);
    if (olayer) out.put(olayer->getCharMap(), n_cells);
    if (vlayer) out.put(vlayer->voxel_grid_.getData(), n_cells * 4);
    for (Recorder* r : recorders) {
      if (r->called) {
        if (memcmp(r->box, box, sizeof(box)) != 0) {
          fprintf(stderr, "costmap_reference_harness: updateCosts saw another box than getBounds reports\n");
          exit(5);
        }
        out.put(r->cells.data(), n_cells);
      } else {
        out.put(master->getCharMap(), n_cells);  // an empty box: updateMap returned before the layers' updateCosts
      }
    }
    if (ilayer) {
      const int R = (int)master->cellDistance(ilayer->inflation_radius_);
      out.i32(R);
      out.f64(layers.getInscribedRadius());
      for (int i = 0; i <= R + 1; ++i)
        for (int j = 0; j <= R + 1; ++j) {
          const uint8_t c = ilayer->computeCost(hypot(i, j));
          out.put(&c, 1);
        }
    }
  }
  if (in.p != in.end) {
    fprintf(stderr, "costmap_reference_harness: case input too long\n");
    exit(3);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  int64_t n_cases = 0;
  if (fread(&n_cases, 8, 1, fi) != 1) return 2;
  for (int64_t c = 0; c < n_cases; ++c) {
    int64_t n = 0;
    if (fread(&n, 8, 1, fi) != 1) return 2;
    std::vector<double> d(n);
    if ((int64_t)fread(d.data(), 8, n, fi) != n) return 2;
    Reader in{d.data(), d.data() + n};
    Writer out;
    runCase(in, out);
    const int64_t n_bytes = (int64_t)out.bytes.size();
    fwrite(&n_bytes, 8, 1, fo);
    fwrite(out.bytes.data(), 1, out.bytes.size(), fo);
  }
  fclose(fi);
  fclose(fo);
  return 0;
}
