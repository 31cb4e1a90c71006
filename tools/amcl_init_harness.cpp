// Driver for the reference amcl core's filter initialisation (pf/, map/ and sensors/amcl_laser.cpp compiled in place, see
// tools/amcl_reference_build.py).  Used by tools/make_amcl_init_goldens.py to write tests/golden/g12_amcl_init.npz.
//
//   amcl_init_harness gauss <in.f64> <out.f64>
//       in:  max_samples seed mean[3] cov[9]       pf_init with pf_pdf_seed reaching `seed` (seed - 1 allocations made first)
//   amcl_init_harness uniform <in.f64> <occ.i8> <out.f64>
//       in:  sx sy scale ox oy max_occ_dist | the 24 laser parameters of amcl_golden_harness | laser x y th |
//            max_samples threshold multiplier has_scan state range_count range_max | ranges[2 range_count]
//       pf_init_model with the node's uniformPoseGenerator, restated below from amcl_node.cpp:1200-1263
//   out: state_after ms used leaf_count cluster_count n_chosen n_scores set_mean[3] set_cov[9] |
//        cluster_count x {count weight mean[3] cov[9]} in order of each cluster's lowest sample index | poses[3 max_samples] |
//        chosen[n_chosen] (candidate index of each sample) | scores[n_scores] (every candidate's score, scored runs only)
// The drand48 state travels as a double, which holds its 48 bits exactly.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <vector>

extern "C" {  // these headers declare C functions without a linkage block of their own
#include "amcl/pf/pf_vector.h"
#include "amcl/pf/pf_kdtree.h"
#include "amcl/pf/pf_pdf.h"
}
#include "amcl/map/map.h"
#include "amcl/pf/pf.h"
#include "amcl/sensors/amcl_laser.h"

namespace {
std::vector<char> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  std::vector<char> b;
  char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + n);
  fclose(f);
  return b;
}
void spit(const char* path, const std::vector<double>& v) {
  FILE* f = fopen(path, "wb");
  if (!f || fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) {
    perror(path);
    exit(2);
  }
  fclose(f);
}
void seedState(uint64_t x) {
  unsigned short s[3] = {(unsigned short)(x & 0xFFFF), (unsigned short)(x >> 16 & 0xFFFF), (unsigned short)(x >> 32 & 0xFFFF)};
  seed48(s);
}
uint64_t readState() {  // seed48 returns the previous state; put it back at once
  unsigned short z[3] = {0, 0, 0};
  const unsigned short* p = seed48(z);
  unsigned short s[3] = {p[0], p[1], p[2]};
  seed48(s);
  return (uint64_t)s[0] | (uint64_t)s[1] << 16 | (uint64_t)s[2] << 32;
}
pf_vector_t noPose(void*) { return pf_vector_zero(); }

// What one init leaves: the set, its leaf count and its clusters, renumbered by their lowest sample index
void describe(pf_t* pf, uint64_t state, double ms, double used, const std::vector<double>& chosen, const std::vector<double>& scores,
              std::vector<double>& out) {
  pf_sample_set_t* set = pf->sets + pf->current_set;
  std::vector<int> order;  // cluster labels by first sample
  for (int i = 0; i < set->sample_count; ++i) {
    const int c = pf_kdtree_get_cluster(set->kdtree, set->samples[i].pose);
    bool seen = false;
    for (int o : order) seen = seen || o == c;
    if (!seen) order.push_back(c);
  }
  out = {(double)state, ms, used, (double)set->kdtree->leaf_count, (double)set->cluster_count, (double)chosen.size(), (double)scores.size()};
  for (int a = 0; a < 3; ++a) out.push_back(set->mean.v[a]);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) out.push_back(set->cov.m[a][b]);
  for (int c : order) {
    const pf_cluster_t& cl = set->clusters[c];
    out.push_back(cl.count);
    out.push_back(cl.weight);
    for (int a = 0; a < 3; ++a) out.push_back(cl.mean.v[a]);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) out.push_back(cl.cov.m[a][b]);
  }
  for (int i = 0; i < set->sample_count; ++i)
    for (int a = 0; a < 3; ++a) out.push_back(set->samples[i].pose.v[a]);
  out.insert(out.end(), chosen.begin(), chosen.end());
  out.insert(out.end(), scores.begin(), scores.end());
}

double msSince(const timespec& t0) {
  timespec t1;
  clock_gettime(CLOCK_MONOTONIC, &t1);
  return (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
}

// The node's state for its pose generator (amcl_node.cpp:1200-1263, restated)
struct Node {
  map_t* map = nullptr;
  std::vector<std::pair<int, int>> free_cells;
  amcl::AMCLLaserData* scan = nullptr;  // last_laser_data_
  double threshold = 0, multiplier = 0;
  long candidates = 0;
  std::vector<double> chosen, scores;
  bool scored = false;

  pf_vector_t freePose() {  // randomFreeSpacePose: the cell first, then theta
    pf_vector_t p;
    const unsigned idx = drand48() * free_cells.size();
    p.v[0] = MAP_WXGX(map, free_cells[idx].first);
    p.v[1] = MAP_WYGY(map, free_cells[idx].second);
    p.v[2] = drand48() * 2 * M_PI - M_PI;
    ++candidates;
    return p;
  }
  double score(const pf_vector_t& p) {  // scorePose: a one-sample set of weight 1.0, unconverged
    pf_sample_t s;
    s.pose = p;
    s.weight = 1.0;
    pf_sample_set_t set;
    memset(&set, 0, sizeof(set));
    set.sample_count = 1;
    set.samples = &s;
    set.converged = 0;
    amcl::AMCLLaser::ApplyModelToSampleSet(scan, &set);
    scores.push_back(s.weight);
    return s.weight;
  }
  static pf_vector_t generate(void* arg) {  // uniformPoseGenerator
    Node* self = static_cast<Node*>(arg);
    double gw = self->threshold;
    pf_vector_t p = self->freePose();
    if (self->scored)
      while (self->score(p) < gw) {
        p = self->freePose();
        gw *= self->multiplier;
      }
    self->chosen.push_back((double)(self->candidates - 1));
    return p;
  }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "gauss")) {
    const std::vector<char> ib = slurp(argv[2]);
    const double* q = reinterpret_cast<const double*>(ib.data());
    const int ms = (int)q[0], seed = (int)q[1];
    pf_vector_t mean;
    pf_matrix_t cov;
    for (int a = 0; a < 3; ++a) mean.v[a] = q[2 + a];
    for (int a = 0; a < 9; ++a) cov.m[a / 3][a % 3] = q[5 + a];
    for (int k = 1; k < seed; ++k) pf_pdf_gaussian_free(pf_pdf_gaussian_alloc(mean, cov));  // pf_pdf_seed reaches seed - 1
    pf_t* pf = pf_alloc(ms, ms, 0.001, 0.1, noPose, nullptr);
    timespec t0;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    pf_init(pf, mean, cov);
    const double t = msSince(t0);
    std::vector<double> out;
    describe(pf, readState(), t, 0, {}, {}, out);
    spit(argv[3], out);
    pf_free(pf);
    return 0;
  }
  if (argc != 5 || strcmp(argv[1], "uniform")) {
    fprintf(stderr, "usage: %s gauss in out | uniform in occ out\n", argv[0]);
    return 2;
  }
  const std::vector<char> ib = slurp(argv[2]);
  const std::vector<char> occ = slurp(argv[3]);
  const double* q = reinterpret_cast<const double*>(ib.data());
  const int sx = (int)q[0], sy = (int)q[1];
  map_t* m = map_alloc();
  m->size_x = sx;
  m->size_y = sy;
  m->scale = q[2];
  m->origin_x = q[3];
  m->origin_y = q[4];
  m->cells = (map_cell_t*)malloc(sizeof(map_cell_t) * (size_t)sx * sy);
  for (size_t i = 0; i < occ.size(); ++i) m->cells[i].occ_state = (int8_t)occ[i];
  const double max_occ_dist = q[5];
  q += 6;
  const int model = (int)q[0], max_beams = (int)q[1];
  amcl::AMCLLaser laser(max_beams, m);
  switch (model) {
    case 0:
      laser.SetModelBeam(q[2], q[3], q[4], q[5], q[6], q[7], q[8]);
      map_update_cspace(m, max_occ_dist);
      break;
    case 1: laser.SetModelLikelihoodField(q[2], q[5], q[6], max_occ_dist); break;
    case 2: laser.SetModelLikelihoodFieldProb(q[2], q[5], q[6], max_occ_dist, q[9] != 0, q[10], q[11], q[12]); break;
    default: laser.SetModelLikelihoodFieldGompertz(q[2], q[5], q[6], max_occ_dist, q[13], q[14], q[15], q[16], q[17], q[18]); break;
  }
  const double radius = q[21];
  laser.SetMapFactors(q[19], q[20], radius);
  q += 24;
  pf_vector_t laser_pose = pf_vector_zero();
  for (int a = 0; a < 3; ++a) laser_pose.v[a] = q[a];
  laser.SetLaserPose(laser_pose);
  q += 3;
  const int ms = (int)q[0];
  Node node;
  node.map = m;
  node.threshold = q[1];
  node.multiplier = q[2];
  const bool has_scan = q[3] != 0;
  const uint64_t state = (uint64_t)q[4];
  const int range_count = (int)q[5];
  const double range_max = q[6];
  q += 7;
  amcl::AMCLLaserData data;
  data.sensor = &laser;
  data.range_count = range_count;
  data.range_max = range_max;
  data.ranges = new double[range_count > 0 ? range_count : 1][2];
  for (int i = 0; i < range_count; ++i) {
    data.ranges[i][0] = q[2 * i];
    data.ranges[i][1] = q[2 * i + 1];
  }
  node.scan = has_scan ? &data : nullptr;
  node.scored = has_scan && node.threshold > 0.0 && node.multiplier < 1.0 && node.multiplier >= 0.0;
  for (int i = 0; i < sx; i++)  // free_space_indices (amcl_node.cpp:1026-1033)
    for (int j = 0; j < sy; j++)
      if (m->cells[MAP_INDEX(m, i, j)].occ_state == -1 && map_occ_dist(m, i, j) > radius) node.free_cells.push_back({i, j});
  pf_t* pf = pf_alloc(ms, ms, 0.001, 0.1, noPose, nullptr);
  seedState(state);
  timespec t0;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  pf_init_model(pf, Node::generate, &node);
  const double t = msSince(t0);
  std::vector<double> out;
  describe(pf, readState(), t, (double)node.candidates, node.chosen, node.scores, out);
  spit(argv[4], out);
  pf_free(pf);
  map_free(m);
  return 0;
}
