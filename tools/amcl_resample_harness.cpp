// Driver for the reference amcl core's resampling (pf/ compiled in place, see tools/amcl_reference_build.py): builds a pf_t,
// creates its set with pf_init_model from a pose list, overwrites the weights and w_slow / w_fast, seeds drand48 and runs
// pf_update_resample once.  Used by tools/make_amcl_resample_goldens.py to write tests/golden/g10_amcl_resample.npz.
//
//   amcl_resample_harness <in.f64> <out.f64>
//   in:  model min_samples max_samples pop_err pop_z dist_threshold w_slow w_fast seed pool_count
//        | poses[3 max_samples] weights[max_samples] pool[3 pool_count]
//   out: leaf_in sample_count w_slow w_fast leaf_count cluster_count converged pool_used next_drand48 ms
//        | poses[3 sample_count] weights[sample_count] cluster_of_sample[sample_count]
//        | per cluster {count weight mean[3] cov[9]} | set mean[3] cov[9]
// random_pose_fn pops the recorded pool, so the only drand48() calls are pf_update_resample's own; next_drand48 is the value
// drawn right after it, which lets the tool check its replay of the stream.
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <vector>

extern "C" {  // pf_kdtree.h has no C++ guard of its own; included first, pf.h's own include of it is then a no-op
#include "amcl/pf/pf_vector.h"
#include "amcl/pf/pf_kdtree.h"
}
#include "amcl/pf/pf.h"

namespace {
std::vector<double> slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  std::vector<double> b;
  double buf[4096];
  size_t n;
  while ((n = fread(buf, sizeof(double), 4096, f)) > 0) b.insert(b.end(), buf, buf + n);
  fclose(f);
  return b;
}
struct PoseList {
  const double* p;
  int n, next;
};
pf_vector_t popPose(void* data) {
  PoseList* l = static_cast<PoseList*>(data);
  if (l->next >= l->n) {
    fprintf(stderr, "pose list exhausted\n");
    exit(3);
  }
  pf_vector_t v = pf_vector_zero();
  for (int a = 0; a < 3; ++a) v.v[a] = l->p[3 * l->next + a];
  l->next++;
  return v;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s in out\n", argv[0]);
    return 2;
  }
  const std::vector<double> in = slurp(argv[1]);
  const double* q = in.data();
  const int model = (int)q[0], min_samples = (int)q[1], max_samples = (int)q[2];
  const double pop_err = q[3], pop_z = q[4], dist_threshold = q[5], w_slow = q[6], w_fast = q[7];
  const long seed = (long)q[8];
  const int pool_count = (int)q[9];
  q += 10;
  PoseList init{q, max_samples, 0};
  const double* weights = q + 3 * max_samples;
  PoseList pool{weights + max_samples, pool_count, 0};

  pf_t* pf = pf_alloc(min_samples, max_samples, 0.001, 0.1, popPose, &pool);
  pf_set_resample_model(pf, model ? PF_RESAMPLE_SYSTEMATIC : PF_RESAMPLE_MULTINOMIAL);
  pf->pop_err = pop_err;
  pf->pop_z = pop_z;
  pf->dist_threshold = dist_threshold;
  pf_init_model(pf, popPose, &init);
  pf_sample_set_t* a = pf->sets + pf->current_set;
  const int leaf_in = a->kdtree->leaf_count;
  for (int i = 0; i < a->sample_count; ++i) a->samples[i].weight = weights[i];
  pf->w_slow = w_slow;
  pf->w_fast = w_fast;

  srand48(seed);
  timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  pf_update_resample(pf);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  const double next = drand48();

  pf_sample_set_t* b = pf->sets + pf->current_set;
  std::vector<double> out = {(double)leaf_in, (double)b->sample_count, pf->w_slow, pf->w_fast, (double)b->kdtree->leaf_count,
                             (double)b->cluster_count, (double)b->converged, (double)pool.next, next,
                             (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6};
  for (int i = 0; i < b->sample_count; ++i)
    for (int k = 0; k < 3; ++k) out.push_back(b->samples[i].pose.v[k]);
  for (int i = 0; i < b->sample_count; ++i) out.push_back(b->samples[i].weight);
  for (int i = 0; i < b->sample_count; ++i) out.push_back(pf_kdtree_get_cluster(b->kdtree, b->samples[i].pose));
  for (int c = 0; c < b->cluster_count; ++c) {
    const pf_cluster_t& cl = b->clusters[c];
    out.push_back(cl.count);
    out.push_back(cl.weight);
    for (int k = 0; k < 3; ++k) out.push_back(cl.mean.v[k]);
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) out.push_back(cl.cov.m[j][k]);
  }
  for (int k = 0; k < 3; ++k) out.push_back(b->mean.v[k]);
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 3; ++k) out.push_back(b->cov.m[j][k]);
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) {
    perror(argv[2]);
    return 2;
  }
  fclose(f);
  pf_free(pf);
  return 0;
}
