// costmap_3d::Costmap3DQuery for a batch of poses (include/navgpu.h): k_c3d_rasterize writes octomap leaves into the
// resident bit volumes, k_c3d_query answers one pose per wave, k_c3d_fold is Costmap3DROS::processPlanCost3D's fold per run.
// All geometry is fp64 under -ffp-contract=off: tests/costmap3d_ref.py evaluates the same expressions in numpy.
#include <float.h>

#include "navgpu_costmap3d.h"

namespace navgpu {

namespace {

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }

// ---- overlap: the 13-axis separating-axis test of a triangle (relative to the cube's centre) against the cube of half edge h.
// Closed sets: touching is overlap.  An axis that degenerates to zero separates nothing.
__device__ __forceinline__ bool separated(V3 a, V3 v0, V3 v1, V3 v2, double h) {
  const double p0 = dot(a, v0), p1 = dot(a, v1), p2 = dot(a, v2);
  const double r = h * (fabs(a.x) + fabs(a.y) + fabs(a.z));
  return fmin(p0, fmin(p1, p2)) > r || fmax(p0, fmax(p1, p2)) < -r;
}
__device__ bool triCubeOverlap(V3 v0, V3 v1, V3 v2, double h) {
  const V3 ax[3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const V3 e[3] = {v1 - v0, v2 - v1, v0 - v2};
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (separated(ax[i], v0, v1, v2, h)) return false;
  if (separated(cross(e[0], e[1]), v0, v1, v2, h)) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (separated(cross(e[i], ax[j]), v0, v1, v2, h)) return false;
  return true;
}

// ---- distance: the closest feature pairs of two disjoint convex polytopes, squared.
__device__ __forceinline__ double pointCube2(V3 p, double h) {  // a triangle vertex against the cube
  const double qx = fmax(fabs(p.x) - h, 0.0), qy = fmax(fabs(p.y) - h, 0.0), qz = fmax(fabs(p.z) - h, 0.0);
  return qx * qx + qy * qy + qz * qz;
}
__device__ __forceinline__ double pointSegment2(V3 p, V3 a, V3 ab) {
  const double t = clamp01(dot(p - a, ab) / dot(ab, ab));
  const V3 d = p - (a + ab * t);
  return dot(d, d);
}
// a cube corner against the triangle: the plane distance where the corner projects into the triangle, else the nearest edge
__device__ double pointTriangle2(V3 p, V3 v0, V3 v1, V3 v2) {
  const V3 e0 = v1 - v0, e1 = v2 - v1, e2 = v0 - v2;
  const V3 n = cross(e0, e1);
  const double s0 = dot(cross(e0, p - v0), n), s1 = dot(cross(e1, p - v1), n), s2 = dot(cross(e2, p - v2), n);
  if (s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0) {
    const double d = dot(p - v0, n);
    return d * d / dot(n, n);
  }
  return fmin(pointSegment2(p, v0, e0), fmin(pointSegment2(p, v1, e1), pointSegment2(p, v2, e2)));
}
// two segments p1 + s d1, p2 + t d2 (neither of zero length)
__device__ double segmentSegment2(V3 p1, V3 d1, V3 p2, V3 d2) {
  const V3 r = p1 - p2;
  const double a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r), c = dot(d1, r), b = dot(d1, d2);
  const double denom = a * e - b * b;
  double s = denom != 0.0 ? clamp01((b * f - c * e) / denom) : 0.0;
  double t = (b * s + f) / e;
  if (t < 0.0) {
    t = 0.0;
    s = clamp01(-c / a);
  } else if (t > 1.0) {
    t = 1.0;
    s = clamp01((b - c) / a);
  }
  const V3 d = (p1 + d1 * s) - (p2 + d2 * t);
  return dot(d, d);
}
__device__ double triCubeDistance2(V3 v0, V3 v1, V3 v2, double h) {
  double best = fmin(pointCube2(v0, h), fmin(pointCube2(v1, h), pointCube2(v2, h)));
  for (int k = 0; k < 8; ++k) {
    const V3 c = {(k & 1) ? h : -h, (k & 2) ? h : -h, (k & 4) ? h : -h};
    best = fmin(best, pointTriangle2(c, v0, v1, v2));
  }
  const V3 tp[3] = {v0, v1, v2};
  const V3 te[3] = {v1 - v0, v2 - v1, v0 - v2};
  const double w = 2.0 * h;
  for (int axis = 0; axis < 3; ++axis) {
    const V3 d2 = {axis == 0 ? w : 0.0, axis == 1 ? w : 0.0, axis == 2 ? w : 0.0};
    for (int k = 0; k < 4; ++k) {  // the four cube edges along this axis
      const double u = (k & 1) ? h : -h, v = (k & 2) ? h : -h;
      const V3 p2 = axis == 0 ? V3{-h, u, v} : (axis == 1 ? V3{u, -h, v} : V3{u, v, -h});
#pragma unroll
      for (int i = 0; i < 3; ++i) best = fmin(best, segmentSegment2(tp[i], te[i], p2, d2));
    }
  }
  return best;
}

// ---- interior: the solid angle of a triangle seen from the origin (van Oosterom and Strackee); the sum over a closed mesh is
// 4 pi times the winding number
__device__ __forceinline__ double solidAngle(V3 a, V3 b, V3 c) {
  const double la = sqrt(dot(a, a)), lb = sqrt(dot(b, b)), lc = sqrt(dot(c, c));
  const double num = dot(a, cross(b, c));
  const double den = la * lb * lc + dot(a, b) * lc + dot(a, c) * lb + dot(b, c) * la;
  return 2.0 * atan2(num, den);
}

__device__ __forceinline__ double waveMin(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ double waveMax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// The cell range a world box [lo, hi] touches along one axis, a cell wider each way (so that rounding cannot lose a touching
// cell) and clipped to [0, size): first > last when empty.  `whole` says that the unclipped range covers the axis.
struct AxisRange {
  int first, last;
  bool whole;
};
__device__ __forceinline__ AxisRange axisRange(double lo, double hi, double origin, double res, uint32_t size) {
  const double f0 = floor((lo - origin) / res) - 1.0, f1 = floor((hi - origin) / res) + 1.0;
  const double top = (double)size - 1.0;
  AxisRange r;
  r.whole = f0 <= 0.0 && f1 >= top;
  const double c0 = fmax(f0, 0.0), c1 = fmin(f1, top);
  if (!(c0 <= c1)) {
    r.first = 0;
    r.last = -1;
  } else {
    r.first = (int)c0;
    r.last = (int)c1;
  }
  return r;
}
__device__ __forceinline__ uint64_t bitRange(int first, int last) {  // 0 <= first <= last <= 63
  const uint64_t upto = last >= 63 ? ~0ull : ((1ull << (last + 1)) - 1ull);
  return upto & ~((1ull << first) - 1ull);
}

struct CellBox {  // a clipped cell range
  AxisRange x, y, z;
  __device__ bool empty() const { return x.first > x.last || y.first > y.last || z.first > z.last; }
};

// What one wave knows about its pose
struct Pose {
  V3 lo, hi;            // the world AABB of the posed mesh
  V3 org;               // the instance's origin
  const double* half;   // LDS [n_half][4] the region's half-spaces {n, d}: a cell is outside when dot(n, centre) - d > extent
  int n_half;
  const uint64_t* plane;
};

enum { kPassCollision = 0, kPassDistance = 1 };

// One walk over the occupied cells of `box` (those of `done` left out): considered cells go to the LDS queue, the queue is
// worked off (cell, triangle) pair by pair.  Collision pass: returns > 0 at the first hit.  Distance pass: lowers best2.
template <int PASS>
__device__ double walk(const C3dDev& d, const Pose& P, const CellBox& box, const CellBox& done, bool have_done, const double* tri, uint32_t* queue,
                       uint32_t* qn, double best2) {
  const int lane = threadIdx.x;
  const double res = d.res, h = 0.5 * d.res;
  const int nx = box.x.last - box.x.first + 1, ny = box.y.last - box.y.first + 1;
  const uint32_t total = (uint32_t)nx * (uint32_t)ny;
  const uint64_t zmask = bitRange(box.z.first, box.z.last);
  const uint64_t zdone = have_done ? bitRange(done.z.first, done.z.last) : 0ull;
  const uint32_t nt = d.nt;
  // columns per chunk: as many as cannot add more than half the queue (at least 32, there are at most 64 levels)
  const uint32_t levels = (uint32_t)(box.z.last - box.z.first + 1);
  const uint32_t step = (kC3dQueue / 2) / levels < 64u ? (kC3dQueue / 2) / levels : 64u;
  bool hit = false;
  for (uint32_t base = 0; base < total; base += step) {
    const uint32_t c = base + lane;
    if ((uint32_t)lane < step && c < total) {
      const int x = box.x.first + (int)(c % (uint32_t)nx), y = box.y.first + (int)(c / (uint32_t)nx);
      const uint32_t col = (uint32_t)y * d.sx + (uint32_t)x;
      uint64_t word = P.plane[col] & zmask;
      if (have_done && x >= done.x.first && x <= done.x.last && y >= done.y.first && y <= done.y.last) word &= ~zdone;
      while (word) {
        const int z = __builtin_ctzll(word);
        word &= word - 1;
        const V3 ctr = {P.org.x + ((double)x + 0.5) * res, P.org.y + ((double)y + 0.5) * res, P.org.z + ((double)z + 0.5) * res};
        bool keep = true;
        for (int k = 0; k < P.n_half; ++k) {  // checkROI: out when the centre is further outside than the cube's extent
          const V3 n = {P.half[4 * k], P.half[4 * k + 1], P.half[4 * k + 2]};
          const double extent = 0.5 * (fabs(n.x * res) + fabs(n.y * res) + fabs(n.z * res));
          keep = keep && !(dot(n, ctr) - P.half[4 * k + 3] > extent);
        }
        if (PASS == kPassDistance && keep) {  // a cell no closer to the mesh's box than the best so far cannot lower it
          const double qx = fmax(fmax(P.lo.x - (ctr.x + h), (ctr.x - h) - P.hi.x), 0.0);
          const double qy = fmax(fmax(P.lo.y - (ctr.y + h), (ctr.y - h) - P.hi.y), 0.0);
          const double qz = fmax(fmax(P.lo.z - (ctr.z + h), (ctr.z - h) - P.hi.z), 0.0);
          keep = qx * qx + qy * qy + qz * qz < best2;
        }
        if (keep) queue[atomicAdd(qn, 1u)] = (col << 6) | (uint32_t)z;  // (at most kC3dQueue / 2 per chunk onto at most kC3dQueue / 2)
      }
    }
    __syncthreads();
    const uint32_t nq = *qn;
    if (nq <= kC3dQueue / 2 && base + step < total) continue;  // gather more cells before working the queue off
    const uint32_t pairs = nq * nt;
    for (uint32_t pb = 0; pb < pairs; pb += 64) {
      const uint32_t p = pb + lane;
      if (p < pairs) {
        const uint32_t e = queue[p / nt];
        const double* T = tri + 9 * (p % nt);
        const uint32_t col = e >> 6;
        const V3 ctr = {P.org.x + ((double)(col % d.sx) + 0.5) * res, P.org.y + ((double)(col / d.sx) + 0.5) * res,
                        P.org.z + ((double)(e & 63u) + 0.5) * res};
        const V3 v0 = V3{T[0], T[1], T[2]} - ctr, v1 = V3{T[3], T[4], T[5]} - ctr, v2 = V3{T[6], T[7], T[8]} - ctr;
        if (PASS == kPassCollision) {
          hit = triCubeOverlap(v0, v1, v2, h);
        } else {
          // the triangle's own box against the cube first
          const double qx = fmax(fmax(fmin(v0.x, fmin(v1.x, v2.x)) - h, -h - fmax(v0.x, fmax(v1.x, v2.x))), 0.0);
          const double qy = fmax(fmax(fmin(v0.y, fmin(v1.y, v2.y)) - h, -h - fmax(v0.y, fmax(v1.y, v2.y))), 0.0);
          const double qz = fmax(fmax(fmin(v0.z, fmin(v1.z, v2.z)) - h, -h - fmax(v0.z, fmax(v1.z, v2.z))), 0.0);
          if (qx * qx + qy * qy + qz * qz < best2) best2 = fmin(best2, triCubeDistance2(v0, v1, v2, h));
        }
      }
      if (PASS == kPassCollision && __any(hit)) break;
    }
    if (PASS == kPassCollision) {
      hit = __any(hit);
      if (!hit && d.closed) {  // no triangle touched: a cell may still lie wholly inside the solid
        for (uint32_t qb = 0; qb < nq; qb += 64) {
          const uint32_t i = qb + lane;
          if (i < nq) {
            const uint32_t e = queue[i], col = e >> 6;
            const V3 ctr = {P.org.x + ((double)(col % d.sx) + 0.5) * res, P.org.y + ((double)(col / d.sx) + 0.5) * res,
                            P.org.z + ((double)(e & 63u) + 0.5) * res};
            if (ctr.x >= P.lo.x && ctr.x <= P.hi.x && ctr.y >= P.lo.y && ctr.y <= P.hi.y && ctr.z >= P.lo.z && ctr.z <= P.hi.z) {
              double omega = 0.0;
              for (uint32_t t = 0; t < nt; ++t) {
                const double* T = tri + 9 * t;
                omega += solidAngle(V3{T[0], T[1], T[2]} - ctr, V3{T[3], T[4], T[5]} - ctr, V3{T[6], T[7], T[8]} - ctr);
              }
              hit = fabs(omega / (4.0 * 3.14159265358979323846)) > 0.5;
            }
          }
          if (__any(hit)) break;
        }
        hit = __any(hit);
      }
    } else {
      best2 = waveMin(best2);
    }
    __syncthreads();
    if (lane == 0) *qn = 0;
    __syncthreads();
    if (PASS == kPassCollision && hit) return 1.0;
  }
  return PASS == kPassCollision ? 0.0 : best2;
}

__global__ __launch_bounds__(64) void k_c3d_query(C3dDev d, C3dQuery q) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* tri = reinterpret_cast<double*>(smem);                                  // [nt][3][3] the pose's world triangles
  uint32_t* queue = reinterpret_cast<uint32_t*>(smem + ((d.nt * 72u + 15u) & ~15u));  // [kC3dQueue]
  uint32_t* qn = queue + kC3dQueue;
  double* half = reinterpret_cast<double*>(qn + 4);  // [5][4]
  const int lane = threadIdx.x;
  const uint32_t p = blockIdx.x;
  if (p >= q.n_poses) return;
  const int32_t inst = q.pose_inst[p];
  if (inst < 0 || (uint32_t)inst >= d.n) return;  // (wave-uniform)
  if (lane == 0) *qn = 0;

  const double* in = q.poses + 7 * (size_t)p;
  const V3 T = {in[0], in[1], in[2]};
  double qx = in[3], qy = in[4], qz = in[5], qw = in[6];
  const double qn2 = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  qx /= qn2, qy /= qn2, qz /= qn2, qw /= qn2;
  const V3 r0 = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qz * qw), 2.0 * (qx * qz + qy * qw)};
  const V3 r1 = {2.0 * (qx * qy + qz * qw), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qx * qw)};
  const V3 r2 = {2.0 * (qx * qz - qy * qw), 2.0 * (qy * qz + qx * qw), 1.0 - 2.0 * (qx * qx + qy * qy)};

  Pose P;
  P.lo = {DBL_MAX, DBL_MAX, DBL_MAX};
  P.hi = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
  for (uint32_t v = lane; v < 3 * d.nt; v += 64) {
    const V3 b = {d.verts[3 * v], d.verts[3 * v + 1], d.verts[3 * v + 2]};
    const V3 w = {dot(r0, b) + T.x, dot(r1, b) + T.y, dot(r2, b) + T.z};
    tri[3 * v] = w.x, tri[3 * v + 1] = w.y, tri[3 * v + 2] = w.z;
    P.lo = {fmin(P.lo.x, w.x), fmin(P.lo.y, w.y), fmin(P.lo.z, w.z)};
    P.hi = {fmax(P.hi.x, w.x), fmax(P.hi.y, w.y), fmax(P.hi.z, w.z)};
  }
  P.lo = {waveMin(P.lo.x), waveMin(P.lo.y), waveMin(P.lo.z)};
  P.hi = {waveMax(P.hi.x), waveMax(P.hi.y), waveMax(P.hi.z)};
  P.org = {d.origins[3 * inst], d.origins[3 * inst + 1], d.origins[3 * inst + 2]};
  const bool distance = q.mode == NAVGPU_C3D_DISTANCE;
  const int cls = distance && q.obstacles[p] ? NAVGPU_C3D_NONLETHAL : NAVGPU_C3D_LETHAL;
  P.plane = d.planes + ((size_t)inst * 2 + cls) * d.cols;

  // RegionsOfInterestAtPose: the half-space {n . x <= dist} in the robot's frame becomes {R n . x <= dist + R n . T}
  const int region = q.regions[p];
  P.n_half = region == NAVGPU_C3D_REGION_RECTANGULAR_PRISM ? 5 : (region == NAVGPU_C3D_REGION_ALL ? 0 : 1);
  P.half = half;
  if (lane < P.n_half) {  // lane k writes half-space k
    V3 n = {0.0, region == NAVGPU_C3D_REGION_LEFT ? -1.0 : 1.0, 0.0};
    double dist = 0.0;
    if (region == NAVGPU_C3D_REGION_RECTANGULAR_PRISM) {  // -x at 0, +-y at scale_y / 2, +-z at scale_z / 2
      n = {lane == 0 ? -1.0 : 0.0, lane == 1 ? 1.0 : (lane == 2 ? -1.0 : 0.0), lane == 3 ? 1.0 : (lane == 4 ? -1.0 : 0.0)};
      dist = lane == 0 ? 0.0 : (lane < 3 ? q.scale_y / 2.0 : q.scale_z / 2.0);
    }
    const V3 w = {dot(r0, n), dot(r1, n), dot(r2, n)};
    half[4 * lane] = w.x, half[4 * lane + 1] = w.y, half[4 * lane + 2] = w.z;
    half[4 * lane + 3] = dist + dot(w, T);
  }
  __syncthreads();

  CellBox tight;
  tight.x = axisRange(P.lo.x, P.hi.x, P.org.x, d.res, d.sx);
  tight.y = axisRange(P.lo.y, P.hi.y, P.org.y, d.res, d.sy);
  tight.z = axisRange(P.lo.z, P.hi.z, P.org.z, d.res, d.sz);
  bool collides = false;
  if (!tight.empty()) collides = walk<kPassCollision>(d, P, tight, tight, false, tri, queue, qn, 0.0) > 0.0;

  double cost = collides ? -1.0 : 0.0;
  if (distance && !collides) {
    const double limit = q.limit <= 0.0 ? DBL_MIN : q.limit;
    double best2 = DBL_MAX, best = DBL_MAX;
    double B = 4.0 * d.res;
    CellBox done = tight;
    bool have_done = false;
    for (;;) {
      const double Bc = fmin(B, limit);
      CellBox box;
      box.x = axisRange(P.lo.x - Bc, P.hi.x + Bc, P.org.x, d.res, d.sx);
      box.y = axisRange(P.lo.y - Bc, P.hi.y + Bc, P.org.y, d.res, d.sy);
      box.z = axisRange(P.lo.z - Bc, P.hi.z + Bc, P.org.z, d.res, d.sz);
      if (!box.empty()) {
        best2 = walk<kPassDistance>(d, P, box, done, have_done, tri, queue, qn, best2);
        best = best2 < DBL_MAX ? sqrt(best2) : DBL_MAX;
        done = box;
        have_done = true;
      }
      // every cell within Bc of the mesh lies in the box: a distance <= Bc is final; so is any once the box covers the map
      if (best <= Bc || Bc >= limit || (box.x.whole && box.y.whole && box.z.whole) || !(B < 1e300)) break;
      B *= 2.0;
    }
    cost = best < limit ? best : limit;
  }
  if (lane == 0) q.pose_costs[p] = cost;
}

// Costmap3DROS::processPlanCost3D's fold (costmap_3d_ros.cpp:494-609), one lane per run
__global__ void k_c3d_fold(C3dQuery q) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= q.n_runs) return;
  const navgpu_c3d_run run = q.runs[r];
  const bool distance = q.mode == NAVGPU_C3D_DISTANCE;
  navgpu_c3d_run_result out;
  out.cost = distance ? DBL_MAX : 0.0;
  out.n_lethal = 0;
  out.first_lethal = -1;
  out.n_done = (int32_t)run.n_poses;
  out.reserved = 0;
  for (uint32_t j = 0; j < run.n_poses; ++j) {
    const double pose_cost = q.pose_costs[run.first_pose + j];
    const bool collision = pose_cost < 0.0;
    if (distance) {
      out.cost = fmin(out.cost, pose_cost);
    } else if (collision) {
      out.cost = out.cost >= 0.0 ? pose_cost : out.cost + pose_cost;
    } else if (out.cost >= 0.0) {
      out.cost += pose_cost;
    }
    if (collision) {
      ++out.n_lethal;
      if (out.first_lethal < 0) out.first_lethal = (int32_t)j;
      if (q.lazy) {
        out.n_done = (int32_t)j + 1;
        break;
      }
    }
  }
  q.results[r] = out;
}

// One thread per (box, column of the box): the box's levels into (MARK) or out of (MARK: the other class, CLEAR: both) the column's words
__global__ void k_c3d_rasterize(C3dDev d, uint32_t instance, int32_t mode, const C3dBoxCells* boxes, uint32_t n_boxes) {
  const uint32_t b = blockIdx.y;
  if (b >= n_boxes || instance >= d.n) return;
  const C3dBoxCells box = boxes[b];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= box.nx * box.ny) return;
  const uint32_t x = box.x0 + i % box.nx, y = box.y0 + i / box.nx;
  if (x >= d.sx || y >= d.sy) return;
  unsigned long long* lethal = reinterpret_cast<unsigned long long*>(d.planes + ((size_t)instance * 2 + NAVGPU_C3D_LETHAL) * d.cols) + (size_t)y * d.sx + x;
  unsigned long long* nonlethal = reinterpret_cast<unsigned long long*>(d.planes + ((size_t)instance * 2 + NAVGPU_C3D_NONLETHAL) * d.cols) + (size_t)y * d.sx + x;
  const unsigned long long m = box.zmask;
  if (mode == NAVGPU_C3D_CLEAR) {
    atomicAnd(lethal, ~m);
    atomicAnd(nonlethal, ~m);
  } else {
    atomicOr(box.cls == NAVGPU_C3D_LETHAL ? lethal : nonlethal, m);
    atomicAnd(box.cls == NAVGPU_C3D_LETHAL ? nonlethal : lethal, ~m);
  }
}

}  // namespace

void launch_c3d_rasterize(const C3dDev& d, uint32_t instance, int32_t mode, const C3dBoxCells* boxes, uint32_t n_boxes, uint32_t max_columns,
                          hipStream_t stream) {
  if (!n_boxes || !max_columns) return;
  for (uint32_t first = 0; first < n_boxes; first += 65535u) {  // (gridDim.y)
    const uint32_t count = n_boxes - first < 65535u ? n_boxes - first : 65535u;
    hipLaunchKernelGGL(k_c3d_rasterize, dim3((max_columns + 255) / 256, count), dim3(256), 0, stream, d, instance, mode, boxes + first, count);
  }
}

void launch_c3d_query(const C3dDev& d, const C3dQuery& q, hipStream_t stream) {
  if (q.n_poses) {
    const size_t lds = ((d.nt * 72u + 15u) & ~15u) + sizeof(uint32_t) * kC3dQueue + 16 + 5 * 4 * sizeof(double);
    hipLaunchKernelGGL(k_c3d_query, dim3(q.n_poses), dim3(64), lds, stream, d, q);
  }
  if (q.n_runs) hipLaunchKernelGGL(k_c3d_fold, dim3((q.n_runs + 63) / 64), dim3(64), 0, stream, q);
}

}  // namespace navgpu
